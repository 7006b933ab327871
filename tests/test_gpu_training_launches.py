"""The D3PM training step's launch sequence: every call `D3PMTrainer.loss_and_grads` makes into gsdd_amd.ops, by name and in order,
against sequences written out here -- the step's head, one forward block and one backward block for each of the four paths (one
condition token or several x fragment images or the generic GEMM), and the tail.  A change to the block shows here as the launches
that moved.

Recording: every public function of gsdd_amd.ops is wrapped on the module (d3pm_train and d3pm call `ops.X`); a call made from
inside another op (ops.attn_train_mode from ops.d3pm_attention_train, ...) is not a launch of the step and is not recorded.  The
names include the host-side helpers the step calls through ops (workspace sizes, image sizes).

Model: the two-layer model of tests/test_gpu_training_cond_tokens.py (K = 32, B = 2), fresh for every case, so each case is a
trainer's first step: the weight images are built (one ops.rows_linear_image_bytes per image for the size of a block and one per
image and block for the layout) and each block's ln1_1 AdaLN table is made at its first use.  L = 96 (spatial (12, 8): attention
workspaces) and L = 40 ((8, 5), L % 32 != 0: none)."""
import inspect

import pytest
import torch

from tests.test_gpu_training_cond_tokens import B, NOISE_SEED, T, batch, make_model

pytestmark = pytest.mark.gpu

N_LAYER = 2


def record_ops(setattr_, ops, trace, detail=None):
    """Wraps every public function of `ops` through setattr_(ops, name, wrapper): `trace` gets the name of each outermost call;
    `detail`, if a list, the name with every argument bound to the signature (tensors as (shape, dtype), scalars by value)."""
    depth = [0]

    def plain(v):
        if torch.is_tensor(v):
            return ("tensor", tuple(v.shape), str(v.dtype))
        if isinstance(v, (list, tuple)):
            return tuple(plain(x) for x in v)
        return str(v) if isinstance(v, torch.device) else v

    def wrap(name, fn):
        sig = inspect.signature(fn)

        def wrapper(*a, **kw):
            if depth[0] == 0:
                trace.append(name)
                if detail is not None:
                    bound = sig.bind(*a, **kw)
                    bound.apply_defaults()
                    detail.append((name, tuple((k, plain(v)) for k, v in bound.arguments.items())))
            depth[0] += 1
            try:
                return fn(*a, **kw)
            finally:
                depth[0] -= 1
        return wrapper

    for name, fn in list(vars(ops).items()):
        if not name.startswith("_") and inspect.isfunction(fn) and fn.__module__ == ops.__name__:
            setattr_(ops, name, wrap(name, fn))


def run_case(trainer_cls, Te, spatial, drop=False, want_probs=False, **trainer_kw):
    """one loss_and_grads of a fresh trainer on a fresh model -> (trainer, loss, gradients)"""
    L = spatial[0] * spatial[1]
    x0, cond = batch(L, Te)
    dm = make_model(spatial)[0]
    if drop:
        dm.learnable_cf = True
        dm.empty_text_embed.data = torch.randn(77, 512, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    dm = dm.cuda()
    dm.set_noise(NOISE_SEED, stream=0)
    tr = trainer_cls(dm, **trainer_kw)
    loss, g = tr.loss_and_grads(x0.cuda(), cond.cuda(), t=torch.tensor([37, 99]).cuda(), pt=(torch.ones(B) / T).cuda(),
                                want_probs=want_probs, drop=torch.tensor([True, False]).cuda() if drop else None)
    return tr, loss, g


def forward_block(Te, row):
    if Te == 1:
        return ["ln_fwd", row, "d3pm_attention_train", "small_linear", "small_linear", row, "ln_fwd", row, "gelu2", row]
    return ["ln_fwd", row, "d3pm_attention_train", row, "adaln_table", "ln_fwd", row, "small_linear", "small_linear",
            "d3pm_cross_attention_train", row, "ln_fwd", row, "gelu2", row]


def backward_block(Te, row):
    mlp = ["wgrad", row, "gelu2", "wgrad", row, "ln_bwd"]
    if Te == 1:
        middle = ["wgrad", "batch_rowsum", "small_linear_bwd", "small_linear_bwd"]
    else:
        middle = ["wgrad", row, "d3pm_cross_attention_bwd", "wgrad", row, "ln_bwd", "adaln_bwd", "small_linear_bwd", "small_linear_bwd",
                  "wgrad"]
    return mlp + middle + [row, "d3pm_attention_bwd", "wgrad", row, "ln_bwd", "adaln_bwd"]


def expected(Te, linear, L, drop, want_probs):
    """-> (head, forward block, between the blocks, backward block, tail)"""
    row = "rows_linear" if linear == "images" else "linear"
    ws = L % 32 == 0
    head = ["adaln_table"] * N_LAYER + ["d3pm_q_sample"] + ["cond_dropout"] * drop + ["d3pm_embed"] + ["d3pm_attention_workspace"] * ws
    if linear == "images":
        n_img = 8 if Te == 1 else 12
        head += ["rows_linear_image_bytes"] * (n_img * (1 + N_LAYER)) + ["rows_linear_pack_many"]
    loss = ["d3pm_train_loss", "d3pm_train_loss_bwd"] if want_probs else ["d3pm_train_loss_grad"]
    between = ["ln_fwd", "linear"] + loss + ["wgrad", "linear", "ln_bwd"] + ["d3pm_attention_bwd_workspace"] * ws \
        + ["d3pm_cross_attention_bwd_workspace"] * (Te > 1)
    tail = ["d3pm_embed_bwd", "batch_rowsum", "colsum"] + ["cond_null_grad"] * (N_LAYER * drop)
    return head, forward_block(Te, row), between, backward_block(Te, row), tail


CASES = [(Te, linear, spatial, False, False) for Te in (1, 3) for linear in ("images", "gemm") for spatial in ((12, 8), (8, 5))] \
    + [(1, "images", (12, 8), True, False), (3, "images", (12, 8), True, False), (1, "images", (12, 8), False, True)]


def case_id(c):
    return f"Te{c[0]}-{c[1]}-L{c[2][0] * c[2][1]}" + ("-drop" if c[3] else "") + ("-probs" if c[4] else "")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_launch_sequence(monkeypatch, case):
    import gsdd_amd
    from gsdd_amd.d3pm_train import D3PMTrainer
    Te, linear, spatial, drop, want_probs = case
    gsdd_amd.lib()
    if linear == "gemm":
        monkeypatch.setenv("GSDD_TRAIN_LINEAR", "gemm")
    trace = []
    record_ops(monkeypatch.setattr, gsdd_amd.ops, trace)
    tr, _, g = run_case(D3PMTrainer, Te, spatial, drop, want_probs)
    assert (tr._images is not None) == (linear == "images")
    assert ("empty_text_embed" in g) == drop
    head, fwd, between, bwd, tail = expected(Te, linear, spatial[0] * spatial[1], drop, want_probs)
    cuts = [0, len(head)]
    for part in [fwd] * N_LAYER + [between] + [bwd] * N_LAYER + [tail]:
        cuts.append(cuts[-1] + len(part))
    got = [trace[a:b] for a, b in zip(cuts, cuts[1:])]
    print(case_id(case), "forward block:", got[1], "backward block:", got[2 + N_LAYER])
    assert len(trace) == cuts[-1], trace
    assert got[0] == head and got[1 + N_LAYER] == between and got[-1] == tail, trace
    assert got[1] == fwd and got[2 + N_LAYER] == bwd, trace
    assert all(blk == got[1] for blk in got[1:1 + N_LAYER]), "the forward blocks differ"
    assert all(blk == got[2 + N_LAYER] for blk in got[2 + N_LAYER:2 + 2 * N_LAYER]), "the backward blocks differ"
