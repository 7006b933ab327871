"""The cross-attention kernels with a condition length per batch element -- gsdd_d3pm_cross_attention_train_len (out + lse),
gsdd_d3pm_cross_attention_bwd_len (dq, dkc, dvc) and the sampler's gsdd_d3pm_cross_attention_len -- against fp64, element by element.

The rule: batch element b attends to its keys 0 .. len[b] - 1 only; keys behind the length are not read; the backward writes the dkc /
dvc rows behind the length as exact zeros.

Reference and bars are those of tests/test_gpu_cross_attention_train.py, unchanged: its `reference()` is called per batch element at
B = 1 with Te = len[b] on the truncated kc / vc, so every bar is the one derived there, evaluated at the length (the kernels run the
same chain over len[b] keys that they run over Te keys without lengths).  No tolerance is introduced here.  Inputs are that file's
`make_inputs` (per-(batch, head) temperatures, one row of equal scores); its 40.5-score row is scaled over all Te keys and is whatever
it is over a prefix.

Shapes (B, L, Te, H): Te in {2, 15, 17, 22, 77}, L in {1, 37, 64, 257} (partial last chunk of 64 rows, blocks that straddle batch
elements, one row per batch element), H in {1, 2, 16}; all but (3, 257, 17, 1) are among that file's SMALL cases.  Length patterns:
every length Te, every length 1, and [1, Te, (Te + 1) // 2] -- the first, the last and a middle key as the boundary.

Per case: out, lse, dq and the dkc / dvc rows in front of the length within their bars (cross_len::* in the parity report); dkc / dvc
rows at and behind the length exactly 0 over a nonzero prefill; sentinels behind every output and behind the workspace's stated size
intact; a second run gives the same bits; B = 3 in one launch equals three B = 1 launches bit for bit; the sampler's kernel within the
out bar of the same fp64 values; NaN, and then 1e30, in the kc / vc rows behind the length change no bit of any output; and every
length = Te gives the bits of the entry points without lengths."""
import pytest
import torch

from tests.conftest import parity_report
from tests.test_gpu_cross_attention_train import SMALL, bits, guarded, intact, make_inputs, reference
from tests.test_gpu_train_kernels import SENT, ratio

pytestmark = pytest.mark.gpu

PREFILL = 123.25
SHAPES = [(3, 37, 2, 2), (3, 64, 15, 16), (3, 257, 17, 1), (3, 257, 22, 16), (3, 1, 77, 16), (3, 257, 77, 2)]
PATTERNS = {"full": lambda Te: [Te, Te, Te], "one": lambda Te: [1, 1, 1], "mixed": lambda Te: [1, Te, (Te + 1) // 2]}
CASES = [(s, p) for s in SHAPES for p in PATTERNS]
IDS = ["B%d_L%d_Te%d_H%d-%s" % (*s, p) for s, p in CASES]
OUTPUTS = ("out", "lse", "dq", "dkc", "dvc")

assert set(SHAPES) - set(SMALL) == {(3, 257, 17, 1)}


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()
    return gsdd_amd


def lengths(Te, pattern):
    host = torch.tensor(PATTERNS[pattern](Te), dtype=torch.int32)
    return host, host.cuda()


def run_pair_len(G, q, kc, vc, dO, B, L, Te, H, len_host, len_dev, host_copy=True):
    """forward + backward with lengths on guarded, prefilled buffers -> (outputs, `intact` flags).  len_dev None: the entry points
    without lengths."""
    M = B * L
    kw = {} if len_dev is None else {"cond_len": len_dev, "cond_len_host": len_host if host_copy else None}
    obuf, out = guarded((M, 4 * H), SENT)
    lbuf, lse = guarded((H * M,), SENT)
    G.ops.d3pm_cross_attention_train(q, kc, vc, B, L, Te, H, out, lse, **kw)
    nws = G.lib().gsdd_d3pm_cross_attention_bwd_workspace_bytes(B, L, Te, H)
    assert nws > 0 and nws % 4 == 0
    wbuf, ws = guarded((nws // 4,), SENT)
    qbuf, dq = guarded((H, M, 4), PREFILL)
    kbuf, dkc = guarded((B * Te, 4 * H), PREFILL)
    vbuf, dvc = guarded((B * Te, 4 * H), -PREFILL)
    G.ops.d3pm_cross_attention_bwd(q, kc, vc, out, dO, lse, B, L, Te, H, ws, dq=dq, dkc=dkc, dvc=dvc, **kw)
    torch.cuda.synchronize()
    ok = {"out": intact(obuf, out.numel()), "lse": intact(lbuf, lse.numel()), "workspace": intact(wbuf, ws.numel()),
          "dq": intact(qbuf, dq.numel()), "dkc": intact(kbuf, dkc.numel()), "dvc": intact(vbuf, dvc.numel())}
    return {"out": out, "lse": lse, "dq": dq, "dkc": dkc, "dvc": dvc}, ok


def padded(x, B, Te, len_host, value):
    """x rows [B Te][4 H] with the rows at and behind every batch element's length filled with `value`"""
    y = x.clone().view(B, Te, -1)
    for b in range(B):
        y[b, int(len_host[b]):] = value
    return y.view(B * Te, -1)


@pytest.mark.parametrize("shape,pattern", CASES, ids=IDS)
def test_cross_attention_len_matches_fp64_per_batch_element(G, shape, pattern):
    B, L, Te, H = shape
    q, kc, vc, dO = make_inputs(B, L, Te, H)
    len_host, len_dev = lengths(Te, pattern)
    M = B * L
    got, ok = run_pair_len(G, q, kc, vc, dO, B, L, Te, H, len_host, len_dev)
    plain = torch.empty((M, 4 * H), dtype=torch.float32, device="cuda")
    G.ops.d3pm_cross_attention(q, kc, vc, B, L, Te, H, plain, cond_len=len_dev, cond_len_host=len_host)
    worst = {k: 0.0 for k in ("out", "lse", "dq", "dk", "dv", "out_sampler_kernel")}
    for b in range(B):
        n = int(len_host[b])
        r, e = slice(b * L, (b + 1) * L), slice(b * Te, b * Te + n)
        ref = reference(q[:, r].contiguous(), kc[e].contiguous(), vc[e].contiguous(), dO[r].contiguous(), 1, L, n, H)
        rows = lambda x: x[r].view(1, L, H, 4).permute(0, 2, 1, 3)            # [L][4 H] -> [1][H][L][4]
        cond = lambda x: x[e].view(1, n, H, 4).permute(0, 2, 1, 3)            # the live rows -> [1][H][n][4]
        w = {
            "out": ratio(rows(got["out"]), ref["out"], ref["bar_out"]),
            "lse": ratio(got["lse"].view(H, M)[:, r].reshape(H, 1, L).permute(1, 0, 2).unsqueeze(-1), ref["lse"], ref["bar_lse"]),
            "dq": ratio(got["dq"][:, r].reshape(H, 1, L, 4).permute(1, 0, 2, 3), ref["dq"], ref["bar_dq"]),
            "dk": ratio(cond(got["dkc"]), ref["dk"], ref["bar_dk"]),
            "dv": ratio(cond(got["dvc"]), ref["dv"], ref["bar_dv"]),
            "out_sampler_kernel": ratio(rows(plain), ref["out"], ref["bar_out"]),
        }
        worst = {k: max(worst[k], w[k]) for k in worst}
        # behind the length: exact zeros over the prefill
        dead = slice(b * Te + n, (b + 1) * Te)
        assert not bool(bits(got["dkc"][dead]).any()) and not bool(bits(got["dvc"][dead]).any()), f"batch element {b}: padding gradient is not +0"
    name = IDS[CASES.index((shape, pattern))]
    print(name, worst)
    parity_report(f"cross_len::{name}", {**{k + "_ratio": v for k, v in worst.items()}, "worst_ratio": max(worst.values()),
                                         "lengths": [int(v) for v in len_host]})
    assert all(ok.values()), f"written outside an output or behind the workspace's stated size: {ok}"
    assert max(worst.values()) <= 1, worst
    # the same inputs give the same bits; without the host copy (the kernels clamp what is already in range) too
    again, ok2 = run_pair_len(G, q, kc, vc, dO, B, L, Te, H, len_host, len_dev, host_copy=False)
    assert all(ok2.values()), ok2
    for k_ in OUTPUTS:
        assert torch.equal(bits(got[k_]), bits(again[k_])), f"{k_}: two runs differ"


@pytest.mark.parametrize("shape,pattern", CASES, ids=IDS)
def test_batch_elements_do_not_depend_on_the_launch(G, shape, pattern):
    """B = 3 in one launch equals three B = 1 launches, bit for bit."""
    B, L, Te, H = shape
    q, kc, vc, dO = make_inputs(B, L, Te, H)
    len_host, len_dev = lengths(Te, pattern)
    M = B * L
    got, _ = run_pair_len(G, q, kc, vc, dO, B, L, Te, H, len_host, len_dev)
    for b in range(B):
        r, e = slice(b * L, (b + 1) * L), slice(b * Te, (b + 1) * Te)
        one, ok = run_pair_len(G, q[:, r].contiguous(), kc[e].contiguous(), vc[e].contiguous(), dO[r].contiguous(), 1, L, Te, H,
                               len_host[b:b + 1].contiguous(), len_dev[b:b + 1].contiguous())
        assert all(ok.values()), ok
        assert torch.equal(bits(got["out"][r]), bits(one["out"])), b
        assert torch.equal(bits(got["lse"].view(H, M)[:, r]), bits(one["lse"].view(H, L))), b
        assert torch.equal(bits(got["dq"][:, r]), bits(one["dq"])), b
        assert torch.equal(bits(got["dkc"][e]), bits(one["dkc"])), b
        assert torch.equal(bits(got["dvc"][e]), bits(one["dvc"])), b


@pytest.mark.parametrize("shape,pattern", CASES, ids=IDS)
def test_padding_is_never_read(G, shape, pattern):
    """NaN, then 1e30, in the kc / vc rows at and behind the length: no bit of any output changes (forward, backward, sampler kernel)."""
    B, L, Te, H = shape
    q, kc, vc, dO = make_inputs(B, L, Te, H)
    len_host, len_dev = lengths(Te, pattern)
    M = B * L
    got, _ = run_pair_len(G, q, kc, vc, dO, B, L, Te, H, len_host, len_dev)
    plain = torch.empty((M, 4 * H), dtype=torch.float32, device="cuda")
    G.ops.d3pm_cross_attention(q, kc, vc, B, L, Te, H, plain, cond_len=len_dev, cond_len_host=len_host)
    for value in (float("nan"), 1e30):
        kp, vp = padded(kc, B, Te, len_host, value), padded(vc, B, Te, len_host, value)
        alt, ok = run_pair_len(G, q, kp, vp, dO, B, L, Te, H, len_host, len_dev)
        assert all(ok.values()), ok
        for k_ in OUTPUTS:
            assert torch.equal(bits(got[k_]), bits(alt[k_])), f"{k_} depends on the padding ({value})"
        plain2 = torch.empty_like(plain)
        G.ops.d3pm_cross_attention(q, kp, vp, B, L, Te, H, plain2, cond_len=len_dev, cond_len_host=len_host)
        assert torch.equal(bits(plain), bits(plain2)), f"the sampler's kernel depends on the padding ({value})"


@pytest.mark.parametrize("shape", SHAPES, ids=["B%d_L%d_Te%d_H%d" % s for s in SHAPES])
def test_full_length_is_the_call_without_lengths(G, shape):
    """len = Te everywhere: the bits of gsdd_d3pm_cross_attention_train / _bwd / gsdd_d3pm_cross_attention, all five outputs."""
    B, L, Te, H = shape
    q, kc, vc, dO = make_inputs(B, L, Te, H)
    len_host, len_dev = lengths(Te, "full")
    got, _ = run_pair_len(G, q, kc, vc, dO, B, L, Te, H, len_host, len_dev)
    old, ok = run_pair_len(G, q, kc, vc, dO, B, L, Te, H, None, None)
    assert all(ok.values()), ok
    for k_ in OUTPUTS:
        assert torch.equal(bits(got[k_]), bits(old[k_])), k_
    a, b = (torch.empty((B * L, 4 * H), dtype=torch.float32, device="cuda") for _ in range(2))
    G.ops.d3pm_cross_attention(q, kc, vc, B, L, Te, H, a, cond_len=len_dev, cond_len_host=len_host)
    G.ops.d3pm_cross_attention(q, kc, vc, B, L, Te, H, b)
    assert torch.equal(bits(a), bits(b))


def test_device_lengths_out_of_range_are_clamped(G):
    """No host copy (a captured step): a device length of 0 or Te + 5 runs as 1 / Te -- inside the rows, never an empty softmax."""
    B, L, Te, H = 3, 37, 17, 16
    q, kc, vc, dO = make_inputs(B, L, Te, H)
    wild = torch.tensor([0, Te + 5, -3], dtype=torch.int32)
    tame = torch.tensor([1, Te, 1], dtype=torch.int32)
    got, ok = run_pair_len(G, q, kc, vc, dO, B, L, Te, H, None, wild.cuda(), host_copy=False)
    want, _ = run_pair_len(G, q, kc, vc, dO, B, L, Te, H, tame, tame.cuda())
    assert all(ok.values()), ok
    for k_ in OUTPUTS:
        assert torch.equal(bits(got[k_]), bits(want[k_])), k_
    with pytest.raises(G.GsddError, match=r"cond_len\[0\] = 0"):
        G.ops.d3pm_cross_attention_train(q, kc, vc, B, L, Te, H, got["out"], got["lse"], cond_len=wild.cuda(), cond_len_host=wild)
