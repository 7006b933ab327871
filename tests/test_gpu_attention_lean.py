"""The adaptive attention kernel's "quiet" waves (kernel note in d3pm_attention.hip): a wave whose bounds prove in the prologue that
every tile of its (b, h) is cleared and that no probability can get near the f16 overflow takes a lean chunk loop -- the hi-only tile
sequence without the general loop's bookkeeping.  GSDD_ATTN_LEAN=0 sends every wave through the general loop: the two runs must agree
bit for bit (output, log-sum-exp, redo counter), on rows where every wave is quiet, where one wave of a workgroup is not, and where
none is.  B = 2, H = 3: 6 (b, h) pairs times 1..5 query blocks, so the workgroup count is no multiple of 8 (the XCD renumbering's
remainder).  L: 384 = one full chunk; 416 = a full chunk + a 32-key one, ragged second query block; 800 / 1184 = two / three full
chunks + a 32-key one; 64 = nothing can be quiet (log2 L < 8), the general path at its smallest."""
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H = 2, 3
LENGTHS = [384, 416, 800, 1184, 64]
CASES = ["quiet", "mixed", "late_norm", "aligned", "growing"]
QSCALE = 0.5 * 1.4426950408889634          # the kernel's q' = q * qscale (log2 domain)


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()
    return gsdd_amd


def make_inputs(case, L):
    g = torch.Generator().manual_seed(1000 + L)
    q = torch.randn(B, H, L, 4, generator=g) * 0.1
    k = torch.randn(B, H, L, 4, generator=g) * 0.1
    # v: the hi-only arithmetic rounds every probability to 11 bits (relative error uniform in +-2^-12, rms 1.4e-4), so a flat row of
    # L keys is off by 1.4e-4 sigma_v / sqrt(L) rms (include/gsdd.h, GSDD_ATTN_P11), about 4.5 times that at the worst of the 1e4..1e5
    # elements of a case.  At L = 384 that is 3.2e-5 sigma_v: unit-scale v cannot meet the kernel's 2e-5 bar there in this mode (measured
    # 5.4e-5, the parent's bits; it is why GSDD_ATTN_AUTO takes hi + lo below L = 2048).  v of the scale of k's own projection, 0.25,
    # predicts 8e-6.
    v = torch.randn(B, H, L, 4, generator=g) * 0.25
    if case == "mixed":           # one 64-query wave of the first block leaves the quiet path, its three neighbours stay
        w0 = 64 if L > 64 else 0
        q[:, :, w0:w0 + 64] *= 40.0
    elif case == "late_norm":     # large ||k|| in one late pair-tile only: the largest tile norm of the (b, h) is no longer small
        t0 = (L // 32 - 1) * 32
        k[:, :, t0:t0 + 32] *= 30.0
    elif case == "aligned":
        # every tile cleared, condition (b) failed: after 64 keys near zero (so m = -2) all keys sit near one vector k0, ||k0|| = 4, and
        # every query is parallel to it with q'.k0 = 13.6 .. 16.  The mean key is then almost k0, the Jensen bound of the final row sum is
        # almost exact and clears every tile although the scores are large -- and 2^(s - m) = 2^18 overflows f16 in the first chunk.
        u = torch.tensor([0.6, -0.48, 0.64, 0.0])
        mag = 0.85 + 0.15 * torch.rand(B, H, L, 1, generator=g)
        mag[:, :, ::16] = 1.0
        q = u * (16.0 / (QSCALE * 4.0)) * mag
        k = 4.0 * u + 0.005 * torch.randn(B, H, L, 4, generator=g)
        k[:, :, :64] = 0.005 * torch.randn(B, H, 64, 4, generator=g)
    elif case == "growing":       # the score maximum grows along the row: accumulators overflow, exponent offsets move
        q = q * 15.0
        k = k * 15.0 * torch.linspace(0.2, 6.0, L).view(1, 1, L, 1)
    return q, k, v


_cache = {}


def reference(case, L):
    """Inputs and the fp64 softmax(q k^T / 2) v, computed once per (case, L)."""
    if (case, L) not in _cache:
        q, k, v = make_inputs(case, L)
        att = torch.softmax((q.double() @ k.double().transpose(-1, -2)) * 0.5, dim=-1)
        want = (att @ v.double()).permute(0, 2, 1, 3).reshape(B * L, H * 4)
        _cache[(case, L)] = (q, k, v, want)
    return _cache[(case, L)]


def quiet_margin(q, k, L):
    """max over (b, h) of ||q'||max * 2 KNmax, and the a-priori budget log2(L) - 8.02 it has to stay under for every tile of every
    (b, h) to be cleared before a key has been seen (then condition (b), ||q'|| KNmax - m <= 15 with m >= -||q'|| KNmax - 3, holds
    with room to spare)."""
    qn = (q.double() * QSCALE).norm(dim=-1).amax(dim=-1)          # (B, H)
    kn = k.double().norm(dim=-1).amax(dim=-1)
    return (qn * 2.0 * kn * 1.001).max().item(), torch.log2(torch.tensor(float(L))).item() - 8.02


def quiet_conditions(q, k, L):
    """The kernel's two quiet tests with its own formulas (fp64; PM = 8), per 64-query wave -> (a holds for every query of the wave,
    b fails for some query of the wave), each a bool tensor over the waves of all (b, h)."""
    qs = q.double() * QSCALE
    qn = qs.norm(dim=-1) * 1.0001 + 1e-30                                        # (B, H, L)
    knm = k.double().norm(dim=-1).amax(dim=-1, keepdim=True) * 1.000001 * 1.0001  # (B, H, 1): largest tile norm, rounded up twice
    ksum = k.double().sum(dim=2, keepdim=True)                                   # (B, H, 1, 4)
    dots = qs * ksum
    jb = torch.log2(torch.tensor(float(L))) + dots.sum(-1) / L - 1e-5 * dots.abs().sum(-1) / L - 0.02
    budget = torch.log2(torch.tensor(float(L))) - 8.0 - 0.02
    kb = torch.maximum(torch.maximum(budget / qn - knm, (jb - 8.0) / qn), torch.zeros(()).double())
    a = knm * 1.001 < kb                                                         # (with a margin for the kernel's float roundings)
    m = torch.ceil((qs @ k.double()[:, :, :64].transpose(-1, -2)).amax(dim=-1)) - 3.0
    b_fails = qn * knm - m > 15.5
    nw = (L + 63) // 64
    pad = nw * 64 - L
    a = torch.nn.functional.pad(a, (0, pad), value=True).view(B, H, nw, 64).all(dim=-1)
    b_fails = torch.nn.functional.pad(b_fails, (0, pad), value=False).view(B, H, nw, 64).any(dim=-1)
    return a, b_fails


def hm(z):
    return z.permute(1, 0, 2, 3).reshape(H, B * z.shape[2], 4).contiguous().cuda()


def run(G, q, k, v, L, mode, lean, monkeypatch):
    """-> (out, lse or None, redo) as CPU tensors.  The sampler entry gives out + redo, the training forward (a8 only) the lse."""
    if lean:
        monkeypatch.delenv("GSDD_ATTN_LEAN", raising=False)
    else:
        monkeypatch.setenv("GSDD_ATTN_LEAN", "0")
    qd, kd, vd = hm(q), hm(k), hm(v)
    out = torch.full((B * L, H * 4), float("nan"), device="cuda")
    redo = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = G.ops.d3pm_attention_workspace(B, L, H, "cuda")
    G.ops.d3pm_attention(qd, kd, vd, B, L, H, out, ws=ws, redo=redo, mode=mode)
    lse = None
    if mode == "a8":
        out2 = torch.full((B * L, H * 4), float("nan"), device="cuda")
        lse = torch.full((H, B * L), float("nan"), device="cuda")
        G.ops.d3pm_attention_train(qd, kd, vd, B, L, H, out2, lse, ws=ws, mode="a8")
        torch.cuda.synchronize()
        assert torch.equal(bits(out2), bits(out)), "training forward and sampler entry run the same kernel"
        lse = lse.cpu()
    torch.cuda.synchronize()
    return out.cpu(), lse, int(redo.item())


def bits(t):
    return t.contiguous().view(torch.int32)


def test_lean_switch_is_translated_per_call(monkeypatch):
    import gsdd_amd  # noqa: F401
    from gsdd_amd import _lib as abi, ops
    header = open(os.path.join(REPO, "include", "gsdd.h")).read()
    m = re.search(r"#define\s+GSDD_ATTN_NOLEAN\s+(\d+)", header)
    assert m and int(m.group(1)) == abi.ATTN_NOLEAN and abi.ATTN_NOLEAN > abi.ATTN_KC256
    monkeypatch.delenv("GSDD_ATTN_LEAN", raising=False)
    assert ops.attn_lean_flag() == 0
    monkeypatch.setenv("GSDD_ATTN_LEAN", "1")
    assert ops.attn_lean_flag() == 0
    monkeypatch.setenv("GSDD_ATTN_LEAN", "0")
    assert ops.attn_lean_flag() == abi.ATTN_NOLEAN
    monkeypatch.setenv("GSDD_ATTN_LEAN", "off")
    with pytest.raises(gsdd_amd.GsddError):
        ops.attn_lean_flag()


@pytest.mark.gpu
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("case", CASES)
def test_lean_on_equals_lean_off_bitwise_and_fp64(G, case, L, monkeypatch):
    """Cases 1 and 3: output, lse and the redo counter of the adaptive kernel with the lean loop on and off, and both within the
    kernel's 2e-5 of fp64.
    late_norm: one late tile of large keys; its waves fail condition (a) and run the general loop in both runs.
    aligned: the rows that clear every tile yet fail condition (b) -- (b) alone keeps these waves out of the loop that has no
    overflow screen (checked on the CPU for the lengths at which the Jensen bound clears everything, 800 and 1184); redo > 0."""
    q, k, v, want = reference(case, L)
    margin, budget = quiet_margin(q, k, L)
    if case == "quiet" and L >= 288:
        assert margin < 0.9 * budget, (margin, budget)               # every wave is quiet by the a-priori bound alone
    if case in ("mixed", "late_norm") or L < 288:
        assert margin > budget, (margin, budget)                     # ... and here some wave provably is not
    if case == "aligned":
        a_holds, b_fails = quiet_conditions(q, k, L)
        print(f"aligned L={L}: waves with (a) for every query {int(a_holds.sum())}/{a_holds.numel()}, with (b) failing {int(b_fails.sum())}")
        if L in (800, 1184):
            assert a_holds.all() and b_fails.all()
    on, lse_on, redo_on = run(G, q, k, v, L, "a8", True, monkeypatch)
    off, lse_off, redo_off = run(G, q, k, v, L, "a8", False, monkeypatch)
    err = (on.double() - want).abs().max().item()
    print(f"case={case} L={L} err_vs_fp64={err:.3e} redo={redo_on}/{redo_off} margin={margin:.3f} budget={budget:.3f}")
    assert torch.equal(bits(on), bits(off))
    assert torch.equal(bits(lse_on), bits(lse_off))
    assert redo_on == redo_off
    if case in ("growing", "aligned") and L > 64:
        assert redo_on > 0           # (at L = 64 the offset comes from all 64 keys: nothing can overflow)
    if case == "quiet":
        assert redo_on == 0
    assert torch.isfinite(lse_on).all()
    assert err < 2e-5, err


@pytest.mark.gpu
@pytest.mark.parametrize("L", [L for L in LENGTHS if L >= 288])
def test_quiet_rows_a8_equals_p11_bitwise(G, L, monkeypatch):
    """Case 2: on all-quiet rows the adaptive kernel runs the hi-only arithmetic in every tile -- the P11 kernel's, which has no lean
    loop and reads no norms: the in-library reference for the lean loop's arithmetic."""
    q, k, v, _ = reference("quiet", L)
    a8, _, _ = run(G, q, k, v, L, "a8", True, monkeypatch)
    p11, _, _ = run(G, q, k, v, L, "11", True, monkeypatch)
    assert torch.equal(bits(a8), bits(p11))


@pytest.mark.gpu
@pytest.mark.parametrize("L", LENGTHS)
def test_nan_query_row_stays_in_its_row(G, L, monkeypatch):
    """Case 4: a NaN in one query row sends its wave to the general loop (both quiet compares are false for a NaN); that output row is
    NaN, every other row has the bits of the run without the NaN.
    The wave then fails the overflow screen in every chunk and runs out of redo attempts: the last attempt has to keep what it
    computed (restoring the chunk-start copy once more dropped the chunk for all 64 queries of the wave: row sums 0, outputs 0 / 0),
    and the NaN query must not drag the bound of its sub-tile's fifteen neighbours to "never cleared"."""
    q, k, v, _ = reference("quiet", L)
    clean, _, _ = run(G, q, k, v, L, "a8", True, monkeypatch)
    row = min(70, L - 1)
    qn = q.clone()
    qn[0, 1, row, 2] = float("nan")
    got, lse, _ = run(G, qn, k, v, L, "a8", True, monkeypatch)
    assert torch.isnan(got[row, 4:8]).all()
    mask = torch.ones_like(got, dtype=torch.bool)
    mask[row, 4:8] = False
    diff = (bits(got) != bits(clean)) & mask
    nanrows = sorted(set((torch.isnan(got) & mask).nonzero()[:, 0].tolist()))
    print(f"L={L}: {len(set(diff.nonzero()[:, 0].tolist()))} other rows differ, NaN in rows {nanrows}, columns "
          f"{sorted(set((torch.isnan(got) & mask).nonzero()[:, 1].tolist()))}, lse NaN at {torch.isnan(lse).nonzero().tolist()[:8]}")
    assert not diff.any()
    assert not torch.isfinite(lse[1, row]) and int((~torch.isfinite(lse)).sum()) == 1
