"""The adaptive attention kernels read what they need of a whole (b, h) -- the largest tile norm, the inf / NaN flag, the sum of the
keys -- from a 32-byte record that d3pm_attn_stats_kernel reduces once per (b, h) ahead of them (kernel note in d3pm_attention.hip),
and evaluate their bounds from it ahead of the first barrier.  Every decision and every output bit has to stay what it was:
A8 with the lean loop on against GSDD_ATTN_LEAN=0 bit for bit, and both within the kernel's 2e-5 of an fp64 softmax(q k^T / 2) v.

B = 2, H = 3: six (b, h) pairs, so a record read from the wrong pair shows, and with 1..5 query blocks per pair the workgroup count is
no multiple of 8 (the XCD renumbering's remainder).  L: 64 = the smallest length with four first-key tiles (nothing can be quiet:
log2 L < 8); 384 = exactly one chunk; 416 = a full chunk + a last chunk of one pair-tile; 800 / 1184 = the lengths of the lean tests'
`aligned` case.  v has the scale of the lean tests, 0.25 (why: tests/test_gpu_attention_lean.py::make_inputs).

One (b, h) with keys of scale 4: its largest tile norm is ~80 times its neighbours', so its a-priori number budget / ||q'|| - KNmax is
negative at every L here and whether a wave of it still counts as quiet is up to the Jensen term (log2 L - 8) / ||q'||.  With the
kernel's formulas in fp64 (`quiet_waves`, no GPU involved): none of its waves is quiet at L = 384, 416 and 800 while every wave of
its five neighbours is -- asserted; at L = 1184 log2 L - 8 has grown to 2.2 and 10 of its 19 waves (those with the smallest ||q||)
are cleared by the Jensen term and are quiet, 9 are not -- printed, and still a mixed (b, h) beside quiet ones.  Whatever the count,
the bits must equal those of the run with the lean loop off, stay within 2e-5 of fp64, and the five other (b, h) must carry the
bits of the all-flat run."""
import ctypes

import pytest
import torch

B, H = 2, 3
LENGTHS = [64, 384, 416, 800, 1184]
LOUD = (1, 1)                                 # the (b, h) whose keys are large / hold the inf
QSCALE = 0.5 * 1.4426950408889634

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()
    return gsdd_amd


def make_inputs(kind, L):
    g = torch.Generator().manual_seed(7000 + L)
    q = torch.randn(B, H, L, 4, generator=g) * 0.05
    k = torch.randn(B, H, L, 4, generator=g) * 0.05
    v = torch.randn(B, H, L, 4, generator=g) * 0.25
    if kind == "loud":
        k[LOUD] = k[LOUD] * (4.0 / 0.05)      # the same draws at scale 4
    elif kind == "inf":
        k[LOUD][min(70, L - 1), 2] = float("inf")
    return q, k, v


_ref = {}


def reference(kind, L):
    """Inputs and the fp64 softmax(q k^T / 2) v in the kernel's output layout, once per (kind, L)."""
    if (kind, L) not in _ref:
        q, k, v = make_inputs(kind, L)
        att = torch.softmax((q.double() @ k.double().transpose(-1, -2)) * 0.5, dim=-1)
        _ref[(kind, L)] = (q, k, v, (att @ v.double()).permute(0, 2, 1, 3).reshape(B * L, H * 4))
    return _ref[(kind, L)]


def hm(z):
    return z.permute(1, 0, 2, 3).reshape(H, B * z.shape[2], 4).contiguous().cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


_runs = {}


def run(G, kind, L, lean, monkeypatch):
    """-> (out, redo, workspace) of A8 through ops.d3pm_attention, on the CPU; once per (kind, L, lean).
    The lean switch is an environment variable that ops.attn_lean_flag() reads on every call and passes on in the mode argument (the
    library reads no environment), so setting it right before the call is enough and a cached result stays valid for its key."""
    if (kind, L, lean) not in _runs:
        if lean:
            monkeypatch.delenv("GSDD_ATTN_LEAN", raising=False)
        else:
            monkeypatch.setenv("GSDD_ATTN_LEAN", "0")
        q, k, v, _ = reference(kind, L)
        out = torch.full((B * L, H * 4), float("nan"), device="cuda")
        redo = torch.zeros(1, dtype=torch.int64, device="cuda")
        ws = G.ops.d3pm_attention_workspace(B, L, H, "cuda")
        G.ops.d3pm_attention(hm(q), hm(k), hm(v), B, L, H, out, ws=ws, redo=redo, mode="a8")
        torch.cuda.synchronize()
        _runs[(kind, L, lean)] = (out.cpu(), int(redo.item()), ws.cpu())
    return _runs[(kind, L, lean)]


def cols(h):
    return slice(4 * h, 4 * h + 4)


def others_equal(got, clean, L):
    """every (b, h) but LOUD has the bits of the all-flat run"""
    for b in range(B):
        for h in range(H):
            if (b, h) != LOUD and not torch.equal(bits(got[b * L:(b + 1) * L, cols(h)]), bits(clean[b * L:(b + 1) * L, cols(h)])):
                return False
    return True


def quiet_waves(q, k, L):
    """the kernel's two quiet conditions with its own formulas in fp64 (PM = 8) -> bool (B, H, waves): (a) and (b) hold for all 64 queries"""
    qs = q.double() * QSCALE
    qn = qs.norm(dim=-1) * 1.0001 + 1e-30
    knm = k.double().norm(dim=-1).amax(dim=-1, keepdim=True) * 1.000001 * 1.0001
    dots = qs * k.double().sum(dim=2, keepdim=True)
    lg = torch.log2(torch.tensor(float(L), dtype=torch.float64))
    jb = lg + dots.sum(-1) / L - 1e-5 * dots.abs().sum(-1) / L - 0.02
    kb = torch.maximum(torch.maximum((lg - 8.02) / qn - knm, (jb - 8.0) / qn), torch.zeros((), dtype=torch.float64))
    m = torch.ceil((qs @ k.double()[:, :, :64].transpose(-1, -2)).amax(dim=-1)) - 3.0
    ok = (knm < kb) & (qn * knm - m <= 15.0)
    nw = (L + 63) // 64
    return torch.nn.functional.pad(ok, (0, nw * 64 - L), value=True).view(B, H, nw, 64).all(dim=-1)


@pytest.mark.parametrize("L", LENGTHS)
def test_quiet_rows_default_equals_nolean(G, L, monkeypatch):
    q, k, v, want = reference("flat", L)
    on, redo_on, _ = run(G, "flat", L, True, monkeypatch)
    off, redo_off, _ = run(G, "flat", L, False, monkeypatch)
    err = (on.double() - want).abs().max().item()
    qw = quiet_waves(q, k, L)
    print(f"flat L={L}: err_vs_fp64={err:.3e} redo={redo_on}/{redo_off} quiet waves {int(qw.sum())}/{qw.numel()}")
    if L >= 384:
        assert qw.all()                       # (the inputs are what the case says: every wave takes the lean loop)
    assert torch.equal(bits(on), bits(off))
    assert redo_on == redo_off == 0
    assert err < 2e-5, err


@pytest.mark.parametrize("L", LENGTHS)
def test_one_loud_bh_keeps_its_neighbours_bits(G, L, monkeypatch):
    q, k, v, want = reference("loud", L)
    on, redo_on, _ = run(G, "loud", L, True, monkeypatch)
    off, redo_off, _ = run(G, "loud", L, False, monkeypatch)
    clean, _, _ = run(G, "flat", L, True, monkeypatch)
    err = (on.double() - want).abs().max().item()
    qw = quiet_waves(q, k, L)
    print(f"loud L={L}: err_vs_fp64={err:.3e} redo={redo_on}/{redo_off} quiet waves of the loud (b, h) {int(qw[LOUD].sum())}/{qw[LOUD].numel()}, "
          f"of the others {int(qw.sum() - qw[LOUD].sum())}/{qw.numel() - qw[LOUD].numel()}")
    if L >= 384:
        others = qw.clone()
        others[LOUD] = True
        assert others.all()                   # the neighbours are quiet ...
        assert not qw[LOUD].all()             # ... and the loud (b, h) is not
        if L <= 800:
            assert not qw[LOUD].any()
    assert torch.equal(bits(on), bits(off))
    assert redo_on == redo_off
    assert err < 2e-5, err
    assert others_equal(on, clean, L)
    b, h = LOUD
    assert not torch.equal(bits(on[b * L:(b + 1) * L, cols(h)]), bits(clean[b * L:(b + 1) * L, cols(h)]))    # (the case did change something)


@pytest.mark.parametrize("L", LENGTHS)
def test_non_finite_tile_norm_stays_general(G, L, monkeypatch):
    on, redo_on, ws = run(G, "inf", L, True, monkeypatch)
    off, redo_off, _ = run(G, "inf", L, False, monkeypatch)
    clean, _, _ = run(G, "flat", L, True, monkeypatch)
    print(f"inf L={L}: redo={redo_on}/{redo_off}")
    assert torch.equal(bits(on), bits(off))
    assert redo_on == redo_off                # (the general loop counts its attempts on the inf; a lean loop would count none)
    assert others_equal(on, clean, L)
    rec = stats_records(ws, L)
    assert rec[LOUD[1] * B + LOUD[0], 5].view(torch.int32).item() == 1
    assert int((rec[:, 5].view(torch.int32) != 0).sum()) == 1


def stats_records(ws, L):
    """the (H * B, 8) float records behind the K / V images, the key sums and the tile norms (layout: include/gsdd.h)"""
    rows = B * L * H
    ntile = (rows + 31) // 32
    off = (rows * 64 + ntile * 20 + 31) // 32 * 32
    return ws[off // 4:off // 4 + 8 * B * H].view(H * B, 8)


@pytest.mark.parametrize("L", LENGTHS)
def test_stats_records_are_the_reductions_of_their_own_bh(G, L, monkeypatch):
    """Record h * B + b against the workspace's own tile norms and key sums: the largest tile norm bit for bit (a maximum has no
    rounding), the flag clear, the key sum within the float summation bound gamma(128) of an fp64 sum of the same float4s, the padding 0.
    With one loud (b, h) a record filed under the wrong pair is off by a factor of 80."""
    _, _, ws = run(G, "loud", L, True, monkeypatch)
    rows = B * L * H
    ntile = rows // 32
    ksum = ws[rows * 16:rows * 16 + 4 * ntile].view(H, B, L // 32, 4)
    knorm = ws[rows * 16 + 4 * ntile:rows * 16 + 5 * ntile].view(H, B, L // 32)
    rec = stats_records(ws, L).view(H, B, 8)
    assert torch.equal(bits(rec[..., 4]), bits(knorm.amax(dim=-1)))
    assert not rec[..., 5:].view(torch.int32).any()
    want = ksum.double().sum(dim=2)
    bound = (L // 32) * 2.0 ** -24 * 1.01 * ksum.double().abs().sum(dim=2) + 1e-30
    assert bool(((rec[..., :4].double() - want).abs() <= bound).all())
    loud = knorm.amax(dim=-1)[LOUD[1], LOUD[0]].item()
    assert loud > 20 * knorm.amax(dim=-1).min().item()


def test_workspace_one_byte_short_is_rejected(G):
    """The records live at the end of the workspace: a buffer of the old size (or one byte short of the new) must fail the size check,
    not be read past its end.  The check precedes every launch."""
    from gsdd_amd import _lib as abi
    L = 416
    lib = G.lib()
    need = lib.gsdd_d3pm_attention_workspace_bytes(B, L, H)
    rows = B * L * H
    assert need >= rows * 64 + (rows // 32) * 20 + B * H * 32
    q, k, v, _ = reference("flat", L)
    qd, kd, vd = hm(q), hm(k), hm(v)
    out = torch.zeros((B * L, H * 4), device="cuda")
    ws = torch.zeros((need,), dtype=torch.uint8, device="cuda")
    for kk, vv in ((kd, vd), (None, None)):
        rc = lib.gsdd_d3pm_attention(abi.ptr(qd), abi.ptr(kk), abi.ptr(vv), B, L, H, abi.ptr(out), abi.ptr(ws), ctypes.c_int64(need - 1),
                                     None, abi.ATTN_A8, abi.stream_ptr())
        assert rc != 0 and "workspace too small" in lib.gsdd_last_error().decode()
    with pytest.raises(G.GsddError, match="workspace too small"):
        G.ops.d3pm_attention(qd, kd, vd, B, L, H, out, ws=ws[:need - need % 4 - 4].view(torch.float32), mode="a8")
    torch.cuda.synchronize()
    assert not out.any() and not ws.any()     # nothing was launched
    abi.check(lib.gsdd_d3pm_attention(abi.ptr(qd), abi.ptr(kd), abi.ptr(vd), B, L, H, abi.ptr(out), abi.ptr(ws), ctypes.c_int64(need), None,
                                      abi.ATTN_A8, abi.stream_ptr()))
    torch.cuda.synchronize()
    assert out.any()
