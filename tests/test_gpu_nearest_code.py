"""gsdd_nearest_code -- the VQ-VAE tokenizer: the register-tiled vector kernel (any E % 4 == 0 up to 256, any K) and the matrix-core kernel
(E = 128, K % 32 == 0, the codebook split over workgroups and merged through 64-bit atomicMin keys kept in idx[] itself) -- against the fp64
first arg-min of the difference form d64[m][k] = sum_e (z[m][e] - cb[k][e])^2, at the shapes where the kernels' index arithmetic changes:
  * vector kernel: the pipelined staging (E <= 128) and the plain staging loop (128 < E <= 256, more than 64 KB of dynamic LDS), a last
    chunk with K % 64 != 0 (rows clamped to K - 1 and zero-filled when staged), K < 64, K = 1, E = 4 (64 of 256 threads stage), M = 1,
    M % 64 != 0;
  * matrix kernel: 1, 2, 3 and 5 tiles per split (K = 32, 96, 160, 192: the double buffer ends on either parity), 128 splits of one tile
    (K = 4096 at small M), nsplit == 1 because there are 1025 row blocks, M = 1, 31, 255, 256, 257.

Inputs, seeded per case: z = randn(M, E), cb = 0.7 randn(K, E) + 0.3 z[randint] (codes near latents: tight races).  Then
  * planted winners: every seam code c (0, 3, 4, 15, 16, 31, 32, 63, 64, the first code of the last 64-code chunk, K - 1 and, on the matrix
    kernel, the first and last code of every split) gets a row m_c of its own with cb[c] = z[m_c] + 0.01 randn -- as many of them, in that
    order, as there are rows;
  * one small-norm row z[m0] = 0.01 randn, which a zero-filled phantom code past K would win;
  * in the duplicate variants cb[c + delta] = cb[c] for c in (3, 16, first code of the last chunk) and delta in (4, 8, 32, 64,
    codes_per_split): lane halves of a tile, threads of a chunk, tiles of a split, chunks, splits.

Acceptance, per row (U = 2^-24): both kernels evaluate (|z|^2 - 2 z.e) + |e|^2 in f32; each of the three sums carries gamma_E of its sum
of absolute products and two more roundings follow, at most gamma_(E+2) (|z|^2 + 2 |z| |e| + |e|^2) in all:
bar(m, k) = (E + 3) U (|z_m| + |e_k|)^2.  A returned index g != want is accepted only if d64[m][g] - d64[m][want] <= 2 max(bar(m, g),
bar(m, want)); a row is *undecided* when its fp64 runner-up (the nearest code whose row is not bit-identical to the winner's) is within
that distance of the winner.  Exact assertions beside it: every planted row returns its planted code, no returned index names a code
that has a bit-identical earlier row (identical rows give bit-identical distances in either kernel, so the earlier one wins every
merge), 0 <= idx < K, zq == cb[idx] bit for bit, the rows behind M of idx (int64 -7) and zq (poison) unchanged.

The unmarked tests need no GPU: the share of undecided rows is <= 2 % in every case and every planted row is decided with its planted
code as the fp64 winner; a plain f32 torch restatement passes every assertion of every small case (the bars are not below f32's own
noise); and that restatement with one fault injected at a time is caught on the case named in FAULT_CASES (the assertions are not
vacuous).  The largest case (262,221 rows) meets the reference conditions on the CPU too; its GPU test makes the fp64 reference again on the
device, in row chunks.

NaN contract (both kernels): a row whose distances are all NaN gets index 0, a NaN code never wins.

Every GPU case records its undecided share, accepted mismatches, their worst ratio to the bar and (matrix kernel) nsplit with
tests.conftest.parity_report (nearest_code::*)."""
import functools
import math
import types

import pytest
import torch

from tests.conftest import parity_report

gpu = pytest.mark.gpu

U = 2.0 ** -24
IDX_SENT = -7
POISON = -7777.0
GUARD = 67
SEAMS = (0, 3, 4, 15, 16, 31, 32, 63, 64)
DUP_DELTAS = (4, 8, 32, 64)
BIG_M = 1024 * 256 + 77


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()
    return gsdd_amd


def matrix_nsplit(M, K):
    """the entry point's three-condition loop"""
    nrb = (M + 255) // 256
    nsplit = 1
    while nrb * nsplit < 1024 and nsplit * 2 <= K // 32 and (K // (nsplit * 2)) % 32 == 0:
        nsplit *= 2
    return nsplit


def case(kernel, E, K, M, dup=False):
    return types.SimpleNamespace(kernel=kernel, E=E, K=K, M=M, dup=dup, id=f"{kernel}_E{E}_K{K}_M{M}" + ("_dup" if dup else ""))


VECTOR_CASES = [case("vector", *s) for s in [(4, 5, 1), (4, 4096, 257), (8, 63, 65), (64, 64, 64), (64, 65, 63), (128, 1, 257), (128, 96, 257),
                                             (132, 65, 257), (132, 192, 64), (256, 64, 65), (256, 4096, 257)]]
VECTOR_CASES += [case("vector", 64, 192, 257, dup=True), case("vector", 256, 192, 257, dup=True)]
MATRIX_CASES = [case("matrix", 128, K, 257) for K in (32, 64, 96, 160, 192, 4096)]
MATRIX_CASES += [case("matrix", 128, 192, M) for M in (1, 31, 255, 256)]
MATRIX_CASES += [case("matrix", 128, 4096, 1)]
MATRIX_CASES += [case("matrix", 128, 192, 257, dup=True), case("matrix", 128, 4096, 257, dup=True)]
BIG_CASE = case("matrix", 128, 64, BIG_M)
SMALL_CASES = VECTOR_CASES + MATRIX_CASES
CASES = {c.id: c for c in SMALL_CASES + [BIG_CASE]}
# inputs made for the matrix kernel (E = 128, K % 32 == 0) that both kernels run
BOTH_CASES = ["matrix_E128_K64_M257", "matrix_E128_K96_M257", "matrix_E128_K192_M257", "matrix_E128_K192_M257_dup", "matrix_E128_K4096_M257",
              "matrix_E128_K4096_M1"]


def make_inputs(c):
    """-> z[M][E], cb[K][E] (f32, CPU), planted {code: row}, m0 (the small-norm row or None), nsplit (matrix kernel, else None)"""
    E, K, M = c.E, c.K, c.M
    g = torch.Generator().manual_seed(1000 * E + K)
    z = torch.randn(M, E, generator=g)
    cb = 0.7 * torch.randn(K, E, generator=g) + 0.3 * z[torch.randint(0, M, (K,), generator=g)]
    nsplit = matrix_nsplit(M, K) if c.kernel == "matrix" else None
    seams = list(SEAMS) + [64 * ((K - 1) // 64), K - 1]
    if nsplit is not None:
        cps = K // nsplit
        for s in range(nsplit):
            seams += [s * cps, s * cps + cps - 1]
    seams = list(dict.fromkeys(s for s in seams if s < K))
    rows = torch.randperm(M, generator=g).tolist()
    if M == 1:                                               # one row: it goes to the last code, behind every guard
        m0, seams = None, [K - 1]
    else:
        m0, rows = rows[0], rows[1:]
    planted = {}
    for code, m in zip(seams, rows):
        cb[code] = z[m] + 0.01 * torch.randn(E, generator=g)
        planted[code] = m
    if m0 is not None:
        z[m0] = 0.01 * torch.randn(E, generator=g)
    if c.dup:
        deltas = list(DUP_DELTAS) + ([K // nsplit] if nsplit is not None else [])
        for src in (3, 16, 64 * ((K - 1) // 64)):
            assert src in planted
            for d in dict.fromkeys(deltas):
                if src + d < K:
                    cb[src + d] = cb[src]
                    planted.pop(src + d, None)               # (a copy that lands on a seam code: that code no longer wins its row)
    return z, cb, planted, m0, nsplit


def reference(z, cb, chunk_elems=1 << 24):
    """fp64 difference-form distances on the device the inputs live on, one row chunk at a time, reduced to what the assertions need.
    -> namespace: want (first arg-min), dwant, gap_ru / bar_ru (runner-up among the codes not bit-identical to the winner: distance above
    the winner and max of the two bars; inf / 0 without one), nz, ne (fp64 norms), first (index of the first bit-identical row of a code),
    undecided (bool per row)."""
    M, E = z.shape
    K = cb.shape[0]
    dev = z.device
    z64, c64 = z.double(), cb.double()
    nz, ne = z64.norm(dim=1), c64.norm(dim=1)
    _, inv = torch.unique(cb, dim=0, return_inverse=True)
    ar = torch.arange(K, device=dev)
    first = torch.full((int(inv.max()) + 1,), K, device=dev, dtype=torch.int64).scatter_reduce(0, inv, ar, "amin")[inv]
    want = torch.empty(M, dtype=torch.int64, device=dev)
    dwant = torch.empty(M, dtype=torch.float64, device=dev)
    gap_ru = torch.full((M,), math.inf, dtype=torch.float64, device=dev)
    bar_ru = torch.zeros(M, dtype=torch.float64, device=dev)
    step = max(1, chunk_elems // (K * E))
    for a in range(0, M, step):
        b = min(M, a + step)
        d = (z64[a:b, None, :] - c64[None, :, :]).square_().sum(-1)                  # [rows][K]
        dmin = d.min(1, keepdim=True).values
        w = torch.where(d == dmin, ar[None, :], K).min(1).values                     # first minimum
        want[a:b], dwant[a:b] = w, dmin[:, 0]
        if K > 1:
            others = torch.where(first[None, :] == first[w][:, None], math.inf, d)
            dr, r = others.min(1)
            has = torch.isfinite(dr)
            bars = (E + 3) * U * torch.maximum((nz[a:b] + ne[r]) ** 2, (nz[a:b] + ne[w]) ** 2)
            gap_ru[a:b] = torch.where(has, dr - dmin[:, 0], math.inf)
            bar_ru[a:b] = torch.where(has, bars, 0.0)
    return types.SimpleNamespace(want=want, dwant=dwant, gap_ru=gap_ru, bar_ru=bar_ru, nz=nz, ne=ne, first=first,
                                 undecided=gap_ru <= 2 * bar_ru, z64=z64, c64=c64, E=E, K=K, M=M)


@functools.lru_cache(maxsize=None)
def small_case(cid):
    """inputs and fp64 reference of a small case, made once on the CPU and shared by every test (nothing writes them)"""
    c = CASES[cid]
    z, cb, planted, m0, nsplit = make_inputs(c)
    return types.SimpleNamespace(c=c, z=z, cb=cb, planted=planted, m0=m0, nsplit=nsplit, ref=reference(z, cb))


def reference_conditions(ref, planted):
    """the conditions on the reference alone -> (undecided share, list of violated conditions)"""
    share = float(ref.undecided.double().mean())
    bad = []
    if share > 0.02:
        bad.append(f"undecided share {share:.4f} > 0.02")
    for code, m in planted.items():
        if int(ref.want[m]) != code:
            bad.append(f"planted row {m}: fp64 winner {int(ref.want[m])}, planted {code}")
        if bool(ref.undecided[m]):
            bad.append(f"planted row {m} (code {code}) is undecided")
    return share, bad


def judge(ref, planted, idx):
    """the assertions on a returned index vector -> (list of violations, accepted mismatches, their worst ratio to the bar)"""
    bad = []
    idx = idx.to(ref.want.device)
    if not bool(((idx >= 0) & (idx < ref.K)).all()):
        return [f"index out of range: min {int(idx.min())}, max {int(idx.max())}, K {ref.K}"], 0, math.inf
    for code, m in planted.items():
        if int(idx[m]) != code:
            bad.append(f"planted row {m}: got {int(idx[m])}, planted {code}")
    later = ref.first[idx] != idx
    if bool(later.any()):
        m = int(later.nonzero()[0])
        bad.append(f"{int(later.sum())} rows name a code with a bit-identical earlier row (row {m}: {int(idx[m])}, first {int(ref.first[idx[m]])})")
    mm = (idx != ref.want).nonzero()[:, 0]
    worst = 0.0
    if mm.numel():
        g = idx[mm]
        dg = (ref.z64[mm] - ref.c64[g]).square().sum(1)
        bars = (ref.E + 3) * U * torch.maximum((ref.nz[mm] + ref.ne[g]) ** 2, (ref.nz[mm] + ref.ne[ref.want[mm]]) ** 2)
        ratio = (dg - ref.dwant[mm]) / (2 * bars)
        worst = float(ratio.max())
        if worst > 1:
            m = int(mm[ratio.argmax()])
            bad.append(f"{int((ratio > 1).sum())} mismatches beyond the bar (row {m}: got {int(idx[m])}, want {int(ref.want[m])}, "
                       f"{worst:.3g} x the bar)")
    return bad, int(mm.numel()), worst


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_kernel(G, z, cb, matrix, with_zq=True):
    """-> idx[M], zq[M][E] or None, whether the rows behind M of both are unchanged"""
    M, E = z.shape
    ibuf = torch.full((M + GUARD,), IDX_SENT, dtype=torch.int64, device="cuda")
    zbuf = torch.full((M + GUARD, E), POISON, device="cuda") if with_zq else None
    G.ops.nearest_code(z, cb, ibuf[:M], zbuf[:M] if with_zq else None, matrix=matrix)
    torch.cuda.synchronize()
    intact = bool((ibuf[M:] == IDX_SENT).all()) and (not with_zq or bool((zbuf[M:] == POISON).all()))
    return ibuf[:M], (zbuf[:M] if with_zq else None), intact


def gpu_case(G, cid, matrix, ref=None, inputs=None, tag=None):
    """run one case through one kernel, with and without zq, record, and assert everything -> idx"""
    if inputs is None:
        sc = small_case(cid)
        z, cb, planted, nsplit, ref = sc.z.cuda(), sc.cb.cuda(), sc.planted, sc.nsplit, sc.ref
    else:
        z, cb, planted, nsplit = inputs
    idx, zq, intact = run_kernel(G, z, cb, matrix)
    idx2, _, intact2 = run_kernel(G, z, cb, matrix, with_zq=False)
    share, cond = reference_conditions(ref, planted)
    bad, n_mm, worst = judge(ref, planted, idx)
    rec = {"undecided_share": share, "undecided_rows": int(ref.undecided.sum()), "accepted_mismatches": n_mm if not bad else -1,
           "mismatches": n_mm, "worst_ratio": worst, "planted": len(planted)}
    if matrix:
        rec["nsplit"] = nsplit
    parity_report(f"nearest_code::{tag or cid}", rec)
    assert not cond, cond
    assert not bad, bad
    assert bits_equal(zq, cb[idx]), "zq != cb[idx]"
    assert torch.equal(idx, idx2), "the call without zq returns other indices"
    assert intact and intact2, "rows behind M of idx or zq were written"
    return idx


# ----------------------------------------------------------------------------- GPU
@gpu
@pytest.mark.parametrize("cid", [c.id for c in VECTOR_CASES])
def test_vector_kernel_matches_fp64(G, cid):
    """the register-tiled kernel; E > 128 takes the plain staging loop and 133 KB of dynamic LDS"""
    gpu_case(G, cid, matrix=False)


@gpu
@pytest.mark.parametrize("cid", [c.id for c in MATRIX_CASES])
def test_matrix_kernel_matches_fp64(G, cid):
    c = CASES[cid]
    assert c.E == 128 and c.K % 32 == 0                                             # the entry point's condition for the matrix kernel
    gpu_case(G, cid, matrix=True)


@gpu
def test_matrix_kernel_single_split_by_row_blocks(G):
    """K = 64 at 1025 row blocks: nsplit == 1 although the codebook has two tiles; the fp64 reference is made on the device in row chunks
    and held to the same conditions as the CPU test holds the small cases to"""
    c = BIG_CASE
    z, cb, planted, m0, nsplit = make_inputs(c)
    assert nsplit == 1 and (c.M + 255) // 256 == 1025
    z, cb = z.cuda(), cb.cuda()
    ref = reference(z, cb, chunk_elems=1 << 27)
    gpu_case(G, c.id, matrix=True, ref=ref, inputs=(z, cb, planted, nsplit))


@gpu
@pytest.mark.parametrize("cid", BOTH_CASES)
def test_both_kernels_differ_only_on_undecided_rows(G, cid):
    sc = small_case(cid)
    z, cb = sc.z.cuda(), sc.cb.cuda()
    idx_m = gpu_case(G, cid, matrix=True, tag=cid + "[both:matrix]")
    idx_v = gpu_case(G, cid, matrix=False, tag=cid + "[both:vector]")
    differ = (idx_m != idx_v).cpu()
    parity_report(f"nearest_code::{cid}[both]", {"kernels_differ": int(differ.sum()), "undecided_rows": int(sc.ref.undecided.sum())})
    assert not bool((differ & ~sc.ref.undecided).any()), differ.nonzero()[:, 0].tolist()


@gpu
@pytest.mark.parametrize("matrix", [False, True], ids=["vector", "matrix"])
def test_nan_contract(G, matrix):
    """E = 128, K = 64, M = 70.  A row with one NaN element and a row of all NaN return index 0 and zq = cb[0]; a code holding a NaN (a code
    other than 0, then code 0, each the winner of a planted row) is never returned for a finite row: its planted row returns the fp64
    winner among the remaining codes under the acceptance rule; no other row changes against the run without NaNs."""
    c = case("matrix", 128, 64, 70)
    z, cb, planted, m0, nsplit = make_inputs(c)
    zd, cd = z.cuda(), cb.cuda()
    base, _, _ = run_kernel(G, zd, cd, matrix)
    base = base.clone()
    bad, _, _ = judge(reference(z, cb), planted, base)
    assert not bad, bad
    # NaN rows
    free = [m for m in range(c.M) if m not in planted.values() and m != m0]
    r1, rall = free[0], free[1]
    z2 = zd.clone()
    z2[r1, 77] = math.nan
    z2[rall] = math.nan
    idx, zq, intact = run_kernel(G, z2, cd, matrix)
    assert int(idx[r1]) == 0 and int(idx[rall]) == 0, (int(idx[r1]), int(idx[rall]))
    assert bits_equal(zq, cd[idx]) and intact
    keep = torch.ones(c.M, dtype=torch.bool, device="cuda")
    keep[[r1, rall]] = False
    assert torch.equal(idx[keep], base[keep]), "a NaN row changed other rows"
    # NaN codes
    for code in (31, 0):
        row = planted[code]
        assert int(base[row]) == code
        cb2 = cb.clone()
        cb2[code, 5] = math.nan
        rest = [k for k in range(c.K) if k != code]
        ref = reference(z, cb[rest])                                                # the reference never sees the NaN code
        back = torch.tensor(rest)
        idx, zq, intact = run_kernel(G, zd, cb2.cuda(), matrix)
        idx = idx.cpu()
        assert not bool((idx == code).any()), "a NaN code was returned"
        pos = torch.full((c.K,), -1, dtype=torch.int64)
        pos[back] = torch.arange(len(rest))
        bad, n_mm, worst = judge(ref, {}, pos[idx])
        assert not bad, bad
        others = base.cpu() != code
        assert torch.equal(idx[others], base.cpu()[others]), "a NaN code changed rows it had not won"
        assert int(others.sum()) < c.M
        assert bits_equal(zq.cpu()[others], cb[idx[others]]) and intact
        parity_report(f"nearest_code::nan_code{code}[{'matrix' if matrix else 'vector'}]",
                      {"row": row, "returned": int(idx[row]), "fp64_runner_up": int(back[ref.want[row]]), "accepted_mismatches": n_mm, "worst_ratio": worst})


# ----------------------------------------------------------------------------- no GPU: the reference's own conditions
@pytest.mark.parametrize("cid", [c.id for c in SMALL_CASES])
def test_cpu_reference_conditions(cid):
    """undecided rows <= 2 % of the case; every planted row decided, its fp64 winner the planted code; the small-norm row is nearer to
    the origin than to any code (a zero phantom code would win it)"""
    sc = small_case(cid)
    share, bad = reference_conditions(sc.ref, sc.planted)
    assert not bad, bad
    c = sc.c
    if c.M > 1:
        seams = [s for s in SEAMS + (64 * ((c.K - 1) // 64), c.K - 1) if s < c.K]
        n = min(c.M - 1, len(dict.fromkeys(seams)))
        assert len(sc.planted) >= n and all(s in sc.planted for s in list(dict.fromkeys(seams))[:n])
        assert float(sc.ref.nz[sc.m0]) ** 2 < float(sc.ref.dwant[sc.m0])
    if c.kernel == "matrix":
        assert sc.nsplit == matrix_nsplit(c.M, c.K) and c.K % (32 * sc.nsplit) == 0


def test_cpu_reference_conditions_of_the_largest_case():
    """the same conditions for the 262,221-row case (not kept: its GPU test makes the reference again, on the device)"""
    z, cb, planted, m0, nsplit = make_inputs(BIG_CASE)
    ref = reference(z, cb, chunk_elems=1 << 25)
    share, bad = reference_conditions(ref, planted)
    assert not bad, bad
    assert nsplit == 1 and len(planted) == 8 and float(ref.nz[m0]) ** 2 < float(ref.dwant[m0])


def test_cpu_nsplit_of_the_matrix_cases():
    """the cases reach what they are listed for: 1, 2, 3 and 5 tiles per split, 128 splits of one tile, one split by row blocks"""
    tiles = {(K, M): (matrix_nsplit(M, K), K // 32 // matrix_nsplit(M, K)) for K, M in
             [(32, 257), (64, 257), (96, 257), (160, 257), (192, 257), (4096, 257), (4096, 1), (64, BIG_M)]}
    assert tiles == {(32, 257): (1, 1), (64, 257): (2, 1), (96, 257): (1, 3), (160, 257): (1, 5), (192, 257): (2, 3),
                     (4096, 257): (128, 1), (4096, 1): (128, 1), (64, BIG_M): (1, 2)}


# ----------------------------------------------------------------------------- no GPU: f32 restatement and injected faults
def f32_restatement(sc, fault=None):
    """((z z).sum - 2 z cb^T) + (cb cb).sum in plain f32 torch, first arg-min; with `fault`, one of the errors the kernels could make"""
    z, cb, K = sc.z, sc.cb, sc.c.K
    en = (cb * cb).sum(1)
    if fault == "no_code_norm":
        en = torch.zeros_like(en)
    d = ((z * z).sum(1, keepdim=True) - 2 * z @ cb.t()) + en[None, :]
    nsplit = sc.nsplit or 1
    cps = K // nsplit
    if fault == "drop_chunk_tail":                           # the last K % 64 codes never compete
        d[:, K - K % 64:] = math.inf
    elif fault == "drop_last_tile":                          # the last 32-code tile of every split never competes
        for s in range(nsplit):
            d[:, (s + 1) * cps - 32:(s + 1) * cps] = math.inf
    elif fault == "phantom_code":                            # a zero-filled code at index K competes
        d = torch.cat([d, (z * z).sum(1, keepdim=True)], 1)
    if fault == "later_tie":
        return d.shape[1] - 1 - d.flip(1).argmin(1)
    if fault == "merge_by_index":                            # the split merge takes the smallest index, not the smallest distance
        return d[:, :cps].argmin(1)
    return d.argmin(1)


@pytest.mark.parametrize("cid", [c.id for c in SMALL_CASES])
def test_cpu_f32_restatement_passes(cid):
    sc = small_case(cid)
    idx = f32_restatement(sc)
    bad, n_mm, worst = judge(sc.ref, sc.planted, idx)
    assert not bad, bad
    assert worst <= 1


# which case catches which fault
FAULT_CASES = [("drop_chunk_tail", "vector_E64_K65_M63"), ("drop_chunk_tail", "vector_E128_K96_M257"),
               ("drop_last_tile", "matrix_E128_K96_M257"), ("drop_last_tile", "matrix_E128_K192_M31"),
               ("later_tie", "vector_E64_K192_M257_dup"), ("later_tie", "vector_E256_K192_M257_dup"),
               ("later_tie", "matrix_E128_K192_M257_dup"), ("later_tie", "matrix_E128_K4096_M257_dup"),
               ("no_code_norm", "vector_E8_K63_M65"), ("no_code_norm", "matrix_E128_K160_M257"),
               ("phantom_code", "vector_E8_K63_M65"), ("phantom_code", "vector_E132_K65_M257"),
               ("merge_by_index", "matrix_E128_K192_M257"), ("merge_by_index", "matrix_E128_K4096_M1")]


@pytest.mark.parametrize("fault,cid", FAULT_CASES)
def test_cpu_injected_fault_is_caught(fault, cid):
    sc = small_case(cid)
    bad, _, _ = judge(sc.ref, sc.planted, f32_restatement(sc, fault))
    assert bad, f"{fault} passes every assertion of {cid}"
