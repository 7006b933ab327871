"""Registers, scratch and LDS of the paired-metrics kernel (csrc/paired_metrics.hip) as hipcc reports them for gfx950: the kernel in its
two forms (with SSIM, and the squared error alone, which stages nothing), no scratch, no spills and no AGPRs, the levels and the
row sums of one tile in LDS as doubles -- 2 x 26 x 26 + 5 x 26 x 16 of them, plus the reduction's words --, and the figures recorded in
profiles/rV_paired_kernel_resources.csv are the compile's."""
import csv
import importlib.util
import os
import shutil

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = {"paired_metrics_kernel<false>", "paired_metrics_kernel<true>"}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not installed")


@pytest.fixture(scope="module")
def rows():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return {r["kernel"]: r for r in mod.collect(["paired_metrics.hip"])}


def test_kernel_set_without_scratch(rows):
    assert set(rows) == KERNELS
    for k, r in rows.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["agprs"] == 0, r
    reduction = 4 * 8 + 4 * 4                                   # one double and one word per wave
    assert rows["paired_metrics_kernel<true>"]["static_lds_bytes"] == (2 * 26 * 26 + 5 * 26 * 16) * 8 + reduction
    assert rows["paired_metrics_kernel<false>"]["static_lds_bytes"] <= 3 * 26 * 8 + reduction    # (one-row placeholders of the arrays)
    # 160 KB of LDS hold five workgroups of the SSIM form; the registers must not be what holds fewer than three waves a SIMD
    assert rows["paired_metrics_kernel<true>"]["vgprs"] <= 168 and rows["paired_metrics_kernel<true>"]["occupancy_waves_per_simd"] >= 3
    assert rows["paired_metrics_kernel<false>"]["vgprs"] <= 32 and rows["paired_metrics_kernel<false>"]["occupancy_waves_per_simd"] == 8


def test_recorded_figures_are_the_compiles(rows):
    with open(os.path.join(REPO, "profiles", "rV_paired_kernel_resources.csv")) as f:
        recorded = {r["kernel"]: r for r in csv.DictReader(f)}
    assert set(recorded) == KERNELS
    for k, b in recorded.items():
        assert all(rows[k][c] == int(b[c]) for c in ("vgprs", "agprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd",
                                                     "static_lds_bytes")), (k, rows[k])
