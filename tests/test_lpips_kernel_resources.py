"""Registers, scratch and LDS of the two LPIPS kernels (csrc/lpips.hip) as hipcc reports them for gfx950: the kernel set, no scratch, no
spills and no AGPRs, the 3 x 256 table of the stem kernel and the four waves' doubles of the distance kernel in LDS, occupancies that
leave both kernels memory-bound, and the figures recorded in profiles/rW_lpips_kernel_resources.csv are the compile's."""
import csv
import importlib.util
import os
import shutil

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = {"lpips_stem_rows_kernel", "lpips_layer_distance_kernel"}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not installed")


@pytest.fixture(scope="module")
def rows():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return {r["kernel"]: r for r in mod.collect(["lpips.hip"])}


def test_kernel_set_without_scratch(rows):
    assert set(rows) == KERNELS
    for k, r in rows.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["agprs"] == 0, r
    assert rows["lpips_stem_rows_kernel"]["static_lds_bytes"] == 3 * 256 * 4
    assert rows["lpips_layer_distance_kernel"]["static_lds_bytes"] == 4 * 8                       # one double per wave
    assert rows["lpips_stem_rows_kernel"]["vgprs"] <= 32 and rows["lpips_stem_rows_kernel"]["occupancy_waves_per_simd"] == 8
    # two positions' float4s of both operands in flight (the loop is unrolled twice) and still six waves a SIMD or more
    assert rows["lpips_layer_distance_kernel"]["vgprs"] <= 80 and rows["lpips_layer_distance_kernel"]["occupancy_waves_per_simd"] >= 6


def test_recorded_figures_are_the_compiles(rows):
    with open(os.path.join(REPO, "profiles", "rW_lpips_kernel_resources.csv")) as f:
        recorded = {r["kernel"]: r for r in csv.DictReader(f)}
    assert set(recorded) == KERNELS
    for k, b in recorded.items():
        assert all(rows[k][c] == int(b[c]) for c in ("vgprs", "agprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd",
                                                     "static_lds_bytes")), (k, rows[k])
