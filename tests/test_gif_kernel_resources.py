"""Registers, scratch and LDS of the GIF quantiser's kernels (csrc/gif.hip) as hipcc reports them for gfx950: exactly three kernels, no
scratch and no spills, the box-sum kernel's table and per-wave accumulators and the map kernel's palette inside the 64 KiB a
workgroup may declare statically, the histogram kernel's 32768 dynamic counters inside the 160 KiB of a CU, and the figures recorded
in profiles/rQ_gif_kernel_resources.csv are the compile's."""
import csv
import importlib.util
import os
import re
import shutil

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = {"gif_histogram_kernel", "gif_box_sums_kernel", "gif_map_kernel"}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not installed")


@pytest.fixture(scope="module")
def gif_rows():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return {r["kernel"]: r for r in mod.collect(["gif.hip"])}


def test_gif_kernels_have_no_scratch(gif_rows):
    assert set(gif_rows) == KERNELS
    for k, r in gif_rows.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["agprs"] == 0, r
    # sixteen waves of the histogram workgroup on four SIMDs: four waves per SIMD, at most 128 registers each
    assert gif_rows["gif_histogram_kernel"]["vgprs"] <= 128 and gif_rows["gif_histogram_kernel"]["occupancy_waves_per_simd"] >= 4


def test_gif_lds_fits(gif_rows):
    # static: the 32 KiB bin -> box table and four [256][4] uint32 accumulator images; the 256 packed palette entries
    assert gif_rows["gif_box_sums_kernel"]["static_lds_bytes"] == 32768 + 4 * 256 * 4 * 4 <= 64 * 1024
    assert gif_rows["gif_map_kernel"]["static_lds_bytes"] == 256 * 4
    # dynamic: the histogram's LDS is what the host wrapper asks for -- one uint32 per bin, opted in above 64 KiB
    assert gif_rows["gif_histogram_kernel"]["static_lds_bytes"] == 0
    with open(os.path.join(REPO, "gif-synthesis-with-discrete-diffusion_amd", "csrc", "gif.hip")) as f:
        src = f.read()
    assert re.search(r"const size_t lds = \(size_t\)GIF_BINS \* sizeof\(uint32_t\);", src)
    assert re.search(r"hipFuncSetAttribute\(\(const void\*\)gif_histogram_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, \(int\)lds\)", src)
    with open(os.path.join(REPO, "gif-synthesis-with-discrete-diffusion_amd", "csrc", "gif_host.hpp")) as f:
        bins = int(re.search(r"constexpr int BINS = (\d+);", f.read()).group(1))
    assert bins == 32768 and bins * 4 <= 160 * 1024


def test_recorded_figures_are_the_compiles(gif_rows):
    with open(os.path.join(REPO, "profiles", "rQ_gif_kernel_resources.csv")) as f:
        recorded = {r["kernel"]: r for r in csv.DictReader(f)}
    assert set(recorded) == KERNELS
    for k, b in recorded.items():
        assert all(gif_rows[k][c] == int(b[c]) for c in ("vgprs", "agprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd",
                                                         "static_lds_bytes")), (k, gif_rows[k])
