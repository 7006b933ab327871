"""Registers, scratch and LDS of the GIF export's delta stage (csrc/gif_delta.hip) as hipcc reports them for gfx950: the kernel in its
two forms (exact, and with a tolerance: the only one that reads the clips), no scratch and no spills (the displayed colour of a thread's
four pixels stays in registers across the frames), the 5 KB table of rectangles and counts in LDS, few enough registers for eight waves
per SIMD, and the figures recorded in profiles/rU_gif_delta_kernel_resources.csv are the compile's."""
import csv
import importlib.util
import os
import shutil

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = {"gif_delta_kernel<false>", "gif_delta_kernel<true>"}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not installed")


@pytest.fixture(scope="module")
def rows():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return {r["kernel"]: r for r in mod.collect(["gif_delta.hip"])}


def test_kernel_set_without_scratch(rows):
    assert set(rows) == KERNELS
    for k, r in rows.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["agprs"] == 0, r
        assert r["static_lds_bytes"] == 5 * 256 * 4 and r["vgprs"] <= 64 and r["occupancy_waves_per_simd"] == 8, r
    assert rows["gif_delta_kernel<false>"]["vgprs"] < rows["gif_delta_kernel<true>"]["vgprs"]     # the exact form carries no pixel floats


def test_recorded_figures_are_the_compiles(rows):
    with open(os.path.join(REPO, "profiles", "rU_gif_delta_kernel_resources.csv")) as f:
        recorded = {r["kernel"]: r for r in csv.DictReader(f)}
    assert set(recorded) == KERNELS
    for k, b in recorded.items():
        assert all(rows[k][c] == int(b[c]) for c in ("vgprs", "agprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd",
                                                     "static_lds_bytes")), (k, rows[k])
