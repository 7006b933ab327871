"""Registers, scratch and LDS of the GIF compositor (csrc/gif_read.hip) as hipcc reports them for gfx950: exactly one kernel, no scratch
and no spills (the per-pixel state of a thread's four pixels stays in registers), no LDS, few enough registers for eight waves per
SIMD (the walk over the frames is a chain of dependent loads that only other waves hide), and the figures recorded in
profiles/rR_gif_read_kernel_resources.csv are the compile's."""
import csv
import importlib.util
import os
import shutil

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = {"gif_compose_kernel"}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not installed")


@pytest.fixture(scope="module")
def rows():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return {r["kernel"]: r for r in mod.collect(["gif_read.hip"])}


def test_one_kernel_without_scratch(rows):
    assert set(rows) == KERNELS
    r = rows["gif_compose_kernel"]
    assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["agprs"] == 0 and r["static_lds_bytes"] == 0, r
    assert r["vgprs"] <= 64 and r["occupancy_waves_per_simd"] == 8, r


def test_recorded_figures_are_the_compiles(rows):
    with open(os.path.join(REPO, "profiles", "rR_gif_read_kernel_resources.csv")) as f:
        recorded = {r["kernel"]: r for r in csv.DictReader(f)}
    assert set(recorded) == KERNELS
    for k, b in recorded.items():
        assert all(rows[k][c] == int(b[c]) for c in ("vgprs", "agprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd",
                                                     "static_lds_bytes")), (k, rows[k])
