"""Registers of the long-clip kernels (d3pm_window_slide_kernel, clip_window_blend_kernel; csrc/d3pm_window.hip) as hipcc reports them
for gfx950: no scratch and no spills in any instantiation the host code launches, no LDS, and the figures are the ones recorded in
profiles/rX_window_kernel_resources.csv."""
import csv
import importlib.util
import os
import shutil

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not installed")

LAUNCHED = {"d3pm_window_slide_kernel", "clip_window_blend_kernel<false>", "clip_window_blend_kernel<true>"}


@pytest.fixture(scope="module")
def window_rows():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "d3pm_window.hip" in mod.SOURCES
    return {r["kernel"]: r for r in mod.collect(["d3pm_window.hip"])}


def test_every_launched_instantiation_has_no_scratch(window_rows):
    assert set(window_rows) == LAUNCHED            # what the host code launches, and nothing else in the file
    for k, r in window_rows.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["static_lds_bytes"] == 0 and r["agprs"] == 0, r
        assert r["vgprs"] <= 64 and r["occupancy_waves_per_simd"] >= 8, r          # elementwise kernels: full occupancy


def test_recorded_figures_are_the_compile_s(window_rows):
    with open(os.path.join(REPO, "profiles", "rX_window_kernel_resources.csv")) as f:
        recorded = {r["kernel"]: r for r in csv.DictReader(f)}
    assert set(recorded) == set(window_rows)
    for k, b in recorded.items():
        assert all(window_rows[k][c] == int(b[c]) for c in ("vgprs", "agprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd")), (k, window_rows[k])
