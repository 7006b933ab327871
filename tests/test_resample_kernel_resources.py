"""Registers of the forward-jump kernel (d3pm_forward_jump_kernel, RePaint's resampling) as hipcc reports them for gfx950: no scratch
in any instantiation the host code launches -- the kernel keeps three scalars and the draw's running best, no row -- and the production
width at two waves per SIMD or more; the figures are the ones recorded in profiles/rG_resample_kernel_resources.csv."""
import csv
import importlib.util
import os
import shutil

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not installed")

LAUNCHED = {f"d3pm_forward_jump_kernel<{j}, {full}>"
            for j, full in [(1, "false"), (2, "false"), (4, "false"), (8, "false"), (16, "false"), (16, "true"), (32, "false")]}


@pytest.fixture(scope="module")
def jump_rows():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "d3pm_jump.hip" in mod.SOURCES
    return {r["kernel"]: r for r in mod.collect(["d3pm_jump.hip"])}


def test_every_launched_instantiation_has_no_scratch(jump_rows):
    assert set(jump_rows) == LAUNCHED              # every width the host code launches, and nothing else in the file
    for k, r in jump_rows.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["vgprs"] <= 256, r
    assert jump_rows["d3pm_forward_jump_kernel<16, true>"]["occupancy_waves_per_simd"] >= 2


def test_recorded_figures_are_the_compile_s(jump_rows):
    with open(os.path.join(REPO, "profiles", "rG_resample_kernel_resources.csv")) as f:
        recorded = {r["kernel"]: r for r in csv.DictReader(f)}
    assert set(recorded) == set(jump_rows)
    for k, b in recorded.items():
        assert all(jump_rows[k][c] == int(b[c]) for c in ("vgprs", "agprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd")), (k, jump_rows[k])
