"""Registers of the condition-dropout kernels (d3pm_cond.hip: cond_dropout_kernel, cond_null_grad_kernel) as hipcc reports them for
gfx950: no scratch in either, and the figures are the ones recorded in profiles/rJ_cond_kernel_resources.csv."""
import csv
import importlib.util
import os
import shutil

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not installed")

LAUNCHED = {"cond_dropout_kernel", "cond_null_grad_kernel"}


@pytest.fixture(scope="module")
def cond_rows():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "d3pm_cond.hip" in mod.SOURCES
    return {r["kernel"]: r for r in mod.collect(["d3pm_cond.hip"])}


def test_both_kernels_have_no_scratch(cond_rows):
    assert set(cond_rows) == LAUNCHED              # the two kernels the host code launches, and nothing else in the file
    for k, r in cond_rows.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["vgprs"] <= 128 and r["static_lds_bytes"] == 0, r


def test_recorded_figures_are_the_compile_s(cond_rows):
    with open(os.path.join(REPO, "profiles", "rJ_cond_kernel_resources.csv")) as f:
        recorded = {r["kernel"]: r for r in csv.DictReader(f)}
    assert set(recorded) == set(cond_rows)
    for k, b in recorded.items():
        assert all(cond_rows[k][c] == int(b[c]) for c in ("vgprs", "agprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd")), (k, cond_rows[k])
