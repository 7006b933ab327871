"""Registers of the optimiser stage's kernels (csrc/optim.hip) as hipcc reports them for gfx950: the four streaming kernels compile
without scratch and without spills, at full occupancy, and the figures are the ones recorded in profiles/rO_optim_kernel_resources.csv."""
import csv
import importlib.util
import os
import shutil

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not installed")

KERNELS = {"grad_sqnorm_kernel", "grad_norm_finalize_kernel", "adamw_ema_multi_kernel", "swap_multi_kernel"}


@pytest.fixture(scope="module")
def optim_rows():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "optim.hip" in mod.SOURCES
    return {r["kernel"]: r for r in mod.collect(["optim.hip"])}


def test_the_four_kernels_have_no_scratch(optim_rows):
    assert set(optim_rows) == KERNELS                  # the four kernels, and nothing else in the file
    for k, r in optim_rows.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["agprs"] == 0, r
        assert r["vgprs"] <= 64 and r["occupancy_waves_per_simd"] == 8, r          # streaming kernels: latency is hidden by waves
    assert optim_rows["adamw_ema_multi_kernel"]["static_lds_bytes"] == 0 and optim_rows["swap_multi_kernel"]["static_lds_bytes"] == 0
    assert optim_rows["grad_sqnorm_kernel"]["static_lds_bytes"] == 32          # the reduction's four doubles, nothing else


def test_recorded_figures_are_the_compile_s(optim_rows):
    with open(os.path.join(REPO, "profiles", "rO_optim_kernel_resources.csv")) as f:
        recorded = {r["kernel"]: r for r in csv.DictReader(f)}
    assert set(recorded) == set(optim_rows)
    for k, b in recorded.items():
        assert all(optim_rows[k][c] == int(b[c]) for c in ("vgprs", "agprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd")), (k, optim_rows[k])
