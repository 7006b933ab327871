"""Registers of the training cross-attention kernels (csrc/d3pm_cross.hip) as hipcc reports them for gfx950: Te is a run-time loop bound
in every one of them, so one compile covers every Te -- no scratch and no spills, the backward's main kernels (dq, and the dK / dV
partials) at two waves per SIMD or more; the figures are the ones recorded in profiles/rH_cross_train_kernel_resources.csv."""
import csv
import importlib.util
import os
import shutil

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not installed")

KERNELS = {"cross_train_fwd_kernel", "cross_bwd_dq_kernel", "cross_bwd_dkv_kernel", "cross_bwd_reduce_kernel"}


@pytest.fixture(scope="module")
def cross_rows():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "d3pm_cross.hip" in mod.SOURCES
    return {r["kernel"]: r for r in mod.collect(["d3pm_cross.hip"])}


def test_no_kernel_is_templated_on_te():
    src = open(os.path.join(REPO, "gif-synthesis-with-discrete-diffusion_amd", "csrc", "d3pm_cross.hip")).read()
    assert "template" not in src


def test_every_kernel_has_no_scratch_and_no_spills(cross_rows):
    assert set(cross_rows) == KERNELS                # every kernel of the file, and nothing else
    for k, r in cross_rows.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["vgprs"] <= 256, r
    for k in ("cross_bwd_dq_kernel", "cross_bwd_dkv_kernel"):
        assert cross_rows[k]["occupancy_waves_per_simd"] >= 2, cross_rows[k]


def test_recorded_figures_are_the_compile_s(cross_rows):
    with open(os.path.join(REPO, "profiles", "rH_cross_train_kernel_resources.csv")) as f:
        recorded = {r["kernel"]: r for r in csv.DictReader(f)}
    assert set(recorded) == set(cross_rows)
    for k, b in recorded.items():
        assert all(cross_rows[k][c] == int(b[c]) for c in ("vgprs", "agprs", "scratch_bytes_per_lane", "vgpr_spill",
                                                           "occupancy_waves_per_simd")), (k, cross_rows[k])
