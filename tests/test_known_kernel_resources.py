"""Registers of the step kernel's families with known positions (d3pm_step_known_kernel, d3pm_step_known_trunc_kernel), as hipcc
reports them for gfx950: no scratch in any instantiation -- a known position keeps three scalars, an unknown one the rows of the plain
kernel -- and the plain and truncated families at the VGPR counts recorded before the families existed (profiles/r9_kernel_resources.csv)."""
import csv
import importlib.util
import os
import shutil

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not installed")


@pytest.fixture(scope="module")
def step_rows():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "d3pm_step.hip" in mod.SOURCES
    return {r["kernel"]: r for r in mod.collect(["d3pm_step.hip"])}


def test_known_families_have_no_scratch(step_rows):
    known = {k: r for k, r in step_rows.items() if k.startswith("d3pm_step_known")}
    want = {f"d3pm_step_known{fam}_kernel<{j}, {full}>" for fam in ("", "_trunc")
            for j, full in [(1, "false"), (2, "false"), (4, "false"), (8, "false"), (16, "false"), (16, "true"), (32, "false")]}
    assert set(known) == want                       # every width the host code launches, plain and truncated
    for k, r in known.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgprs"] <= 256, r
    for fam in ("", "_trunc"):                      # the production width keeps the plain production kernel's two waves per SIMD
        assert known[f"d3pm_step_known{fam}_kernel<16, true>"]["occupancy_waves_per_simd"] >= 2


def test_plain_and_truncated_families_keep_their_registers(step_rows):
    with open(os.path.join(REPO, "profiles", "r9_kernel_resources.csv")) as f:
        before = {r["kernel"]: r for r in csv.DictReader(f) if r["kernel"].startswith(("d3pm_step_kernel", "d3pm_step_trunc_kernel"))}
    assert len(before) == 39
    for k, b in before.items():
        assert k in step_rows, k
        assert step_rows[k]["vgprs"] == int(b["vgprs"]) and step_rows[k]["scratch_bytes_per_lane"] == int(b["scratch_bytes_per_lane"]), (k, step_rows[k])
    # the recorded figures of the new families are the compile's
    with open(os.path.join(REPO, "profiles", "r10_known_kernel_resources.csv")) as f:
        recorded = {r["kernel"]: r for r in csv.DictReader(f)}
    assert set(recorded) == {k for k in step_rows if k.startswith("d3pm_step_")}
    for k, b in recorded.items():
        assert all(step_rows[k][c] == int(b[c]) for c in ("vgprs", "agprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd")), (k, step_rows[k])
