"""Registers, scratch and occupancy of the composed-guidance kernel (csrc/d3pm_compose.hip) as hipcc reports them for gfx950: the exact
kernel set -- one instantiation per class width J = 1, 2, 4, 8, 16, 32 and the FULL one of K = 4096 --, no scratch, no spills and no
AGPRs at any width, at least two waves per SIMD wherever a position's three rows live in registers (J <= 16; J = 32 runs two passes
and holds one row), and the figures recorded in profiles/rY_compose_kernel_resources.csv are the compile's."""
import csv
import importlib.util
import os
import shutil

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = {f"d3pm_compose_kernel<{J}, false>" for J in (1, 2, 4, 8, 16, 32)} | {"d3pm_compose_kernel<16, true>"}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not installed")


@pytest.fixture(scope="module")
def rows():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return {r["kernel"]: r for r in mod.collect(["d3pm_compose.hip"])}


def width(kernel):
    return int(kernel.split("<")[1].split(",")[0])


def test_kernel_set_without_scratch(rows):
    assert set(rows) == KERNELS
    for k, r in rows.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["agprs"] == 0, r
        assert r["static_lds_bytes"] == 0, r                      # the wave reductions are shuffles
        assert r["vgprs"] <= 256, r
        if width(k) <= 16:
            assert r["occupancy_waves_per_simd"] >= 2, r
    # three live rows of 4 J registers each are what the one-pass widths cost; the two-pass J = 32 holds one row
    assert rows["d3pm_compose_kernel<16, true>"]["vgprs"] >= 192 and rows["d3pm_compose_kernel<32, false>"]["vgprs"] >= 128
    assert rows["d3pm_compose_kernel<32, false>"]["occupancy_waves_per_simd"] >= 2


def test_recorded_figures_are_the_compiles(rows):
    with open(os.path.join(REPO, "profiles", "rY_compose_kernel_resources.csv")) as f:
        recorded = {r["kernel"]: r for r in csv.DictReader(f)}
    assert set(recorded) == KERNELS
    for k, b in recorded.items():
        assert all(rows[k][c] == int(b[c]) for c in ("vgprs", "agprs", "scratch_bytes_per_lane", "vgpr_spill", "occupancy_waves_per_simd",
                                                     "static_lds_bytes")), (k, rows[k])
