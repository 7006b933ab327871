"""The sampler's production layer and attention kernels compile for gfx950 without scratch (register spills).

A spill costs a store and a reload through the memory hierarchy for every lane of every wave: in the fused layer kernel it was 260 B per
lane, 34 MB written per launch.  hipcc reports the figure at compile time, so this needs no GPU."""
import importlib.util
import os
import shutil

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not installed")


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def resources():
    return _tool().collect()


def _production(rows, name):
    got = [r for r in rows if r["kernel"].startswith(name)]
    assert got, f"no {name} instantiation in the compile"
    return got


def test_layer_h2_kernels_have_no_scratch(resources):
    rows = _production(resources, "d3pm_layer_h2_kernel")
    assert len(rows) == 3
    for r in rows:
        assert r["scratch_bytes_per_lane"] == 0, r
        assert r["vgprs"] <= 256 and r["occupancy_waves_per_simd"] >= 2, r


def test_attention_kernels_have_no_scratch(resources):
    for r in _production(resources, "d3pm_attention_v4_kernel"):
        assert r["scratch_bytes_per_lane"] == 0, r
