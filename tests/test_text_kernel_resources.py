"""Registers, scratch and LDS of the text tower's own kernels (csrc/text_tower.hip) as hipcc reports them for gfx950: no scratch and no
LDS, and the figures recorded in profiles/rD_text_kernel_resources.csv are the compile's.  The tower's attention kernel is
csrc/clip_attention.hip's (tests/test_clip_attention_kernel_resources.py)."""
import csv
import importlib.util
import os
import shutil

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = {"text_embed_kernel", "text_pool_kernel"}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not installed")


@pytest.fixture(scope="module")
def text_rows():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return {r["kernel"]: r for r in mod.collect(["text_tower.hip"])}


def test_text_kernels_have_no_scratch(text_rows):
    assert set(text_rows) == KERNELS
    for k, r in text_rows.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["vgprs"] <= 256, r
        assert r["static_lds_bytes"] == 0, r


def test_recorded_figures_are_the_compiles(text_rows):
    with open(os.path.join(REPO, "profiles", "rD_text_kernel_resources.csv")) as f:
        recorded = {r["kernel"]: r for r in csv.DictReader(f)}
    assert set(recorded) == KERNELS
    for k, b in recorded.items():
        assert all(text_rows[k][c] == int(b[c]) for c in ("vgprs", "agprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd",
                                                          "static_lds_bytes")), (k, text_rows[k])
