"""Registers, scratch and LDS of the image tower's kernels (csrc/clip_vision.hip) as hipcc reports them for gfx950: no scratch anywhere,
the attention kernel's three LDS images (Q, K, V rows of D + 4 floats for 80 positions) inside the 64 KiB a workgroup may declare
statically, and the figures recorded in profiles/rP_vision_kernel_resources.csv are the compile's."""
import csv
import importlib.util
import os
import shutil

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = {"clip_frame_patches_kernel", "clip_vision_embed_kernel", "clip_attention_kernel<64>", "clip_attention_kernel<32>",
           "clip_attention_kernel<16>"}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not installed")


@pytest.fixture(scope="module")
def vision_rows():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return {r["kernel"]: r for r in mod.collect(["clip_vision.hip"])}


def test_vision_kernels_have_no_scratch(vision_rows):
    assert set(vision_rows) == KERNELS
    for k, r in vision_rows.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["vgprs"] <= 256, r


def test_attention_lds_fits(vision_rows):
    # three images of 80 rows x (D + 4) floats, and nothing else
    assert vision_rows["clip_attention_kernel<64>"]["static_lds_bytes"] == 3 * 80 * 68 * 4 <= 64 * 1024
    assert vision_rows["clip_attention_kernel<32>"]["static_lds_bytes"] == 3 * 80 * 36 * 4
    assert vision_rows["clip_attention_kernel<16>"]["static_lds_bytes"] == 3 * 80 * 20 * 4
    assert vision_rows["clip_frame_patches_kernel"]["static_lds_bytes"] == 0 and vision_rows["clip_vision_embed_kernel"]["static_lds_bytes"] == 0
    # five waves of a workgroup must be able to live on a CU's four SIMDs: at least two waves per SIMD
    for k in KERNELS:
        assert vision_rows[k]["occupancy_waves_per_simd"] >= 2, k


def test_recorded_figures_are_the_compiles(vision_rows):
    with open(os.path.join(REPO, "profiles", "rP_vision_kernel_resources.csv")) as f:
        recorded = {r["kernel"]: r for r in csv.DictReader(f)}
    assert set(recorded) == KERNELS
    for k, b in recorded.items():
        assert all(vision_rows[k][c] == int(b[c]) for c in ("vgprs", "agprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd",
                                                            "static_lds_bytes")), (k, vision_rows[k])
