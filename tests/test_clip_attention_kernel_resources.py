"""Registers, scratch and LDS of the attention kernel both CLIP towers share (csrc/clip_attention.hip, clip_attention_kernel<D, CAUSAL>)
as hipcc reports them for gfx950, for all six instantiations: no scratch, the three LDS images (Q, K, V rows of D + 4 floats for 80
positions) inside the 64 KiB a workgroup may declare statically, the figures recorded in
profiles/rS_clip_attention_kernel_resources.csv are the compile's, and none is worse than what the two separate kernels this one
replaced had (the text tower's causal one and the image tower's non-causal one, as their resource files recorded them)."""
import csv
import importlib.util
import os
import shutil

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# (D, CAUSAL) -> (VGPRs, waves per SIMD, static LDS bytes) of the kernel it replaced
REPLACED = {(64, True): (47, 3, 65280), (32, True): (39, 5, 34560), (16, True): (35, 8, 19200),
            (64, False): (47, 3, 65280), (32, False): (42, 5, 34560), (16, False): (35, 8, 19200)}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not installed")


def name(d, causal):
    return f"clip_attention_kernel<{d}, {'true' if causal else 'false'}>"


KERNELS = {name(d, c) for d, c in REPLACED}


@pytest.fixture(scope="module")
def attention_rows():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return {r["kernel"]: r for r in mod.collect(["clip_attention.hip"])}


def test_attention_kernels_have_no_scratch(attention_rows):
    assert set(attention_rows) == KERNELS
    for k, r in attention_rows.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["vgprs"] <= 256, r


def test_attention_lds_fits(attention_rows):
    for causal in (True, False):
        # three images of 80 rows x (D + 4) floats, and nothing else
        assert attention_rows[name(64, causal)]["static_lds_bytes"] == 3 * 80 * 68 * 4 <= 64 * 1024
        assert attention_rows[name(32, causal)]["static_lds_bytes"] == 3 * 80 * 36 * 4
        assert attention_rows[name(16, causal)]["static_lds_bytes"] == 3 * 80 * 20 * 4
    # five waves of a workgroup must be able to live on a CU's four SIMDs: at least two waves per SIMD
    for k in KERNELS:
        assert attention_rows[k]["occupancy_waves_per_simd"] >= 2, k


def test_no_instantiation_is_worse_than_the_kernel_it_replaced(attention_rows):
    for (d, causal), (vgprs, occupancy, lds) in REPLACED.items():
        r = attention_rows[name(d, causal)]
        assert r["static_lds_bytes"] == lds and r["occupancy_waves_per_simd"] == occupancy and r["vgprs"] <= vgprs, r


def test_recorded_figures_are_the_compiles(attention_rows):
    with open(os.path.join(REPO, "profiles", "rS_clip_attention_kernel_resources.csv")) as f:
        recorded = {r["kernel"]: r for r in csv.DictReader(f)}
    assert set(recorded) == KERNELS
    for k, b in recorded.items():
        assert all(attention_rows[k][c] == int(b[c]) for c in ("vgprs", "agprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd",
                                                               "static_lds_bytes")), (k, attention_rows[k])
