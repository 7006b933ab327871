#!/usr/bin/env python3
"""Registers, scratch and occupancy of the sampler's kernels as hipcc reports them for gfx950 (-Rpass-analysis=kernel-resource-usage).
Cross-compiles the device code of the sampler's source files with build.sh's flags (no GPU needed) and writes one CSV row per kernel
instantiation.  Scratch is what a kernel spills: every byte per lane is a store and a reload through the memory hierarchy.
usage: kernel_resources.py [out.csv [source.hip ...]]   (default profiles/r5_kernel_resources.csv; '-' prints to stdout; sources default
to the sampler's, e.g. `kernel_resources.py profiles/rQ_gif_kernel_resources.csv gif.hip`)"""
import concurrent.futures
import csv
import io
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "gif-synthesis-with-discrete-diffusion_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# the flags of build.sh
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mllvm", "-amdgpu-mfma-vgpr-form",
         "-Wno-unused-function"]
# the sampler's per-block kernels: attention (+ its K / V pre-split), the fused layer (+ logits); the purity-prior step's kernels; the
# reverse step (and the training objective's kernels that share its file); the forward jump of RePaint's resampling; the training
# step's cross-attention over several condition tokens; its condition dropout and null-embedding gradient; its optimiser stage; the
# slide between two windows of a long rollout and the stitched decode's window blend
SOURCES = ["d3pm_attention.hip", "d3pm_layer.hip", "d3pm_purity.hip", "d3pm_step.hip", "d3pm_jump.hip", "d3pm_cross.hip", "d3pm_cond.hip",
           "optim.hip", "d3pm_window.hip"]
FIELDS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
          "Occupancy [waves/SIMD]": "occupancy_waves_per_simd", "VGPRs Spill": "vgpr_spill", "LDS Size [bytes/block]": "static_lds_bytes"}


def demangle(names):
    tool = shutil.which("llvm-cxxfilt", path=os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "llvm", "bin")) \
        or shutil.which("c++filt")
    if tool is None:
        return list(names)
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return [o.replace("void ", "").replace("gsdd::", "").split("(")[0] for o in out]


def compile_one(src):
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([HIPCC, *FLAGS, "-Rpass-analysis=kernel-resource-usage", "--offload-device-only", "-c",
                            os.path.join(CSRC, src), "-o", os.path.join(td, "k.o")], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {src}:\n{r.stderr[-2000:]}")
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = {"source": src, "mangled": m.group(1)}
            rows.append(cur)
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z ]*(?: \[[^\]]+\])?): (\S+) \[-Rpass-analysis", line)
        if m and cur is not None and m.group(1) in FIELDS:
            v = m.group(2)
            cur[FIELDS[m.group(1)]] = int(v) if v.lstrip("-").isdigit() else v
    return [r for r in rows if "kernel" in r["mangled"].lower()]


def collect(sources=SOURCES):
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(sources)) as ex:
        rows = [r for part in ex.map(compile_one, sources) for r in part]
    for r, name in zip(rows, demangle([r["mangled"] for r in rows])):
        r["kernel"] = name
    return rows


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "r5_kernel_resources.csv")
    rows = collect(sys.argv[2:] or SOURCES)
    cols = ["source", "kernel", "vgprs", "agprs", "sgprs", "scratch_bytes_per_lane", "vgpr_spill", "occupancy_waves_per_simd",
            "static_lds_bytes"]
    buf = io.StringIO()
    w = csv.DictWriter(buf, fieldnames=cols, extrasaction="ignore", lineterminator="\n")
    w.writeheader()
    for r in sorted(rows, key=lambda r: (r["source"], r["kernel"])):
        w.writerow(r)
    if out == "-":
        sys.stdout.write(buf.getvalue())
    else:
        with open(out, "w") as f:
            f.write(buf.getvalue())
        print(f"wrote {out}: {len(rows)} kernels")


if __name__ == "__main__":
    main()
