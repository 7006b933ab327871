#!/usr/bin/env python3
"""Static census of the vector instructions one wave of an attention kernel instantiation issues outside its tile loop, part by part.
Cross-compiles d3pm_attention.hip to assembly with build.sh's flags (no GPU needed), from the working tree and, with --rev, from a git
revision, then walks the listing along the path of a QUIET wave of a long row (L >= 768, a chunk in the middle of the row, lean loop,
no log-sum-exp) and counts v_* instructions and s_nop per part:
  prologue    entry .. first barrier: q splits, first chunk's staging, and (since the (b, h) statistics kernel) the lane's own query
              numbers, the Jensen bound and the row minima
  first_keys  .. the fourth v_ceil_f32: the offsets m from the first 64 keys (a rolled loop is walked four times)
  bounds      .. the chunk loop's header: the quiet decision (before that kernel: also the Jensen bound and the row minima)
  loop        one pass through the chunk loop with ONE pair-tile iteration (loop bodies are walked once)
  epilogue    after the chunk loop's barrier: merge, divide, store
Branches on exec are decided by rule (execz falls through, execnz is taken, back edges are not taken); every forward branch on scc / vcc
needs a decision, given in the order met as a string of T (taken) / N: the script stops at the first one it has no letter for and
prints the lines before it, from which the condition is read.  The strings below are those of the builds the CSV was made from; a
compiler or source change that moves blocks needs new ones.
usage: attn_census.py [--rev REV --rev-decisions STR] [--decisions STR] [--kernel 'ILi384ELi8E'] [out.csv | -]"""
import argparse
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "gif-synthesis-with-discrete-diffusion_amd"
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mllvm", "-amdgpu-mfma-vgpr-form",
         "-Wno-unused-function", "-w"]
FILES = [f"{PKG}/csrc/d3pm_attention.hip", f"{PKG}/csrc/common.hpp", "include/gsdd.h"]
# Decision strings by build.  --rev-decisions defaults to the one of the commit right before the (b, h) statistics kernel (what
# profiles/rF_attn_census.csv was made against); any other revision needs its own string on the command line: the one of the commit
# before the per-query prologue, against which profiles/rB_attn_census.csv was made, is BEFORE_PER_QUERY_PROLOGUE.  A wrong string does
# not fail, it walks another path: check the part counts of a known build first.
BEFORE_PER_QUERY_PROLOGUE = "NTNNNNNNNNTNNTT"
PARENT_DECISIONS = "NTTTTTNNNNTNNTT"
THIS_DECISIONS = "NTTTTTNNNNTNNTT"
PARTS = ["prologue", "first_keys", "bounds", "loop", "epilogue"]


def assembly(rev):
    with tempfile.TemporaryDirectory() as td:
        for f in FILES:
            dst = os.path.join(td, f)
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            if rev is None:
                shutil.copy(os.path.join(REPO, f), dst)
            else:
                with open(dst, "wb") as out:
                    out.write(subprocess.run(["git", "-C", REPO, "show", f"{rev}:{f}"], capture_output=True, check=True).stdout)
        out = os.path.join(td, "k.s")
        subprocess.run([HIPCC, *FLAGS, "--offload-device-only", "-S", os.path.join(td, FILES[0]), "-o", out], check=True)
        return open(out).read().splitlines()


def kernel_lines(lines, tag):
    start = next(i for i, l in enumerate(lines) if l.startswith("_ZN4gsdd24d3pm_attention_v4_kernel" + tag) and ":" in l)
    end = next(i for i in range(start, len(lines)) if lines[i].strip() == "s_endpgm")
    return lines[start:end + 1]


def census(lines, decisions):
    label_at = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"(\.LBB\w+):", l))}
    pc, part, ceils, ndec = 0, "prologue", 0, 0
    visited, backs, counts = set(), collections.Counter(), collections.Counter()
    while True:
        l = lines[pc]
        visited.add(pc)
        toks = l.split()
        op = toks[0] if l.startswith("\t") and toks else ""
        if part == "bounds" and "Loop Header" in l:
            part = "loop"
        if op.startswith("v_"):
            counts[(part, "valu")] += 1
            if op.startswith("v_ceil_f32") and part == "first_keys":
                ceils += 1
                if ceils == 4:
                    part = "bounds"
        elif op == "s_nop":
            counts[(part, "s_nop")] += 1
        elif op == "s_barrier":
            part = {"prologue": "first_keys", "loop": "epilogue"}.get(part, part)
        elif op == "s_endpgm":
            return counts
        m = re.match(r"\s+(s_c?branch\w*)\s+(\.LBB\w+)", l)
        if m:
            kind, tgt = m.group(1), label_at[m.group(2)]
            back = tgt in visited
            if kind == "s_branch":
                if back:
                    raise SystemExit(f"unconditional back branch at line {pc + 1}")
                take = True
            elif kind == "s_cbranch_execz":
                take = False
            elif kind == "s_cbranch_execnz":
                take = not back
            elif back:
                backs[pc] += 1
                take = part == "first_keys" and backs[pc] < 4
            else:
                if ndec >= len(decisions):
                    ctx = "\n".join(lines[max(0, pc - 10):pc + 1])
                    raise SystemExit(f"decision {ndec} missing (part {part}, line {pc + 1} of the kernel):\n{ctx}")
                take = decisions[ndec] == "T"
                ndec += 1
            if take:
                pc = tgt
                continue
        pc += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rev", default=None, help="also count this git revision (the parent build)")
    ap.add_argument("--rev-decisions", default=PARENT_DECISIONS,
                    help="branch decisions of --rev; the default fits only the commit right before the (b, h) statistics kernel")
    ap.add_argument("--decisions", default=THIS_DECISIONS)
    ap.add_argument("--kernel", default="ILi384ELi8E", help="mangled template arguments of the instantiation")
    ap.add_argument("out", nargs="?", default="-")
    a = ap.parse_args()
    builds = ([("parent", a.rev, a.rev_decisions)] if a.rev else []) + [("this", None, a.decisions)]
    rows = ["build,part,vector_instructions,s_nop"]
    for name, rev, dec in builds:
        c = census(kernel_lines(assembly(rev), a.kernel), dec)
        for part in PARTS:
            rows.append(f"{name},{part},{c[(part, 'valu')]},{c[(part, 's_nop')]}")
        outside = [p for p in PARTS if p != "loop"]
        rows.append(f"{name},all_but_loop,{sum(c[(p, 'valu')] for p in outside)},{sum(c[(p, 's_nop')] for p in outside)}")
    text = "\n".join(rows) + "\n"
    if a.out == "-":
        sys.stdout.write(text)
    else:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
