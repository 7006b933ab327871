#!/usr/bin/env python3
"""Generate tests/golden/attention_ends_bits.npz: the output, log-sum-exp and redo-counter bits of the matrix-pipe attention kernel as
the library under GSDD_LIB_PATH (default: the tree's libgsdd.so) computes them on the MI355X, for the inputs, lengths, modes and coding
of tests/test_gpu_attention_ends.py.  It was run with the build that preceded the "prologue once per query, epilogue on all lanes"
change; rerun it only with a build whose bits are meant to become the new reference.

Usage:  python tests/golden/make_golden_attention_ends.py [out.npz]
"""
import importlib.util
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

import numpy as np
import torch

_spec = importlib.util.spec_from_file_location("attention_ends", os.path.join(os.path.dirname(HERE), "test_gpu_attention_ends.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)


def main():
    import gsdd_amd
    assert torch.cuda.is_available(), "the fixture holds what the MI355X computes"
    os.environ.pop("GSDD_ATTN_LEAN", None)
    os.environ.pop("GSDD_ATTN_P", None)
    gsdd_amd.lib()
    results = {}
    for case in T.CASES:
        for L in T.LENGTHS:
            res = T.run_case(gsdd_amd, case, L)
            q, k, v = T.make_inputs(case, L)
            if case != "nan":
                ref = T.fp64_reference(q, k, v, L)
                errs = {n: (torch.from_numpy(res[n]).view(torch.float32).double() - ref).abs().max().item() for n in res if n.startswith("out_")}
                print(f"{case} L={L} redo={res['redo'].tolist()} " + " ".join(f"{n}={e:.2e}" for n, e in errs.items()))
            else:
                print(f"{case} L={L} redo={res['redo'].tolist()} NaN words: " +
                      " ".join(f"{n}={int(np.isnan(res[n].view(np.float32)).sum())}" for n in res if n != "redo"))
            results[(case, L)] = {n: (a if n == "redo" else T.canon(a)) for n, a in res.items()}
    path = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    np.savez_compressed(path, **T.encode(results))
    back = T.decode(np.load(path, allow_pickle=False))
    for key, res in results.items():
        for n, a in res.items():
            assert np.array_equal(back[key][n], a), (key, n)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
