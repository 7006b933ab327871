#!/usr/bin/env python3
"""Generate tests/golden/adam_plain_bits.npz: the p, m and v words that `gsdd_adam_multi_dev` -- the plain Adam kernel of the captured
training step -- wrote on the MI355X, for tensors of 1, 3, 4095 and 4097 elements, betas (0.5, 0.999), eps 1e-8, lr 1e-3 and steps 1, 2
and 1000, each from the same nonzero state.  The inputs are drawn here with numpy and stored beside the results, so the fixture depends
on no generator's version.

It was run once, against the library built from commit 0d16a5c ("D3PM trainer: clipped AdamW, averaged weights, LR warm-up on the
device").  It is NOT to be rerun against a later library: the fixture's only purpose is to hold that commit's bits, so that the stage's
update kernel can be held to them whatever becomes of gsdd_adam_multi_dev
(tests/test_gpu_optim_kernels.py::test_stage_with_nothing_on_gives_the_recorded_plain_adam_bits).

Usage:  GSDD_LIB_PATH=<libgsdd.so of 0d16a5c> python tests/golden/make_golden_adam_plain.py [out.npz]
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "adam_plain_bits.npz")
SIZES = [1, 3, 4095, 4097]
STEPS = [1, 2, 1000]
LR, B1, B2, EPS = 1e-3, 0.5, 0.999, 1e-8
CHUNK = 4096


def draw_inputs():
    """the four tensors' p, g, m, v, each concatenated in SIZES' order (float32)"""
    rng = np.random.default_rng(20261020)
    p, g, m, v = [], [], [], []
    for n in SIZES:
        p.append(rng.standard_normal(n).astype(np.float32))
        gi = (rng.standard_normal(n) * 1e-2).astype(np.float32)
        gi[::11] = 0.0
        g.append(gi)
        m.append((rng.standard_normal(n) * 1e-2).astype(np.float32))
        v.append((rng.random(n) * 1e-4).astype(np.float32))
    return tuple(np.concatenate(x) for x in (p, g, m, v))


def main():
    assert torch.cuda.is_available(), "the fixture holds what the MI355X computes"
    L = C.CDLL(os.environ["GSDD_LIB_PATH"])
    L.gsdd_last_error.restype = C.c_char_p
    L.gsdd_adam_multi_dev.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    p0, g0, m0, v0 = draw_inputs()
    offs = np.concatenate([[0], np.cumsum([(n + 3) & ~3 for n in SIZES])]).astype(np.int64)      # every tensor on a multiple of 4
    starts = np.concatenate([[0], np.cumsum(SIZES)])

    def place(flat):
        buf = torch.zeros(int(offs[-1]), device="cuda")
        for n, o, s in zip(SIZES, offs[:-1], starts[:-1]):
            buf[int(o):int(o) + n].copy_(torch.from_numpy(flat[s:s + n]))
        return buf

    def gather(buf):
        host = buf.cpu().numpy()
        return np.concatenate([host[int(o):int(o) + n] for n, o in zip(SIZES, offs[:-1])]).view(np.uint32)

    out = {"sizes": np.array(SIZES, dtype=np.int64), "steps": np.array(STEPS, dtype=np.int64),
           "hyper": np.array([LR, B1, B2, EPS], dtype=np.float64), "p": p0, "g": g0, "m": m0, "v": v0}
    for step in STEPS:
        p, g, m, v = place(p0), place(g0), place(m0), place(v0)
        rows = []
        for n, o in zip(SIZES, offs[:-1]):
            for s in range(0, n, CHUNK):
                rows.append([t.data_ptr() + 4 * (int(o) + s) for t in (p, g, m, v)] + [min(CHUNK, n - s)])
        table = torch.tensor(rows, dtype=torch.int64, device="cuda")
        step_dev = torch.tensor([step], dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        rc = L.gsdd_adam_multi_dev(C.c_void_p(table.data_ptr()), len(rows), LR, B1, B2, EPS, C.c_void_p(step_dev.data_ptr()),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, L.gsdd_last_error().decode()
        torch.cuda.synchronize()
        assert np.array_equal(gather(g), g0.view(np.uint32))
        for name, t, t0 in (("p", p, p0), ("m", m, m0), ("v", v, v0)):
            out[f"{name}_step{step}"] = gather(t)
            print(f"step {step} {name}: {int((out[f'{name}_step{step}'] != t0.view(np.uint32)).sum())} of {t0.size} words moved")
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    np.savez(path, **out)
    back = np.load(path, allow_pickle=False)
    for k, a in out.items():
        assert np.array_equal(back[k], a), k
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
