"""Numpy restatement of the long-clip geometry (d3pm.long_plan), the slide between two windows (gsdd_d3pm_window_slide) and the
window blend (gsdd_clip_window_blend), written from the definitions and sharing no code with the package."""
import numpy as np


def windows(F, n, k):
    s = F - k
    return 1 + -(-max(n - F, 0) // s)


def frame_map(F, n, k):
    """-> [(window, frame within the window)] per long frame: the first window that sampled it."""
    s, out = F - k, []
    for f in range(n):
        if f < F:
            out.append((0, f))
        else:
            w = next(w for w in range(1, n + 1) if w * s + k <= f < w * s + F)
            out.append((w, f - w * s))
    return out


def slide(tok, long_rows, x_known, known, t2, w, *, F, k, n, K, t0, final=False):
    """The slide on copies of the buffers -> (tok, long_rows, x_known, known, t2, next w, bad count)."""
    tok, long_rows, x_known, known, t2 = (a.copy() for a in (tok, long_rows, x_known, known, t2))
    Bs, Lw = tok.shape
    hw, s = Lw // F, F - k
    for fr in range(0 if w == 0 else k, F):
        lf = w * s + fr
        if lf < n:
            long_rows[:, lf * hw:(lf + 1) * hw] = tok[:, fr * hw:(fr + 1) * hw]
    if final:
        return tok, long_rows, x_known, known, t2, w, 0
    tail = tok[:, s * hw:]
    x_known[:, :k * hw] = tail
    bad = int(((tail < 0) | (tail >= K)).sum())
    known[:] = 0
    known[:, :k * hw] = 1
    tok[:] = K
    t2[:] = t0
    return tok, long_rows, x_known, known, t2, w + 1, bad


def blend(win, out, f0, n_ov, mode):
    """win (B, C, Fw, H, W), out (B, C, Fo, H, W) -> the merged clip, in the dtype of `out` (pass float64 copies of the float32
    inputs for the reference the kernel's crossfade is held against)."""
    out = out.copy()
    Fw, Fo = win.shape[2], out.shape[2]
    for j in range(Fw):
        f = f0 + j
        if f >= Fo:
            break
        if j < n_ov:
            if mode == "keep":
                continue
            if mode == "linear":
                a = (j + 1) / (n_ov + 1)
                out[:, :, f] = out[:, :, f] + a * (win[:, :, j].astype(out.dtype) - out[:, :, f])
                continue
        out[:, :, f] = win[:, :, j]
    return out
