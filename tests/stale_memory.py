"""What uninitialised memory held, made visible.  A helper module for tests/test_stale_memory_host.py (no GPU) and
tests/test_gpu_stale_memory.py; it imports without a GPU.

The contract under test: no output of the library depends on the previous contents of memory that the library, or the caller on its
behalf, obtained uninitialised.  A kernel that breaks it gives different bits for different previous contents, so the check is an
equality over the fill bytes and needs no tolerance.

  stale(byte)   context manager: while active, torch.empty / empty_like / empty_strided and Tensor.new_empty return tensors whose whole
                storage holds `byte`; the fill runs on the current stream.  During a stream capture the allocation passes through
                unfilled and is counted (a recorded fill would be replayed, and would hide what it is meant to show).
  BYTES         0x00 (zero), 0xFF (NaN / -1), 0x7F (+huge: what a max over unwritten slots picks up, a NaN is swallowed by fmaxf),
                0xFE (-huge / a negative integer: likewise for a min).
  scan          every call of the four functions in the package and in src/, by `ast`, as (file, enclosing function).
  SITES/EXEMPT  the ledger: which GPU case reaches each site, or why none has to."""
import ast
import contextlib
import glob
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = "gif-synthesis-with-discrete-diffusion_amd"
BYTES = (0x00, 0xFF, 0x7F, 0xFE)
FUNCTIONS = ("empty", "empty_like", "empty_strided", "new_empty")
_SCOPES = ("<listcomp>", "<dictcomp>", "<setcomp>", "<genexpr>")       # frames of their own before Python 3.12, no functions

_active = None


class Stale:
    """What one `stale(byte)` context saw: `fills` and `passed` count the filled allocations and the ones passed through unfilled
    (stream capture, the meta device, no bytes), `sites` maps a (file, function) call site to its number of fills."""

    def __init__(self, byte):
        if not 0 <= int(byte) <= 255:
            raise ValueError(f"stale: {byte!r} is not a byte")
        self.byte = int(byte)
        self.fills = 0
        self.passed = 0
        self.sites = {}
        self.passed_sites = {}

    def reached(self, prefix=""):
        """the sites filled so far whose file starts with `prefix`"""
        return {s for s in self.sites if s[0].startswith(prefix)}


def call_site(frame):
    """(file relative to the repository, enclosing function) of a frame; a comprehension counts to the function around it"""
    while frame.f_code.co_name in _SCOPES and frame.f_back is not None and frame.f_back.f_code.co_filename == frame.f_code.co_filename:
        frame = frame.f_back
    path = os.path.realpath(frame.f_code.co_filename)
    rel = os.path.relpath(path, REPO)
    return (path if rel.startswith("..") else rel.replace(os.sep, "/")), frame.f_code.co_name


def _capturing(t):
    return t.is_cuda and torch.cuda.is_current_stream_capturing()


def _fill(state, t, frame):
    site = call_site(frame)
    if not torch.is_tensor(t) or t.device.type == "meta" or t.untyped_storage().nbytes() == 0 or _capturing(t):
        state.passed += 1
        state.passed_sites[site] = state.passed_sites.get(site, 0) + 1
        return t
    with torch.no_grad():
        raw = _REAL["empty"](0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())
        raw.fill_(state.byte)                                        # on the current stream, like the allocation's first use
    state.fills += 1
    state.sites[site] = state.sites.get(site, 0) + 1
    return t


_REAL = {}


def _wrap(state, real):
    def allocate(*args, **kwargs):
        return _fill(state, real(*args, **kwargs), sys._getframe(1))
    allocate.__name__ = getattr(real, "__name__", "allocate")
    allocate.__wrapped__ = real
    return allocate


@contextlib.contextmanager
def stale(byte):
    """-> Stale.  Not re-entrant: a nested use raises."""
    global _active
    if _active is not None:
        raise RuntimeError("stale() is already active: nested use is not supported")
    state = Stale(byte)
    saved = {"empty": torch.empty, "empty_like": torch.empty_like, "empty_strided": torch.empty_strided,
             "new_empty": torch.Tensor.new_empty}
    _REAL.update(saved)
    _active = state
    try:
        torch.empty = _wrap(state, saved["empty"])
        torch.empty_like = _wrap(state, saved["empty_like"])
        torch.empty_strided = _wrap(state, saved["empty_strided"])
        torch.Tensor.new_empty = _wrap(state, saved["new_empty"])
        yield state
    finally:
        torch.empty, torch.empty_like, torch.empty_strided = saved["empty"], saved["empty_like"], saved["empty_strided"]
        torch.Tensor.new_empty = saved["new_empty"]
        _REAL.clear()
        _active = None


def bits(t):
    """a host copy of `t` on an integer view, so that equal NaNs compare equal"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.uint8) if t.element_size() == 1 else t.reshape(-1).view(torch.uint8) if t.numel() else t.reshape(-1)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool(torch.equal(a, b))


def host_bits(out):
    """{name: tensor | bytes | number} -> {name: uint8 host tensor}"""
    import numpy as np
    res = {}
    for k, v in out.items():
        if isinstance(v, (bytes, bytearray)):
            v = torch.from_numpy(np.frombuffer(bytes(v), dtype=np.uint8).copy())
        elif not torch.is_tensor(v):
            v = torch.as_tensor(v)
        res[k] = bits(v)
    return res


def sweep(run, order=(BYTES[0],) + BYTES):
    """run() -> {name: output}, called once under every byte of `order` (default: 0x00 twice, then the other three)
    -> [(byte, {name: host bits}, Stale)].  The host copies are made inside the context: they wait for the kernels."""
    results = []
    for byte in order:
        with stale(byte) as st:
            host = host_bits(run())
        results.append((byte, host, st))
    return results


def differing(a, b):
    """the names whose bits differ between two host dicts"""
    return sorted(k for k in set(a) | set(b) if k not in a or k not in b or a[k].shape != b[k].shape or not torch.equal(a[k], b[k]))


def verdict(results):
    """results of `sweep` -> (names that differ between the two 0x00 runs, {byte: names that differ from the first 0x00 run} for the
    bytes where any does, the call sites reached in every run)"""
    zero = results[0][1]
    unstable = differing(zero, results[1][1])
    by_byte = {byte: differing(zero, host) for byte, host, _ in results[2:]}
    reached = set.intersection(*(set(st.sites) for _, _, st in results))
    return unstable, {b: v for b, v in by_byte.items() if v}, reached


# ----------------------------------------------------------------------------- the scan
def scanned_files():
    out = sorted(glob.glob(os.path.join(REPO, PACKAGE, "*.py")))
    out += sorted(glob.glob(os.path.join(REPO, "src", "**", "*.py"), recursive=True))
    return out


class _Scan(ast.NodeVisitor):
    def __init__(self, rel):
        self.rel, self.stack, self.found = rel, [], []

    def _function(self, node):
        self.stack.append(node.name)
        self.generic_visit(node)
        self.stack.pop()

    visit_FunctionDef = visit_AsyncFunctionDef = _function

    def visit_Lambda(self, node):
        self.stack.append("<lambda>")
        self.generic_visit(node)
        self.stack.pop()

    def visit_Call(self, node):
        f = node.func
        name = f.attr if isinstance(f, ast.Attribute) else f.id if isinstance(f, ast.Name) else None
        if name in FUNCTIONS and (name == "new_empty" or isinstance(f, ast.Name)
                                  or (isinstance(f.value, ast.Name) and f.value.id == "torch")):
            self.found.append(((self.rel, self.stack[-1] if self.stack else "<module>"), node.lineno))
        self.generic_visit(node)


def scan(files=None):
    """-> {(file, function): [line, ...]} for every call of torch.empty / empty_like / empty_strided (also imported by name) and
    of .new_empty in `files` (default: the package and src/)"""
    out = {}
    for path in files if files is not None else scanned_files():
        rel = os.path.relpath(path, REPO).replace(os.sep, "/")
        with open(path) as f:
            v = _Scan(rel)
            v.visit(ast.parse(f.read(), path))
        for site, line in v.found:
            out.setdefault(site, []).append(line)
    return out


# ----------------------------------------------------------------------------- the ledger
P = PACKAGE + "/"
# (file, function) of every torch.empty / empty_like / empty_strided / new_empty call in the package and in src/ -> the cases of
# tests/test_gpu_stale_memory.py that must reach it (a kernel-level case where there is one, and a composite).  Keyed by function, not
# by line: unrelated edits do not churn the table.  tests/test_stale_memory_host.py holds it equal to the scan.
SITES = {
    (P + "_clip.py", "_get_buffers"): ("clip_towers",),
    (P + "_clip.py", "_pool_project"): ("clip_towers",),
    (P + "d3pm.py", "__init__"): ("sampler[partial]", "sampler[prior2]"),              # _Lane: the q_sample start, the purity scratch
    (P + "d3pm.py", "_train_loss"): ("sampler[single_calls]",),
    (P + "d3pm.py", "p_sample_tokens"): ("sampler[single_calls]",),
    (P + "d3pm.py", "workspace"): ("sampler[sample]", "sampler[Te22-cond_len]"),
    (P + "d3pm_train.py", "__call__"): ("trainer[Te1]", "trainer[Te3-dropout]"),        # _RowGemm
    (P + "d3pm_train.py", "_block_forward"): ("trainer[Te1]", "trainer[Te3-dropout]"),
    (P + "d3pm_train.py", "_build"): ("trainer[Te1]", "trainer[Te3-dropout]"),          # _LinearImages
    (P + "d3pm_train.py", "_drop_condition"): ("trainer[Te3-dropout]",),
    (P + "d3pm_train.py", "_forward"): ("trainer[Te1]", "trainer[Te3-dropout]"),
    (P + "d3pm_train.py", "_head_backward"): ("trainer[Te1]", "trainer[Te3-dropout]"),
    (P + "d3pm_train.py", "_prepare"): ("trainer[Te1]", "trainer[Te3-dropout]"),
    (P + "d3pm_train.py", "t"): ("trainer[Te1]", "trainer[Te3-dropout]"),               # _RowGemm.t
    (P + "data.py", "preprocess"): ("pool_preprocess_rows", "gif_files"),
    (P + "i3d.py", "_mixed"): ("i3d",),
    (P + "i3d.py", "_pool"): ("i3d",),
    (P + "i3d.py", "_unit"): ("i3d",),
    (P + "ops.py", "_gif_words"): ("gif_kernels[per_clip]", "gif_kernels[per_frame]", "gif_files"),
    (P + "ops.py", "_train_outputs"): ("train_loss[K32]", "train_loss[K4096]", "sampler[single_calls]"),
    (P + "ops.py", "adaln_table"): ("adaln", "sampler[sample]"),
    (P + "ops.py", "axial_attention_bwd"): ("axial_attention[1x4x16x16-C64]", "axial_attention[1x16x8x4-C256]", "vqvae[train]"),
    (P + "ops.py", "batch_rowsum"): ("wgrad_colsum_rowsum", "trainer[Te1]"),
    (P + "ops.py", "bn_relu_bwd"): ("bn_relu_bwd", "vqvae[train]"),
    (P + "ops.py", "bn_train"): ("bn_train", "vqvae[train]"),
    (P + "ops.py", "buffer"): ("gif_kernels[per_clip]", "gif_kernels[per_frame]", "gif_files"),          # gif_delta's
    (P + "ops.py", "clip_frame_patches"): ("clip_kernels", "clip_towers"),
    (P + "ops.py", "codebook_ema_stats"): ("codebook_ema", "vqvae[train]"),
    (P + "ops.py", "codebook_ema_update"): ("codebook_ema", "vqvae[train]"),
    (P + "ops.py", "cond_dropout"): ("sampler_rows[K32]", "sampler_rows[K4096]", "trainer[Te3-dropout]"),
    (P + "ops.py", "d3pm_attention_bwd"): ("attention_train[B2-L64-default]", "attention_train[B2-L40-no_workspace]", "trainer[Te1]"),
    (P + "ops.py", "d3pm_attention_bwd_workspace"): ("attention_train[B2-L64-default]", "attention_train[B1-L320-split]", "trainer[Te1]"),
    (P + "ops.py", "d3pm_attention_workspace"): ("attention[L32]", "attention[L288]", "attention_train[B2-L96-default]", "sampler[sample]"),
    (P + "ops.py", "d3pm_cross_attention_bwd"): ("cross_attention[B3-L37-Te2-H3]", "cross_attention[B2-L64-Te77-H1-len]", "trainer[Te3-dropout]"),
    (P + "ops.py", "d3pm_cross_attention_bwd_workspace"): ("cross_attention[B3-L37-Te2-H3]", "cross_attention[B2-L64-Te77-H1-len]",
                                                           "trainer[Te3-dropout]"),
    (P + "ops.py", "d3pm_layer_pack"): ("sampler[x3p]",),
    (P + "ops.py", "d3pm_layer_pack_h2"): ("sampler[sample]", "sampler[fast]"),
    (P + "ops.py", "d3pm_train_loss_bwd"): ("train_loss[K32]", "train_loss[K4096]"),
    (P + "ops.py", "d3pm_train_loss_grad"): ("train_loss[K32]", "train_loss[K4096]", "trainer[Te1]"),
    (P + "ops.py", "gelu2"): ("gelu2", "trainer[Te1]"),
    (P + "ops.py", "gif_compose"): ("gif_kernels[per_clip]", "gif_kernels[per_frame]", "gif_files"),
    (P + "ops.py", "gif_diffuse"): ("gif_kernels[per_clip]", "gif_kernels[per_frame]", "gif_files"),
    (P + "ops.py", "gif_map"): ("gif_kernels[per_clip]", "gif_kernels[per_frame]"),
    (P + "ops.py", "gif_palette_sums"): ("gif_kernels[per_clip]", "gif_kernels[per_frame]", "gif_files"),
    (P + "ops.py", "lincomb"): ("relu_mask_lincomb", "vqvae[train]"),
    (P + "ops.py", "ln_apply"): ("pool_preprocess_rows",),
    (P + "ops.py", "ln_bwd"): ("ln_bwd", "trainer[Te1]"),
    (P + "ops.py", "ln_fwd"): ("ln_fwd", "trainer[Te1]"),
    (P + "ops.py", "mse"): ("mse", "vqvae[eval]"),
    (P + "ops.py", "ncdhw_to_rows"): ("pool_preprocess_rows", "vqvae[eval]", "i3d"),
    (P + "ops.py", "nearest_code"): ("nearest_code[matrix-E128-K64-M257]", "nearest_code[matrix-E128-K64-M1]", "vqvae[eval]"),
    (P + "ops.py", "philox_uniform"): ("sampler_rows[K32]", "sampler_rows[K4096]"),
    (P + "ops.py", "relu_mask"): ("relu_mask_lincomb", "vqvae[train]"),
    (P + "ops.py", "small_linear"): ("small_linear", "sampler[sample]", "trainer[Te3-dropout]"),
    (P + "ops.py", "small_linear_bwd"): ("small_linear", "trainer[Te1]"),
    (P + "vision.py", "_extra_buffers"): ("clip_towers",),
    (P + "vqvae.py", "_decode_rows"): ("vqvae[eval]", "vqvae[train]"),
    (P + "vqvae.py", "_encode_rows"): ("vqvae[eval]", "vqvae[train]"),
    (P + "vqvae.py", "_quantise_train"): ("vqvae[train]",),
    (P + "vqvae.py", "_res_stack"): ("vqvae[eval]", "vqvae[train]"),
    (P + "vqvae.py", "encode"): ("vqvae[eval]",),
    (P + "vqvae.py", "forward"): ("vqvae[eval]",),
    (P + "vqvae_trainer.py", "_forward"): ("vqvae[train]",),
    (P + "vqvae_trainer.py", "_res_stack_bwd"): ("vqvae[train]",),
    (P + "vqvae_trainer.py", "_res_stack_fwd"): ("vqvae[train]",),
    (P + "vqvae_trainer.py", "backward"): ("vqvae[train]",),
}
# sites no GPU case has to reach, each with its reason
EXEMPT = {
    (P + "parallel.py", "gather_tokens"): "the receive buffers of an all_gather over a process group: reached with more than one rank only, "
                                          "and the collective overwrites every element before anything reads it",
}
