"""Host-side helpers shared by the two trainers: a zero-initialised gradient arena (one fill per step instead of one per tensor)
and Adam over all parameters in one launch (gsdd_adam_multi) -- or, with clipping / weight decay / averaged weights / the non-finite guard,
the three launches of the optimiser stage (gsdd_grad_sqnorm, gsdd_grad_norm_finalize, gsdd_adamw_ema_multi)."""
import warnings

import numpy as np
import torch

from ._lib import check, lib, ptr, stream_ptr

ADAM_CHUNK = 4096


class GradArena:
    """Hands out zero-filled views of one flat fp32 buffer.  `reset()` zeroes the buffer (one kernel); a request that does not fit
    falls back to torch.zeros and grows the buffer for the next step."""

    def __init__(self, device, capacity=0):
        self.device, self.buf, self.off, self.want = device, None, 0, int(capacity)
        self.spilled = False               # a request of this step did not fit (its tensor lives outside the buffer)

    def reset(self):
        self.spilled = False
        if self.buf is None or self.buf.numel() < self.want:
            self.buf = torch.zeros((self.want,), dtype=torch.float32, device=self.device)
        else:
            self.buf.zero_()
        self.off = 0
        self.want = 0

    def zeros(self, shape):
        n = int(np.prod(shape)) if len(shape) else 1
        n4 = (n + 3) & ~3                                  # keep every view 16-byte aligned (float4 kernels)
        self.want += n4
        if self.buf is not None and self.off + n4 <= self.buf.numel():
            v = self.buf[self.off:self.off + n].view(shape)
            self.off += n4
            return v
        self.spilled = True
        return torch.zeros(shape, dtype=torch.float32, device=self.device)

    def zeros_like(self, t):
        return self.zeros(tuple(t.shape))


class GradBook:
    """One step's gradients: the name -> gradient dict `g`, the arena they are zero-filled views of, and -- with a reducer (a
    parallel.GradReducer) -- the data-parallel buckets they leave in.  `bucket()` all-reduces (in place, async) what the arena handed
    out since the last bucket, anonymous scratch included; a bucket that has been issued must never be written again, so a gradient
    is requested only when its kernel is about to be enqueued.  `finish(names)` issues the remainder, sends whatever lives outside
    the issued range (the first step, when the arena is not sized yet, or a step that outgrew it) as one concatenated bucket and
    waits.  Without a reducer nothing is issued, `names` (any iterable) is not read and `g` is returned as handed out."""

    def __init__(self, arena, reducer=None):
        self.arena, self.red, self.g, self.mark = arena, reducer, {}, 0
        arena.reset()                             # every gradient is a zero-filled view of one buffer: one fill per step

    def zeros(self, name, like):
        self.g[name] = self.arena.zeros_like(like)
        return self.g[name]

    def scratch(self, shape):
        """zero-filled arena memory that is no parameter's gradient: it may ride in a bucket, it is never in `g`"""
        return self.arena.zeros(tuple(shape))

    def bucket(self):
        a = self.arena
        if self.red is not None and a.buf is not None and self.mark < a.off <= a.buf.numel():
            self.red.add(a.buf[self.mark:a.off])
            self.mark = a.off

    def finish(self, names):
        if self.red is None:
            return self.g
        self.bucket()
        a = self.arena
        lo = a.buf.data_ptr() if a.buf is not None else 0
        issued = lambda t: lo and lo <= t.data_ptr() < lo + 4 * self.mark
        self.red.add_concatenated(self.g, [n for n in names if not issued(self.g[n])])
        self.red.finish()
        return self.g


def linear_warmup(base_lr, warmup_steps):
    """step -> base_lr * min(1, step / warmup_steps), the step counted from 1 (a learning-rate schedule for D3PMTrainer(lr_schedule=))"""
    base_lr, warmup_steps = float(base_lr), int(warmup_steps)
    if warmup_steps < 1:
        raise ValueError(f"linear_warmup: warmup_steps must be at least 1, got {warmup_steps}")
    return lambda step: base_lr * min(1.0, step / warmup_steps)


def check_stage_args(max_grad_norm, weight_decay, ema_decay):
    if max_grad_norm is not None and not float(max_grad_norm) > 0:
        raise ValueError(f"max_grad_norm must be positive, got {max_grad_norm}")
    if not float(weight_decay) >= 0:
        raise ValueError(f"weight_decay must not be negative, got {weight_decay}")
    if ema_decay is not None and not 0 <= float(ema_decay) < 1:
        raise ValueError(f"ema_decay must be in [0, 1), got {ema_decay}")


def flat_offsets(sizes):
    """offsets of tensors of `sizes` elements in MultiAdam's flat m / v / ema buffers (every tensor starts on a multiple of 4)"""
    return np.concatenate([[0], np.cumsum([(n + 3) & ~3 for n in sizes])]).astype(np.int64)


def unflatten(flat, named_shapes):
    """a flat m / v / ema buffer -> {name: tensor of its shape} for [(name, shape)] in the optimiser's parameter order"""
    shapes = [(nm, tuple(sh)) for nm, sh in named_shapes]
    sizes = [int(np.prod(sh)) if len(sh) else 1 for _, sh in shapes]
    offs = flat_offsets(sizes)
    if flat.numel() != int(offs[-1]):
        raise ValueError(f"the flat buffer holds {flat.numel()} values, this parameter list needs {int(offs[-1])}")
    return {nm: flat[int(o):int(o) + n].reshape(sh).clone() for (nm, sh), n, o in zip(shapes, sizes, offs[:-1])}


class MultiAdam:
    """Adam state (m, v flat) for a fixed list of parameters; `step(grads)` = one gsdd_adam_multi launch.

    With max_grad_norm / weight_decay / ema_decay / skip_nonfinite / device_lr set, `step` is the optimiser stage of include/gsdd.h
    instead: gsdd_grad_sqnorm + gsdd_grad_norm_finalize (whenever clipping or skip_nonfinite is on) and gsdd_adamw_ema_multi, three
    launches whatever the number of parameters.  The optimiser then owns the device state block (step, lr, norm, clip coefficient,
    finite flag, skip count), the per-block partial sums and -- with ema_decay -- a flat `ema` buffer laid out like m and v,
    initialised from the parameters here.  decay_mask: name -> bool, which tensors take weight decay (a missing name decays; None:
    all do).  A skipped step (non-finite norm) still advances step_count: host and device counts stay equal without a read-back."""

    def __init__(self, params, lr, betas, eps, max_grad_norm=None, weight_decay=0.0, decay_mask=None, ema_decay=None,
                 skip_nonfinite=False, device_lr=False):
        self.params = list(params)                                        # [(name, tensor)]
        self.lr, self.betas, self.eps = lr, betas, eps
        self.step_count = 0
        dev = self.params[0][1].device
        sizes = [p.numel() for _, p in self.params]
        self.offs = flat_offsets(sizes)
        self.m = torch.zeros((int(self.offs[-1]),), dtype=torch.float32, device=dev)
        self.v = torch.zeros_like(self.m)
        self._key, self._table = None, None
        check_stage_args(max_grad_norm, weight_decay, ema_decay)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.weight_decay, self.skip_nonfinite = float(weight_decay), bool(skip_nonfinite)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.decays = [bool(self.weight_decay > 0 and (decay_mask is None or decay_mask.get(name, True))) for name, _ in self.params]
        self.staged = bool(self.max_grad_norm is not None or self.weight_decay > 0 or self.ema_decay is not None
                           or self.skip_nonfinite or device_lr)
        self.ema = self.words = self.partials = None
        self._swap_key, self._swap_table = None, None
        if self.staged:
            self.n_blocks = int(sum((n + ADAM_CHUNK - 1) // ADAM_CHUNK for n in sizes))
            self.partials = torch.zeros((self.n_blocks,), dtype=torch.float64, device=dev)
            # gsdd_optim_state as 8 x 32 bits: step (int64), skipped_steps (int64), lr, grad_norm, clip_coef (f32), finite (int32)
            words = np.zeros((8,), dtype=np.int32)
            words.view(np.float32)[6] = 1.0
            words[7] = 1
            self.words = torch.from_numpy(words).to(dev)
            if self.ema_decay is not None:
                self.ema = torch.zeros_like(self.m)
                self._ema_from_params()

    def _ema_from_params(self):
        for (_, p), off in zip(self.params, self.offs[:-1]):
            self.ema[int(off):int(off) + p.numel()].copy_(p.detach().reshape(-1))

    # ---- the device words of the stage
    @property
    def grad_norm(self):
        """the last step's global gradient norm, a device scalar (reading it waits for the step)"""
        return None if self.words is None else self.words.view(torch.float32)[5]

    @property
    def clip_coef(self):
        return None if self.words is None else self.words.view(torch.float32)[6]

    @property
    def skipped_steps(self):
        return 0 if self.words is None else int(self.words.view(torch.int64)[1])

    def write_step_words(self, step, lr):
        """step and lr of the coming update into the state block (two fills): the launch-by-launch step does it inside `step`, a
        captured step's owner before each replay"""
        self.words.view(torch.int64)[0:1].fill_(int(step))
        self.words.view(torch.float32)[4:5].fill_(float(lr))

    def state(self):
        st = {"m": self.m.detach().cpu(), "v": self.v.detach().cpu(), "step": int(self.step_count)}
        if self.staged:
            st["skipped_steps"] = self.skipped_steps
        if self.ema is not None:
            st["ema"] = self.ema.detach().cpu()
        return st

    def load_state(self, st):
        if st is None:
            return
        if st["m"].numel() != self.m.numel():
            raise ValueError(f"Adam state holds {st['m'].numel()} values, this parameter list needs {self.m.numel()}")
        self.m.copy_(st["m"])
        self.v.copy_(st["v"])
        self.step_count = int(st["step"])
        if self.staged:
            self.words.view(torch.int64)[1:2].fill_(int(st.get("skipped_steps", 0)))
        if self.ema is not None:
            if st.get("ema") is None:
                warnings.warn("MultiAdam: the optimiser state carries no averaged weights (a checkpoint from before ema_decay was "
                              "set): the average starts from the current parameters")
                self._ema_from_params()
            else:
                if st["ema"].numel() != self.ema.numel():
                    raise ValueError(f"the averaged weights hold {st['ema'].numel()} values, this parameter list needs {self.ema.numel()}")
                self.ema.copy_(st["ema"])

    def _build_table(self, grads):
        rows = []
        mb, vb = self.m.data_ptr(), self.v.data_ptr()
        eb = self.ema.data_ptr() if self.ema is not None else None
        cols = 7 if self.staged else 5
        for (name, p), off, dec in zip(self.params, self.offs[:-1], self.decays):
            n = p.numel()
            starts = np.arange(0, n, ADAM_CHUNK, dtype=np.int64)
            t = np.zeros((len(starts), cols), dtype=np.int64)
            t[:, 0] = p.data_ptr() + 4 * starts
            t[:, 1] = (grads[name].data_ptr() + 4 * starts) if grads is not None else 0
            t[:, 2] = mb + 4 * (off + starts)
            t[:, 3] = vb + 4 * (off + starts)
            t[:, 4] = np.minimum(ADAM_CHUNK, n - starts)
            if self.staged:                                    # the wide table: running average and flags (bit 0: the tensor decays)
                t[:, 5] = (eb + 4 * (off + starts)) if eb is not None else 0
                t[:, 6] = 1 if dec else 0
            rows.append(t)
        return np.concatenate(rows)

    def swap_ema(self, stream=None):
        """Exchanges the parameters and their running averages, exactly (one gsdd_swap_multi launch); twice = the identity."""
        if self.ema is None:
            raise ValueError("this optimiser keeps no averaged weights (ema_decay is None)")
        key = tuple(p.data_ptr() for _, p in self.params)
        if key != self._swap_key:
            self._swap_table = torch.from_numpy(self._build_table(None)).to(self.params[0][1].device)
            self._swap_key = key
        check(lib().gsdd_swap_multi(ptr(self._swap_table), self._swap_table.shape[0], stream_ptr(stream)))

    def ema_tensors(self):
        """{name: averaged tensor} (clones, on the device), in the parameter list's order"""
        return {name: self.ema[int(off):int(off) + p.numel()].reshape(p.shape).clone()
                for (name, p), off in zip(self.params, self.offs[:-1])}

    def step(self, grads, stream=None, step_dev=None, write_words=True):
        """step_dev: int64[1] device tensor holding the step count of THIS update (>= 1): the launch then bakes nothing that changes
        from step to step (captured training step); the host-side count still advances so that checkpoints see it.
        The staged optimiser keeps step and lr in its state block: write_words=False (a step being captured) leaves them to the
        caller, who sets them with `write_step_words` before each replay; step_dev is not used."""
        for name, p in self.params:
            g = grads[name]
            if not g.is_contiguous() or g.shape != p.shape:
                grads[name] = g.contiguous().view(p.shape)
        key = tuple(grads[name].data_ptr() for name, _ in self.params) + tuple(p.data_ptr() for _, p in self.params)
        if key != self._key:
            self._table = torch.from_numpy(self._build_table(grads)).to(self.params[0][1].device)
            self._key = key
        self.step_count += 1
        if self.staged:
            L, s, tb = lib(), stream_ptr(stream), self._table
            if write_words:
                self.write_step_words(self.step_count, self.lr)
            if self.max_grad_norm is not None or self.skip_nonfinite:
                check(L.gsdd_grad_sqnorm(ptr(tb), tb.shape[0], ptr(self.partials), s))
                check(L.gsdd_grad_norm_finalize(ptr(self.partials), tb.shape[0],
                                                float("inf") if self.max_grad_norm is None else self.max_grad_norm,
                                                1 if self.skip_nonfinite else 0, ptr(self.words), s))
            check(L.gsdd_adamw_ema_multi(ptr(tb), tb.shape[0], self.betas[0], self.betas[1], self.eps, self.weight_decay,
                                         self.ema_decay or 0.0, ptr(self.words), s))
            return
        if step_dev is not None:
            check(lib().gsdd_adam_multi_dev(ptr(self._table), self._table.shape[0], self.lr, self.betas[0], self.betas[1], self.eps,
                                            ptr(step_dev), stream_ptr(stream)))
            return
        check(lib().gsdd_adam_multi(ptr(self._table), self._table.shape[0], self.lr, self.betas[0], self.betas[1], self.eps,
                                    self.step_count, stream_ptr(stream)))
