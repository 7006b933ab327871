"""What a captured graph replays on, and who owns it.  A helper module for tests/test_capture_audit_host.py (no GPU) and
tests/test_gpu_capture_lifetime.py; it imports without a GPU.

The contract under test: a captured graph keeps alive everything it replays on.  Every address baked into a graph either passed
through `ptr()` while the graph was recorded, or sits in a device table of raw addresses (MultiAdam._table, _LinearImages.table).

  Recorder      replaces `ptr` in the modules that import it by name and notes, for every tensor handed to the C ABI, its address range
                and a WEAK reference to its storage.  It pins nothing: a recorder that kept what it records would hide the bug.
  owners        weak references to the tensors whose raw data_ptr() goes into the device tables.
  decode_*      the address columns of those tables, read on the host.
  classify      where an address range lies in a torch.cuda.memory_snapshot(): private (the graph's pool), live, free, unknown.
  audit         the violations: a recorded range or an owner whose storage is gone (and not in the graph's own pool), a range the
                allocator holds as free, a table address no owner covers."""
import collections
import ctypes
import importlib
import os
import sys
import traceback

import numpy as np
import torch
from torch.multiprocessing.reductions import StorageWeakRef

MODULES = ("gsdd_amd.ops", "gsdd_amd._optim", "gsdd_amd.data")        # they import `ptr` by name from gsdd_amd._lib

Record = collections.namedtuple("Record", "address nbytes ref base storage_bytes label")
Owner = collections.namedtuple("Owner", "name ref base nbytes")
Violation = collections.namedtuple("Violation", "label address nbytes reason")

IMAGE_ROW = np.dtype([("w", "<u8"), ("n_out", "<i4"), ("n_in", "<i4"), ("ld", "<i4"), ("transpose", "<i4"), ("img", "<u8")])
WORST = ("private", "live", "free", "unknown")                        # a range that straddles blocks takes the worst class it touches


def _weak(t):
    s = t.untyped_storage()
    return StorageWeakRef(s), int(s.data_ptr()), int(s.nbytes())


class Recorder:
    """Context manager: while active, `ptr` of MODULES is a wrapper that appends a Record per non-None tensor to `records` and then
    calls the real `ptr`.  `is_device` decides which tensors are recorded and `forward` what produces the pointer; the defaults are
    `t.is_cuda` and the module's own `ptr` (which refuses a CPU tensor) -- the host test injects both to record CPU tensors."""

    def __init__(self, is_device=None, forward=None):
        self.records = []
        self._is_device = is_device if is_device is not None else (lambda t: t.is_cuda)
        self._forward = forward
        self._saved = []

    def _wrapper(self, real):
        records, is_device, forward = self.records, self._is_device, self._forward or real
        here = os.path.basename(__file__)

        def ptr(t):
            if t is not None and is_device(t):
                fr = [f for f in traceback.extract_stack(sys._getframe(1), limit=2)]
                label = " < ".join(f"{f.name} ({os.path.basename(f.filename)}:{f.lineno})" for f in reversed(fr)
                                   if os.path.basename(f.filename) != here)
                ref, base, sbytes = _weak(t)
                records.append(Record(int(t.data_ptr()), int(t.numel() * t.element_size()), ref, base, sbytes, label))
            return forward(t)
        return ptr

    def __enter__(self):
        for name in MODULES:
            mod = importlib.import_module(name)
            self._saved.append((mod, mod.ptr))
            mod.ptr = self._wrapper(mod.ptr)
        return self

    def __exit__(self, *exc):
        while self._saved:
            mod, real = self._saved.pop()
            mod.ptr = real
        return False


def host_ptr(t):
    """what the host test forwards to: the pointer of any tensor, no device check"""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ----------------------------------------------------------------------------- the addresses that never pass through ptr()
def owner(name, t):
    ref, base, nbytes = _weak(t)
    return Owner(name, ref, base, nbytes)


def owners(trainer):
    """-> [Owner]: weak references to the tensors whose raw data_ptr() a captured step finds in a device table or a copy node -- the
    parameters, the gradient arena, Adam's tables and state, the weight images and their descriptor table, the f32 null embedding.
    What a configuration does not have is skipped."""
    out = []

    def add(name, t):
        if torch.is_tensor(t) and t.numel():
            out.append(owner(name, t))

    dm = trainer.dm
    for n, p in dm.transformer.named_parameters():
        add("param." + n, p)
    add("param.empty_text_embed", getattr(dm, "empty_text_embed", None))
    add("arena.buf", getattr(trainer._arena, "buf", None))
    adam = trainer._adam
    for n in ("m", "v", "ema", "_table", "words", "partials", "_swap_table"):
        add("adam." + n, getattr(adam, n, None))
    im = trainer._images
    if im is not None:
        add("images.buf", getattr(im, "buf", None))
        add("images.table", getattr(im, "table", None))
        for i, t in enumerate(getattr(im, "_retired", None) or ()):
            add(f"images.retired{i}", t)
    add("null32", trainer._null32)
    return out


def decode_adam_table(table_host, staged):
    """MultiAdam._build_table's rows on the host (int64 [rows, 5 or 7]) -> {column name: (addresses, element counts)} for the address
    columns: 0 to 3 (parameter, gradient, m, v), plus 5 (the running average) when staged.  Null addresses (no gradient column in the
    swap table, no average) are left out."""
    t = np.asarray(table_host).astype(np.int64).reshape(-1, 7 if staged else 5)
    cols = {"param": 0, "grad": 1, "m": 2, "v": 3}
    if staged:
        cols["ema"] = 5
    out = {}
    for name, c in cols.items():
        keep = t[:, c] != 0
        if keep.any():
            out[name] = (t[keep, c].copy(), t[keep, 4].copy())
    return out


def decode_image_table(table_host):
    """_LinearImages.table on the host (uint8) -> {"w": weight addresses, "img": image addresses}, one entry per descriptor"""
    rows = np.ascontiguousarray(np.asarray(table_host, dtype=np.uint8)).view(IMAGE_ROW)
    return {"w": rows["w"].astype(np.int64), "img": rows["img"].astype(np.int64)}


def owner_of(address, nbytes, owner_list):
    """the name of the owner whose storage holds [address, address + nbytes), or None"""
    for o in owner_list:
        if o.base <= address and address + max(int(nbytes), 1) <= o.base + o.nbytes:
            return o.name
    return None


def unowned(label, addresses, owner_list, nbytes=None):
    """-> [Violation] for every address (with its byte count, default 4) that lies in no owner's storage"""
    out = []
    nbytes = [4] * len(addresses) if nbytes is None else nbytes
    for a, n in zip(addresses, nbytes):
        if owner_of(int(a), int(n), owner_list) is None:
            out.append(Violation(label, int(a), int(n), "a table address outside every owner recorded at capture time"))
    return out


# ----------------------------------------------------------------------------- the allocator's view
def _blocks(seg):
    """-> [(address, size, state)] of a segment; blocks without an address are laid end to end from the segment's address"""
    out, at = [], int(seg["address"])
    for b in seg.get("blocks", ()):
        a = int(b.get("address", at))
        out.append((a, int(b["size"]), b.get("state", "inactive")))
        at = a + int(b["size"])
    return out


def _private(seg, pool, before):
    if "segment_pool_id" in seg:
        pid = tuple(seg["segment_pool_id"])
        return pid == tuple(pool) if pool is not None else pid != (0, 0)
    if before is not None:                                   # no pool ids: a segment that appeared during the capture is the graph's
        return int(seg["address"]) not in {int(s["address"]) for s in before}
    return False


def classify(ranges, snapshot, pool=None, before=None):
    """ranges: [(address, nbytes)]; snapshot: what torch.cuda.memory_snapshot() returns -> one class per range:
    "private" (a segment of the graph's pool: `pool` is the graph's pool id, None takes every non-default pool; snapshots without
    pool ids: a segment that is not in `before`, the segment list from before the capture), "live" (an active_allocated block),
    "free" (an inactive block, or one whose free is pending), "unknown" (in no segment: a host pointer, which ptr() never produces).
    A range that touches several blocks takes the worst class among them, in the order private < live < free < unknown."""
    segs = sorted(((int(s["address"]), int(s["total_size"]), s) for s in snapshot), key=lambda x: x[0])
    out = []
    for address, nbytes in ranges:
        lo, hi = int(address), int(address) + max(int(nbytes), 1)
        worst, covered = 0, 0
        for sa, ssz, seg in segs:
            if sa + ssz <= lo or sa >= hi:
                continue
            if _private(seg, pool, before):
                covered += min(hi, sa + ssz) - max(lo, sa)
                continue
            for ba, bsz, state in _blocks(seg):
                n = min(hi, ba + bsz) - max(lo, ba)
                if n <= 0:
                    continue
                covered += n
                worst = max(worst, WORST.index("live" if state == "active_allocated" else "free"))
        if covered < hi - lo:
            worst = WORST.index("unknown")
        out.append(WORST[worst])
    return out


def audit(records, owner_refs, snapshot=None, pool=None, before=None, addresses=None):
    """-> [Violation], empty when clean.
    A record (or an owner) is a violation if its storage weak reference has expired and its range is not in the graph's own pool
    (without a snapshot nothing is known to be private: every expired reference counts -- the sampler's bare captures have no pool).
    With a snapshot a record is also a violation if the allocator holds its range as free, or knows no segment for it.
    addresses: {label: (addresses, byte counts or None)} decoded from the device tables; each must lie in an owner's storage."""
    out, seen = [], set()
    items = [(r.label, r.address, r.nbytes, r.ref) for r in records if r.nbytes > 0]
    items += [("owner " + o.name, o.base, o.nbytes, o.ref) for o in owner_refs]
    cls = classify([(a, n) for _, a, n, _ in items], snapshot, pool, before) if snapshot is not None else [None] * len(items)
    for (label, a, n, ref), c in zip(items, cls):
        reason = None
        if ref.expired() and c != "private":
            reason = "the storage is gone (no tensor owns this range any more)" + (f"; the allocator has it as {c}" if c else "")
        elif c == "free":
            reason = "the allocator holds this range as free"
        elif c == "unknown":
            reason = "the range lies in no segment of the allocator"
        if reason is not None and (label, a, n) not in seen:
            seen.add((label, a, n))
            out.append(Violation(label, a, n, reason))
    for label, (addr, nbytes) in (addresses or {}).items():
        out += unowned(label, addr, owner_refs, nbytes)
    return out
