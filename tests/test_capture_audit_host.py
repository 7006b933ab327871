"""tests/capture_audit.py checked without a GPU: the recorder on CPU tensors (what it notes, that it keeps nothing alive, that `ptr` comes
back after an exception), `classify` on hand-written allocator snapshots, the table decoders on tables MultiAdam and _LinearImages
build on the CPU, and the hook of `_lib.ptr` that lets an ops.Graph keep what it records."""
import gc

import numpy as np
import pytest
import torch

from tests import capture_audit as ca


def recorder():
    return ca.Recorder(is_device=lambda t: True, forward=ca.host_ptr)


def call_lincomb_like(ops, a, b):
    """stands in for an ops wrapper: hands two tensors to the module's `ptr`"""
    return ops.ptr(a), ops.ptr(b), ops.ptr(None)


def test_recorder_notes_ranges_and_keeps_nothing_alive():
    import gsdd_amd
    from gsdd_amd import _optim, data, ops
    real = (ops.ptr, _optim.ptr, data.ptr)
    a, b = torch.arange(64, dtype=torch.float32), torch.zeros(10, dtype=torch.float64)
    view = a[16:32]
    with recorder() as rec:
        assert ops.ptr is not real[0] and _optim.ptr is not real[1] and data.ptr is not real[2]
        pa, pv, none = call_lincomb_like(ops, a, view)
        _optim.ptr(b)
    assert (ops.ptr, _optim.ptr, data.ptr) == real
    assert none is None and pa.value == a.data_ptr() and pv.value == view.data_ptr()
    ra, rv, rb = rec.records                                     # (None is not recorded)
    assert (ra.address, ra.nbytes, ra.base, ra.storage_bytes) == (a.data_ptr(), 256, a.data_ptr(), 256)
    assert (rv.address, rv.nbytes, rv.base, rv.storage_bytes) == (a.data_ptr() + 64, 64, a.data_ptr(), 256)
    assert (rb.address, rb.nbytes) == (b.data_ptr(), 80)
    assert "call_lincomb_like" in ra.label and "test_recorder_notes_ranges" in ra.label and "test_capture_audit_host.py" in ra.label
    assert not any(r.ref.expired() for r in rec.records) and ca.audit(rec.records, []) == []
    # a deleted tensor shows as expired -- the recorder itself holds nothing
    del b
    gc.collect()
    assert rb.ref.expired() and not ra.ref.expired()
    got = ca.audit(rec.records, [])
    assert [(v.label, v.address, v.nbytes) for v in got] == [(rb.label, rb.address, 80)] and "gone" in got[0].reason
    # a view keeps its storage alive
    del a
    gc.collect()
    assert not ra.ref.expired() and not rv.ref.expired()
    del view
    gc.collect()
    assert ra.ref.expired() and rv.ref.expired() and len(ca.audit(rec.records, [])) == 3
    assert gsdd_amd._lib._keeper is None


def test_ptr_is_restored_after_an_exception():
    from gsdd_amd import _optim, data, ops
    real = (ops.ptr, _optim.ptr, data.ptr)
    with pytest.raises(RuntimeError, match="inside"):
        with recorder():
            assert ops.ptr is not real[0]
            raise RuntimeError("inside")
    assert (ops.ptr, _optim.ptr, data.ptr) == real
    # the default recorder forwards to the real ptr, which refuses a CPU tensor -- and records none
    import gsdd_amd
    with ca.Recorder() as rec:
        with pytest.raises(gsdd_amd.GsddError):
            ops.ptr(torch.zeros(3))
    assert rec.records == [] and ops.ptr is real[0]


def test_a_recording_graph_keeps_what_ptr_sees():
    """`_lib.ptr` appends to the list of the graph being recorded, and to nothing otherwise (the launch path outside a capture pays one
    comparison).  The device check comes first, so the hook is driven here through a tensor stand-in that claims to be on the device."""
    import gsdd_amd
    from gsdd_amd import _lib, ops

    class OnDevice:
        is_cuda = True

        def is_contiguous(self):
            return True

        def data_ptr(self):
            return 4096

    g = ops.Graph()
    assert g.kept == [] and _lib._keeper is None
    t = OnDevice()
    assert ops.ptr(t).value == 4096 and g.kept == []
    _lib._keeper = g.kept                                       # what Graph.begin does after the capture has begun
    try:
        assert ops.ptr(t).value == 4096 and ops.ptr(None) is None
    finally:
        _lib._keeper = None
    assert g.kept == [t]
    with pytest.raises(gsdd_amd.GsddError):
        ops.ptr(torch.zeros(2))


# ----------------------------------------------------------------------------- classify
MB = 1 << 20


def snapshot(with_address=True, with_pool=True):
    def seg(address, blocks, pool=(0, 0)):
        bl, at = [], address
        for size, state in blocks:
            b = {"size": size, "requested_size": size, "state": state}
            if with_address:
                b["address"] = at
            bl.append(b)
            at += size
        s = {"device": 0, "address": address, "total_size": at - address, "blocks": bl, "segment_type": "large"}
        if with_pool:
            s["segment_pool_id"] = pool
        return s
    return [seg(16 * MB, [(MB, "active_allocated"), (MB, "inactive"), (2 * MB, "active_allocated"), (MB, "active_pending_free")]),
            seg(64 * MB, [(4 * MB, "active_allocated"), (4 * MB, "inactive")], pool=(0, 7))]


@pytest.mark.parametrize("with_address", [True, False])
def test_classify_on_hand_written_snapshots(with_address):
    snap = snapshot(with_address)
    ranges = [(16 * MB + 100, 1000),               # inside an active block
              (17 * MB + 8, 64),                   # inside an inactive block
              (17 * MB - 16, 32),                  # straddles active | inactive: the worst class wins
              (18 * MB, 2 * MB),                   # exactly an active block
              (20 * MB + 4, 4),                    # a block whose free is pending
              (64 * MB + 5 * MB, 128),             # the private pool's segment, whatever the block's state
              (40 * MB, 16),                       # in no segment
              (21 * MB - 8, 16),                   # runs off the end of a segment
              (16 * MB, 0)]                        # an empty range counts as its first byte
    want = ["live", "free", "free", "live", "free", "private", "unknown", "unknown", "live"]
    assert ca.classify(ranges, snap, pool=(0, 7)) == want
    assert ca.classify(ranges, snap) == want                                   # no pool named: every non-default pool is private
    other = ["free" if w == "private" else w for w in want]
    assert ca.classify(ranges, snap, pool=(0, 9)) == other                     # another graph's pool is not this graph's


def test_classify_without_pool_ids_diffs_the_segment_lists():
    snap = snapshot(with_pool=False)
    r = [(64 * MB + 5 * MB, 128), (16 * MB + 100, 8)]
    assert ca.classify(r, snap) == ["free", "live"]
    assert ca.classify(r, snap, before=snap[:1]) == ["private", "live"]       # the second segment appeared during the capture
    assert ca.classify(r, snap, before=snap) == ["free", "live"]


def test_audit_reads_the_snapshot():
    a = torch.zeros(8)
    with recorder() as rec:
        from gsdd_amd import ops
        ops.ptr(a)
    r = rec.records[0]
    live = [{"address": r.base - 64, "total_size": 4096, "segment_pool_id": (0, 0),
             "blocks": [{"size": 4096, "state": "active_allocated"}]}]
    freed = [dict(live[0], blocks=[{"size": 4096, "state": "inactive"}])]
    private = [dict(freed[0], segment_pool_id=(0, 3))]
    assert ca.audit(rec.records, [], live) == []
    assert [v.reason for v in ca.audit(rec.records, [], freed)] == ["the allocator holds this range as free"]
    assert "no segment" in ca.audit(rec.records, [], [])[0].reason
    del a
    gc.collect()
    assert "gone" in ca.audit(rec.records, [], live)[0].reason               # somebody else's block now: live, and not ours
    assert ca.audit(rec.records, [], private, pool=(0, 3)) == []             # the graph's own pool outlives the tensor


# ----------------------------------------------------------------------------- the table decoders
def adam_case(staged):
    from gsdd_amd._optim import MultiAdam
    g = torch.Generator().manual_seed(1)
    params = [("a", torch.randn(5, generator=g)), ("b", torch.randn(3, 7, generator=g)), ("c", torch.randn(4096 + 2, generator=g))]
    kw = dict(max_grad_norm=1.0, ema_decay=0.999) if staged else {}
    opt = MultiAdam(params, 1e-3, (0.9, 0.96), 1e-8, **kw)
    arena = torch.zeros(8 + 24 + 4100)
    grads = {"a": arena[0:5], "b": arena[8:29].view(3, 7), "c": arena[32:32 + 4098]}
    own = [ca.owner("param." + n, p) for n, p in params] + [ca.owner("arena.buf", arena), ca.owner("adam.m", opt.m), ca.owner("adam.v", opt.v)]
    if staged:
        own.append(ca.owner("adam.ema", opt.ema))
    return opt, params, arena, grads, own


@pytest.mark.parametrize("staged", [False, True])
def test_adam_table_addresses_lie_in_their_owners(staged):
    opt, params, arena, grads, own = adam_case(staged)
    cols = ca.decode_adam_table(opt._build_table(grads), staged)
    assert set(cols) == {"param", "grad", "m", "v"} | ({"ema"} if staged else set())
    for name, (addr, count) in cols.items():
        assert len(addr) == 4 and list(count) == [5, 21, 4096, 2]
        names = [ca.owner_of(int(a), 4 * int(n), own) for a, n in zip(addr, count)]
        want = {"param": ["param.a", "param.b", "param.c", "param.c"], "grad": ["arena.buf"] * 4}.get(name, ["adam." + name] * 4)
        assert names == want, name
        assert ca.unowned("adam table " + name, addr, own, 4 * count) == []
    assert ca.audit([], own, addresses={k: (a, 4 * n) for k, (a, n) in cols.items()}) == []
    # the swap table carries no gradient column
    assert "grad" not in ca.decode_adam_table(opt._build_table(None), staged)
    # one gradient moved to a fresh tensor (a replaced arena): reported against the gradient column, and only there
    moved = dict(grads, b=torch.zeros(3, 7))
    cols = ca.decode_adam_table(opt._build_table(moved), staged)
    got = ca.audit([], own, addresses={k: (a, 4 * n) for k, (a, n) in cols.items()})
    assert [(v.label, v.address, v.nbytes) for v in got] == [("grad", moved["b"].data_ptr(), 84)]
    # ... and an arena that died is reported as an owner
    del arena, grads, moved
    gc.collect()
    assert [v.label for v in ca.audit([], own)] == ["owner arena.buf"]


def test_image_table_addresses_lie_in_their_owners():
    from gsdd_amd.d3pm_train import _LinearImages
    from tests.test_optim_host import tiny_model
    tr = tiny_model(2).transformer
    im = _LinearImages(tr)
    im._build()                                                # (CPU: the table and the image buffer, no launch)
    cols = ca.decode_image_table(im.table.numpy())
    assert len(cols["w"]) == len(cols["img"]) == im.n_desc == 2 * 12 and list(cols["w"]) == im.ptrs
    own = [ca.owner("param." + n, p) for n, p in tr.named_parameters()] + [ca.owner("images.buf", im.buf)]
    assert ca.unowned("image table w", cols["w"], own) == [] and ca.unowned("image table img", cols["img"], own) == []
    assert {ca.owner_of(int(a), 4, own) for a in cols["img"]} == {"images.buf"}
    assert all(ca.owner_of(int(a), 4, own).startswith("param.blocks.") for a in cols["w"])
    old = cols["img"]
    im.cross, im.ptrs = True, None
    im._build()                                                # the cross-attention images join: a new buffer, a new table
    assert len(ca.unowned("image table img", old, [ca.owner("images.buf", im.buf)])) == len(old)


def test_owners_of_a_trainer_skip_what_a_configuration_lacks():
    from gsdd_amd._optim import GradArena, MultiAdam
    from gsdd_amd.d3pm_train import D3PMTrainer
    from tests.test_optim_host import tiny_model
    dm = tiny_model(1)
    tr = D3PMTrainer(dm)
    tr._arena = GradArena("cpu", 16)
    tr._arena.reset()
    tr._adam = MultiAdam(list(dm.transformer.named_parameters()), 1e-3, (0.5, 0.999), 1e-8)
    names = [o.name for o in ca.owners(tr)]
    n_param = len(list(dm.transformer.named_parameters()))
    assert names[:n_param] == ["param." + n for n, _ in dm.transformer.named_parameters()]
    assert names[n_param:] == ["param.empty_text_embed", "arena.buf", "adam.m", "adam.v"]
    tr._adam = MultiAdam(list(dm.transformer.named_parameters()), 1e-3, (0.5, 0.999), 1e-8, max_grad_norm=1.0, ema_decay=0.9)
    tr._null32 = torch.zeros(77, 512)
    names = [o.name for o in ca.owners(tr)][n_param:]
    assert names == ["param.empty_text_embed", "arena.buf", "adam.m", "adam.v", "adam.ema", "adam.words", "adam.partials", "null32"]
    assert not any(o.ref.expired() for o in ca.owners(tr))
