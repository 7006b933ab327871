"""A captured graph keeps alive everything it replays on -- checked on both capture sites, on the MI355X.

The trainer's step (`D3PMTrainer._capture`, torch.cuda.graph) and the sampler's ops (`_Lane.issue`, ops.Graph) are recorded with
tests/capture_audit.py: every tensor handed to the C ABI while the graph is recorded, weakly; the tensors whose raw addresses sit in
the device tables (`owners`); the tables themselves, decoded on the host.  `audit` then says whether every one of those ranges is still
owned -- by a live tensor, or by the graph's own allocator pool.

SAFETY RULE OF THIS FILE: a graph is replayed only after `audit()` has returned clean for it at that moment.  The trainer's graphs are
wrapped in `Guarded`, whose replay() audits first; the sampler's replays go through `LaneAudit`, which does not launch a graph with a
violation.  A violation fails the test there and nothing further is launched.  The planted graphs of the first test are never launched.
No test frees memory under a graph to see what happens: the events are the reads, allocations and further steps a training loop makes.

Model: the d3pm_L64 golden model (two layers, K = 32, L = 64, cond_dim = 32; the captured step needs L % 32 == 0), cfg["B"] = 2 clips in
the trainer scenarios; the sampler scenarios take 8 clips, the fewest that run in two lanes (a lane keeps at least 4).

Every trainer scenario runs twice in the reproducible mode (deterministic=True), with and without its host-side events, on the same
batches, timesteps and noise stream: the losses and every weight must be bit-identical -- the events are host-side reads and
allocations and may not move a bit of a replayed step.  No tolerance is involved.  Scenarios 3 and 5 make further optimiser steps on
other batch shapes: those steps belong to both runs (they move the weights), the events around them to one; both are also compared with
the launch-by-launch trainer at the bounds of test_captured_training_step_equals_the_eager_steps."""
import gc

import numpy as np
import pytest
import torch

from tests import capture_audit as ca
from tests.test_gpu_parity import build_d3pm
from tests.test_gpu_training import build

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()
    return gsdd_amd


def show(violations, limit=12):
    return f"{len(violations)} violation(s): " + "; ".join(f"{v.label} @ {v.address:#x} + {v.nbytes}: {v.reason}" for v in violations[:limit])


def release():
    """graphs are released before a test returns: one that the cyclic collector frees during a later test's capture aborts the process"""
    gc.collect()
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- (a) the audit sees a planted violation
def test_the_audit_names_a_planted_violation(G):
    """Two graphs that would replay on memory nobody owns; neither is ever launched.
    1. an ops.Graph on a side stream around one ops.lincomb: while the graph keeps what it recorded the audit is clean; with its list
       emptied (the library before ops.Graph kept anything) and the output dropped, the audit names the output's range.
    2. a torch.cuda.graph around one ops.lincomb that reads a default-pool tensor allocated before the capture and dropped after it:
       the audit names that range; the output, allocated inside the capture, lies in the graph's pool and is no violation."""
    ops = G.ops
    n = 4096
    graph = None
    try:
        a, b, c = (torch.full((n,), float(i), device="cuda") for i in (1, 2, 3))
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            warm = torch.empty_like(b)                        # the capture's allocation then comes from the stream's cached block
            del warm
            g = ops.Graph()
            with ca.Recorder() as rec:
                g.begin(st)
                try:
                    out = ops.lincomb(a, b, c, 0.5, stream=st)
                finally:
                    g.end(st)
        assert G._lib._keeper is None
        assert len(rec.records) == 4 and all("lincomb" in r.label for r in rec.records)
        addr = out.data_ptr()
        assert sum(t is out for t in g.kept) == 1 and len(g.kept) == 4
        del out
        gc.collect()
        assert ca.audit(rec.records, []) == [], "the graph does not keep the output it recorded"
        g.kept.clear()                                        # the planted violation: nobody owns the output any more
        gc.collect()
        got = ca.audit(rec.records, [])
        assert [(v.address, v.nbytes) for v in got] == [(addr, 4 * n)] and "lincomb" in got[0].label, show(got)
        del g                                                 # destroyed unlaunched

        graph = torch.cuda.CUDAGraph()
        before = torch.cuda.memory_snapshot()
        with ca.Recorder() as rec:
            with torch.cuda.graph(graph):
                out = ops.lincomb(a, b, c, 0.5)
        pool, a_addr = graph.pool(), a.data_ptr()
        assert ca.audit(rec.records, [], torch.cuda.memory_snapshot(), pool=pool, before=before) == []
        del out                                               # allocated inside the capture: the graph's pool holds it
        gc.collect()
        got = ca.audit(rec.records, [], torch.cuda.memory_snapshot(), pool=pool, before=before)
        assert got == [], "a tensor of the graph's own pool was reported: " + show(got)
        del a                                                 # the planted violation: a default-pool input dropped under the graph
        gc.collect()
        got = ca.audit(rec.records, [], torch.cuda.memory_snapshot(), pool=pool, before=before)
        assert [(v.address, v.nbytes) for v in got] == [(a_addr, 4 * n)] and "lincomb" in got[0].label, show(got)
    finally:
        if graph is not None:
            graph.reset()                                     # destroyed unlaunched
        del graph
        release()


# ----------------------------------------------------------------------------- (b) the trainer
class Guarded:
    """stands in for st["graph"]: replay() audits the graph first and launches nothing on a violation"""

    def __init__(self, graph, check):
        self.graph, self.check, self.replays = graph, check, 0

    def replay(self):
        got = self.check()
        assert not got, "not replayed -- " + show(got)
        self.replays += 1
        self.graph.replay()

    def pool(self):
        return self.graph.pool()


class Audited:
    """A trainer whose every capture is recorded and whose every replay is guarded."""

    def __init__(self, trainer):
        self.tr, self.info, self.guards = trainer, {}, []
        real = trainer._capture

        def capture(*args, **kw):
            before = torch.cuda.memory_snapshot()
            with ca.Recorder() as rec:
                st = real(*args, **kw)
            self.note(st, rec.records, before)
            return st
        trainer._capture = capture

    def note(self, st, records, before):
        tr = self.tr
        adam, im = tr._adam, tr._images
        addresses = {}
        for col, (addr, count) in ca.decode_adam_table(adam._table.cpu().numpy(), adam.staged).items():       # read once, outside the capture
            addresses["adam table " + col] = (addr, 4 * count)
        if im is not None:
            for col, addr in ca.decode_image_table(im.table.cpu().numpy()).items():
                addresses["image table " + col] = (addr, None)
        info = dict(records=records, owners=ca.owners(tr), addresses=addresses, before=before, pool=st["graph"].pool())
        self.info[id(st)] = info
        snap = torch.cuda.memory_snapshot()
        cls = ca.classify([(r.address, r.nbytes) for r in records], snap, info["pool"], before)
        print(f"captured: {len(records)} recorded ranges {dict((c, cls.count(c)) for c in set(cls))}, {len(info['owners'])} owners, pool "
              f"{info['pool']}, pool ids in the snapshot {sorted({tuple(s.get('segment_pool_id', ())) for s in snap})}, blocks carry an "
              f"address: {all('address' in b for s in snap for b in s['blocks'])}, pinned bytes "
              f"{ {k: v.numel() * v.element_size() for k, v in st.get('pins', {}).items()} }")
        st["graph"] = Guarded(st["graph"], lambda: self.audit(st))
        self.guards.append(st["graph"])

    def audit(self, st):
        i = self.info[id(st)]
        gc.collect()
        return ca.audit(i["records"], i["owners"], torch.cuda.memory_snapshot(), pool=i["pool"], before=i["before"],
                        addresses=i["addresses"])

    def audit_all(self):
        return [v for st in self.tr._graphs.values() for v in self.audit(st)]

    def close(self):
        """Every graph is destroyed here, explicitly: a failed assertion keeps frames (and through them a graph) alive in its traceback,
        and a CUDAGraph that the cyclic collector frees during a later test's capture aborts the process."""
        torch.cuda.synchronize()
        self.tr._graph, self.tr._graphs = None, {}
        for g in self.guards:
            g.graph.reset()
        self.guards, self.info = [], {}


def churn(aud):
    """what any other user of the allocator does between two steps: buffers of the sizes the step's own buffers have are allocated,
    written and dropped again"""
    sizes = sorted({o.nbytes for i in aud.info.values() for o in i["owners"] if not o.name.startswith("param.")})
    junk = [torch.full((n,), 0x4b, dtype=torch.uint8, device="cuda") for n in sizes for _ in range(2)]
    torch.cuda.synchronize()
    del junk
    gc.collect()


def batches(cfg, n, Te=1, seed=41, B=None):
    B = cfg["B"] if B is None else B
    g = torch.Generator().manual_seed(seed)
    return [dict(x0=torch.randint(0, cfg["K"], (B, cfg["L"]), generator=g).cuda(), cond=torch.randn(B, Te, cfg["cond_dim"], generator=g).cuda(),
                 t=torch.randint(0, cfg["T"], (B,), generator=g).cuda(), pt=torch.full((B,), 1.0 / cfg["T"]).cuda()) for _ in range(n)]


def shaped(step, B):
    """the step's batch cut or repeated to B clips"""
    reps = -(-B // step["x0"].shape[0])
    return {k: torch.cat([v] * reps)[:B].contiguous() for k, v in step.items()}


class Scenario:
    trainer_kw = {}
    sync_around_steps = False
    captures = 1                       # how often the run captures

    def setup(self, dm):
        pass

    def steps(self, cfg):
        return batches(cfg, 6)

    def events(self, aud, dm, i, step):
        """host-side events before step i (i >= 3: the step before was captured or replayed)"""


def run(G, golden, sc, events, graph=True, monkeypatch=None):
    """-> (losses, weights by name) of the scenario's steps; graph=False: the launch-by-launch trainer (GSDD_TRAIN_GRAPH=0)"""
    from gsdd_amd.d3pm_train import D3PMTrainer
    sd, _, cfg = golden("d3pm_L64")
    monkeypatch.setenv("GSDD_TRAIN_GRAPH", "1" if graph else "0")
    dm = build(G, sd, cfg).train()
    dm.empty_text_embed.data = torch.randn(77, cfg["cond_dim"], generator=torch.Generator().manual_seed(9), dtype=torch.float64).cuda()
    sc.setup(dm)
    dm.set_noise(cfg["noise_seed"], stream=3)
    tr = D3PMTrainer(dm, **dict(dict(lr=1e-3, deterministic=True), **sc.trainer_kw))
    aud = Audited(tr)
    losses = []
    try:
        for i, step in enumerate(sc.steps(cfg)):
            if i >= 3 and graph:
                if events:
                    sc.events(aud, dm, i, step)
                    gc.collect()
                got = aud.audit_all()
                assert not got, f"before step {i}, nothing replayed -- " + show(got)
            if sc.sync_around_steps and events:
                torch.cuda.synchronize()
            losses.append(tr.step(**step)[0].item())
            if sc.sync_around_steps and events:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        assert not tr._graph_failed and (tr._graph is not None) == graph
        if graph:
            assert tr.captures == sc.captures and tr._graph["graph"].replays >= 3, (tr.captures, tr._graph["graph"].replays)
        weights = {k: v.detach().clone() for k, v in dm.transformer.state_dict().items()}
        weights["empty_text_embed"] = dm.empty_text_embed.detach().clone()
        return losses, weights
    finally:
        aud.close()
        del aud, tr, dm
        release()


def twin_runs(G, golden, monkeypatch, sc, eager=False):
    plain = run(G, golden, sc, False, monkeypatch=monkeypatch)
    with_events = run(G, golden, sc, True, monkeypatch=monkeypatch)
    print("losses without / with the events:", plain[0], with_events[0])
    assert with_events[0] == plain[0], "the host-side events moved a loss"
    moved = [k for k, w in plain[1].items() if not torch.equal(with_events[1][k], w)]
    assert not moved, f"the host-side events moved {len(moved)} weight tensors: {moved[:6]}"
    assert all(np.isfinite(plain[0]))
    if eager:
        ref = run(G, golden, sc, False, graph=False, monkeypatch=monkeypatch)
        np.testing.assert_allclose(with_events[0], ref[0], rtol=2e-5)
        for k, w in ref[1].items():
            if k.endswith("attn1.key.bias"):              # (mathematically zero gradient: see test_captured_training_step_equals_the_eager_steps)
                continue
            torch.testing.assert_close(with_events[1][k], w, atol=2e-6, rtol=1e-5, msg=lambda m, k=k: f"{k}: {m}")


class Nothing(Scenario):
    def events(self, aud, dm, i, step):
        gc.collect()
        torch.cuda.synchronize()


class ReadTheArena(Scenario):
    """The recipe of DESIGN.md section 9 at L = 64: synchronize() around every step, eager reductions over the arena between replays.
    This is the scenario that found the cause of that item: with gsdd_batch_rowsum's zero fill as a hipMemsetAsync node the arena
    held 4.8e24 here after the second replay (attn2.proj / attn2.value gradients first), while the run without the reads stayed clean.
    The bound on the arena's largest entry is a sanity bar, not a tolerance: the loss is O(10) and the weights O(1), a gradient entry
    of 1e6 is not a gradient."""
    sync_around_steps = True

    def events(self, aud, dm, i, step):
        buf = aud.tr._arena.buf
        stats = (buf.abs().max().item(), buf.sum().item(), bool(torch.isfinite(buf).all()))
        assert stats[2] and stats[0] < 1e6, stats


class ShortBatch(Scenario):
    """an epoch's short last batch (B = 1) gets its own graph; then back to the full-batch graph"""
    captures = 2

    def steps(self, cfg):
        s = batches(cfg, 6)
        return s[:3] + [shaped(s[3], 1)] + s[3:]

    def events(self, aud, dm, i, step):
        churn(aud)
        if i == 4:
            assert len(aud.tr._graphs) == 2


class ThirdShape(ShortBatch):
    """a third batch shape pops the oldest graph; the two that remain audit clean (run()'s audit before every step), and the full
    batch is captured again when it returns"""
    captures = 4

    def steps(self, cfg):
        s = batches(cfg, 6)
        return s[:3] + [shaped(s[3], 1), shaped(s[4], 3)] + s[3:]

    def events(self, aud, dm, i, step):
        churn(aud)
        assert len(aud.tr._graphs) == (1 if i == 3 else 2)


class LargerEagerCalls(Scenario):
    """Eager loss_and_grads calls between replays, as a validation pass makes them.  A call on 2 B clips does NOT grow the arena at any
    shape: the arena holds the parameter gradients and the position-embedding scratch, nothing sized by the batch (asserted below).  What
    does grow it is a call whose gradient dict has one more entry, the learned null embedding's (condition dropout with learnable_cf):
    that call raises the arena's demand and the next one replaces `buf`.  A call with three condition tokens after one-token steps
    replaces the weight images and their table (the cross-attention images join).  The noise stream and the loss history, which such
    calls advance on purpose, are put back: the two runs must see the same draws."""

    def events(self, aud, dm, i, step):
        if i != 3:
            return
        tr = aud.tr
        keep = (dm.noise_stream, dm.Lt_history.clone(), dm.Lt_count.clone(), dm.empty_text_embed.data.clone())
        buf0, img0, tab0, B = tr._arena.buf, tr._images.buf, tr._images.table, step["x0"].shape[0]
        big = shaped(step, 2 * B)
        tr.loss_and_grads(big["x0"], big["cond"], t=big["t"], pt=big["pt"])
        assert tr._arena.buf is buf0 and tr._arena.want <= buf0.numel(), "a larger batch grew the arena"
        dm.learnable_cf = True
        mask = torch.tensor([True] + [False] * (B - 1)).cuda()
        for _ in range(2):                                   # the first call raises the demand, the second one's reset replaces buf
            tr.loss_and_grads(step["x0"], step["cond"], t=step["t"], pt=step["pt"], drop=mask)
        dm.learnable_cf = False
        assert tr._arena.buf is not buf0 and tr._arena.buf.numel() > buf0.numel(), "the arena did not grow"
        cond3 = torch.randn(B, 3, step["cond"].shape[2], generator=torch.Generator().manual_seed(3)).cuda()
        tr.loss_and_grads(step["x0"], cond3, t=step["t"], pt=step["pt"])
        assert tr._images.buf is not img0 and tr._images.table is not tab0, "the weight images were not rebuilt"
        dm.noise_stream = keep[0]
        dm.Lt_history.copy_(keep[1])
        dm.Lt_count.copy_(keep[2])
        dm.empty_text_embed.data.copy_(keep[3])
        del buf0, img0, tab0
        churn(aud)


class OptimiserStage(Scenario):
    """clipping, decay, averaged weights, the guard and a warm-up schedule: the state block, the partial sums and the EMA swap table
    are in play; the averaged weights are swapped in and out between replays"""

    def __init__(self):
        from gsdd_amd.d3pm_train import linear_warmup
        self.trainer_kw = dict(lr_schedule=linear_warmup(1e-3, 5), max_grad_norm=1.0, weight_decay=0.01, ema_decay=0.99, skip_nonfinite=True)

    def events(self, aud, dm, i, step):
        with aud.tr.ema_weights():
            pass
        churn(aud)


class DropoutAndLengths(Scenario):
    """condition dropout with a learned null embedding (the f32 copy, the write-back copy node) on three condition tokens with
    per-sample lengths (the static length buffer)"""

    def setup(self, dm):
        dm.learnable_cf, dm.cond_drop_prob = True, 0.5

    def steps(self, cfg):
        return [dict(s, cond_len=[3, 2][:cfg["B"]]) for s in batches(cfg, 6, Te=3)]

    def events(self, aud, dm, i, step):
        churn(aud)


SCENARIOS = {"nothing": (Nothing, False), "read_the_arena": (ReadTheArena, False), "short_batch": (ShortBatch, True),
             "larger_eager_calls": (LargerEagerCalls, False), "third_shape": (ThirdShape, True), "optimiser_stage": (OptimiserStage, False),
             "dropout_and_lengths": (DropoutAndLengths, False)}


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_trainer_graphs_replay_on_memory_they_own(G, golden, monkeypatch, name):
    cls, eager = SCENARIOS[name]
    twin_runs(G, golden, monkeypatch, cls(), eager=eager)


def test_a_captured_step_pins_its_buffers(G, golden, monkeypatch):
    """st["pins"] holds the very tensors the trainer had at capture time, and a replaced arena belongs to later steps only"""
    from gsdd_amd.d3pm_train import D3PMTrainer
    sd, _, cfg = golden("d3pm_L64")
    monkeypatch.setenv("GSDD_TRAIN_GRAPH", "1")
    dm = build(G, sd, cfg).train()
    dm.set_noise(cfg["noise_seed"], stream=3)
    tr = D3PMTrainer(dm, lr=1e-3, deterministic=True)
    aud = Audited(tr)
    try:
        for step in batches(cfg, 3):
            tr.step(**step)
        pins = tr._graph["pins"]
        assert set(pins) == {"arena.buf", "adam.table", "adam.m", "adam.v", "images.buf", "images.table"}
        assert pins["arena.buf"] is tr._arena.buf and pins["adam.table"] is tr._adam._table and pins["images.buf"] is tr._images.buf
        assert not hasattr(tr._images, "_retired")
        old = ca.owner("arena.buf", tr._arena.buf)
        tr._arena.buf = None                                  # what GradArena.reset does when a step outgrew the buffer
        gc.collect()
        assert not old.ref.expired() and aud.audit_all() == []
        tr._arena.buf = pins["arena.buf"]
        print("bytes a captured step pins at B = 2, L = 64:", {k: v.numel() * v.element_size() for k, v in pins.items()},
              "total", sum(v.numel() * v.element_size() for v in pins.values()))
    finally:
        aud.close()
        del aud, tr, dm
        release()


# ----------------------------------------------------------------------------- (c) the sampler
class LaneAudit:
    """Wraps _Lane.issue: a "capture" is recorded per (lane, kind); before every "replay" that graph's records are audited with the
    weak-reference check (a bare stream capture has no pool: whatever it touches must be owned), and a graph with a violation is not
    launched.  The violations are collected; the test fails after the call."""

    def __init__(self, monkeypatch, lane_cls):
        self.records, self.lanes, self.violations, self.replays = {}, [], [], 0
        real = lane_cls.issue

        def issue(lane, kind, action, trace=None):
            key = (id(lane), kind)
            if action == "capture":
                with ca.Recorder() as rec:
                    real(lane, kind, action, trace)
                gc.collect()
                self.records[key] = rec.records
                self.lanes.append(lane)                       # (ids stay unique for the call; the lane's own buffers live as long anyway)
                return
            if action == "replay":
                got = ca.audit(self.records[key], [])
                if got:
                    self.violations += got
                    return
                self.replays += 1
            real(lane, kind, action, trace)
        monkeypatch.setattr(lane_cls, "issue", issue)

    def reset(self):
        self.records, self.lanes, self.violations, self.replays = {}, [], [], 0


SB = 8


def sampler_cases(cfg):
    g = torch.Generator().manual_seed(5)
    cond, cf = torch.randn(SB, 1, cfg["cond_dim"], generator=g).cuda(), torch.randn(SB, 1, cfg["cond_dim"], generator=g).cuda()
    cond3, cf3 = torch.randn(SB, 3, cfg["cond_dim"], generator=g).cuda(), torch.randn(SB, 3, cfg["cond_dim"], generator=g).cuda()
    content = torch.randint(0, cfg["K"], (SB, cfg["L"]), generator=g).cuda()
    mask = (torch.rand(SB, cfg["L"], generator=g) < 0.4).cuda()
    texts = ["x"] * SB

    def purity(dm):
        ns = [0] * cfg["T"]
        ns[1:33] = [2] * 32                                   # 32 reveals of two positions, then the final step
        ns[0] = 1
        dm.n_sample, dm.prior_ps, dm.prior_rule = ns, 64, 2

    # name -> (set-up, call, lanes, guidance copies, op kinds that must have been captured)
    return {
        "plain_two_lanes": (None, lambda dm, kw: dm.sample(texts, None, cond, cond.clone(), filter_ratio=0, **kw), 2, 1, {"step"}),
        "guided": (None, lambda dm, kw: dm.sample(texts, None, cond, cf, filter_ratio=0, **kw), 2, 2, {"step"}),
        "skip_step": (None, lambda dm, kw: dm.sample_fast(texts, None, cond, filter_ratio=0, skip_step=3, cf_condition_embed=cf, **kw), 2, 2,
                      {"step"}),
        "purity_with_final": (purity, lambda dm, kw: dm.sample(texts, None, cond, cf, filter_ratio=0, **kw), 2, 2, {"reveal"}),
        "resample_jumps": (None, lambda dm, kw: dm.sample(texts, None, cond, cf, content_token=content, filter_ratio=0, known_mask=mask,
                                                          resample_jump=10, resample_times=2, **kw), 2, 2, {"step", "jump"}),
        "known_hold": (None, lambda dm, kw: dm.sample(texts, None, cond, cf, content_token=content, filter_ratio=0, known_mask=mask,
                                                      known_mode="hold", **kw), 2, 2, {"step"}),
        "condition_lengths": (None, lambda dm, kw: dm.sample(texts, None, cond3, cf3, filter_ratio=0, condition_len=[3, 1, 2, 3, 2, 1, 3, 2],
                                                             cf_condition_len=[3] * SB, **kw), 2, 2, {"step"}),
    }


@pytest.mark.parametrize("case", ["plain_two_lanes", "guided", "skip_step", "purity_with_final", "resample_jumps", "known_hold",
                                  "condition_lengths"])
def test_sampler_graphs_replay_on_memory_they_own(G, golden, monkeypatch, case):
    from gsdd_amd.d3pm import _Lane
    sd, _, cfg = golden("d3pm_L64")
    setup, call, lanes, rep, kinds = sampler_cases(cfg)[case]
    dm = build_d3pm(G, sd, cfg)
    if setup is not None:
        setup(dm)
    la = LaneAudit(monkeypatch, _Lane)
    try:
        dm.set_noise(77, stream=3)
        got = call(dm, {})["content_token"]
        torch.cuda.synchronize()
        assert dm._last_lanes == lanes and {k for _, k in la.records} == kinds and len(la.records) == lanes * len(kinds)
        assert all(ln.rep == rep for ln in la.lanes)
        n_rec = {k: len(v) for k, v in la.records.items()}
        print(f"{case}: {la.replays} replays audited, recorded ranges per graph {sorted(n_rec.values())}, kept per graph "
              f"{sorted(len(g.kept) for ln in {id(ln): ln for ln in la.lanes}.values() for g in ln.graphs.values())}")
        assert not la.violations, "graphs not replayed -- " + show(la.violations)
        assert la.replays >= 20 * lanes
        got = got.cpu()
        dm.set_noise(77, stream=3)
        want = call(dm, {"use_graph": False})["content_token"].cpu()
        assert torch.equal(got, want), f"{int((got != want).sum())} tokens differ from the eager run"
    finally:
        la.reset()
        dm._last_graphs = None
        del dm
        release()
