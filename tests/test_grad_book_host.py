"""The trainer's gradient book (gsdd_amd._optim.GradBook) on CPU tensors with a stand-in reducer: which gradients leave in which
data-parallel bucket.  The rule it keeps: a range of the arena that has been issued is never issued (or written) again, and every
named gradient is all-reduced exactly once -- from the arena where it fits, in one concatenated bucket where it does not.  No GPU
and no library call."""
import torch

from gsdd_amd._optim import GradArena, GradBook
from gsdd_amd.parallel import GradReducer

SHAPES = {"head.w": (6, 5), "head.b": (5,), "b1.w": (8, 8), "b1.b": (7,), "b0.w": (3, 3), "b0.b": (2,), "emb": (4, 6), "late": (9,)}
NAMES = sorted(SHAPES)                  # (the caller's parameter order is not the request order)


class Recorder(GradReducer):
    """records each add as (data pointer, element count); `add` writes a marker into the tensor, as the all-reduce writes in place"""

    def __init__(self):
        super().__init__()
        self.adds, self.finished = [], 0

    def active(self):
        return True

    def add(self, t):
        assert t.dim() == 1 and t.is_contiguous() and t.dtype == torch.float32
        self.adds.append((t.data_ptr(), t.numel()))
        t += 1.0

    def finish(self):
        self.finished += 1


def run_step(arena, red, shapes=SHAPES, names=NAMES):
    """a step in the trainer's shape: head + bucket, two blocks (each with anonymous scratch) + bucket, embeddings with scratch, one
    gradient after the last explicit bucket -> (the book, the dict as returned, {name: value every entry was given before any add})"""
    book = GradBook(arena, red)
    vals, handed = {}, {}

    def fill(name, v):
        vals[name] = float(len(vals) + 2)
        v.fill_(vals[name])
        handed[name] = v

    for n in ("head.w", "head.b"):
        fill(n, book.zeros(n, torch.empty(shapes[n])))
    book.bucket()
    for blk in ("b1", "b0"):
        scratch = book.scratch((5,))
        assert not bool(scratch.any())
        for n in (blk + ".w", blk + ".b"):
            fill(n, book.zeros(n, torch.empty(shapes[n])))
    book.bucket()
    dpos = book.scratch((3, 4))
    fill("emb", book.zeros("emb", torch.empty(shapes["emb"])))
    assert not bool(dpos.any())
    fill("late", book.zeros("late", torch.empty(shapes["late"])))
    return book, book.finish(names), vals, handed


def check_reduced_once(g, vals, shapes=SHAPES):
    assert sorted(g) == sorted(shapes)                                      # no scratch in the dict
    for n, v in vals.items():
        assert tuple(g[n].shape) == tuple(shapes[n]), n
        assert torch.equal(g[n], torch.full(shapes[n], v + 1.0)), n       # the recorder's + 1 reached it exactly once


def inside(t, lo, n):
    return lo <= t.data_ptr() and t.data_ptr() + 4 * t.numel() <= lo + 4 * n


def test_first_step_spills_everything_into_one_concatenated_bucket():
    red = Recorder()
    book, g, vals, handed = run_step(GradArena("cpu"), red)
    assert book.arena.spilled and len(red.adds) == 1 and red.finished == 1
    ptr, n = red.adds[0]
    assert n == sum(torch.Size(s).numel() for s in SHAPES.values())
    assert all(inside(g[k], ptr, n) for k in NAMES)                          # re-bound to views of the one bucket ...
    assert g[NAMES[0]].data_ptr() == ptr                                     # ... laid out in the caller's order
    check_reduced_once(g, vals)                                              # ... with the values they had, reduced once
    assert all(g[k].data_ptr() != handed[k].data_ptr() for k in NAMES)


def test_second_step_issues_ascending_disjoint_slices_of_the_arena():
    arena, red = GradArena("cpu"), Recorder()
    run_step(arena, Recorder())
    book, g, vals, handed = run_step(arena, red)
    assert not arena.spilled and red.finished == 1
    base, end = arena.buf.data_ptr(), arena.buf.data_ptr()
    for ptr, n in red.adds:                                                  # ascending, disjoint, contiguous: each starts where the last ended
        assert ptr == end and n > 0
        end = ptr + 4 * n
    assert len(red.adds) == 3 and end == base + 4 * arena.off <= base + 4 * arena.buf.numel()
    for k in NAMES:
        assert g[k] is handed[k]                                             # nothing re-bound
        assert sum(inside(g[k], ptr, n) for ptr, n in red.adds) == 1, k
    assert inside(g["late"], *red.adds[2]) and inside(g["emb"], *red.adds[2])   # requested after the last explicit bucket: issued by finish
    check_reduced_once(g, vals)


def test_a_step_that_outgrows_the_arena_spills_into_one_extra_bucket():
    """what the first Te > 1 step does to a trainer that had seen one token: more is requested than the last step sized the arena for"""
    small = dict(SHAPES, **{"b1.w": (2, 2), "emb": (2,), "late": (1,)})     # 104 floats of arena; the full step asks for 192
    arena, red = GradArena("cpu"), Recorder()
    run_step(arena, Recorder(), small)
    run_step(arena, Recorder(), small)
    assert not arena.spilled
    book, g, vals, handed = run_step(arena, red)                            # the full shapes into the arena sized for `small`
    assert arena.spilled
    base, size = arena.buf.data_ptr(), arena.buf.numel()
    in_arena = [k for k in NAMES if inside(handed[k], base, size)]
    spilled = [k for k in NAMES if k not in in_arena]
    assert spilled == ["b1.w", "emb"]        # one in the middle of the step, one at its end; "late", after them, fits again
    arena_adds = [a for a in red.adds if base <= a[0] < base + 4 * size]
    extra = [a for a in red.adds if a not in arena_adds]
    assert len(extra) == 1 and extra[0][1] == sum(g[k].numel() for k in spilled)
    end = base
    for ptr, n in arena_adds:
        assert ptr == end
        end = ptr + 4 * n
    for k in in_arena:
        assert g[k] is handed[k] and sum(inside(g[k], ptr, n) for ptr, n in arena_adds) == 1, k
    for k in spilled:
        assert inside(g[k], *extra[0]), k
    check_reduced_once(g, vals)
    red2 = Recorder()
    book, g, vals, handed = run_step(arena, red2)                           # the step after: all in the arena again
    assert not arena.spilled and len(red2.adds) == 3 and all(g[k] is handed[k] for k in NAMES)
    check_reduced_once(g, vals)


def test_without_a_reducer_nothing_is_issued():
    arena = GradArena("cpu")
    for _ in range(2):
        book, g, vals, handed = run_step(arena, None)
        assert sorted(g) == sorted(SHAPES) and all(g[k] is handed[k] for k in NAMES)
        for k, v in vals.items():
            assert torch.equal(g[k], torch.full(SHAPES[k], v)), k


def test_scratch_rides_in_a_bucket_but_not_in_the_dict():
    arena, red = GradArena("cpu"), Recorder()
    run_step(arena, Recorder())
    book = GradBook(arena, red)
    a = book.zeros("a", torch.empty(4))
    s = book.scratch((2, 4))
    views = {"v0": s[0], "v1": s[1]}
    book.g.update(views)                                                    # row blocks of scratch bound by name, as attn1.query / key / value are
    book.bucket()
    assert len(red.adds) == 1 and inside(a, *red.adds[0]) and inside(s, *red.adds[0])
    g = book.finish(["a", "v0", "v1"])
    assert len(red.adds) == 1 and sorted(g) == ["a", "v0", "v1"] and g["v1"] is views["v1"]      # nothing issued twice
