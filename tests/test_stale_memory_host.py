"""tests/stale_memory.py checked without a GPU: what the four fill bytes decode to, that contiguous and strided results of all four
allocation functions are filled to the last byte of their storage, that the real functions come back (also after an exception) and that
nested use raises, the pass-through during a stream capture, the call-site record, the ledger against an `ast` scan of the package and
of src/, and -- on four CPU stand-in ops that misuse their scratch -- that the harness fails, with exactly the bytes it is built on."""
import functools
import math
import os

import pytest
import torch

from tests import stale_memory as sm
from tests.stale_memory import BYTES, EXEMPT, SITES, stale

HERE = "tests/test_stale_memory_host.py"
REAL = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)


def current():
    return (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)


def storage_bytes(t):
    return torch.empty(0, dtype=torch.uint8).set_(t.untyped_storage())


# ----------------------------------------------------------------------------- the helper
def test_bytes_decode_as_documented():
    assert BYTES == (0x00, 0xFF, 0x7F, 0xFE)
    got = {}
    for byte in BYTES:
        with stale(byte):
            got[byte] = {dt: torch.empty((3,), dtype=dt) for dt in (torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8)}
    for dt in got[0x00]:
        assert bool((got[0x00][dt] == 0).all())
    ff, p, m = got[0xFF], got[0x7F], got[0xFE]
    assert bool(torch.isnan(ff[torch.float32]).all()) and bool(torch.isnan(ff[torch.float64]).all())
    assert ff[torch.int32].tolist() == [-1] * 3 and ff[torch.int64].tolist() == [-1] * 3 and ff[torch.uint8].tolist() == [255] * 3
    assert 3.3e38 < float(p[torch.float32][0]) < 3.4028235e38 and 1.3e306 < float(p[torch.float64][0]) < 1.5e306     # finite, +huge
    assert p[torch.int32].tolist() == [2139062143] * 3 and int(p[torch.int64][0]) == 0x7F7F7F7F7F7F7F7F and p[torch.uint8].tolist() == [127] * 3
    assert -1.8e38 < float(m[torch.float32][0]) < -1.6e38 and math.isfinite(float(m[torch.float64][0])) and float(m[torch.float64][0]) < -1e300
    assert int(m[torch.int32][0]) == -16843010 and int(m[torch.int64][0]) < 0 and m[torch.uint8].tolist() == [254] * 3


@pytest.mark.parametrize("byte", BYTES[1:])
def test_every_function_fills_its_whole_storage(byte):
    base = torch.zeros((4, 6))
    with stale(byte) as st:
        made = {"empty": torch.empty((5, 7)), "empty_kw": torch.empty(size=(2, 3), dtype=torch.int64),
                "empty_like": torch.empty_like(base), "empty_like_strided": torch.empty_like(base.t()),
                "empty_strided": torch.empty_strided((3, 4), (1, 5)), "empty_strided_gaps": torch.empty_strided((2, 2), (7, 3)),
                "new_empty": base.new_empty((3, 3)), "new_empty_dtype": base.new_empty((2,), dtype=torch.int32)}
        assert torch.empty((0,)).numel() == 0                            # nothing to fill: passed through
    assert not made["empty_like_strided"].is_contiguous() and not made["empty_strided"].is_contiguous()
    for name, t in made.items():
        raw = storage_bytes(t)
        assert raw.numel() >= t.numel() * t.element_size() and bool((raw == byte).all()), name       # the gaps between strides too
    assert st.fills == len(made) and st.passed == 1 and st.byte == byte
    assert st.sites == {(HERE, "test_every_function_fills_its_whole_storage"): len(made)}


def test_functions_are_restored_also_after_an_exception_and_nesting_raises():
    assert current() == REAL
    with stale(0x7F):
        assert all(a is not b for a, b in zip(current(), REAL))
        with pytest.raises(RuntimeError, match="nested"):
            with stale(0x00):
                pass
        assert all(a is not b for a, b in zip(current(), REAL))           # the refused inner use did not restore the outer one's
    assert current() == REAL
    with pytest.raises(ValueError, match="inside"):
        with stale(0xFF):
            raise ValueError("inside")
    assert current() == REAL and float(torch.empty((1,)).new_empty((1,)).numel()) == 1
    with pytest.raises(ValueError):
        with stale(256):
            pass
    assert current() == REAL


def test_torch_modules_and_ops_still_work_inside():
    with stale(0xFF) as st:
        lin = torch.nn.Linear(5, 3)                                      # its parameters come from torch.empty, then its init writes them
        y = lin(torch.ones(2, 5))
        s = torch.stack([torch.ones(3), torch.zeros(3)])
        c = torch.cat([s, s])
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(lin.weight).all()) and s.tolist() == [[1.0] * 3, [0.0] * 3] and c.shape == (4, 3)
    assert st.fills >= 2 and all(not site[0].startswith("tests/") for site in st.sites)       # torch's own call sites, by absolute path


def allocate_in_a_comprehension():
    return [torch.empty((2,)) for _ in range(3)]


def test_call_sites_are_keyed_by_file_and_function():
    with stale(0x7F) as st:
        allocate_in_a_comprehension()
        (lambda: torch.empty((1,)))()
    assert st.sites == {(HERE, "allocate_in_a_comprehension"): 3, (HERE, "<lambda>"): 1} and st.fills == 4
    assert st.reached("tests/") == set(st.sites) and st.reached(sm.PACKAGE) == set()


def test_no_fill_during_a_stream_capture(monkeypatch):
    monkeypatch.setattr(sm, "_capturing", lambda t: True)                # what torch.cuda.is_current_stream_capturing() says in a capture
    with stale(0xFF) as st:
        t = torch.empty((4,), dtype=torch.int32)
        t.zero_()
    assert st.fills == 0 and st.passed == 1 and st.sites == {} and st.passed_sites == {(HERE, "test_no_fill_during_a_stream_capture"): 1}
    assert t.tolist() == [0] * 4
    assert sm._capturing is not None


def test_sweep_order_and_verdict():
    order = []

    def run():
        order.append(sm._active.byte)
        return {"t": torch.empty((2,), dtype=torch.uint8), "fixed": torch.ones(2), "bytes": b"abc", "number": 3}
    res = sm.sweep(run)
    assert order == [0x00, 0x00, 0xFF, 0x7F, 0xFE] and [r[0] for r in res] == order and sm._active is None
    unstable, by_byte, reached = sm.verdict(res)
    assert unstable == [] and by_byte == {0xFF: ["t"], 0x7F: ["t"], 0xFE: ["t"]} and reached == {(HERE, "run")}
    nan = torch.tensor([float("nan"), 1.0])
    assert sm.same_bits(nan, nan.clone()) and not sm.same_bits(nan, torch.tensor([float("nan"), 2.0]))
    assert sm.differing({"a": sm.bits(nan)}, {"a": sm.bits(nan.clone()), "b": sm.bits(nan)}) == ["b"]


# ----------------------------------------------------------------------------- the ledger
def test_ledger_equals_the_scan():
    found = sm.scan()
    assert len(found) >= 60 and sum(len(v) for v in found.values()) >= 127
    ledger = set(SITES) | set(EXEMPT)
    assert not set(SITES) & set(EXEMPT)
    missing, gone = set(found) - ledger, ledger - set(found)
    assert not missing, f"allocation sites no case of tests/test_gpu_stale_memory.py is named for (add them to SITES): {sorted(missing)}"
    assert not gone, f"ledger entries whose site allocates nothing any more: {sorted(gone)}"
    assert all(isinstance(v, tuple) and v and all(isinstance(i, str) for i in v) for v in SITES.values())
    assert all(isinstance(r, str) and len(r) > 20 and "\n" not in r for r in EXEMPT.values())
    assert len(EXEMPT) <= 0.05 * len(found), f"{len(EXEMPT)} of {len(found)} sites exempt: more than 5 %"


def test_ledger_names_cases_that_exist():
    from tests import test_gpu_stale_memory as gpu
    ids = {i for v in SITES.values() for i in v}
    assert ids <= set(gpu.CASES), sorted(ids - set(gpu.CASES))


def test_scan_finds_every_spelling(tmp_path):
    src = tmp_path / "m.py"
    src.write_text("import torch\nfrom torch import empty_like\n\n"
                   "class A:\n    def f(self, x):\n        return torch.empty((2,)), x.new_empty((3,)), [torch.empty_strided((1,), (1,)) for _ in x]\n\n"
                   "def g(x):\n    def inner():\n        return empty_like(x)\n    return inner, x.empty, torch.zeros(2)\n\n"
                   "buf = torch.empty((1,))\n")
    found = sm.scan([str(src)])
    rel = os.path.relpath(str(src), sm.REPO).replace(os.sep, "/")
    assert found == {(rel, "f"): [6, 6, 6], (rel, "inner"): [10], (rel, "<module>"): [13]}


# ----------------------------------------------------------------------------- the harness can fail
X = torch.tensor([0.5, 2.0, 1.25, 3.0, 0.75])


def op_sums_into_scratch():
    acc = torch.empty((1,))
    acc += X.sum()                                                       # (a) accumulates into what it never cleared
    return {"sum": acc}


def op_max_over_partly_written():
    buf = torch.empty((8,))
    buf[:5] = X
    return {"max": functools.reduce(torch.fmax, buf.unbind())}           # (b) fmaxf over 8 slots, 5 written (positive values)


def op_min_over_partly_written():
    buf = torch.empty((8,))
    buf[:5] = -X
    return {"min": functools.reduce(torch.fmin, buf.unbind())}           # (c) fminf likewise (negative values)


def op_counts_into_scratch():
    count = torch.empty((3,), dtype=torch.int32)
    count.index_add_(0, torch.tensor([0, 2, 2, 1, 2]), torch.ones(5, dtype=torch.int32))       # (d) increments what it never cleared
    return {"count": count}


def op_writes_before_it_reads():
    buf = torch.empty((8,))
    buf[:5] = X
    buf[5:] = 0
    count = torch.empty((3,), dtype=torch.int32).zero_()
    count.index_add_(0, torch.tensor([0, 2, 2, 1, 2]), torch.ones(5, dtype=torch.int32))
    return {"sum": buf.sum(), "max": functools.reduce(torch.fmax, buf.unbind()), "count": count, "strided": torch.empty_strided((2, 2), (1, 2)).copy_(X[:4].view(2, 2))}


@pytest.mark.parametrize("op,exposed_by", [(op_sums_into_scratch, {0xFF, 0x7F, 0xFE}), (op_max_over_partly_written, {0x7F}),
                                           (op_min_over_partly_written, {0xFE}), (op_counts_into_scratch, {0xFF, 0x7F, 0xFE}),
                                           (op_writes_before_it_reads, set())],
                         ids=["sum", "max", "min", "count", "correct"])
def test_each_fault_is_exposed_by_exactly_its_bytes(op, exposed_by):
    """A stale NaN is swallowed by fmaxf / fminf: only +huge betrays a max over unwritten slots, only -huge a min; NaN and both
    huge values betray a sum, -1 and the large integers a count.  Under 0x00 -- what fresh memory usually holds -- all five pass."""
    res = sm.sweep(op)
    unstable, by_byte, reached = sm.verdict(res)
    assert unstable == [] and set(by_byte) == exposed_by and reached == {(HERE, op.__name__)}
    assert all(st.fills >= 1 for _, _, st in res)
