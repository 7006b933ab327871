"""Host side of the training cross-attention (gsdd_d3pm_cross_attention_train / _bwd / _bwd_workspace_bytes): the library exports and
the binding declares the three entry points, the workspace query is positive and grows with L and Te, argument errors come back as
GSDD_E_ARG with a message before anything is launched (no GPU is needed to see them), and the descriptor codes of gsdd_abi_sizeof are
the ones they were."""
import ctypes
import os

import pytest

import gsdd_amd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gsdd_d3pm_cross_attention_train", "gsdd_d3pm_cross_attention_bwd", "gsdd_d3pm_cross_attention_bwd_workspace_bytes")
E_ARG = -1
P = ctypes.c_void_p(0x7000000000)          # a non-null "device" address: an argument error returns before any pointer is used


def test_symbols_are_exported_declared_and_bound():
    L = gsdd_amd.lib()
    header = open(os.path.join(REPO, "include", "gsdd.h")).read()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in gsdd_amd.EXPORTS and header.count(s + "(") == 1, s
    assert L.gsdd_version() >= 105
    assert L.gsdd_abi_sizeof(6) == -1 and all(L.gsdd_abi_sizeof(c) > 0 for c in (0, 1, 2, 3, 4, 5, 7))
    from gsdd_amd import ops
    for f in ("d3pm_cross_attention_train", "d3pm_cross_attention_bwd", "d3pm_cross_attention_bwd_workspace"):
        assert callable(getattr(ops, f))


def test_workspace_is_positive_and_monotone():
    ws = gsdd_amd.lib().gsdd_d3pm_cross_attention_bwd_workspace_bytes
    H = 16
    for B in (1, 3, 16):
        for Te in (1, 2, 22, 77):
            sizes = [ws(B, L, Te, H) for L in (1, 37, 64, 65, 257, 4096)]
            assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == len(sizes), (B, Te, sizes)
        for L in (1, 64, 4096):
            sizes = [ws(B, L, Te, H) for Te in (1, 2, 15, 16, 17, 22, 33, 77)]
            assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == len(sizes), (B, L, sizes)
    # delta f32 [H][M] (padded to 256 B) + one 8-float partial per (batch element, chunk of 64 rows, head, key)
    assert ws(16, 4096, 22, 16) == 16 * 4096 * 16 * 4 + 16 * 64 * 16 * 22 * 32
    assert ws(16, 4096, 22, 16) % 4 == 0 and ws(3, 37, 2, 2) % 4 == 0


def _last_error():
    return gsdd_amd.lib().gsdd_last_error().decode()


@pytest.mark.parametrize("Te", [0, 78, -1])
def test_te_out_of_range_is_an_argument_error(Te):
    L = gsdd_amd.lib()
    assert L.gsdd_d3pm_cross_attention_train(P, P, P, 2, 64, Te, 16, P, P, None) == E_ARG
    assert "gsdd_d3pm_cross_attention_train" in _last_error() and "Te" in _last_error()
    assert L.gsdd_d3pm_cross_attention_bwd(P, P, P, P, P, P, 2, 64, Te, 16, P, P, P, P, 1 << 30, None) == E_ARG
    assert "gsdd_d3pm_cross_attention_bwd" in _last_error() and "Te" in _last_error()


def test_null_pointers_sizes_and_a_short_workspace_are_argument_errors():
    L = gsdd_amd.lib()
    fwd, bwd = L.gsdd_d3pm_cross_attention_train, L.gsdd_d3pm_cross_attention_bwd
    for i in (0, 1, 2, 7, 8):                                          # q, kc, vc, out, lse
        args = [P, P, P, 2, 64, 3, 16, P, P, None]
        args[i] = None
        assert fwd(*args) == E_ARG and "null pointer" in _last_error(), i
    for i in (3, 4, 6):                                                # B, L, H
        args = [P, P, P, 2, 64, 3, 16, P, P, None]
        args[i] = 0
        assert fwd(*args) == E_ARG and "bad sizes" in _last_error(), i
    need = L.gsdd_d3pm_cross_attention_bwd_workspace_bytes(2, 64, 3, 16)
    ok = [P, P, P, P, P, P, 2, 64, 3, 16, P, P, P, P, need, None]
    for i in (0, 1, 2, 3, 4, 5, 10, 11, 12, 13):                       # q, kc, vc, o, dO, lse, dq, dkc, dvc, workspace
        args = list(ok)
        args[i] = None
        assert bwd(*args) == E_ARG and "null pointer" in _last_error(), i
    for i in (6, 7, 9):
        args = list(ok)
        args[i] = 0
        assert bwd(*args) == E_ARG and "bad sizes" in _last_error(), i
    args = list(ok)
    args[14] = need - 1
    assert bwd(*args) == E_ARG and "workspace too small" in _last_error()
