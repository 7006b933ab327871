"""Host side of the condition lengths (caption padding masked in cross-attention): the three _len entry points are exported, declared
and bound with their argument types; argument errors come back as GSDD_E_ARG with a message before anything is launched (no GPU is
needed to see them) -- null pointers, Te outside [1, 77], a host length outside [1, Te] (the message names index and value), a
workspace one byte short; `check_condition_len` accepts and rejects what it should; and CLIPTextEmbedding.forward(return_lengths=True)
returns end-of-text + 1 from the ids it tokenized, on the PyTorch path of a CPU module, with the features of the call without the
flag."""
import ctypes
import os

import pytest
import torch

import gsdd_amd
from gsdd_amd import d3pm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
P = ctypes.c_void_p(0x7000000000)          # a non-null "device" address: an argument error returns before any pointer is used
_p, _i, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
ARGTYPES = {
    "gsdd_d3pm_cross_attention_len": [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p],
    "gsdd_d3pm_cross_attention_train_len": [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p, _p],
    "gsdd_d3pm_cross_attention_bwd_len": [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p, _p, _p, _i64, _p],
}
B, L, Te, H = 2, 64, 3, 16


def _last_error():
    return gsdd_amd.lib().gsdd_last_error().decode()


def host_lengths(*values):
    a = (ctypes.c_int32 * len(values))(*values)
    return a, ctypes.cast(a, ctypes.c_void_p)


def calls(lens=P, te=Te, need=None):
    """name -> argument list of a valid call with fake pointers (the host lengths `lens`, Te `te`)"""
    Lb = gsdd_amd.lib()
    need = Lb.gsdd_d3pm_cross_attention_bwd_workspace_bytes(B, L, Te, H) if need is None else need
    return {
        "gsdd_d3pm_cross_attention_len": [P, P, P, P, lens, B, L, te, H, P, None],
        "gsdd_d3pm_cross_attention_train_len": [P, P, P, P, lens, B, L, te, H, P, P, None],
        "gsdd_d3pm_cross_attention_bwd_len": [P, P, P, P, P, P, P, lens, B, L, te, H, P, P, P, P, need, None],
    }


# positions of the pointers that must not be null (cond_len_host, right behind cond_len, may be)
POINTERS = {"gsdd_d3pm_cross_attention_len": (0, 1, 2, 3, 9), "gsdd_d3pm_cross_attention_train_len": (0, 1, 2, 3, 9, 10),
            "gsdd_d3pm_cross_attention_bwd_len": (0, 1, 2, 3, 4, 5, 6, 12, 13, 14, 15)}


def test_symbols_are_exported_declared_and_bound():
    Lb = gsdd_amd.lib()
    header = open(os.path.join(REPO, "include", "gsdd.h")).read()
    for s, types in ARGTYPES.items():
        assert hasattr(Lb, s) and s in gsdd_amd.EXPORTS and header.count(s + "(") == 1, s
        assert list(getattr(Lb, s).argtypes) == types, s
    assert Lb.gsdd_version() >= 109
    import inspect
    from gsdd_amd import ops
    for f in ("d3pm_cross_attention", "d3pm_cross_attention_train", "d3pm_cross_attention_bwd"):
        prm = inspect.signature(getattr(ops, f)).parameters
        assert prm["cond_len"].default is None and prm["cond_len_host"].default is None, f


@pytest.mark.parametrize("name", list(ARGTYPES))
def test_argument_errors_come_back_before_any_launch(name):
    f = getattr(gsdd_amd.lib(), name)
    for i in POINTERS[name]:
        args = calls()[name]
        args[i] = None
        assert f(*args) == E_ARG and "null pointer" in _last_error(), i
    for te in (0, 78):
        assert f(*calls(te=te)[name]) == E_ARG
        assert name in _last_error() and "Te" in _last_error()
    for idx, bad in ((0, 0), (1, Te + 1)):
        values = [1, Te]
        values[idx] = bad
        keep, lens = host_lengths(*values)
        assert f(*calls(lens=lens)[name]) == E_ARG
        msg = _last_error()
        assert name in msg and f"cond_len[{idx}] = {bad}" in msg and f"[1, {Te}]" in msg, msg
        del keep


def test_a_workspace_one_byte_short_is_an_argument_error():
    Lb = gsdd_amd.lib()
    need = Lb.gsdd_d3pm_cross_attention_bwd_workspace_bytes(B, L, Te, H)
    keep, lens = host_lengths(1, Te)                                   # valid lengths: the workspace is what is wrong
    args = calls(lens=lens, need=need - 1)["gsdd_d3pm_cross_attention_bwd_len"]
    assert Lb.gsdd_d3pm_cross_attention_bwd_len(*args) == E_ARG and "workspace too small" in _last_error()
    del keep


def test_check_condition_len():
    ok = d3pm.check_condition_len([1, 22, 7], 3, 22)
    assert ok.dtype == torch.int32 and not ok.is_cuda and ok.is_contiguous() and ok.tolist() == [1, 22, 7]
    for given in (torch.tensor([1, 22, 7]), torch.tensor([1, 22, 7], dtype=torch.int32), torch.tensor([1, 22, 7], dtype=torch.uint8)):
        assert torch.equal(d3pm.check_condition_len(given, 3, 22), ok)
    assert d3pm.check_condition_len([1], 1, 1).tolist() == [1]
    for bad, what in (([0, 1, 1], r"condition_len\[0\] = 0"), ([1, 1, 23], r"condition_len\[2\] = 23"), ([1, -4, 2], r"\[1\] = -4"),
                      ([1, 2], "shape"), ([[1, 2, 3]], "shape"), (3, "shape"), ([1.0, 2.0, 3.0], "integers"),
                      ([True, True, True], "integers")):
        with pytest.raises(gsdd_amd.GsddError, match=what):
            d3pm.check_condition_len(bad, 3, 22)
    with pytest.raises(gsdd_amd.GsddError, match=r"cf_condition_len\[1\] = 2"):
        d3pm.check_condition_len([1, 2], 2, 1, "cf_condition_len")       # one condition token: all ones
    # the sampler's pair: no lengths -> None; the unconditional copy defaults to full length; one token -> nothing to mask
    assert d3pm._guidance_lens(None, None, 3, 22, True) is None
    c, u = d3pm._guidance_lens([1, 2, 3], None, 3, 22, True)
    assert c.tolist() == [1, 2, 3] and u.tolist() == [22, 22, 22]
    c, u = d3pm._guidance_lens(None, [4, 5, 6], 3, 22, True)
    assert c.tolist() == [22, 22, 22] and u.tolist() == [4, 5, 6]
    assert d3pm._guidance_lens([1, 2, 3], [4, 5, 6], 3, 22, False)[1] is None
    assert d3pm._guidance_lens([1, 1, 1], None, 3, 1, True) is None


def test_generator_switch_and_config_key(monkeypatch):
    from gsdd_amd.hydra_lite import compose
    monkeypatch.setenv("PROJECT_ROOT", REPO)
    gen = compose(os.path.join(REPO, "configs"), "eval.yaml", []).model.generator
    assert gen.mask_text_padding is False
    gen = compose(os.path.join(REPO, "configs"), "eval.yaml", ["model.generator.mask_text_padding=true"]).model.generator
    assert gen.mask_text_padding is True
    import inspect
    prm = list(inspect.signature(gsdd_amd.DiscreteDiffusion.__init__).parameters)
    assert prm[-2:] == ["mask_text_padding", "kwargs"]                 # the last named argument: the reference's prefix is kept
    assert "text_len" in inspect.signature(gsdd_amd.DiscreteDiffusion.sample_videos).parameters


def test_provider_returns_eot_plus_one(tmp_path):
    from tests.test_gpu_text_tokens import byte_level_provider
    texts = ["", "a", " ".join(["w"] * 25), "a dog runs"]              # (byte-level vocabulary, no merges: one token per character)
    p = byte_level_provider(tmp_path, 32, 2, per_token=True)          # a CPU module: the PyTorch path
    plain = p(texts)
    feats, lens = p(texts, return_lengths=True)
    assert lens.dtype == torch.int32 and not lens.is_cuda and lens.tolist() == [2, 3, 22, 10]
    assert tuple(feats.shape) == (4, 22, 32) and torch.equal(feats, plain)
    ids = p.tokenize(texts)
    assert lens.tolist() == [int(r.tolist().index(p.tokenizer.eos_token_id)) + 1 for r in ids]
    pooled = byte_level_provider(tmp_path, 32, 2)
    feats, lens = pooled(texts, return_lengths=True)
    assert tuple(feats.shape) == (4, 32) and lens.tolist() == [1, 1, 1, 1] and torch.equal(feats, pooled(texts))
