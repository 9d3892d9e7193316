"""yume_attn_fwd_band (sliding-window / causal attention, ABI 9 + one export): what can be said without a GPU. The export exists, is declared,
bound and wrapped, the ABI number did not move (no existing argument list changed), and the host-side validation answers by name before
any launch (NULL stream, pointers never dereferenced on the host)."""
import ctypes
import os
import re

import pytest
import torch

import attn_band_cases as bc
from conftest import ROOT

PTR = 4096            # any 16-byte aligned non-NULL value passes the common checks


def _lib():
    import __graft_entry__ as g
    g.build()
    from yume_amd import _lib
    return _lib


def _call(lib, Q=PTR, K=PTR, Vt=PTR, O=PTR, Lq=301, Lk=257, H=3, ldvt=264, variant=0, q_pos0=0, left=5, right=0):
    return lib.yume_attn_fwd_band(Q, H * 128, K, H * 128, Vt, ldvt, O, H * 128, Lq, Lk, H, 0.088, 0, variant, q_pos0, left, right, None, 0, None)


def test_export_header_binding_and_wrapper_agree():
    _l = _lib()
    hdr = open(os.path.join(ROOT, "include", "yume_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    syms = sorted(set(re.findall(r"\b(yume_[a-z0-9_]+)\s*\(", src)))
    assert "yume_attn_fwd_band" in syms
    assert "yume_attn_fwd_band" in _l.SIGNATURES and len(_l.SIGNATURES["yume_attn_fwd_band"]) == 20
    assert sorted(_l.SIGNATURES) == syms
    assert hasattr(ctypes.CDLL(_l.LIB_PATH), "yume_attn_fwd_band")
    lib = _l.load()
    # an added export changes no argument list: the ABI number stays
    assert lib.yume_abi_version() == _l.ABI_VERSION == 9 == int(re.search(r"#define YUME_ABI_VERSION (\d+)", hdr).group(1))
    doc = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int yume_attn_fwd_band\(", hdr, flags=re.S).group(1)
    assert "replaces:" in doc and "wan23/modules/attention.py" in doc and "wan23/modules/model.py:158-202" in doc
    import inspect
    from yume_amd import ops
    sig = inspect.signature(ops.attn_fwd).parameters
    assert sig["window"].default == (-1, -1) and sig["q_pos0"].default == 0


@pytest.mark.parametrize("name,kw,code,word", bc.REFUSALS, ids=[r[0] for r in bc.REFUSALS])
def test_refusals_answer_by_name_before_any_launch(name, kw, code, word):
    lib = _lib().load()
    assert _call(lib, **kw) == code
    msg = lib.yume_last_error().decode()
    assert "attn_fwd_band" in msg and word in msg, msg


def test_a_weighted_last_key_and_a_window_do_not_combine():
    _lib()
    from yume_amd import ops
    t = torch.zeros(8, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="last_key_weight"):
        ops.attn_fwd(t, t, t, t, 8, 8, 1, last_key_weight=3.0, window=(2, 0))


def test_the_seam_and_the_model_take_the_arguments():
    """without a GPU: the signatures, and the refusals that stay (dropout; the CLIP tower's causal)"""
    import inspect
    from yume_amd import attention
    for fn in (attention.flash_attention, attention.attention):
        p = inspect.signature(fn).parameters
        assert p["causal"].default is False and tuple(p["window_size"].default) == (-1, -1)
    src = open(os.path.join(ROOT, "yume_amd", "attention.py")).read()
    assert "no window" not in src
    from yume_amd.dit import DiTEngine

    class M:
        window_size = (7, 3)
    e = DiTEngine(M(), "wan23")
    assert e.window_size == (7, 3) and e._window_args(5) == {"window": (7, 3), "q_pos0": 5}
    e.window_size = (-1, -1)
    assert e._window_args(5) == {}
    e.window_size = (-2, 0)
    with pytest.raises(ValueError, match="window_size"):
        e._window_args(0)
    e.window_size = (4, 4)
    for who in ("forward_pair / forward_cfg", "forward_batch"):
        with pytest.raises(NotImplementedError, match="window_size"):
            e._refuse_window(who)
