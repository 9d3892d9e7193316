"""yume_attn_fwd_seg (segmented cross-attention, ABI 9 + one export): what can be said without a GPU. The export exists, is declared and
bound, the ABI number did not move (no existing argument list changed), and the host-side validation answers by name before any launch."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

EINVAL, EUNSUP = -1, -3
PTR = 4096            # pointers are never dereferenced on the host: any 16-byte aligned non-NULL value passes the common checks


def _lib():
    import __graft_entry__ as g
    g.build()
    from yume_amd import _lib
    return _lib


def _call(lib, nseg=2, Lq_seg=64, seg_pitch=None, Lk=(78, 5), weights=(434.0, 507.0), variant=0, H=2, kptrs=None, vptrs=None, ldvt=None):
    n = len(Lk)
    seg_pitch = Lq_seg if seg_pitch is None else seg_pitch
    ldvt = ldvt if ldvt is not None else (max(max(Lk), 8) + 7) // 8 * 8
    karr = (ctypes.c_void_p * n)(*(kptrs if kptrs is not None else [PTR] * n))
    varr = (ctypes.c_void_p * n)(*(vptrs if vptrs is not None else [PTR] * n))
    larr = (ctypes.c_int64 * n)(*Lk)
    warr = None if weights is None else (ctypes.c_float * n)(*weights)
    return lib.yume_attn_fwd_seg(PTR, H * 128, karr, H * 128, varr, ldvt, PTR, H * 128, nseg, Lq_seg, seg_pitch, larr, H, 0.088, 0, variant,
                                 warr, None)


def test_export_header_and_binding_agree():
    _l = _lib()
    hdr = open(os.path.join(ROOT, "include", "yume_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    syms = sorted(set(re.findall(r"\b(yume_[a-z0-9_]+)\s*\(", src)))
    assert "yume_attn_fwd_seg" in syms
    assert "yume_attn_fwd_seg" in _l.SIGNATURES
    assert sorted(_l.SIGNATURES) == syms
    assert hasattr(ctypes.CDLL(_l.LIB_PATH), "yume_attn_fwd_seg")
    lib = _l.load()
    # an added export changes no argument list: the ABI number stays
    assert lib.yume_abi_version() == _l.ABI_VERSION == 9 == int(re.search(r"#define YUME_ABI_VERSION (\d+)", hdr).group(1))
    from yume_amd import ops
    assert callable(ops.attn_fwd_seg)


@pytest.mark.parametrize("nseg", [0, 9, -1])
def test_nseg_out_of_range_is_einval(nseg):
    lib = _lib().load()
    assert _call(lib, nseg=nseg) == EINVAL
    assert b"nseg" in lib.yume_last_error()


def test_pitch_below_the_segment_length_is_einval():
    lib = _lib().load()
    assert _call(lib, Lq_seg=64, seg_pitch=63) == EINVAL
    assert b"seg_pitch" in lib.yume_last_error()


@pytest.mark.parametrize("Lk", [(78, 0), (-3, 5), (0, 0)])
def test_empty_key_count_is_einval(Lk):
    lib = _lib().load()
    assert _call(lib, Lk=Lk, ldvt=80) == EINVAL
    assert b"Lk[" in lib.yume_last_error()


@pytest.mark.parametrize("w", [0.0, 0.5, -1.0, float("nan"), float("inf"), float(2 ** 21)])
@pytest.mark.parametrize("variant", [0, 2, 10])
def test_weight_out_of_range_is_einval_by_name(w, variant):
    lib = _lib().load()
    for weights in ((w, 2.0), (2.0, w)):
        assert _call(lib, weights=weights, variant=variant) == EINVAL
        assert b"last_key_weight" in lib.yume_last_error()
    assert _call(lib, nseg=1, Lk=(78,), weights=(w,), variant=variant) == EINVAL      # also where one segment delegates
    assert b"last_key_weight" in lib.yume_last_error()


def test_null_pointer_in_an_array_is_einval():
    lib = _lib().load()
    for kw in (dict(kptrs=[PTR, None]), dict(kptrs=[None, PTR]), dict(vptrs=[PTR, None]), dict(vptrs=[None, PTR])):
        assert _call(lib, **kw) == EINVAL
        assert b"NULL" in lib.yume_last_error()
    # the arrays themselves
    larr = (ctypes.c_int64 * 2)(78, 5)
    arr = (ctypes.c_void_p * 2)(PTR, PTR)
    assert lib.yume_attn_fwd_seg(PTR, 256, None, 256, arr, 80, PTR, 256, 2, 64, 64, larr, 2, 0.088, 0, 0, None, None) == EINVAL
    assert b"NULL" in lib.yume_last_error()
    assert lib.yume_attn_fwd_seg(PTR, 256, arr, 256, arr, 80, PTR, 256, 2, 64, 64, None, 2, 0.088, 0, 0, None, None) == EINVAL
    assert b"NULL" in lib.yume_last_error()


@pytest.mark.parametrize("Lk", [(78, 129), (129, 5), (512, 512)])
def test_short_key_kernel_refuses_more_than_128_keys(Lk):
    lib = _lib().load()
    for weights in (None, (2.0, 3.0)):
        assert _call(lib, Lk=Lk, weights=weights, variant=10) == EINVAL
        assert b"variant 10" in lib.yume_last_error() and b"128" in lib.yume_last_error()


@pytest.mark.parametrize("variant", [1, 4, 7, 8, 9])
@pytest.mark.parametrize("flags", [0, 0x100 | 0x200])
@pytest.mark.parametrize("nseg", [1, 2])
def test_variants_without_a_segmented_kernel_are_eunsup_and_named(variant, flags, nseg):
    lib = _lib().load()
    for Lk in ((78, 5), (512, 512)):
        assert _call(lib, nseg=nseg, Lk=Lk[:nseg], weights=None, variant=variant | flags, ldvt=512) == EUNSUP
        assert f"variant {variant}" in lib.yume_last_error().decode()
