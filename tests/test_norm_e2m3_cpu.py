"""tests/norm_e2m3_cases.py without a GPU: the table covers what it claims, and yume_adaln_modulate_mx_e2m3 refuses every bad shape or pitch
through the raw C-ABI before any launch (pointers never dereferenced)."""
import ctypes

import pytest

import norm_e2m3_cases as n6
from yume_amd import _lib


def test_table_covers_both_sides_of_the_two_row_threshold_and_every_form():
    assert len(n6.IDS) == len(set(n6.IDS)) == 30
    assert {c[1] for c in n6.CASES} == {1, 3, 1023, 1024, 1030} and {c[2] for c in n6.CASES} == {128, 384}
    assert {c[3] for c in n6.CASES} == {"noidx", "idx", "norm3"}
    assert {n6.instance(T, C) for _, T, C, _ in n6.CASES} == {"adaln_e2m3<3>", "adaln2_e2m3"}
    assert n6.instance(1023, 384) == "adaln_e2m3<3>" and n6.instance(1024, 384) == "adaln2_e2m3"
    for _, T, C, form in n6.CASES:
        x, mul, add, ts, idx, add_one = n6.make_case(T, C, form)
        ldq, lde = n6.pitches(C)
        assert x.shape == (T, C + 4) and ldq % 16 == 0 and lde % 16 == 0 and ldq > 3 * C // 4 and lde > C // 32
        assert (idx is not None) == (form == "idx") and add_one == (form != "norm3") and ts == (0 if form == "norm3" else 2 * C)


BAD = [("c_48", dict(C=48)), ("c_8224", dict(C=8224)), ("ldq_8", dict(ldq=96 + 8)), ("ldq_short", dict(ldq=80)), ("lde_8", dict(lde=8)),
       ("lde_20", dict(lde=20)), ("ldx_odd", dict(ldx=130)), ("tab_stride_odd", dict(ts=258)), ("q_misaligned", dict(q_off=8)), ("null_e", dict(e=None))]


@pytest.mark.parametrize("name,kw", BAD, ids=[b[0] for b in BAD])
def test_refused_before_any_launch(name, kw):
    lib = _lib.load()
    P = ctypes.c_void_p
    C = kw.get("C", 128)
    rc = lib.yume_adaln_modulate_mx_e2m3(P(4096), kw.get("ldx", C + 4), 5, C, 1e-6, P(4096), P(4096), kw.get("ts", 2 * C), None, 1,
                                         P(4096 + kw.get("q_off", 0)), kw.get("ldq", 3 * C // 4), kw.get("e", P(4096)) if "e" in kw else P(4096),
                                         kw.get("lde", 16), None)
    assert rc == -1
    assert b"adaln_modulate_mx_e2m3" in lib.yume_last_error()
