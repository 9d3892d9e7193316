"""yume_quant_rows_mx_e4m3, yume_attn_vt_mx_e4m3 and yume_attn_fwd_f8mx (ABI 9 + three exports): what can be said without a GPU. The exports
exist, are declared and bound, and every refusal of tests/attn_f8_cases.py REFUSALS is answered on the host, by name, before any launch."""
import os
import re

import pytest

import attn_f8_cases as fc
from conftest import ROOT

EXPORTS = ("yume_quant_rows_mx_e4m3", "yume_attn_vt_mx_e4m3", "yume_attn_fwd_f8mx")
NAMES = {"rows": b"quant_rows_mx_e4m3", "vt": b"attn_vt_mx_e4m3", "fwd": b"attn_fwd_f8mx"}


def _lib():
    import __graft_entry__ as g
    g.build()
    from yume_amd import _lib
    return _lib.load()


def test_exports_are_declared_bound_and_wrapped_and_the_abi_version_stays():
    lib = _lib()
    from yume_amd import _lib as binding, ops
    hdr = open(os.path.join(ROOT, "include", "yume_hip.h")).read()
    for name in EXPORTS:
        assert hasattr(lib, name) and name in binding.SIGNATURES and re.search(r"\bint %s\(" % name, hdr)
    assert binding.ABI_VERSION == 9 == int(re.search(r"#define YUME_ABI_VERSION (\d+)", hdr).group(1))      # functions added, no argument list changed
    assert callable(ops.quant_rows_mx_e4m3) and callable(ops.attn_vt_mx_e4m3) and callable(ops.attn_fwd_f8mx)


def test_the_valid_calls_of_the_refusal_table_pass_every_check():
    """with nothing changed a row's call passes the host checks: it would launch — so only its checks are asked for here, through a call
    that differs in ONE harmless way, R == 0, which returns YUME_OK in front of the launch"""
    lib = _lib()
    assert fc.refusal_call(lib, "rows", dict(R=0)) == 0


@pytest.mark.parametrize("name, entry, kw, word", fc.REFUSALS, ids=[r[0] for r in fc.REFUSALS])
def test_refusals_answer_by_name_before_any_launch(name, entry, kw, word):
    lib = _lib()
    assert fc.refusal_call(lib, entry, kw) == fc.EINVAL
    msg = lib.yume_last_error()
    assert NAMES[entry] in msg and word.encode() in msg, msg


def test_the_refusal_table_covers_what_the_header_promises():
    words = {(entry, tuple(sorted(kw))) for _, entry, kw, _ in fc.REFUSALS}
    for need in (("fwd", ("Q8",)), ("fwd", ("ldvt8",)), ("fwd", ("ldev",)), ("fwd", ("ldeq",)), ("rows", ("K", "ldq", "ldx")), ("fwd", ("Lq",)),
                 ("fwd", ("Lk",)), ("fwd", ("H",)), ("fwd", ("ldk",)), ("vt", ("ldvt8",)), ("vt", ("ldev",)), ("rows", ("lde",))):
        assert need in words, need
