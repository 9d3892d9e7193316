"""Every REFUSAL of tests/gemm_f6_cases.py returns its code through the raw C-ABI before any launch: the pointers handed over are never
dereferenced (no GPU is needed), and the message names the entry."""
import pytest

import gemm_f6_cases as f6
from yume_amd import _lib


@pytest.mark.parametrize("name,entry,kw,code", f6.REFUSALS, ids=[r[0] for r in f6.REFUSALS])
def test_refused_before_any_launch(name, entry, kw, code):
    lib = _lib.load()
    assert f6.refusal_call(lib, entry, kw) == code
    assert f"gemm_f6_{entry}".encode() in lib.yume_last_error()


def test_the_valid_call_of_the_refusal_table_would_pass_the_checks_with_a_null_operand_refused():
    """the base call differs from every refusal row in the named field only: with nothing changed the one thing wrong is checked here, a NULL
    scale pointer"""
    import ctypes
    lib = _lib.load()
    P = ctypes.c_void_p
    assert lib.yume_gemm_f6_mx(P(4096), 192, None, 16, P(4096), 192, P(4096), 16, None, 256, 256, 256, f6.EPI_F32, P(4096), 256, None, 0, None, None) == f6.EINVAL
    assert lib.yume_gemm_f6_mxout(P(4096), 192, P(4096), 16, P(4096), 192, P(4096), 16, None, 256, 256, 256, f6.EPI_MX6_GELU, P(4096), 192, None, 16,
                                  None) == f6.EINVAL
