"""CPU-only checks of the LDA entry points: the init product of one edge against glibc's rand_r (the restatement of
tests/test_gpu_lda.py), the error convention of all five entry points, and the layout of the binding's record."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_lda import init_product

GM_ERR_INVALID, GM_ERR_UNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def lib():
    from graphmat_amd import build
    build.build()
    from graphmat_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("e", [1, 2, 3, 5, 17, 1000003, 2 ** 31 - 1])
def test_edge_init_matches_the_restatement(lib, e):
    out = np.zeros(20, np.float64)
    assert lib.gm_lda_edge_init(e, 20, out.ctypes.data) == 0
    ref = init_product(e)
    assert (out.view(np.uint64) == ref.view(np.uint64)).all(), (out, ref)
    assert (out > 0).all() and abs(out.sum() - e) <= 1e-9 * e


def test_error_convention(lib):
    out = (C.c_double * 20)()
    it = C.c_int(0)
    total = C.c_double(0)
    fake = C.c_void_p(16)  # never dereferenced: the graph is null
    assert lib.gm_run_lda_init(None, fake, 20, None) == GM_ERR_INVALID
    assert lib.gm_lda_global_n(None, fake, 20, out, None) == GM_ERR_INVALID
    assert lib.gm_run_lda(None, fake, 20, 1.0, 5.0, 60.0, 1, C.byref(it), None, None) == GM_ERR_INVALID
    assert lib.gm_run_lda(None, None, 20, 1.0, 5.0, 60.0, 0, C.byref(it), None, None) == GM_ERR_INVALID
    assert lib.gm_run_lda_loglik(None, fake, 20, 5.0, 60, C.byref(total), None) == GM_ERR_INVALID
    assert b"null" in lib.gm_last_error()
    assert lib.gm_lda_edge_init(3, 7, out) == GM_ERR_UNSUPPORTED
    assert b"fixed menu" in lib.gm_last_error()
    assert lib.gm_lda_edge_init(3, 20, None) == GM_ERR_INVALID
    assert it.value == 0 and total.value == 0.0


def test_record_layout():
    from graphmat_amd import _lib
    assert C.sizeof(_lib.Lda20) == 176
    assert _lib.Lda20.type.offset == 160 and _lib.Lda20.token_loglik.offset == 168
