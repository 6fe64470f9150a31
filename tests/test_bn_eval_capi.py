"""dro_batchnorm_eval_act without a GPU: every argument check returns its code
before any launch and leaves a message in dro_last_error(); the symbol is
declared in the header, listed in _lib.EXPORTED and typed; the ABI version did
not move (the entry point is additive)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dro-sfm_amd", "libdro_amd.so")
HEADER = os.path.join(ROOT, "include", "dro_amd.h")
NULL, SHAPE, MODE = -1, -2, -3
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("libdro_amd.so not built: run `make -C dro-sfm_amd/csrc`")
    import torch  # noqa: F401  (HIP runtime of torch first, as the product does)
    from dro_sfm_amd.hip import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def p():
    buf = (ctypes.c_float * 64)()
    yield ctypes.cast(buf, ctypes.c_void_p)


def call(lib, p, **kw):
    a = dict(x=p, gamma=p, beta=p, mean=p, var=p, skip=p, relu=1, N=1, C=2, HW=4, eps=1e-5, y=p)
    a.update(kw)
    return lib.dro_batchnorm_eval_act(a["x"], a["gamma"], a["beta"], a["mean"], a["var"], a["skip"], a["relu"],
                                      a["N"], a["C"], a["HW"], a["eps"], a["y"], None)


def test_export_declared(lib):
    from dro_sfm_amd.hip import _lib
    declared = set(re.findall(r"\b(dro_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    n = "dro_batchnorm_eval_act"
    assert n in declared and n in _lib.EXPORTED and hasattr(lib, n)
    assert lib.dro_batchnorm_eval_act.argtypes is not None and len(lib.dro_batchnorm_eval_act.argtypes) == 13
    assert lib.dro_abi_version() == 10


@pytest.mark.parametrize("which", ["x", "y", "mean", "var"])
def test_null_required_pointer(lib, p, which):
    assert call(lib, p, eps=-1.0) == MODE                    # another message first
    assert call(lib, p, **{which: None}) == NULL
    assert b"batchnorm_eval_act" in lib.dro_last_error() and b"NULL" in lib.dro_last_error()


@pytest.mark.parametrize("which", ["gamma", "beta"])
def test_exactly_one_of_gamma_beta_null(lib, p, which):
    assert call(lib, p, relu=2) == MODE
    assert call(lib, p, **{which: None}) == NULL
    assert b"batchnorm_eval_act" in lib.dro_last_error() and b"gamma and beta together" in lib.dro_last_error()


@pytest.mark.parametrize("sizes", [dict(N=0), dict(C=0), dict(HW=0), dict(N=-1), dict(C=-3), dict(HW=-2),
                                   dict(N=2, C=1024, HW=1 << 20), dict(N=1, C=1, HW=0x7FFFFFFF, x=None)])
def test_sizes_out_of_range(lib, p, sizes):
    """N * C * HW = 2^31 is refused, 2^31 - 1 is not (the NULL x is then what is reported)."""
    want = NULL if sizes.get("HW") == 0x7FFFFFFF else SHAPE
    assert call(lib, p, relu=2) == MODE
    assert call(lib, p, **sizes) == want
    if want == SHAPE:
        assert b"batchnorm_eval_act" in lib.dro_last_error() and b"sizes" in lib.dro_last_error()


@pytest.mark.parametrize("relu", [-1, 2, 7])
def test_relu_not_a_flag(lib, p, relu):
    assert call(lib, p, N=0) == SHAPE
    assert call(lib, p, relu=relu) == MODE
    assert b"batchnorm_eval_act" in lib.dro_last_error() and b"relu" in lib.dro_last_error()


@pytest.mark.parametrize("eps", [-1e-5, -INF, INF, NAN])
def test_eps_negative_or_not_finite(lib, p, eps):
    assert call(lib, p, N=0) == SHAPE
    assert call(lib, p, eps=eps) == MODE
    assert b"batchnorm_eval_act" in lib.dro_last_error() and b"eps" in lib.dro_last_error()
