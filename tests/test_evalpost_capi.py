"""dro_post_process_inv_depth and its Python wrappers without a GPU: bad
arguments are rejected before any launch, with a message."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dro-sfm_amd", "libdro_amd.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("libdro_amd.so not built: run `make -C dro-sfm_amd/csrc`")
    from dro_sfm_amd.hip import _lib
    return _lib.load()


def test_post_process_arguments_rejected(lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for args in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p), (p, p, p, None, p), (p, p, p, p, None)):
        inv, flipped, pp, depth, depth_pp = args
        assert lib.dro_post_process_inv_depth(inv, flipped, 1, 2, 2, 0, pp, depth, depth_pp, None) == -1
        assert b"NULL" in lib.dro_last_error()
    # W = 1: linspace(0, 1, 1) has no step; B = 0; B past the grid's y range
    for B, H, W in ((1, 2, 1), (0, 2, 2), (65536, 2, 2), (1, 0, 2)):
        assert lib.dro_post_process_inv_depth(p, p, B, H, W, 0, p, p, p, None) == -2, (B, H, W)
        assert b"sizes" in lib.dro_last_error()
    for method in (3, -1):
        assert lib.dro_post_process_inv_depth(p, p, 1, 2, 2, method, p, p, p, None) == -3
        assert b"method" in lib.dro_last_error()


def test_unknown_method_raises_value_error():
    from dro_sfm_amd.utils.depth import fuse_inv_depth, post_process_inv_depth
    x = torch.ones(1, 1, 2, 4)
    with pytest.raises(ValueError, match="Unknown post-process method"):
        post_process_inv_depth(x, x, method="median")
    with pytest.raises(ValueError, match="Unknown post-process method"):
        fuse_inv_depth(x, x, method="median")
    assert torch.equal(fuse_inv_depth(x, 3 * x), 2 * x)
    assert torch.equal(fuse_inv_depth(x, 3 * x, "max"), 3 * x) and torch.equal(fuse_inv_depth(x, 3 * x, "min"), x)


def test_post_process_rejects_cpu_tensors():
    import dro_sfm_amd.hip as hip
    from dro_sfm_amd.utils.depth import post_process_inv_depth
    x = torch.ones(1, 1, 2, 4)
    with pytest.raises(RuntimeError):
        hip.post_process_inv_depth(x, x)
    with pytest.raises(RuntimeError):
        post_process_inv_depth(x, x, method="max")
