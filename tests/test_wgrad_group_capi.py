"""Grouped weight gradient, C ABI checks that need no GPU: bad groups are
rejected with a status and a message before anything is launched, and the new
exports are declared in include/dro_amd.h and listed in _lib.EXPORTED."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dro_amd.h")
NEW = ("dro_conv2d_weight_grad_group", "dro_conv2d_weight_grad_group_workspace_bytes",
       "dro_conv2d_weight_grad_group_capacity")


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (HIP runtime of torch first, as the product does)
    from dro_sfm_amd.hip import _lib
    return _lib.load()


def test_exports_declared(lib):
    from dro_sfm_amd.hip import _lib
    declared = set(re.findall(r"\b(dro_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    for n in NEW:
        assert n in declared and n in _lib.EXPORTED and hasattr(lib, n), n


def test_capacity(lib):
    m, u = ctypes.c_int(0), ctypes.c_int(0)
    size = lib.dro_conv2d_weight_grad_group_capacity(ctypes.byref(m), ctypes.byref(u))
    print(f"grouped weight gradient: {m.value} members, {u.value} use slots, {size} bytes of kernel arguments")
    assert m.value >= 8 and u.value >= 16
    assert 0 < size <= 4096


def _members(n, nuse=1, Cin=8, Cout=4, B=1, H=8, W=8):
    """n members over fake (never dereferenced) device addresses."""
    from dro_sfm_amd.hip.conv import DroSlice, DroWgradMember, DroWgradUse
    fake = 0x1000
    sl = (DroSlice * 1)(DroSlice(fake, Cin, Cin, 0, 0))
    uses = (DroWgradUse * max(nuse, 1))()
    for u in uses:
        u.srcs, u.dout, u.y = ctypes.cast(sl, ctypes.c_void_p), fake, fake
    members = (DroWgradMember * n)()
    for m in members:
        m.uses, m.nuse, m.nsrc = ctypes.cast(uses, ctypes.c_void_p), nuse, 1
        m.B, m.H, m.W, m.Cout, m.alpha = B, H, W, Cout, 1.0
        m.grad_weight, m.grad_bias, m.accumulate = fake, None, 1
    return members, (sl, uses)


def test_bad_groups_rejected_before_launch(lib):
    group, ws_bytes = lib.dro_conv2d_weight_grad_group, lib.dro_conv2d_weight_grad_group_workspace_bytes
    cap = ctypes.c_int(0)
    lib.dro_conv2d_weight_grad_group_capacity(ctypes.byref(cap), None)
    ws = ctypes.c_void_p(0x2000)
    big = 1 << 30

    def err():
        return lib.dro_last_error()

    one, keep1 = _members(1)
    assert group(None, 1, 3, 3, 0, ws, big, None) == -1 and b"NULL members" in err()
    assert group(one, 0, 3, 3, 0, ws, big, None) == -2 and b"members" in err()
    many, keep2 = _members(cap.value + 1)
    assert group(many, cap.value + 1, 3, 3, 0, ws, big, None) == -2 and b"members" in err()
    for nuse in (0, 17):
        bad, keep3 = _members(1, nuse=nuse)
        assert group(bad, 1, 3, 3, 0, ws, big, None) == -2 and b"uses per member" in err(), nuse
    assert group(one, 1, 7, 7, 0, ws, big, None) == -2 and b"kernel shape" in err()
    assert group(one, 1, 3, 3, 4, ws, big, None) == -3 and b"activation" in err()
    need = ws_bytes(one, 1, 3, 3)
    assert need >= 4 * 8 * 9 * 4
    assert group(one, 1, 3, 3, 0, ws, need - 1, None) == -2 and b"workspace" in err()
    assert group(one, 1, 3, 3, 0, None, 0, None) == -2 and b"workspace" in err()
    # the size query rejects the same groups with 0
    assert ws_bytes(None, 1, 3, 3) == 0 and ws_bytes(one, 1, 7, 7) == 0 and ws_bytes(many, cap.value + 1, 3, 3) == 0
