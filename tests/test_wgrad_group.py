"""Grouped weight gradient (dro_conv2d_weight_grad_group): several weights of
one kernel shape and activation in one launch + one finish, against the fp64
sum of the per-use autograd gradients on the CPU.  Tolerance and error measure
are test_conv_engine.py's (TOL = 1e-4, max|a-b| / max|b|).  The shapes are the
smallest at which the per-member indexing can go wrong: ragged tiles, several
output / input channel tiles, multi-use beside single-use members, a member
with a single pixel tile, broadcast sources, sizes off the 4x16 / 8x8 tile."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
ACTS = {None: lambda x: x, "relu": torch.relu}
ACT_ID = {None: 0, "relu": 1}


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def make_src(kind, B, C, H, W, g):
    if kind == "bcast":
        return torch.randn(B, C, 1, 1, generator=g), lambda t: t.expand(B, C, H, W)
    if kind == "slice":
        return torch.randn(B, C + 5, H, W, generator=g), lambda t: t[:, 3:3 + C]
    return torch.randn(B, C, H, W, generator=g), lambda t: t


def M(srcs, Cout, B, H, W, uses=1, bias=True, alpha=1.0, acc=True):
    return dict(srcs=tuple(srcs), Cout=Cout, B=B, H=H, W=W, uses=uses, bias=bias, alpha=alpha, acc=acc)


GROUPS = {
    # three 3x3 members: ragged tiles and one (o, c) tile | 3 o-tiles | 2 c-tiles, 3 uses
    "mixed3x3": ((3, 3), None, [
        M([("dense", 37), ("slice", 11)], 45, 3, 7, 13, alpha=1.0),
        M([("dense", 64)], 130, 1, 16, 24, bias=False, alpha=0.25, acc=False),
        M([("dense", 70)], 64, 2, 9, 9, uses=3, alpha=0.5)]),
    # relu with saved outputs: a member of ONE pixel tile, and a broadcast source
    "relu3x3": ((3, 3), "relu", [
        M([("dense", 16)], 24, 1, 8, 8),
        M([("dense", 20), ("bcast", 6)], 32, 2, 10, 12, uses=2)]),
    "1x5": ((1, 5), None, [M([("dense", 33)], 70, 2, 5, 19), M([("slice", 66)], 20, 1, 10, 7, uses=2)]),
    "5x1": ((5, 1), None, [M([("dense", 33)], 70, 2, 5, 19), M([("slice", 66)], 20, 1, 10, 7, uses=2)]),
    "1x1": ((1, 1), None, [M([("dense", 130)], 9, 2, 5, 19, bias=False), M([("dense", 7)], 65, 1, 10, 7)]),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """CPU inputs and fp64 reference gradients of a group (computed once)."""
    (KH, KW), act, members = GROUPS[name]
    g = torch.Generator().manual_seed(sorted(GROUPS).index(name) + 7)
    out = []
    for m in members:
        Cin, Cout, B, H, W = sum(c for _, c in m["srcs"]), m["Cout"], m["B"], m["H"], m["W"]
        w = 0.1 * torch.randn(Cout, Cin, KH, KW, generator=g)
        b = 0.1 * torch.randn(Cout, generator=g)
        gw_ref = torch.zeros(Cout, Cin, KH, KW, dtype=torch.float64)
        gb_ref = torch.zeros(Cout, dtype=torch.float64)
        uses = []
        for _ in range(m["uses"]):
            bases, views = zip(*[make_src(k, B, c, H, W, g) for k, c in m["srcs"]])
            dout = torch.randn(B, Cout, H, W, generator=g)
            wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
            x = torch.cat([v(t.double()) for v, t in zip(views, bases)], 1)
            y = m["alpha"] * ACTS[act](F.conv2d(x, wd, bd, padding=(KH // 2, KW // 2)))
            (y * dout.double()).sum().backward()
            gw_ref += wd.grad
            gb_ref += bd.grad
            uses.append((bases, views, dout, y.detach().float() if act else None))
        init_w = torch.randn(Cout, Cin, KH, KW, generator=g)
        init_b = torch.randn(Cout, generator=g)
        out.append((m, uses, init_w, init_b, gw_ref, gb_ref))
    return out


def launch(name):
    """One grouped launch through the C ABI; returns [(gw, gb)] per member."""
    from dro_sfm_amd.hip import _lib
    from dro_sfm_amd.hip.conv import DroWgradMember, DroWgradUse, _slices
    lib = _lib.load()
    (KH, KW), act, _ = GROUPS[name]
    ref = reference(name)
    members = (DroWgradMember * len(ref))()
    keep, res = [], []
    for i, (m, uses, init_w, init_b, _, _) in enumerate(ref):
        arr = (DroWgradUse * len(uses))()
        for j, (bases, views, dout, y) in enumerate(uses):
            srcs = [v(t.to(DEV)) for v, t in zip(views, bases)]
            sl, d = _slices(srcs), dout.to(DEV)
            yy = y.to(DEV) if y is not None else None
            keep.append((srcs, sl, d, yy))
            arr[j].srcs = ctypes.cast(sl, ctypes.c_void_p)
            arr[j].dout = d.data_ptr()
            arr[j].y = yy.data_ptr() if yy is not None else None
        keep.append(arr)
        gw, gb = init_w.to(DEV), (init_b.to(DEV) if m["bias"] else None)
        res.append((gw, gb))
        mb = members[i]
        mb.uses, mb.nuse, mb.nsrc = ctypes.cast(arr, ctypes.c_void_p), len(uses), len(m["srcs"])
        mb.B, mb.H, mb.W, mb.Cout, mb.alpha = m["B"], m["H"], m["W"], m["Cout"], m["alpha"]
        mb.grad_weight, mb.grad_bias = gw.data_ptr(), gb.data_ptr() if gb is not None else None
        mb.accumulate = int(m["acc"])
    nb = lib.dro_conv2d_weight_grad_group_workspace_bytes(members, len(ref), KH, KW)
    assert nb > 0, lib.dro_last_error()
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    st = lib.dro_conv2d_weight_grad_group(members, len(ref), KH, KW, ACT_ID[act], ws.data_ptr(), nb, None)
    assert st == 0, lib.dro_last_error()
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_group_matches_autograd(name):
    got = launch(name)
    for i, ((m, _, init_w, init_b, gw_ref, gb_ref), (gw, gb)) in enumerate(zip(reference(name), got)):
        base_w = init_w.to(DEV) if m["acc"] else 0.0
        ew = rel(gw - base_w, gw_ref)
        print(f"{name} member {i}: weight {ew:.2e}")
        assert ew < TOL, (name, i)
        if m["bias"]:
            eb = rel(gb - (init_b.to(DEV) if m["acc"] else 0.0), gb_ref)
            print(f"{name} member {i}: bias {eb:.2e}")
            assert eb < TOL, (name, i)


def test_group_is_bitwise_repeatable():
    """Fixed reduction order: two identical launches give equal bits."""
    a, b = launch("mixed3x3"), launch("mixed3x3")
    for (gw0, gb0), (gw1, gb1) in zip(a, b):
        assert torch.equal(gw0, gw1)
        assert gb0 is None or torch.equal(gb0, gb1)


def test_capacity_plus_one_members_split_into_two_launches():
    """The Python grouping helper cuts capacity + 1 tiny members of one stream
    and shape into two launches; every member still gets its gradient."""
    from dro_sfm_amd.hip import conv as C
    cap = C._group_capacity()[0]
    assert cap >= 8 and C._group_capacity()[1] >= 16
    g = torch.Generator().manual_seed(5)
    B, H, W, Cin, Cout = 1, 5, 6, 3, 4
    stream = torch.cuda.current_stream()
    items, refs = [], []
    for _ in range(cap + 1):
        x, dout = torch.randn(B, Cin, H, W, generator=g), torch.randn(B, Cout, H, W, generator=g)
        wd = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
        (F.conv2d(x.double(), wd, padding=1) * dout.double()).sum().backward()
        gw, gb = torch.zeros(Cout, Cin, 3, 3, device=DEV), torch.zeros(Cout, device=DEV)
        refs.append((gw, gb, wd.grad, dout.double().sum((0, 2, 3))))
        meta = (B, H, W, Cin, Cout, 3, 3, 0, 1.0, gw, gb, 1, None)
        items.append((meta, [([x.to(DEV)], dout.to(DEV), None)], [stream]))
    assert not C._READY
    C.GROUP_LOG[0] = True
    del C.GROUP_LAUNCHES[:]
    try:
        for it in items:
            assert C._groupable(it)
            C._ready(it)
        C.flush_ready_groups()
        sizes = [len(members) for _, _, _, members in C.GROUP_LAUNCHES]
    finally:
        C.GROUP_LOG[0] = False
        del C.GROUP_LAUNCHES[:]
    torch.cuda.synchronize()
    assert sizes == [cap, 1]
    for gw, gb, rw, rb in refs:
        assert rel(gw, rw) < TOL and rel(gb, rb) < TOL
