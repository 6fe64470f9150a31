"""Context hoist of the SepConvGRU backward (hip.conv.CtxHoist): the context
source of an update block is the same tensor in every GRU application, so its
share of the backward is taken once per (block, half) from the summed
pre-activation gradients.  Pieces: the fixed-order n-way sum (dro_sum_n), the
data-gradient kernels dropping the row tiles of a source without a target, the
data gradient through a column range of a wider weight
(dro_conv2d_backward_gapped), weight gradients written into a column range of a
wider weight (the _ex calls, dro_wgrad_gap), a depth-block-shaped recurrence on
the trainer's direct path with the hoist on and off, and a trainer step under a
captured gradient exchange in which no bucket completes before the context
columns of its weights are queued.  Error measure and bound are tests/conv_variants.py's
(max|a-b| / max|b| < 1e-4 against fp64 on the CPU); shapes are ragged against
the 4x16 / 8x8 pixel tiles, context ranges are multiples of the 32-row tile."""
import copy
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
SHAPES = {"1x5": ((1, 5), 2, 13, 37), "5x1": ((5, 1), 2, 19, 45)}


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


# ------------------------------------------------------------------ n-way sum
@pytest.mark.parametrize("n", [1, 2, 8])
@pytest.mark.parametrize("numel", [1, 255, 4 * 1000 + 3])
def test_sum_n_is_the_left_to_right_sum(n, numel):
    from dro_sfm_amd.hip import conv as C
    g = torch.Generator().manual_seed(100 * n + numel % 97)
    # set a at 16-byte aligned pointers (float4 items + scalar tail), set b at
    # pointers one float off (scalar items only), twice the size
    a = [torch.randn(numel, generator=g).to(DEV) for _ in range(n)]
    b = [torch.randn(2 * numel + 1, generator=g).to(DEV)[1:] for _ in range(n)]
    guard = torch.full((2 * numel + 8,), 7.5, device=DEV)
    out_b = guard[1:1 + 2 * numel]
    out_a, _ = C.sum_n(a, None, b, out_b)
    one = C.sum_n(a)
    torch.cuda.synchronize()
    ra, rb = a[0].clone(), b[0].clone()
    for k in range(1, n):
        ra, rb = ra + a[k], rb + b[k]
    assert torch.equal(out_a, ra) and torch.equal(one, ra)
    assert torch.equal(out_b, rb)
    assert guard[0] == 7.5 and bool((guard[1 + 2 * numel:] == 7.5).all())     # nothing past the ends


def test_sum_n_in_place_chain():
    """More than 8 tensors: later launches continue from the running sum, in place."""
    from dro_sfm_amd.hip import conv as C
    g = torch.Generator().manual_seed(4)
    ts = [torch.randn(3, 5, 7, generator=g).to(DEV) for _ in range(11)]
    qs = [torch.randn(2, 9, generator=g).to(DEV) for _ in range(11)]
    sz, sq = C.CtxHoist._sums(list(ts), list(qs))
    torch.cuda.synchronize()
    rz, rq = ts[0].clone(), qs[0].clone()
    for k in range(1, 11):
        rz, rq = rz + ts[k], rq + qs[k]
    assert torch.equal(sz, rz) and torch.equal(sq, rq)


# ------------------------------------------------------------------ data gradients
@functools.lru_cache(maxsize=None)
def conv_case(name, mid):
    """Inputs of one conv over [dense 32, dense `mid`, dense 14, bcast 6]
    (Cout 40) and the fp64 data gradients, computed once on the CPU."""
    (KH, KW), B, H, W = SHAPES[name]
    g = torch.Generator().manual_seed(11 + mid + KH)
    chans = (32, mid, 14, 6)
    w = 0.1 * torch.randn(40, sum(chans), KH, KW, generator=g)
    gout = torch.randn(B, 40, H, W, generator=g)
    xs = [torch.zeros(B, c, H, W, dtype=torch.float64, requires_grad=True) for c in chans]
    y = F.conv2d(torch.cat(xs, 1), w.double(), padding=(KH // 2, KW // 2))
    (y * gout.double()).sum().backward()
    return w, gout, chans, [x.grad for x in xs]


def run_dgrad(name, mid, skip):
    """conv2d_backward's data gradients with every target, or without source 1's."""
    from dro_sfm_amd.hip import conv as C
    (KH, KW), B, H, W = SHAPES[name]
    w, gout, chans, _ = conv_case(name, mid)
    srcs = [torch.zeros(B, c, H, W, device=DEV) for c in chans[:3]]
    srcs.append(torch.zeros(B, chans[3], 1, 1, device=DEV).expand(B, chans[3], H, W))
    tg = [torch.full((B, c, H, W), 3.25, device=DEV) for c in chans]
    offered = [t if not (skip and i == 1) else None for i, t in enumerate(tg)]
    C._conv_bwd(srcs, w.to(DEV), None, gout.to(DEV), 0, 1.0, offered, [0, 0, 1, 0])
    torch.cuda.synchronize()
    return tg


@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("mid", [32, 16])
def test_data_gradient_without_a_target(name, mid):
    """Source 1 without a target: its buffer stays untouched and the other
    sources' gradients keep their bits -- with 32 channels (its row tile is
    dropped by the kernel) and with 16 (not tile aligned: computed, discarded)."""
    _, _, _, ref = conv_case(name, mid)
    full, part = run_dgrad(name, mid, False), run_dgrad(name, mid, True)
    assert bool((part[1] == 3.25).all())
    for i in (0, 2, 3):
        assert torch.equal(full[i], part[i]), i
    for i in (0, 1, 3):
        assert rel(full[i], ref[i]) < TOL, i
    assert rel(full[2] - 3.25, ref[2]) < TOL      # the accumulated target


@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("acc", [0, 1])
def test_gapped_data_gradient(name, acc):
    """conv^T(G, W[:, 32:64]) read from the [40, 84, .] weight in place."""
    from dro_sfm_amd.hip import conv as C
    (KH, KW), B, H, W = SHAPES[name]
    w, gout, _, ref = conv_case(name, 32)
    buf = torch.full((B, 32, H, W), 0.5, device=DEV)
    C.conv2d_backward_gapped(gout.to(DEV), w.to(DEV), 0, 32, [buf], [acc])
    torch.cuda.synchronize()
    err = rel(buf - (0.5 if acc else 0.0), ref[1])
    print(f"gapped data gradient {name} acc {acc}: {err:.2e}")
    assert err < TOL


def test_gapped_data_gradient_rejects_what_the_halo_kernel_cannot_run():
    from dro_sfm_amd.hip import conv as C
    gout = torch.zeros(1, 8, 6, 6, device=DEV)
    buf = torch.zeros(1, 4, 6, 6, device=DEV)
    with pytest.raises(RuntimeError, match="gapped"):       # 7x7: not a halo shape
        C.conv2d_backward_gapped(gout, torch.zeros(8, 12, 7, 7, device=DEV), 0, 8, [buf], [0])
    with pytest.raises(RuntimeError, match="gapped"):       # the gap past the weight row
        C.conv2d_backward_gapped(gout, torch.zeros(8, 12, 1, 5, device=DEV), 0, 12, [buf], [0])
    with pytest.raises(RuntimeError, match="gapped"):       # rows of 11 x 5 floats: not float4 runs
        C.conv2d_backward_gapped(gout, torch.zeros(8, 11, 1, 5, device=DEV), 0, 4, [buf], [0])


# ------------------------------------------------------------------ gapped weight gradients
# weight columns: [dense 32 | context 32 | dense 14 | broadcast 6] = 84
CALIB = 2.5e-5                  # tests/conv_variants.py: a plain fp32 F.conv2d against fp64


def row_rel(a, b):
    """max over output channels of max|a[o]-b[o]| / max|b[o]|."""
    a, b = a.detach().double().cpu().flatten(1), b.detach().double().cpu().flatten(1)
    return ((a - b).abs().amax(1) / b.abs().amax(1).clamp_min(1e-30)).max().item()


@functools.lru_cache(maxsize=None)
def wgrad_case(name, Cout, nuse):
    """nuse uses of one [Cout, 84, .] weight that share the context source; the
    fp64 weight / bias gradients summed over the uses.  The inputs are such
    that plain fp32 F.conv2d gradients stay under the calibration bound."""
    (KH, KW), B, H, W = SHAPES[name]
    g = torch.Generator().manual_seed(5 + Cout + nuse + KH)
    pad = (KH // 2, KW // 2)
    ctx = torch.randn(B, 32, H, W, generator=g)
    uses, gw64, gb64 = [], 0.0, 0.0
    gw32 = 0.0
    for _ in range(nuse):
        a, c = torch.randn(B, 32, H, W, generator=g), torch.randn(B, 14, H, W, generator=g)
        bc = torch.randn(B, 6, 1, 1, generator=g)
        dout = torch.randn(B, Cout, H, W, generator=g)
        x = torch.cat([a, ctx, c, bc.expand(B, 6, H, W)], 1)
        for dt in (torch.float64, torch.float32):
            w = torch.zeros(Cout, 84, KH, KW, dtype=dt, requires_grad=True)
            b = torch.zeros(Cout, dtype=dt, requires_grad=True)
            (F.conv2d(x.to(dt), w, b, padding=pad) * dout.to(dt)).sum().backward()
            if dt == torch.float64:
                gw64, gb64 = gw64 + w.grad, gb64 + b.grad
            else:
                gw32 = gw32 + w.grad
        uses.append((a, c, bc, dout))
    assert rel(gw32, gw64) < CALIB and row_rel(gw32, gw64) < CALIB      # the inputs are well conditioned
    return ctx, uses, gw64, gb64


def _member(use_srcs, douts, Cout, B, H, W, gw, gb, acc, keep):
    from dro_sfm_amd.hip.conv import DroWgradMember, DroWgradUse, _slices
    arr = (DroWgradUse * len(douts))()
    for j, (srcs, d) in enumerate(zip(use_srcs, douts)):
        sl = _slices(srcs)
        keep.append((srcs, sl, d))
        arr[j].srcs, arr[j].dout, arr[j].y = ctypes.cast(sl, ctypes.c_void_p), d.data_ptr(), None
    keep.append(arr)
    m = DroWgradMember()
    m.uses, m.nuse, m.nsrc = ctypes.cast(arr, ctypes.c_void_p), len(douts), len(use_srcs[0])
    m.B, m.H, m.W, m.Cout, m.alpha = B, H, W, Cout, 1.0
    m.grad_weight, m.grad_bias, m.accumulate = gw.data_ptr(), gb.data_ptr() if gb is not None else None, int(acc)
    return m


def _run_members(form, KH, KW, members, gaps, cins):
    """The members through dro_conv2d_weight_grad_multi_ex (one call each) or
    one dro_conv2d_weight_grad_group_ex launch."""
    from dro_sfm_amd.hip import _lib
    from dro_sfm_amd.hip.conv import DroWgradGap, DroWgradMember
    lib = _lib.load()
    if form == "group":
        n = len(members)
        ms, gs = (DroWgradMember * n)(*members), (DroWgradGap * n)(*[DroWgradGap(*g) for g in gaps])
        nb = lib.dro_conv2d_weight_grad_group_workspace_bytes(ms, n, KH, KW)
        assert nb > 0, lib.dro_last_error()
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        st = lib.dro_conv2d_weight_grad_group_ex(ms, gs, n, KH, KW, 0, ws.data_ptr(), nb, None)
        assert st == 0, lib.dro_last_error()
    else:
        for m, g, cin in zip(members, gaps, cins):
            nb = lib.dro_conv2d_weight_grad_multi_workspace_bytes(m.nuse, m.B, m.H, m.W, cin, m.Cout, KH, KW)
            ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=DEV)
            gap = DroWgradGap(*g)
            st = lib.dro_conv2d_weight_grad_multi_ex(m.uses, m.nuse, m.nsrc, m.B, m.H, m.W, m.Cout, KH, KW, 0,
                                                     ctypes.c_float(1.0), m.grad_weight, m.grad_bias, m.accumulate,
                                                     ctypes.byref(gap), ws.data_ptr(), nb, None)
            assert st == 0, lib.dro_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("form,nuse", [("per-weight", 1), ("multi", 3), ("group", 8)])
@pytest.mark.parametrize("Cout", [40, 72])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_gapped_weight_gradient(name, Cout, form, nuse, acc):
    """A weight over [a | context | c | broadcast] takes its gradient from two
    members: the uses without the context (gap at 32, 32 long) and one use of
    the context with the summed output gradients (gap at 0, 32 long)."""
    from dro_sfm_amd.hip import conv as C
    (KH, KW), B, H, W = SHAPES[name]
    ctx, uses, gw64, gb64 = wgrad_case(name, Cout, nuse)
    g = torch.Generator().manual_seed(77)
    sent_w, sent_b = torch.randn(Cout, 84, KH, KW, generator=g).to(DEV), torch.randn(Cout, generator=g).to(DEV)
    gw, gb = sent_w.clone(), sent_b.clone()
    keep = []
    use_srcs = [[a.to(DEV), c.to(DEV), bc.to(DEV).expand(B, 6, H, W)] for a, c, bc, _ in uses]
    douts = [d.to(DEV) for _, _, _, d in uses]
    gsum = C.sum_n(douts)
    rest = _member(use_srcs, douts, Cout, B, H, W, gw, gb, acc, keep)
    cmem = _member([[ctx.to(DEV)]], [gsum], Cout, B, H, W, gw, None, acc, keep)
    gaps = [(84, 32, 32), (84, 0, 32)]
    cins = [52, 32]
    _run_members(form, KH, KW, [rest], gaps[:1], cins[:1])
    assert torch.equal(gw[:, 32:64], sent_w[:, 32:64])      # the context columns are not touched
    if form == "group":       # the context member beside its multi-use sibling, one launch
        gw.copy_(sent_w)
        gb.copy_(sent_b)
        _run_members(form, KH, KW, [rest, cmem], gaps, cins)
    else:
        _run_members(form, KH, KW, [cmem], gaps[1:], cins[1:])
    got_w = gw - sent_w if acc else gw
    got_b = gb - sent_b if acc else gb
    errs = (rel(got_w, gw64), row_rel(got_w, gw64), rel(got_b, gb64))
    print(f"{name} Cout {Cout} {form} acc {acc}: weight {errs[0]:.2e}, per row {errs[1]:.2e}, bias {errs[2]:.2e}")
    assert max(errs) < TOL


def test_gapless_ex_calls_are_the_plain_calls():
    """gap(s) = NULL and (wcin = Cin, gap_len = 0): the bits of the plain entry points."""
    from dro_sfm_amd.hip import _lib
    from dro_sfm_amd.hip.conv import DroWgradGap, DroWgradMember
    lib = _lib.load()
    (KH, KW), B, H, W = SHAPES["1x5"]
    g = torch.Generator().manual_seed(9)
    xs = [[torch.randn(B, 37, H, W, generator=g).to(DEV)] for _ in range(2)]
    ds = [torch.randn(B, 70, H, W, generator=g).to(DEV) for _ in range(2)]
    res = []
    for gaps in ("plain", None, [(37, 0, 0)], [(37, 37, 0)]):
        gw, gb, keep = torch.zeros(70, 37, KH, KW, device=DEV), torch.zeros(70, device=DEV), []
        m = (DroWgradMember * 1)(_member(xs, ds, 70, B, H, W, gw, gb, 0, keep))
        nb = lib.dro_conv2d_weight_grad_group_workspace_bytes(m, 1, KH, KW)
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        if gaps == "plain":
            st = lib.dro_conv2d_weight_grad_group(m, 1, KH, KW, 0, ws.data_ptr(), nb, None)
        else:
            ga = (DroWgradGap * 1)(DroWgradGap(*gaps[0])) if gaps else None
            st = lib.dro_conv2d_weight_grad_group_ex(m, ga, 1, KH, KW, 0, ws.data_ptr(), nb, None)
        assert st == 0, lib.dro_last_error()
        torch.cuda.synchronize()
        res.append((gw, gb))
    for gw, gb in res[1:]:
        assert torch.equal(gw, res[0][0]) and torch.equal(gb, res[0][1])
    # a gap that does not fit the weight row is refused
    bad = (DroWgradGap * 1)(DroWgradGap(40, 0, 8))
    assert lib.dro_conv2d_weight_grad_group_ex(m, bad, 1, KH, KW, 0, ws.data_ptr(), nb, None) != 0


# ------------------------------------------------------------------ module level
HD, CD, FD, ITERS, MB, MH, MW = 32, 32, 31, 4, 2, 13, 37


@functools.lru_cache(maxsize=None)
def recurrence_case():
    """Weights, inputs and fp64 CPU gradients of a depth-block-shaped recurrence:
    4 SepConvGRU applications over [h | context 32 | features 31 | state 1]."""
    from dro_sfm_amd.networks.optim import update as U
    torch.manual_seed(21)
    gru = U.SepConvGRU(hidden_dim=HD, input_dim=CD + FD + 1)
    with torch.no_grad():
        for p in gru.parameters():
            p.mul_(0.5)
    g = torch.Generator().manual_seed(22)
    inp = dict(h0=torch.randn(MB, HD, MH, MW, generator=g).tanh(), ctx=torch.randn(MB, CD, MH, MW, generator=g).relu(),
               feat=[torch.randn(MB, FD, MH, MW, generator=g) for _ in range(ITERS)],
               state=[torch.randn(MB, 1, MH, MW, generator=g) for _ in range(ITERS)],
               gout=[torch.randn(MB, HD, MH, MW, generator=g) for _ in range(ITERS)])
    ref = copy.deepcopy(gru).double()
    leaves = dict(h0=inp["h0"].double().requires_grad_(), ctx=inp["ctx"].double().requires_grad_(),
                  feat=[t.double().requires_grad_() for t in inp["feat"]])
    prev = U.conv_backend()
    U.set_conv_backend("miopen")       # F.conv2d: the fp64 CPU evaluation
    try:
        h, outs = leaves["h0"], []
        for t in range(ITERS):
            h = ref(h, [leaves["ctx"], leaves["feat"][t], inp["state"][t].double()])
            outs.append(h)
        sum((o * go.double()).sum() for o, go in zip(outs, inp["gout"])).backward()
    finally:
        U.set_conv_backend(prev)
    grads = dict(h0=leaves["h0"].grad, ctx=leaves["ctx"].grad, feat=[t.grad for t in leaves["feat"]],
                 params={k: p.grad for k, p in ref.named_parameters()}, outs=[o.detach() for o in outs])
    return gru.state_dict(), inp, grads


class Recurrence:
    """The recurrence on the trainer's direct path (flat parameter and gradient buffers)."""

    def __init__(self):
        from dro_sfm_amd.networks.optim.update import SepConvGRU
        from dro_sfm_amd.trainers.dp_trainer import GradBuckets, flatten_parameters
        sd, inp, _ = recurrence_case()
        self.gru = SepConvGRU(hidden_dim=HD, input_dim=CD + FD + 1)
        self.gru.load_state_dict(sd)
        self.gru.to(DEV)
        self.buckets = GradBuckets(list(self.gru.parameters()), groups=self.gru.dro_param_groups())
        flatten_parameters(self.buckets.params, self.buckets.offsets, self.buckets.flat.numel(),
                           self.buckets.flat.device)
        self.h0 = inp["h0"].to(DEV).requires_grad_()
        self.ctx = inp["ctx"].to(DEV).requires_grad_()
        self.feat = [t.to(DEV).requires_grad_() for t in inp["feat"]]
        self.state = [t.to(DEV) for t in inp["state"]]
        self.gout = [t.to(DEV) for t in inp["gout"]]

    def leaves(self):
        return [self.h0, self.ctx, *self.feat]

    def forward(self):
        import dro_sfm_amd.hip as H
        from dro_sfm_amd.hip import conv as C
        with C.weight_grad_scope():
            ctx, h, outs = H.grad_sink(self.ctx), self.h0, []
            for t in range(ITERS):
                h = H.grad_sink(self.gru(h, [ctx, H.grad_sink(self.feat[t]), self.state[t]], context=0))
                outs.append(h)
        return outs, sum((o * go).sum() for o, go in zip(outs, self.gout))

    def check(self, scale=1.0):
        _, _, ref = recurrence_case()
        errs = {"ctx": rel(self.ctx.grad, scale * ref["ctx"]), "h0": rel(self.h0.grad, scale * ref["h0"])}
        for t in range(ITERS):
            errs[f"feat{t}"] = rel(self.feat[t].grad, scale * ref["feat"][t])
        for k, p in self.gru.named_parameters():
            errs[k] = rel(p.grad, scale * ref["params"][k])
        print({k: f"{v:.1e}" for k, v in errs.items()})
        assert max(errs.values()) < TOL, errs


@pytest.fixture
def hoist_switch():
    from dro_sfm_amd.hip import conv as C
    prev = C._CTX_HOIST[0]
    yield C
    C.set_context_hoist(prev)


def test_recurrence_hoist_on_and_off(hoist_switch):
    C = hoist_switch
    if not C._GRU_CHAIN:
        pytest.skip("GRU chain disabled (DRO_GRU_CHAIN=0)")
    _, _, ref = recurrence_case()
    fwd = {}
    for on in (False, True):
        C.set_context_hoist(on)
        r = Recurrence()
        s0, c0, f0 = dict(C.CtxHoist.stats), dict(C.GruChain.stats), C.GruChain.folded
        outs, loss = r.forward()
        loss.backward(retain_graph=True)
        torch.cuda.synchronize()
        d = {k: C.CtxHoist.stats[k] - s0[k] for k in s0}
        assert d == ({"hoisted": 2 * ITERS, "flushes": 1, "sums": 2} if on else {"hoisted": 0, "flushes": 0, "sums": 0})
        # the halves stay linked either way
        assert C.GruChain.stats["bwd_linked"] - c0["bwd_linked"] == ITERS and C.GruChain.folded - f0 == ITERS
        assert not C._PENDING and not C._READY
        fwd[on] = [o.detach().clone() for o in outs]
        for o, o64 in zip(outs, ref["outs"]):
            assert rel(o, o64) < TOL
        r.check()
        # a second backward through the same graph runs unhoisted and unlinked
        # and adds the same gradients again
        loss.backward()
        torch.cuda.synchronize()
        assert C.CtxHoist.stats["hoisted"] - s0["hoisted"] == (2 * ITERS if on else 0)
        r.check(2.0)
    for a, b in zip(fwd[False], fwd[True]):
        assert torch.equal(a, b)            # the forward pass is untouched


def test_recurrence_hoist_graph_replay(hoist_switch):
    """Captured forward + backward with the hoist on: replays agree bit for bit
    and with the fp64 reference."""
    C = hoist_switch
    C.set_context_hoist(True)
    r = Recurrence()

    def step():
        r.buckets.flat.zero_()
        for t in r.leaves():
            t.grad = None
        r.forward()[1].backward()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s0 = C.CtxHoist.stats["flushes"]
    with torch.cuda.graph(graph):
        step()
    assert C.CtxHoist.stats["flushes"] == s0 + 1
    snaps = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        snaps.append([r.buckets.flat.clone(), *[t.grad.clone() for t in r.leaves()]])
    for a, b in zip(*snaps):
        assert torch.equal(a, b)
    r.check()


# ------------------------------------------------------------------ completeness under gradient exchange
def _exchange_worker(rank, port, out):
    """World-size-1 RCCL group, the bucketed exchange forced on.  Every bucket
    that completes is checked: no queued or waiting weight gradient, and no
    hoisted half that has not queued its context columns yet, still targets it."""
    import os
    import torch.distributed as dist
    from dro_sfm_amd.hip import conv as C
    from dro_sfm_amd.trainers.dp_trainer import DataParallelTrainer, GraphedTrainStep, graph_safe_nccl_env
    from test_dp_gpu import _batch, _model
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    graph_safe_nccl_env()
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    late = []

    def watch(tr):
        complete = tr.grads._complete

        def checked(b):
            sl = tr.grads._slice(tr.grads.buckets[b])
            lo, hi = sl.data_ptr(), sl.data_ptr() + sl.numel() * 4
            inside = lambda t: t is not None and lo <= t.data_ptr() < hi
            for items in (list(C._PENDING.values()), [it for grp in C._READY.values() for it in grp]):
                late.extend(("queued", b) for it in items if inside(it[0][9]) or inside(it[0][10]))
            late.extend(("hoist", b) for h in C._HOISTS for ent in h.halves.values()
                        if ent.sums is None and any(inside(t) for t in ent.gw))
            return complete(b)
        tr.grads._complete = checked

    with torch.backends.cudnn.flags(enabled=False):
        batch = _batch(0, 0)
        K0 = batch["intrinsics"].clone()
        flats, stats = {}, {}
        for on in (False, True):
            C.set_context_hoist(on)
            m = _model()
            tr = DataParallelTrainer(m, lr=0.0, capturable=True, bucket_mb=1.0, always_reduce=True)
            watch(tr)
            s0 = dict(C.CtxHoist.stats)
            gs = GraphedTrainStep(tr, batch, warmup=2, flips=(False,), reduce_in_graph=True)
            stats[on] = {k: C.CtxHoist.stats[k] - s0[k] for k in s0}
            batch["intrinsics"].copy_(K0)
            gs.step(batch, flip=False)
            torch.cuda.synchronize()
            flats[on] = tr.grads.flat.detach().cpu().clone()
            nb, in_bwd = len(tr.grads.buckets), tr.grads.issued_in_backward
            if on:
                zero_cols = []
                net = m.depth_net
                for blk, gru in ((net.update_block_depth, "depth_gru"), (net.update_block_pose, "pose_gru")):
                    hd = getattr(blk, gru).hidden_dim
                    for k, p in getattr(blk, gru).named_parameters():
                        if k.endswith("weight"):
                            cd = p.shape[1] - 2 * hd      # [h | context | features + state = hd]
                            cols = p.grad[:, hd:hd + cd].abs().amax((0, 2, 3))
                            zero_cols += [(gru, k, int(c)) for c in (cols == 0).nonzero().flatten()]
            del gs
        a, b = flats[True], flats[False]
        out["res"] = (late, stats, nb, in_bwd, float((a - b).abs().max() / b.abs().max()),
                      float((a - b).norm() / b.norm()), zero_cols)
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_context_columns_complete_before_their_bucket():
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    with mp.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_exchange_worker, args=(port, out), nprocs=1, join=True)
        late, stats, nb, in_bwd, mx, l2, zero_cols = out["res"]
    print(f"hoist on vs off: max {mx:.2e}, rel L2 {l2:.2e}; buckets {nb}, issued in backward {in_bwd}; {stats}")
    assert nb > 2 and in_bwd == nb
    assert stats[False]["hoisted"] == 0 and stats[True]["hoisted"] > 0 and stats[True]["flushes"] > 0
    assert not late, late
    assert not zero_cols, zero_cols
    assert mx < TOL
