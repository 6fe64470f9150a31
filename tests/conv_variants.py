"""The conv engine's variant table (csrc/conv.hip): one kernel-level fp64 case
per kernel instantiation the host plans can select.

The shape alone decides which instantiation a call gets (plan_igemm,
plan_igemm_flat, plan_class_dgrad, plan_wgrad2, k7_splits, launch_thin), so
every case DECLARES the plan class it is meant to reach -- halo or flat, BM,
the wave groups per tile (kin), split-K or not -- and `expect`, the launch-log
names (dro_conv_log_read) that follow from it.  tests/test_conv_variants.py
checks the declaration against dro_conv2d_plan_cin / dro_conv2d_strided_plan on
the CPU (a threshold retune fails there, naming the case) and, on the GPU,
that the names were launched and that every result matches fp64
torch.nn.functional.conv2d.

What the plan functions can reach (derived from them, csrc/conv.hip):

* halo kernels (1x1, 1x5, 5x1, 3x3; weight tensors of >= 4 weights whose rows
  [Cin][T] are a multiple of 4 long -- the others go flat), blocks = row tiles x
  pixel tiles:
  BM = 64 needs ceil(rows / 64) x pixel tiles >= 480, and then blocks >= 480,
  so kin is 2 (480..511 blocks) or 1 -- never 4, and never split-K (< 120).
  BM = 32: kin 4 below 256 blocks, 2 below 512, else 1, clamped to the chunk
  count.  Split-K needs blocks < 120 and ksplit <= chunks / kin; a kin clamped
  below 4 has chunks <= 3, hence chunks / kin = 1: split-K occurs with
  kin = 4 only (at least 8 chunks).
* flat kernel (everything else, and the strided convs): BM 64 from 448
  blocks, split-K below 960 blocks when ceil(480 / blocks) > 1.
* thin 7x7 path (one source of <= 8 channels): the data gradient takes 1, 2
  or 4 output-channel spans from the flat plan's split count.

wgrad2_group_kernel<KH, KW, act> is covered by tests/test_wgrad_group*.py
(GROUP_COVERED below), not here.

`python -m tests.conv_variants --subset NAME` runs the cases of one subset in
this process and exits non-zero on a mismatch: tests/test_conv_toggles.py
starts it with one of the library's process-wide switches set.
"""
import contextlib
import ctypes
import math
import os
import sys
from dataclasses import dataclass

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TOL = 1e-4          # the project's bound: global and per channel
CALIB = 2.5e-5      # a plain fp32 F.conv2d must stay below this against fp64 (4x margin)
DEV = "cuda"
ACT_ID = {None: 0, "relu": 1, "sigmoid": 2, "tanh": 3}
ACTS = {None: lambda x: x, "relu": torch.relu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}
HALO_SHAPES = {(1, 1), (1, 5), (5, 1), (3, 3)}

# covered by tests/test_wgrad_group.py / test_wgrad_group_capi.py / test_wgrad_group_trainer.py
GROUP_COVERED = frozenset(f"wgrad2_group_kernel<{kh}, {kw}, {a}>"
                          for kh, kw in HALO_SHAPES for a in range(4))


# ------------------------------------------------------------------ launch log
@contextlib.contextmanager
def conv_log():
    """The set of kernel names the conv engine launched inside the block
    (dro_conv_log / dro_conv_log_read); filled on exit."""
    from dro_sfm_amd.hip import _lib
    lib = _lib.load()
    names = set()
    lib.dro_conv_log(1)
    try:
        yield names
    finally:
        lib.dro_conv_log(0)
        n = lib.dro_conv_log_read(None, 0)
        buf = ctypes.create_string_buffer(int(n) + 1)
        lib.dro_conv_log_read(buf, n + 1)
        names.update(line.split("\t")[0] for line in buf.value.decode().splitlines() if line)


# ------------------------------------------------------------------ the table
@dataclass(frozen=True)
class Plan:
    """Plan class of one GEMM: halo kernel or flat, BM, wave groups per tile, split-K."""
    halo: bool
    bm: int
    kin: int = 1
    split: bool = False


def H(bm, kin, split=False):
    return Plan(True, bm, kin, split)


def Fl(bm, split=False):
    return Plan(False, bm, 1, split)


@dataclass(frozen=True)
class Case:
    name: str
    call: str                       # conv2d | strided | gru_half | gru_cand_bwd | gru_gates_bwd | bn_stage
    srcs: tuple                     # ((kind, channels), ...): dense | slice | bcast
    cout: int                       # output channels (gru_*: the hidden size)
    k: tuple
    act: object
    alpha: float
    B: int
    H: int
    W: int
    plans: dict                     # GEMM label -> Plan (the labels of gemms())
    stride: int = 1
    pad: int = 0
    bias: bool = True
    split_bwd: bool = False         # conv2d: data and weight gradient in separate calls (the trainer's path)
    spans: int = 0                  # thin data gradient: output-channel spans
    subsets: tuple = ()
    seed: int = 0
    extra: tuple = ()               # further expected names

    @property
    def cin(self):
        return sum(c for _, c in self.srcs)

    @property
    def wcin(self):
        """Input channels of the weight tensors (the GRU's: hidden + inputs)."""
        return self.cin + (self.cout if self.call.startswith("gru") else 0)

    @property
    def thin(self):
        return self.call == "conv2d" and self.k == (7, 7) and len(self.srcs) == 1 and self.cin <= 8

    def gemms(self):
        """label -> (rows, kch) of every GEMM the case launches on the planned kernels."""
        ci, co = self.cin, self.cout
        if self.call in ("conv2d", "bn_stage", "strided"):
            return {"fwd": (co, ci), "dgrad": (ci, co)}
        hd, cin = co, co + ci
        if self.call == "gru_half":
            return {"gates": (2 * hd, cin), "blend": (hd, cin), "dcand": (cin, hd), "dgates": (cin, 2 * hd)}
        if self.call == "gru_cand_bwd":
            return {"dcand": (cin, hd)}
        return {"dgates": (cin, 2 * hd)}

    @property
    def expect(self):
        return frozenset(_expect(self))


def _dconv(p, k, mode, act, epi):
    if p.halo:
        return f"dconv_kernel<{p.bm}, {k[0]}, {k[1]}, {mode}, {act}, {epi}, {p.kin}>"
    return f"igemm_kernel<{p.bm}, {mode}, {act}, {epi}>"


def _cinp(c):
    return 1 if c == 1 else 2 if c == 2 else 4 if c <= 4 else 8


def _k7_wgrad(case):
    dense = len(case.srcs) == 1 and case.srcs[0][0] == "dense"
    if case.call == "strided":
        return case.k == (7, 7) and case.pad == 3 and case.stride == 2 and case.cin in (3, 6)
    return case.k == (7, 7) and dense and case.cin in (1, 6)


def _expect(c):
    """The launch-log names that follow from the declared plan classes (the
    default build of the library: no process-wide switch set)."""
    a, k, P = ACT_ID[c.act], c.k, c.plans
    if c.call == "strided":
        names = [f"igemm_kernel<{P['fwd'].bm}, 0, {a}, 0>"]
        if c.act is None:
            names.append(f"igemm_kernel<{P['dgrad'].bm}, 1, 0, 0>" + (" parity classes" if c.stride == 2 else ""))
            names.append(f"wgrad_k7_kernel<{c.stride}, {c.cin}>" if _k7_wgrad(c) else "wgrad_kernel(")
        return names
    if c.call == "gru_half":
        return [_dconv(P["gates"], k, 0, 2, 2), _dconv(P["blend"], k, 0, 3, 1), _dconv(P["dcand"], k, 1, 0, 0),
                _dconv(P["dgates"], k, 1, 0, 0), f"wgrad2_kernel<{k[0]}, {k[1]}, 0, false, 1>"]
    if c.call == "gru_cand_bwd":
        return [_dconv(P["dcand"], k, 1, 0, 3)]
    if c.call == "gru_gates_bwd":
        return [_dconv(P["dgates"], k, 1, 0, 4)]
    if c.call == "bn_stage":
        return [_dconv(P["fwd"], k, 0, 0, 5), _dconv(P["dgrad"], k, 1, 0, 6), _dconv(P["dgrad"], k, 1, 0, 0),
                "wgrad2_kernel<3, 3, 0, false, 1>"]
    # conv2d
    halo_w = k in HALO_SHAPES
    pre = a != 0 or c.alpha != 1.0
    # the activation derivative is folded into the gradient kernels' staging
    # when both run on kernels that can (conv2d_backward_impl)
    fold_d = pre and (P["dgrad"].halo or c.thin) and (halo_w or c.split_bwd)
    fold_w = pre and (P["dgrad"].halo or c.thin) and halo_w
    names = [f"thin_fwd_kernel<{a}>" if c.thin else _dconv(P["fwd"], k, 0, a, 0)]
    ga = a if fold_d else 0
    names.append(f"thin_dgrad_kernel<{ga}, {_cinp(c.cin)}>" if c.thin else _dconv(P["dgrad"], k, 1, ga, 0))
    if halo_w:
        names.append(f"wgrad2_kernel<{k[0]}, {k[1]}, {a if fold_w else 0}, false, 1>")
        names.append(f"wgrad2_kernel<{k[0]}, {k[1]}, {a}, true, 1>")     # the deferred multi-use call
    else:
        names.append(f"wgrad_k7_kernel<1, {c.cin}>" if _k7_wgrad(c) else "wgrad_kernel(")
    return names + list(c.extra)


def _mk(name, call, srcs, cout, k, act, alpha, B, Hh, W, plans, **kw):
    srcs = tuple((s, c) for s, c in srcs)
    return Case(name, call, srcs, cout, k, act, alpha, B, Hh, W, plans, **kw)


def _conv(name, srcs, cout, k, act, B, Hh, W, fwd, dgrad, alpha=1.0, **kw):
    return _mk(name, "conv2d", srcs, cout, k, act, alpha, B, Hh, W, {"fwd": fwd, "dgrad": dgrad}, **kw)


D, S, BC = "dense", "slice", "bcast"

# Pixel-tile counts (B x ceil(H / TH) x ceil(W / TW), tiles 8 x 8 for 3x3, 5x1
# and 1x1, 4 x 16 for 1x5) used below; every H and W is ragged against its tile:
#   2 x 19 x 45 -> 36 (8x8)      2 x 13 x 37 -> 24 (4x16)
#   2 x 37 x 150 -> 190 (8x8)    2 x 37 x 150 -> 200 (4x16), 2 x 37 x 230 -> 300 (4x16)
#   3 x 37 x 150 -> 285 (8x8)
#   2 x 61 x 237 -> 480 (both)   2 x 61 x 250 -> 512 (both)
CASES = [
    # ---- 3x3 halo kernel: CK 8 (BM 32) / 4 (BM 64)
    _conv("c33_bm32_k4", [(D, 28)], 30, (3, 3), "relu", 2, 19, 45, H(32, 4), H(32, 4)),
    _conv("c33_bm32_k4_none", [(S, 28)], 30, (3, 3), None, 2, 19, 45, H(32, 4), H(32, 4)),
    _conv("c33_bm32_k2", [(D, 20), (S, 8)], 30, (3, 3), "relu", 3, 37, 150, H(32, 2), H(32, 2)),
    _conv("c33_bm32_k2_none", [(D, 28)], 30, (3, 3), None, 3, 37, 150, H(32, 2), H(32, 2)),
    _conv("c33_bm32_k1", [(D, 44)], 46, (3, 3), "relu", 3, 37, 150, H(32, 1), H(32, 1)),
    _conv("c33_bm32_k1_none", [(S, 44)], 46, (3, 3), None, 3, 37, 150, H(32, 1), H(32, 1)),
    _conv("c33_bm64_k2", [(D, 28)], 30, (3, 3), "relu", 2, 61, 237, H(64, 2), H(64, 2)),
    _conv("c33_bm64_k2_none", [(S, 28)], 30, (3, 3), None, 2, 61, 237, H(64, 2), H(64, 2)),
    _conv("c33_bm64_k1", [(D, 28)], 30, (3, 3), "relu", 2, 61, 250, H(64, 1), H(64, 1)),
    _conv("c33_bm64_k1_none", [(D, 20), (BC, 8)], 30, (3, 3), None, 2, 61, 250, H(64, 1), H(64, 1)),
    # 9 / 10 chunks over kin 4 x ksplit 2: splits of 5 + 4 chunks, the last wave group short
    _conv("c33_split", [(D, 68)], 74, (3, 3), None, 1, 13, 21, H(32, 4, True), H(32, 4, True)),
    # the heads: few output channels (forward kin 4), many input channels (data gradient kin 1)
    _conv("c33_head_sigmoid", [(D, 68)], 3, (3, 3), "sigmoid", 2, 37, 150, H(32, 4), H(32, 1)),
    _conv("c33_head_tanh", [(S, 68)], 1, (3, 3), "tanh", 2, 37, 150, H(32, 4), H(32, 1)),
    # weight rows [Cin][T] whose length is no multiple of 4 go to the flat kernel (the
    # halo kernel's 16-byte weight runs would straddle the end of the tensor), whether
    # or not the whole tensor's count is one
    _conv("c33_odd_rows", [(D, 26)], 30, (3, 3), None, 2, 19, 45, Fl(32, True), Fl(32, True)),
    _conv("c33_odd_weights", [(D, 27)], 30, (3, 3), "relu", 2, 19, 45, Fl(32, True), Fl(32, True)),
    _conv("c11_odd_weights", [(S, 27)], 29, (1, 1), None, 2, 19, 45, Fl(32), Fl(32)),
    _conv("c15_odd_weights", [(D, 21)], 23, (1, 5), "tanh", 2, 13, 37, Fl(32), Fl(32)),
    # ---- 1x5 halo kernel: CK 16 (BM 32) / 8 (BM 64), tiles 4 x 16
    # (every kin > 1 case has, in the forward or the data gradient, a chunk count
    # that puts the last, partial chunk into the last wave group)
    _conv("c15_bm32_k4", [(D, 30), (S, 22)], 56, (1, 5), None, 2, 13, 37, H(32, 4), H(32, 4)),
    _conv("c15_bm32_k2", [(D, 20)], 22, (1, 5), None, 2, 37, 230, H(32, 2), H(32, 2)),
    _conv("c15_bm32_k1", [(S, 40)], 45, (1, 5), None, 2, 37, 230, H(32, 1), H(32, 1)),
    _conv("c15_bm64_k2", [(D, 20)], 28, (1, 5), "sigmoid", 2, 61, 237, H(64, 2), H(64, 2)),
    _conv("c15_bm64_k1", [(D, 14), (BC, 6)], 22, (1, 5), None, 2, 61, 250, H(64, 1), H(64, 1)),
    _conv("c15_split", [(D, 132)], 136, (1, 5), None, 1, 13, 37, H(32, 4, True), H(32, 4, True)),
    # ---- 5x1 halo kernel: CK 16 / 8, tiles 8 x 8
    _conv("c51_bm32_k4", [(D, 30), (S, 22)], 56, (5, 1), None, 2, 19, 45, H(32, 4), H(32, 4)),
    _conv("c51_bm32_k2", [(D, 20)], 22, (5, 1), None, 3, 37, 150, H(32, 2), H(32, 2)),
    _conv("c51_bm32_k1", [(S, 40)], 45, (5, 1), None, 3, 37, 150, H(32, 1), H(32, 1)),
    _conv("c51_bm64_k2", [(D, 20)], 28, (5, 1), "tanh", 2, 61, 237, H(64, 2), H(64, 2)),
    _conv("c51_bm64_k1", [(D, 14), (BC, 6)], 22, (5, 1), None, 2, 61, 250, H(64, 1), H(64, 1)),
    _conv("c51_split", [(D, 132)], 136, (5, 1), None, 1, 13, 21, H(32, 4, True), H(32, 4, True)),
    # ---- 1x1 halo kernel: CK 32 / 16
    _conv("c11_bm32_k4", [(D, 100)], 104, (1, 1), "relu", 2, 19, 45, H(32, 4), H(32, 4)),
    _conv("c11_bm32_k4_mask", [(S, 100)], 104, (1, 1), None, 2, 19, 45, H(32, 4), H(32, 4), alpha=0.25),
    _conv("c11_bm32_k2", [(D, 40)], 45, (1, 1), "relu", 2, 37, 150, H(32, 2), H(32, 2)),
    _conv("c11_bm32_k2_none", [(S, 40)], 45, (1, 1), None, 2, 37, 150, H(32, 2), H(32, 2)),
    _conv("c11_bm32_k1", [(D, 40)], 45, (1, 1), None, 3, 37, 150, H(32, 1), H(32, 1)),
    _conv("c11_bm64_k2", [(D, 40)], 60, (1, 1), None, 2, 61, 237, H(64, 2), H(64, 2)),
    _conv("c11_bm64_k1", [(D, 40)], 45, (1, 1), None, 2, 61, 250, H(64, 1), H(64, 1)),
    _conv("c11_split", [(D, 260)], 270, (1, 1), None, 1, 13, 21, H(32, 4, True), H(32, 4, True)),
    # ---- flat kernel through conv2d (a 5x3 kernel has no halo variant): both modes
    _conv("flat_bm32_split", [(D, 37), (S, 11)], 45, (5, 3), "sigmoid", 3, 7, 13, Fl(32, True), Fl(32, True)),
    _conv("flat_bm32", [(D, 34)], 36, (5, 3), None, 2, 37, 230, Fl(32), Fl(32)),
    _conv("flat_bm64_split", [(D, 34)], 36, (5, 3), None, 2, 61, 237, Fl(64, True), Fl(64, True)),
    _conv("flat_bm64", [(D, 34)], 36, (5, 3), None, 2, 61, 256, Fl(64), Fl(64)),
    # ---- thin 7x7 path: CINP 1 / 2 / 4 / 8, 1 / 2 / 4 output-channel spans
    _conv("thin_c1_s4", [(D, 1)], 20, (7, 7), "relu", 3, 13, 21, Fl(32), Fl(32, True), spans=4,
          subsets=("nothin", "k7wgradoff")),
    _conv("thin_c1_s1_trainer", [(D, 1)], 4, (7, 7), "relu", 2, 9, 11, Fl(32), Fl(32), spans=1, split_bwd=True),
    _conv("thin_c2_s2", [(D, 2)], 7, (7, 7), None, 2, 9, 11, Fl(32), Fl(32, True), spans=2, alpha=0.5,
          subsets=("nothin",)),
    _conv("thin_c2_s4", [(S, 2)], 20, (7, 7), "tanh", 3, 13, 21, Fl(32), Fl(32, True), spans=4),
    _conv("thin_c3_s1", [(D, 3)], 4, (7, 7), "tanh", 3, 13, 21, Fl(32), Fl(32), spans=1),
    _conv("thin_c4_s2", [(S, 4)], 7, (7, 7), None, 2, 9, 11, Fl(32), Fl(32, True), spans=2),
    _conv("thin_c6_s4", [(D, 6)], 20, (7, 7), "relu", 3, 13, 21, Fl(32, True), Fl(32, True), spans=4,
          subsets=("nothin", "k7wgradoff")),
    _conv("thin_c6_bcast_trainer", [(BC, 6)], 20, (7, 7), "relu", 3, 13, 21, Fl(32, True), Fl(32, True), spans=4,
          split_bwd=True),
    _conv("thin_c8_s1", [(S, 8)], 16, (7, 7), None, 2, 96, 160, Fl(64), Fl(64), spans=1),
    # ---- strided convolutions (flat kernel only; stride-2 data gradient per parity class)
    _mk("s2_stem3", "strided", [(D, 3)], 72, (7, 7), None, 1.0, 3, 45, 77, {"fwd": Fl(32), "dgrad": Fl(32, True)},
        stride=2, pad=3, bias=False, subsets=("k7fwd", "k7wgradoff")),
    _mk("s2_stem6", "strided", [(D, 6)], 72, (7, 7), None, 1.0, 3, 45, 77, {"fwd": Fl(32, True), "dgrad": Fl(32, True)},
        stride=2, pad=3, bias=False, subsets=("k7fwd", "k7wgradoff")),
    _mk("s2_stem3_64", "strided", [(D, 3)], 64, (7, 7), None, 1.0, 1, 64, 96, {"fwd": Fl(32), "dgrad": Fl(32, True)},
        stride=2, pad=3, bias=False, subsets=("k7fwd",)),
    _mk("s2_c33", "strided", [(D, 20)], 24, (3, 3), None, 1.0, 2, 17, 23, {"fwd": Fl(32), "dgrad": Fl(32)},
        stride=2, pad=1),
    _mk("s2_c33_bm64", "strided", [(D, 16)], 24, (3, 3), None, 1.0, 2, 61, 237, {"fwd": Fl(32), "dgrad": Fl(64)},
        stride=2, pad=1, bias=False),
    _mk("s2_c11", "strided", [(D, 10)], 12, (1, 1), None, 1.0, 3, 9, 7, {"fwd": Fl(32), "dgrad": Fl(32)},
        stride=2, pad=0, bias=False),
    _mk("s2_c33_relu", "strided", [(D, 20)], 24, (3, 3), "relu", 1.0, 2, 17, 23, {"fwd": Fl(32), "dgrad": Fl(32)},
        stride=2, pad=1),
    _mk("s1_c33_nopad", "strided", [(D, 16)], 40, (3, 3), None, 1.0, 2, 12, 20, {"fwd": Fl(32), "dgrad": Fl(32, True)},
        stride=1, pad=0),
    # ---- SepConvGRU entry points: gates (EPI 2) + candidate (EPI 1) forward, the
    # plain backward, and the two folded data gradients (EPI 3 / 4)
    _mk("gru15_k4", "gru_half", [(D, 14), (BC, 6)], 32, (1, 5), None, 1.0, 2, 13, 37,
        {"gates": H(32, 4), "blend": H(32, 4), "dcand": H(32, 2), "dgates": H(32, 4)}),
    _mk("gru15_k2", "gru_half", [(S, 20)], 32, (1, 5), None, 1.0, 2, 37, 150,
        {"gates": H(32, 2), "blend": H(32, 4), "dcand": H(32, 2), "dgates": H(32, 2)}),
    _mk("gru51_k4", "gru_half", [(D, 14), (BC, 6)], 32, (5, 1), None, 1.0, 2, 19, 45,
        {"gates": H(32, 4), "blend": H(32, 4), "dcand": H(32, 2), "dgates": H(32, 4)}),
    _mk("gru51_k2", "gru_half", [(S, 20)], 32, (5, 1), None, 1.0, 2, 37, 150,
        {"gates": H(32, 2), "blend": H(32, 4), "dcand": H(32, 2), "dgates": H(32, 2)}),
    _mk("grucand15", "gru_cand_bwd", [(D, 14), (S, 6)], 32, (1, 5), None, 1.0, 2, 13, 37, {"dcand": H(32, 2)}),
    _mk("grucand51", "gru_cand_bwd", [(D, 14), (S, 6)], 32, (5, 1), None, 1.0, 2, 37, 150, {"dcand": H(32, 2)}),
    _mk("grucand33", "gru_cand_bwd", [(D, 20)], 32, (3, 3), None, 1.0, 1, 13, 37, {"dcand": H(32, 4)}),
    _mk("grugates15", "gru_gates_bwd", [(D, 14), (S, 6)], 32, (1, 5), None, 1.0, 2, 13, 37, {"dgates": H(32, 4)}),
    _mk("grugates51", "gru_gates_bwd", [(D, 14), (S, 6)], 32, (5, 1), None, 1.0, 2, 37, 150, {"dgates": H(32, 2)}),
    _mk("grugates33", "gru_gates_bwd", [(D, 20)], 32, (3, 3), None, 1.0, 1, 13, 37, {"dgates": H(32, 4, True)}),
    # ---- BatchNorm fused into the 3x3 convs (hip/bnconv.py): a stride-1 stage of
    # two BasicBlocks -- statistics epilogue (EPI 5) behind a plain, a BN+ReLU
    # (XF 1) and a BN+skip+ReLU (XF 2) staging; data gradients with the BN
    # backward's sums (EPI 6) and its apply staged (XF 3)
    _mk("bn_stage_bm64_k2", "bn_stage", [(D, 24)], 24, (3, 3), None, 1.0, 2, 61, 237, {"fwd": H(64, 2), "dgrad": H(64, 2)},
        bias=False),
    _mk("bn_stage_bm64_k1", "bn_stage", [(D, 24)], 24, (3, 3), None, 1.0, 2, 61, 250, {"fwd": H(64, 1), "dgrad": H(64, 1)},
        bias=False),
    _mk("bn_stage_bm32_k4", "bn_stage", [(D, 28)], 28, (3, 3), None, 1.0, 2, 19, 45, {"fwd": H(32, 4), "dgrad": H(32, 4)},
        bias=False),
]
CASES = [Case(**{**c.__dict__, "seed": 1000 + i}) for i, c in enumerate(CASES)]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# what each process-wide switch of the library must put in the launch log when
# its subset runs (tests/test_conv_toggles.py)
TOGGLES = {
    "k7fwd": ("DRO_K7_FWD", ["fwd_k7s2_kernel<3>", "fwd_k7s2_kernel<6>"], []),
    "k7wgradoff": ("DRO_K7_WGRAD_OFF", ["wgrad_kernel("], ["wgrad_k7_kernel"]),
    "nothin": ("DRO_CONV_NO_THIN", ["igemm_kernel<32, 0, 1, 0>", "igemm_kernel<32, 1, 0, 0>", "igemm_kernel<32, 0, 0, 0>"],
               ["thin_fwd_kernel", "thin_dgrad_kernel"]),
}


# ------------------------------------------------------------------ inputs
def make_src(kind, B, C, Hh, W, g):
    """(base tensor, view function).  kind: 'dense' | 'slice' (channels 3..3+C of
    a wider tensor whose other channels hold NaN: a channel over-read shows
    in the output) | 'bcast' ([B,C,1,1] expanded over H x W)."""
    if kind == "bcast":
        return torch.randn(B, C, 1, 1, generator=g), lambda t: t.expand(B, C, Hh, W)
    if kind == "slice":
        base = torch.full((B, C + 5, Hh, W), float("nan"))
        base[:, 3:3 + C] = torch.randn(B, C, Hh, W, generator=g)
        return base, lambda t: t[:, 3:3 + C]
    return torch.randn(B, C, Hh, W, generator=g), lambda t: t


def _grad_of(kind, base_grad, C):
    return base_grad[:, 3:3 + C] if kind == "slice" else base_grad


def out_hw(c):
    if c.call != "strided":
        return c.H, c.W
    return (c.H + 2 * c.pad - c.k[0]) // c.stride + 1, (c.W + 2 * c.pad - c.k[1]) // c.stride + 1


def build_inputs(c):
    """CPU fp32 inputs of a case (deterministic in the case's seed)."""
    g = torch.Generator().manual_seed(c.seed)
    B, Hh, W, (KH, KW) = c.B, c.H, c.W, c.k
    Ho, Wo = out_hw(c)
    rnd = lambda *s: torch.randn(*s, generator=g)
    inp = {}
    if c.call in ("conv2d", "strided"):
        inp["srcs"] = [make_src(kd, B, C, Hh, W, g) for kd, C in c.srcs]
        inp["w"] = rnd(c.cout, c.cin, KH, KW) / math.sqrt(c.cin * KH * KW)
        inp["b"] = rnd(c.cout) * 0.1 if c.bias else None
        inp["gout"] = rnd(B, c.cout, Ho, Wo)
        if c.call == "conv2d" and c.k in HALO_SHAPES:      # a second use for the multi-use weight gradient
            inp["srcs2"] = [make_src(kd, B, C, Hh, W, g) for kd, C in c.srcs]
            inp["gout2"] = rnd(B, c.cout, Hh, W)
        return inp
    if c.call == "bn_stage":
        C = c.cout
        inp["x"] = 0.5 + rnd(B, C, Hh, W)
        inp["gout"] = rnd(B, C, Hh, W)
        for i in range(2):
            for j in (1, 2):
                inp[f"{i}.conv{j}.weight"] = rnd(C, C, 3, 3) / math.sqrt(C * 9)
                inp[f"{i}.bn{j}.weight"] = 0.5 + torch.rand(C, generator=g)
                inp[f"{i}.bn{j}.bias"] = 0.6 * torch.rand(C, generator=g) - 0.3
        return inp
    hd, cin = c.cout, c.cout + c.cin
    sc = 1.0 / math.sqrt(cin * KH * KW)
    inp["xs"] = [make_src(kd, B, C, Hh, W, g) for kd, C in c.srcs]
    if c.call == "gru_half":
        inp["h"] = rnd(B, hd, Hh, W).tanh()
        inp["ws"] = [rnd(hd, cin, KH, KW) * sc for _ in range(3)]
        inp["bs"] = [rnd(hd) * 0.1 for _ in range(3)]
        inp["gout"] = rnd(B, hd, Hh, W)
    elif c.call == "gru_cand_bwd":
        inp.update(rh=rnd(B, hd, Hh, W), wq=rnd(hd, cin, KH, KW) * sc, dq=rnd(B, hd, Hh, W),
                   zr=torch.sigmoid(rnd(B, 2 * hd, Hh, W)), h=rnd(B, hd, Hh, W), dh0=rnd(B, hd, Hh, W),
                   dzr0=rnd(B, 2 * hd, Hh, W), gx0=[rnd(B, C, Hh, W) for _, C in c.srcs])
    else:
        inp.update(h2=rnd(B, hd, Hh, W), wzr=rnd(2 * hd, cin, KH, KW) * sc, dzr2=rnd(B, 2 * hd, Hh, W),
                   dh2_0=rnd(B, hd, Hh, W), gx0=[rnd(B, C, Hh, W) for _, C in c.srcs],
                   zr1=torch.sigmoid(rnd(B, 2 * hd, Hh, W)), q1=torch.tanh(rnd(B, hd, Hh, W)), h1=rnd(B, hd, Hh, W),
                   dzr1_0=rnd(B, 2 * hd, Hh, W), dh1_0=rnd(B, hd, Hh, W))
    return inp


# ------------------------------------------------------------------ reference (torch on the CPU, any dtype)
def _act_ref(pre, act, alpha, mask):
    """act(pre) * alpha; ReLU takes its on/off decision from `mask` (the fp32
    result's: a pre-activation within fp32 rounding of 0 may fall either side)."""
    if act == "relu":
        m = (pre.detach() > 0) if mask is None else mask
        return pre * m.to(pre.dtype) * alpha
    return ACTS[act](pre) * alpha


def _gru_ref(h, xs, wz, bz, wr, br, wq, bq, pad):
    hx = torch.cat([h, *xs], 1)
    z = torch.sigmoid(F.conv2d(hx, wz, bz, padding=pad))
    r = torch.sigmoid(F.conv2d(hx, wr, br, padding=pad))
    q = torch.tanh(F.conv2d(torch.cat([r * h, *xs], 1), wq, bq, padding=pad))
    return (1 - z) * h + z * q


def reference(c, inp, dt, masks=None):
    """{label: tensor} of the case in dtype `dt` on the CPU.  masks: the ReLU
    decisions to take ({label: bool tensor}); None takes this evaluation's own."""
    masks = masks or {}
    KH, KW = c.k
    pad = (KH // 2, KW // 2)
    leaf = lambda t: t.to(dt).requires_grad_()
    res = {}
    if c.call in ("conv2d", "strided"):
        bases = [leaf(b) for b, _ in inp["srcs"]]
        x = torch.cat([v(t) for (_, v), t in zip(inp["srcs"], bases)], 1)
        w = leaf(inp["w"])
        b = leaf(inp["b"]) if inp["b"] is not None else None
        if c.call == "strided":
            pre = F.conv2d(x, w, b, stride=c.stride, padding=c.pad)
        else:
            pre = F.conv2d(x, w, b, padding=pad)
        out = _act_ref(pre, c.act, c.alpha, masks.get("out"))
        res["out"] = out.detach()
        if c.call == "strided" and c.act is not None:
            return res                                  # forward-only (no backward through a fused activation)
        gs = torch.autograd.grad(out, bases + [w] + ([b] if b is not None else []), inp["gout"].to(dt))
        for i, (kd, C) in enumerate(c.srcs):
            res[f"dx{i}"] = _grad_of(kd, gs[i], C)
        res["dw"] = gs[len(bases)]
        if b is not None:
            res["db"] = gs[-1]
        if "srcs2" in inp:
            x2 = torch.cat([v(t.to(dt)) for t, v in inp["srcs2"]], 1)
            out2 = _act_ref(F.conv2d(x2, w, b, padding=pad), c.act, c.alpha, masks.get("out2"))
            res["out2"] = out2.detach()
            g2 = torch.autograd.grad(out2, [w] + ([b] if b is not None else []), inp["gout2"].to(dt))
            res["dw_multi"] = res["dw"] + g2[0]
            if b is not None:
                res["db_multi"] = res["db"] + g2[1]
        return res
    if c.call == "bn_stage":
        p = {k: leaf(v) for k, v in inp.items() if "." in k}
        x = leaf(inp["x"])
        h = x
        for i in range(2):
            def bn(z, name):
                return F.batch_norm(z, None, None, p[name + ".weight"], p[name + ".bias"], training=True, eps=1e-5)
            z1 = bn(F.conv2d(h, p[f"{i}.conv1.weight"], padding=1), f"{i}.bn1")
            m1 = masks.get(f"b{i}.bn1", z1.detach() > 0)
            y = z1 * m1.to(dt)
            z2 = bn(F.conv2d(y, p[f"{i}.conv2.weight"], padding=1), f"{i}.bn2") + h
            m2 = masks.get(f"b{i}.bn2", z2.detach() > 0)
            h = z2 * m2.to(dt)
            res[f"mask:b{i}.bn1"], res[f"mask:b{i}.bn2"] = m1, m2
        names = sorted(p)
        gs = torch.autograd.grad(h, [x] + [p[n] for n in names], inp["gout"].to(dt))
        res["out"], res["dx0"] = h.detach(), gs[0]
        for n, g_ in zip(names, gs[1:]):
            res[("dw_" if "conv" in n else "g_") + n] = g_
        return res
    hd = c.cout
    xb = [leaf(b) for b, _ in inp["xs"]]
    xs = [v(t) for (_, v), t in zip(inp["xs"], xb)]
    if c.call == "gru_half":
        h = leaf(inp["h"])
        ws, bs = [leaf(t) for t in inp["ws"]], [leaf(t) for t in inp["bs"]]
        out = _gru_ref(h, xs, ws[0], bs[0], ws[1], bs[1], ws[2], bs[2], pad)
        gs = torch.autograd.grad(out, [h] + xb + ws + bs, inp["gout"].to(dt))
        res["out"], res["dh"] = out.detach(), gs[0]
        for i, (kd, C) in enumerate(c.srcs):
            res[f"dx{i}"] = _grad_of(kd, gs[1 + i], C)
        n = 1 + len(xb)
        for i in range(3):
            res[f"dw{i}"], res[f"db{i}"] = gs[n + i], gs[n + 3 + i]
        return res
    t = lambda k: inp[k].to(dt)
    if c.call == "gru_cand_bwd":
        # d(r*h) of the candidate conv feeds stage 2: dzr[:, hd:] = d(rh) h r (1 - r), dh += d(rh) r
        rh = leaf(inp["rh"])
        q = F.conv2d(torch.cat([rh, *xs], 1), t("wq"), None, padding=pad)
        gs = torch.autograd.grad(q, [rh] + xb, t("dq"))
        r = t("zr")[:, hd:]
        res["dzr_r"] = gs[0] * t("h") * r * (1 - r)
        res["dzr_z"] = t("dzr0")[:, :hd]                      # the z half untouched
        res["dh"] = t("dh0") + gs[0] * r
        for i, (kd, C) in enumerate(c.srcs):                  # source i overwritten (even) / added into (odd)
            res[f"dx{i}"] = _grad_of(kd, gs[1 + i], C) + (inp["gx0"][i].to(dt) if i % 2 else 0)
        return res
    # gru_gates_bwd: the finished d h of this half is the first half's dh': stage 1 in the epilogue
    h2 = leaf(inp["h2"])
    zr = F.conv2d(torch.cat([h2, *xs], 1), t("wzr"), None, padding=pad)
    gs = torch.autograd.grad(zr, [h2] + xb, t("dzr2"))
    dhn = t("dh2_0") + gs[0]
    z1, q1, h1 = t("zr1")[:, :hd], t("q1"), t("h1")
    res["dh2"] = dhn
    for i, (kd, C) in enumerate(c.srcs):
        res[f"dx{i}"] = _grad_of(kd, gs[1 + i], C) + (inp["gx0"][i].to(dt) if i % 2 else 0)
    res["dq1"] = dhn * z1 * (1 - q1 * q1)
    res["dzr1_z"] = dhn * (q1 - h1) * z1 * (1 - z1)
    res["dzr1_r"] = t("dzr1_0")[:, hd:]                       # the r half untouched
    res["dh1"] = t("dh1_0") + dhn * (1 - z1)                  # added into (prev_dh_accumulate)
    return res


# ------------------------------------------------------------------ the kernels (GPU)
def run_gpu(c, inp):
    """({label: tensor}, {label: ReLU mask}) of the case on the HIP conv engine."""
    import dro_sfm_amd.hip as hip
    from dro_sfm_amd.hip import _lib, conv as C
    lib = _lib.load()
    KH, KW = c.k
    res, masks = {}, {}
    dev = lambda t: t.to(DEV)
    if c.call == "strided":
        x = dev(inp["srcs"][0][0]).requires_grad_()
        w = dev(inp["w"]).requires_grad_()
        b = dev(inp["b"]).requires_grad_() if inp["b"] is not None else None
        if c.act is not None:
            with torch.no_grad():
                res["out"] = hip.conv2d_strided(x, w, b, c.stride, c.pad, act=c.act)
            masks["out"] = (res["out"] > 0).cpu()
            return res, masks
        out = hip.conv2d_strided(x, w, b, c.stride, c.pad)
        out.backward(dev(inp["gout"]))
        res.update(out=out.detach(), dx0=x.grad, dw=w.grad)
        if b is not None:
            res["db"] = b.grad
        return res, masks
    if c.call == "conv2d":
        joint = not c.split_bwd
        bases = [dev(b).requires_grad_() for b, _ in inp["srcs"]]
        views = [v(t) for (_, v), t in zip(inp["srcs"], bases)]
        w = dev(inp["w"]).requires_grad_(joint)
        b = dev(inp["b"]).requires_grad_(joint) if inp["b"] is not None else None
        out = hip.conv2d(views, w, b, act=c.act, alpha=c.alpha)
        out.backward(dev(inp["gout"]))
        res["out"] = out.detach()
        masks["out"] = (res["out"] > 0).cpu()
        for i, (kd, Cc) in enumerate(c.srcs):
            res[f"dx{i}"] = _grad_of(kd, bases[i].grad, Cc)
        if joint:
            res["dw"] = w.grad
            if b is not None:
                res["db"] = b.grad
        else:
            # the weight gradient in a call of its own, as the trainer's direct path makes it
            gw = torch.empty_like(w)
            gb = torch.empty(c.cout, device=DEV) if b is not None else None
            vs = [v.detach() for v in views]
            C._conv_bwd(vs, w.detach(), res["out"] if c.act else None, dev(inp["gout"]), ACT_ID[c.act], c.alpha,
                        [None] * len(vs), [0] * len(vs), gw, gb, 0)
            res["dw"] = gw
            if gb is not None:
                res["db"] = gb
        if "srcs2" in inp:
            # the deferred multi-use weight gradient over this use and a second one, added into a gradient
            v2 = [dev(v(t)) for t, v in inp["srcs2"]]
            with torch.no_grad():
                y2 = hip.conv2d(v2, w.detach(), b.detach() if b is not None else None, act=c.act, alpha=c.alpha)
            res["out2"] = y2
            masks["out2"] = (y2 > 0).cpu()
            uses = [([v.detach() for v in views], dev(inp["gout"]), res["out"]), (v2, dev(inp["gout2"]), y2)]
            gw0, gb0 = torch.randn_like(w), torch.randn(c.cout, device=DEV)
            gw, gb = gw0.clone(), gb0.clone()
            arr = (C.DroWgradUse * 2)()
            keep = []
            for i, (ss, dout, y) in enumerate(uses):
                sl = C._slices(ss)
                keep.append(sl)
                arr[i].srcs = ctypes.cast(sl, ctypes.c_void_p)
                arr[i].dout = dout.data_ptr()
                arr[i].y = y.data_ptr() if c.act else None
            nb = lib.dro_conv2d_weight_grad_multi_workspace_bytes(2, c.B, c.H, c.W, c.cin, c.cout, KH, KW)
            ws = torch.empty(max(int(nb), 1), dtype=torch.uint8, device=DEV)
            st = lib.dro_conv2d_weight_grad_multi(arr, 2, len(c.srcs), c.B, c.H, c.W, c.cout, KH, KW, ACT_ID[c.act],
                                                  ctypes.c_float(c.alpha), gw.data_ptr(),
                                                  gb.data_ptr() if b is not None else None, 1, ws.data_ptr(), nb, None)
            assert st == 0, lib.dro_last_error()
            torch.cuda.synchronize()
            res["dw_multi"] = gw - gw0
            if b is not None:
                res["db_multi"] = gb - gb0
        return res, masks
    if c.call == "bn_stage":
        from dro_sfm_amd.hip import bnconv
        from dro_sfm_amd.hip.ops import record_bilinear_cells
        from dro_sfm_amd.networks.optim import extractor
        stage = extractor._stage(c.cout, c.cout, 1)
        with torch.no_grad():
            for n, p in stage.named_parameters():
                p.copy_(inp[n])
        stage = stage.to(DEV).train()
        for i in range(2):
            for nm in ("bn1", "bn2"):
                object.__setattr__(getattr(stage[i], nm), "_dro_tag", f"b{i}.{nm}")
        x = dev(inp["x"]).requires_grad_()
        bnconv.set_bn_fusion("all")
        try:
            with record_bilinear_cells() as rec:
                out = extractor.run_stage(stage, x)
            out.backward(dev(inp["gout"]))
        finally:
            bnconv.set_bn_fusion(True)
        masks.update({tag[1]: m.bool().cpu() for tag, m in rec.calls if tag[0] == "relu"})
        res.update(out=out.detach(), dx0=x.grad)
        for n, p in stage.named_parameters():
            res[("dw_" if "conv" in n else "g_") + n] = p.grad
        return res, masks
    hd = c.cout
    pad = (KH // 2, KW // 2)
    xb = [dev(b).requires_grad_(c.call == "gru_half") for b, _ in inp["xs"]]
    xs = [v(t) for (_, v), t in zip(inp["xs"], xb)]
    if c.call == "gru_half":
        h = dev(inp["h"]).requires_grad_()
        convs = [torch.nn.Conv2d(hd + c.cin, hd, c.k, padding=pad).to(DEV) for _ in range(3)]
        for cv, w_, b_ in zip(convs, inp["ws"], inp["bs"]):
            cv.weight, cv.bias = torch.nn.Parameter(dev(w_)), torch.nn.Parameter(dev(b_))
        out = hip.sepconvgru_half(h, convs[0], convs[1], convs[2], xs)
        out.backward(dev(inp["gout"]))
        res.update(out=out.detach(), dh=h.grad)
        for i, (kd, Cc) in enumerate(c.srcs):
            res[f"dx{i}"] = _grad_of(kd, xb[i].grad, Cc)
        for i, cv in enumerate(convs):
            res[f"dw{i}"], res[f"db{i}"] = cv.weight.grad, cv.bias.grad
        return res, masks
    gx = [dev(t).clone() for t in inp["gx0"]]
    acc = [0] + [i % 2 for i in range(len(xs))]
    if c.call == "gru_cand_bwd":
        dh, dzr = dev(inp["dh0"]).clone(), dev(inp["dzr0"]).clone()
        torch.ops.dro.convgru_candidate_backward([dev(inp["rh"]), *xs], dev(inp["wq"]), dev(inp["dq"]), dev(inp["zr"]),
                                                 dev(inp["h"]), dzr, dh, [torch.empty(0, device=DEV), *gx], acc)
        res.update(dzr_r=dzr[:, hd:], dzr_z=dzr[:, :hd], dh=dh)
    else:
        dh2, dzr1, dh1 = dev(inp["dh2_0"]).clone(), dev(inp["dzr1_0"]).clone(), dev(inp["dh1_0"]).clone()
        dq1 = torch.empty_like(dh1)
        acc[0] = 1
        torch.ops.dro.convgru_gates_backward([dev(inp["h2"]), *xs], dev(inp["wzr"]), dev(inp["dzr2"]), [dh2, *gx], acc,
                                             dev(inp["zr1"]), dev(inp["q1"]), dev(inp["h1"]), dq1, dzr1, dh1, 1)
        res.update(dh2=dh2, dq1=dq1, dzr1_z=dzr1[:, :hd], dzr1_r=dzr1[:, hd:], dh1=dh1)
    for i in range(len(xs)):
        res[f"dx{i}"] = gx[i]
    torch.cuda.synchronize()
    return res, masks


# ------------------------------------------------------------------ comparison
def _per_channel(d, ref, dim):
    """The largest max|a - b| over a channel in units of that channel's max|ref|
    (0 where both vanish, inf where only the reference does)."""
    dims = [i for i in range(d.dim()) if i != dim]
    dm, rm = d.amax(dims), ref.amax(dims)
    ratio = torch.where(rm > 0, dm / rm.clamp_min(1e-300),
                        torch.where(dm > 0, torch.full_like(dm, float("inf")), torch.zeros_like(dm)))
    return ratio.max().item()


def channel_dim(label, t):
    """out / source gradients / states: channel = dim 1; weight gradients: the
    output-channel rows, dim 0; biases and BN affine gradients: global only."""
    if t.dim() != 4:
        return None
    return 0 if label.startswith("dw") else 1


def compare(got, ref, bound):
    """([(label, global error, per-channel error)] over `bound`, the worst
    figure).  Global: max|a - b| / max|ref| < bound; per channel (where the
    tensor has channels): max|a - b| over the channel <= bound x max|ref| over
    it.  A NaN anywhere in the result fails both."""
    bad, worst = [], 0.0
    for label, r in ref.items():
        if label.startswith("mask:") or label == "out2":
            continue
        a, b = got[label].detach().double().cpu(), r.detach().double().cpu()
        assert a.shape == b.shape, (label, a.shape, b.shape)
        d = (a - b).abs()
        if torch.isnan(d).any():
            bad.append((label, float("inf"), float("inf")))
            worst = float("inf")
            continue
        glob = (d.max() / b.abs().max().clamp_min(1e-30)).item()
        cd = channel_dim(label, b)
        pc = _per_channel(d, b.abs(), cd) if cd is not None else 0.0
        worst = max(worst, glob, pc)
        if not (glob < bound and pc <= bound):
            bad.append((label, glob, pc))
    return bad, worst


def calibrate(c):
    """A plain fp32 evaluation on the CPU against the fp64 one (ReLU decisions
    shared): the offenders over CALIB, and the worst figure."""
    inp = build_inputs(c)
    r32 = reference(c, inp, torch.float32)
    masks = {k: (v > 0) for k, v in r32.items() if k in ("out", "out2") and c.act == "relu"}
    masks.update({k[5:]: v for k, v in r32.items() if k.startswith("mask:")})
    r64 = reference(c, inp, torch.float64, masks)
    return compare(r32, r64, CALIB)


def check_gpu(c):
    """Run the case on the GPU with the launch log on; returns (logged names,
    offenders over TOL, worst figure)."""
    inp = build_inputs(c)
    with conv_log() as names:
        got, masks = run_gpu(c, inp)
        torch.cuda.synchronize()
    ref = reference(c, inp, torch.float64, masks)
    bad, worst = compare(got, ref, TOL)
    return names, bad, worst


# ------------------------------------------------------------------ child process of tests/test_conv_toggles.py
def main(argv):
    subset = argv[argv.index("--subset") + 1]
    env, must, must_not = TOGGLES[subset]
    assert os.environ.get(env), f"{env} is not set"
    seen, failed = set(), []
    for c in CASES:
        if subset not in c.subsets:
            continue
        names, bad, worst = check_gpu(c)
        seen |= names
        print(f"{c.name}: worst {worst:.2e} names {sorted(names)}", flush=True)
        if bad:
            failed.append((c.name, bad))
    missing = [n for n in must if n not in seen]
    stray = [n for n in seen if any(n.startswith(p) for p in must_not)]
    if failed or missing or stray:
        print(f"FAILED parity {failed} missing {missing} stray {stray}", flush=True)
        return 1
    print("ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
