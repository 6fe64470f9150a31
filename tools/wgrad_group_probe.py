"""Grouped weight gradient in isolation: one group of the benchmark step,
launched as ONE dro_conv2d_weight_grad_group call and as one
dro_conv2d_weight_grad_multi call per member, timed with events on an
otherwise idle GPU.

usage: python tools/wgrad_group_probe.py [fnet|gru1x5|heads] [iters=50] [grouped|single|both]
Under `rocprofv3 --kernel-trace --stats` for per-kernel times, or
`rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` (one counter per run) for
the HBM traffic per launch."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dro_sfm_amd.hip import _lib  # noqa: E402
from dro_sfm_amd.hip.conv import DroWgradMember, DroWgradUse, _slices  # noqa: E402

# (KH, KW, act, [(uses, B, H, W, Cin, Cout)]): groups of the KITTI self-supervised step
GROUPS = {
    "fnet": (3, 3, 0, [(1, 6, 48, 160, 64, 64)] * 4),
    "gru1x5": (1, 5, 0, [(8, 2, 24, 80, 160, 128), (8, 2, 24, 80, 160, 64)]),
    "heads": (3, 3, 1, [(8, 2, 24, 80, 64, 192), (8, 2, 24, 80, 128, 63), (8, 2, 24, 80, 64, 64)]),
}


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "fnet"
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    which = sys.argv[3] if len(sys.argv) > 3 else "both"
    KH, KW, act, shapes = GROUPS[name]
    lib = _lib.load()
    dev = "cuda"
    members = (DroWgradMember * len(shapes))()
    keep, single = [], []
    flops = bytes_min = 0.0
    for i, (uses, B, H, W, Cin, Cout) in enumerate(shapes):
        arr = (DroWgradUse * uses)()
        for j in range(uses):
            x, g = torch.randn(B, Cin, H, W, device=dev), torch.randn(B, Cout, H, W, device=dev)
            y = torch.rand(B, Cout, H, W, device=dev) if act else None
            sl = _slices([x])
            keep.append((x, g, y, sl))
            arr[j].srcs, arr[j].dout = ctypes.cast(sl, ctypes.c_void_p), g.data_ptr()
            arr[j].y = y.data_ptr() if act else None
        gw, gb = torch.zeros(Cout, Cin, KH, KW, device=dev), torch.zeros(Cout, device=dev)
        keep.append((arr, gw, gb))
        m = members[i]
        m.uses, m.nuse, m.nsrc = ctypes.cast(arr, ctypes.c_void_p), uses, 1
        m.B, m.H, m.W, m.Cout, m.alpha = B, H, W, Cout, 1.0
        m.grad_weight, m.grad_bias, m.accumulate = gw.data_ptr(), gb.data_ptr(), 1
        nb1 = lib.dro_conv2d_weight_grad_multi_workspace_bytes(uses, B, H, W, Cin, Cout, KH, KW)
        single.append((arr, uses, B, H, W, Cout, gw, gb, torch.empty(max(nb1, 1), dtype=torch.uint8, device=dev), nb1))
        flops += 2.0 * Cout * Cin * KH * KW * B * H * W * uses
        # algorithmic bytes: every input and output gradient (and saved output) read once, the gradient written
        bytes_min += 4.0 * (uses * B * H * W * (Cin + Cout * (2 if act else 1)) + Cout * Cin * KH * KW)
    nb = lib.dro_conv2d_weight_grad_group_workspace_bytes(members, len(shapes), KH, KW)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)

    def grouped():
        st = lib.dro_conv2d_weight_grad_group(members, len(shapes), KH, KW, act, ws.data_ptr(), nb, None)
        assert st == 0, lib.dro_last_error()

    def per_weight():
        for arr, uses, B, H, W, Cout, gw, gb, w1, nb1 in single:
            st = lib.dro_conv2d_weight_grad_multi(arr, uses, 1, B, H, W, Cout, KH, KW, act, ctypes.c_float(1.0),
                                                  gw.data_ptr(), gb.data_ptr(), 1, w1.data_ptr(), nb1, None)
            assert st == 0, lib.dro_last_error()

    print(f"{name}: {len(shapes)} members, {flops / 1e9:.2f} GFLOP, algorithmic {bytes_min / 1e6:.1f} MB, "
          f"group workspace {nb / 1e6:.1f} MB, per-weight workspaces {sum(s[-1] for s in single) / 1e6:.1f} MB")
    for label, fn in (("grouped", grouped), ("single", per_weight)):
        if which not in (label, "both"):
            continue
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        us = t0.elapsed_time(t1) * 1e3 / iters
        print(f"  {label}: {us:.1f} us per group (main + finish launches), {flops / us / 1e6:.1f} TF/s "
              f"= {flops / us / 1e6 / 157.3:.2f} of the f32 MFMA peak")


if __name__ == "__main__":
    main()
