"""Inference throughput: the eager eval forward against the fused eval
BatchNorm and against models.session.InferenceSession's graph replays.

Times, in one process and alternating, on seeded inputs (no dataset):
  (a) eager, fused eval BN off -- the path as it was before the session
      existed (its code is unchanged), the reference for time;
  (b) eager, fused eval BN on (networks.optim.extractor.fused_eval_batchnorm);
  (c) an InferenceSession: fused eval BN, the forward replayed from a hipGraph.
Workloads: the three of tools/eval_throughput.py through evaluate_depth
(KITTI 192x640 N=2 it8-seq4-inter-out at B=1 and B=4, ScanNet 240x320 N=4
it12-h-out at B=1), and reconstruct_sequence on T=32 KITTI-size frames (the
workload of tools/reconstruct_throughput.py).  Each variant is warmed up (the
session captures there), then timed with device events in `--repeats` chunks
of about `--seconds / --repeats` each, a chunk of (a), of (b), of (c); the
spread is (max - min) / median over the chunks.  A workload is accepted when
(c) beats (a) by more than the sum of their spreads and (b) is not slower than
(a) by more than the sum of theirs.  The outputs of (a) and (c) are compared
at the timed sizes: max|d| / max|ref| (they differ by the BN formula's
rounding, which the recurrence carries on).

The kernel alone: hip.batchnorm_eval_act at the largest eval site, fnet's
layer1 at KITTI B=4 (the 12 images of one forward, [12, 64, 48, 160]), against
ATen's batch_norm + add + relu, in bytes moved (8 per element, 12 with the
skip) over the median time of a call, calls issued back to back.

    python tools/infer_session_throughput.py > profiles/infer_session_throughput.txt
"""
import argparse
import os
import statistics
import sys
from collections import OrderedDict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

COPY_CEILING = 6.29e12      # bytes/s, the device-to-device copy rate measured on MI355X


def chunk_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def alternate(variants, args):
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    iters = {v: max(2, int(args.seconds * 1e3 / args.repeats / chunk_ms(fn, 3))) for v, fn in variants.items()}
    times = {v: [] for v in variants}
    for _ in range(args.repeats):
        for vname, fn in variants.items():
            times[vname].append(chunk_ms(fn, iters[vname]))
    return times, iters


def summary(ts):
    med = statistics.median(ts)
    return med, (max(ts) - min(ts)) / med


def verdict(times):
    (a, sa), (b, sb), (c, sc) = (summary(times[v]) for v in ("eager", "eager_fused_bn", "session"))
    c_wins = (a - c) / a > sa + sc
    b_ok = (b - a) / a <= sa + sb
    return c_wins and b_ok, (f"session {a / c:.2f}x eager ({'beats' if c_wins else 'does NOT beat'} it by more than the "
                             f"spreads' sum {100 * (sa + sc):.1f}%), eager_fused_bn {a / b:.2f}x eager "
                             f"({'not slower' if b_ok else 'SLOWER'} beyond {100 * (sa + sb):.1f}%)")


def three(model, call):
    """The variants of one workload: call(model_or_session) under each setting."""
    from dro_sfm_amd.models.session import InferenceSession
    from dro_sfm_amd.networks.optim.extractor import fused_eval_batchnorm
    session = InferenceSession(model)

    def fused():
        with fused_eval_batchnorm(True):
            return call(model)

    return OrderedDict(eager=lambda: call(model), eager_fused_bn=fused, session=lambda: call(session)), session


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def kernel_alone(args, dev):
    import dro_sfm_amd.hip as hip
    from dro_sfm_amd.networks.optim.extractor import BatchNorm2d
    N, C, H, W = 12, 64, 48, 160
    g = torch.Generator().manual_seed(7)
    x, skip = torch.randn(N, C, H, W, generator=g).to(dev), torch.randn(N, C, H, W, generator=g).to(dev)
    bn = BatchNorm2d(C).to(dev).eval()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(C, generator=g))
        for with_skip in (False, True):
            s = skip if with_skip else None
            variants = OrderedDict(hip=lambda: hip.batchnorm_eval_act(x, bn, skip=s),
                                   aten=lambda: bn.act(x, skip=s))
            err = rel(variants["hip"](), variants["aten"]())
            times, iters = alternate(variants, args)
            nbytes = (12 if with_skip else 8) * x.numel()
            line = [f"batchnorm_eval_act [{N},{C},{H},{W}] skip={with_skip} relu=True ({nbytes / 1e6:.1f} MB moved):"]
            for v in variants:
                med, spread = summary(times[v])
                rate = nbytes / (med * 1e-3)
                line.append(f"{v} {med * 1e3:.1f} us/call (spread {100 * spread:.1f}% over {len(times[v])} x {iters[v]} "
                            f"calls), {rate / 1e12:.2f} TB/s = {100 * rate / COPY_CEILING:.0f}% of the 6.29 TB/s copy "
                            f"ceiling")
            line.append(f"outputs agree: {err:.1e}")
            print("  ".join(line), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seconds", type=float, default=2.5, help="timed seconds per variant and workload (>= 2)")
    ap.add_argument("--repeats", type=int, default=5, help="alternating chunks per variant")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=32, help="T of the reconstruct_sequence workload (0: skip)")
    ap.add_argument("--workloads", nargs="*", default=None, help="of tools/eval_throughput.py (default: all)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("infer_session_throughput: needs a ROCm device (timings on a CPU say nothing)")
    import eval_throughput as ET
    from dro_sfm_amd.models.evaluate import evaluate_depth
    dev = torch.device("cuda", 0)
    accepted = []
    kernel_alone(args, dev)
    for name, wl in ET.WORKLOADS:
        if args.workloads is not None and name not in args.workloads:
            continue
        model, batch, params = ET.make(wl, dev)
        variants, session = three(model, lambda m: evaluate_depth(m, batch, params))
        times, iters = alternate(variants, args)
        a, c = variants["eager"](), variants["session"]()
        torch.cuda.synchronize()
        err = rel(c["inv_depth"], a["inv_depth"])
        line = [f"evaluate_depth {name} {wl['version']} B={wl['B']} N={wl['N']} {wl['H']}x{wl['W']}:"]
        for v in variants:
            med, spread = summary(times[v])
            line.append(f"{v} {wl['B'] * 1e3 / med:.1f} img/s ({med:.2f} ms/call, spread {100 * spread:.1f}% over "
                        f"{len(times[v])} x {iters[v]} calls)")
        ok, txt = verdict(times)
        accepted.append(ok)
        line.append(txt)
        line.append(f"session vs eager outputs: inv_pp {err:.1e} of max, {session.captures} capture(s)")
        print("  ".join(line), flush=True)
        session.release()
        del model, batch, variants, session
    if args.frames >= 3:
        from common import det_init, kitti_K, smooth_images
        from dro_sfm_amd.models.reconstruct import default_params, reconstruct_sequence
        from dro_sfm_amd.models.SfmModelMF import SfmModelMF
        from dro_sfm_amd.networks.depth_pose.DepthPoseNet import DepthPoseNet
        T, H, W = args.frames, 192, 640
        model = SfmModelMF(flip_lr_prob=0.0, min_depth=0.5, max_depth=80.0)
        model.add_depth_net(det_init(DepthPoseNet(version="it8-seq4-inter-out", min_depth=0.5, max_depth=80.0)))
        model = model.to(dev)
        frames, K = smooth_images(T, H, W, 41).to(dev), kitti_K(1)[0].to(dev)
        rp = default_params(kitti=True)
        variants, session = three(model, lambda m: reconstruct_sequence(m, frames, K, rp))
        times, iters = alternate(variants, args)
        a, c = variants["eager"](), variants["session"]()
        torch.cuda.synchronize()
        line = [f"reconstruct_sequence it8-seq4-inter-out T={T} {H}x{W} ({T - 2} frames reconstructed, 4 per forward):"]
        for v in variants:
            med, spread = summary(times[v])
            line.append(f"{v} {(T - 2) * 1e3 / med:.1f} frames/s ({med:.2f} ms/call, spread {100 * spread:.1f}% over "
                        f"{len(times[v])} x {iters[v]} calls)")
        ok, txt = verdict(times)
        accepted.append(ok)
        line.append(txt)
        line.append(f"session vs eager outputs: depths {rel(c['depths'], a['depths']):.1e} of max, points "
                    f"{c['points'].shape[0]} vs {a['points'].shape[0]}, {session.captures} capture(s)")
        print("  ".join(line), flush=True)
    print(f"acceptance: {'ACCEPTED' if accepted and all(accepted) else 'NOT accepted'} "
          f"({sum(accepted)} of {len(accepted)} workloads)", flush=True)


if __name__ == "__main__":
    main()
