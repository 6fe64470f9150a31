"""Validation throughput: evaluate_depth against the two-pass sequence.

Times, in one process and alternating, on seeded inputs (no dataset):
  (a) models.evaluate.evaluate_depth -- one forward of batch 2B, one
      post-process launch, the metric kernels;
  (b) what a user would write from the pieces that existed before it: the
      model called twice (plain and flipped), post_process_inv_depth and
      inv2depth in torch ops, four compute_depth_metrics calls.
Workloads: KITTI 192x640, N=2, it8-seq4-inter-out at B=1 and B=4 (375x1242
sparse ground truth, garg crop); ScanNet 240x320, N=4, it12-h-out at B=1
(480x640 dense ground truth).  Each variant is warmed up, then timed with
device events in `--repeats` chunks of about `--seconds / --repeats` each,
a chunk of (a) then a chunk of (b); images/s = B / median chunk time per
call, the spread is (max - min) / median over the chunks.

    python tools/eval_throughput.py > profiles/eval_throughput.txt
"""
import argparse
import os
import statistics
import sys
from collections import OrderedDict
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

WORKLOADS = (
    ("kitti_b1", dict(version="it8-seq4-inter-out", B=1, N=2, H=192, W=640, gt=(375, 1242), frac=0.05,
                      min_depth=0.5, max_depth=80.0, crop="garg")),
    ("kitti_b4", dict(version="it8-seq4-inter-out", B=4, N=2, H=192, W=640, gt=(375, 1242), frac=0.05,
                      min_depth=0.5, max_depth=80.0, crop="garg")),
    ("scannet_b1", dict(version="it12-h-out", B=1, N=4, H=240, W=320, gt=(480, 640), frac=0.9,
                        min_depth=0.2, max_depth=10.0, crop="")),
)


def two_pass(model, batch, params):
    """ModelWrapper.evaluate_depth (model_wrapper.py:355-399) from the package's
    pieces without models/evaluate.py and csrc/evalpost.hip."""
    from dro_sfm_amd.utils.depth import compute_depth_metrics, compute_pose_metrics, inv2depth
    model.eval()
    with torch.no_grad():
        out = model(batch)
        inv = out["inv_depths"][0]
        depth = inv2depth(inv)
        B, C, H, W = inv.shape
        K = batch["intrinsics"].clone()
        K[:, 0, 0] = -K[:, 0, 0]
        K[:, 0, 2] = W - K[:, 0, 2]
        flipped = model(dict(batch, rgb=torch.flip(batch["rgb"], [3]),
                             rgb_context=[torch.flip(r, [3]) for r in batch["rgb_context"]],
                             intrinsics=K))["inv_depths"][0]
        hat = torch.flip(flipped, [3])
        fused = 0.5 * (inv + hat)
        xs = torch.linspace(0.0, 1.0, W, device=inv.device, dtype=inv.dtype).repeat(B, C, H, 1)
        mask = 1.0 - torch.clamp(20.0 * (xs - 0.05), 0.0, 1.0)
        mask_hat = torch.flip(mask, [3])
        inv_pp = mask_hat * inv + mask * hat + (1.0 - mask - mask_hat) * fused
        depth_pp = inv2depth(inv_pp)
        pose_errs = compute_pose_metrics(params, gt=batch["pose_context"], pred=out["poses"]).to(inv.device)
        metrics = OrderedDict()
        for mode in ("", "_pp", "_gt", "_pp_gt"):
            m = compute_depth_metrics(params, gt=batch["depth"], pred=depth_pp if "pp" in mode else depth,
                                      use_gt_scale="gt" in mode)
            metrics["depth" + mode] = torch.cat([m, pose_errs])
    return {"metrics": metrics, "inv_depth": inv_pp}


def make(wl, dev):
    from common import det_init, smooth_images
    from dro_sfm_amd.models.SfmModelMF import SfmModelMF
    from dro_sfm_amd.networks.depth_pose.DepthPoseNet import DepthPoseNet
    B, N, H, W = wl["B"], wl["N"], wl["H"], wl["W"]
    net = det_init(DepthPoseNet(version=wl["version"], min_depth=wl["min_depth"], max_depth=wl["max_depth"]))
    model = SfmModelMF(flip_lr_prob=0.0, min_depth=wl["min_depth"], max_depth=wl["max_depth"])
    model.add_depth_net(net)
    model = model.to(dev)
    g = torch.Generator().manual_seed(11)
    GH, GW = wl["gt"]
    gt = torch.zeros(B, 1, GH, GW)
    keep = torch.rand(B, 1, GH, GW, generator=g) < wl["frac"]
    lo, hi = wl["min_depth"], wl["max_depth"]
    gt[keep] = (lo + 0.1 + (hi - lo - 0.2) * torch.rand(B, 1, GH, GW, generator=g))[keep]
    K = torch.tensor([[0.58 * W, 0.0, 0.49 * W], [0.0, 1.92 * H, 0.46 * H], [0.0, 0.0, 1.0]]).repeat(B, 1, 1)
    poses = []
    for _ in range(N):
        T = torch.eye(4).repeat(B, 1, 1)
        T[:, :3, 3] = 0.1 * torch.randn(B, 3, generator=g)
        poses.append(T.to(dev))
    batch = {"rgb": smooth_images(B, H, W, 31).to(dev),
             "rgb_context": [smooth_images(B, H, W, 32 + j).to(dev) for j in range(N)],
             "intrinsics": K.to(dev), "depth": gt.to(dev), "pose_context": poses}
    params = SimpleNamespace(crop=wl["crop"], min_depth=lo, max_depth=hi)
    return model, batch, params


def chunk_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seconds", type=float, default=2.5, help="timed seconds per variant and workload (>= 2)")
    ap.add_argument("--repeats", type=int, default=5, help="alternating chunks per variant")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workloads", nargs="*", default=[n for n, _ in WORKLOADS])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_throughput: needs a ROCm device (timings on a CPU say nothing)")
    from dro_sfm_amd.models.evaluate import evaluate_depth
    dev = torch.device("cuda", 0)
    for name, wl in WORKLOADS:
        if name not in args.workloads:
            continue
        model, batch, params = make(wl, dev)
        variants = OrderedDict(evaluate_depth=lambda: evaluate_depth(model, batch, params),
                               two_pass=lambda: two_pass(model, batch, params))
        outs = {}
        for vname, fn in variants.items():
            for _ in range(args.warmup):
                outs[vname] = fn()
        torch.cuda.synchronize()
        a, b = outs["evaluate_depth"], outs["two_pass"]
        err = float((a["inv_depth"] - b["inv_depth"]).abs().max() / b["inv_depth"].abs().max())
        merr = max(float(((a["metrics"][k] - b["metrics"][k]).abs() / b["metrics"][k].abs().clamp_min(1e-6)).max())
                   for k in b["metrics"])
        iters = {v: max(2, int(args.seconds * 1e3 / args.repeats / chunk_ms(fn, 3))) for v, fn in variants.items()}
        times = {v: [] for v in variants}
        for _ in range(args.repeats):
            for vname, fn in variants.items():
                times[vname].append(chunk_ms(fn, iters[vname]))
        line = [f"{name} {wl['version']} B={wl['B']} N={wl['N']} {wl['H']}x{wl['W']}:"]
        for vname, ts in times.items():
            med = statistics.median(ts)
            line.append(f"{vname} {wl['B'] * 1e3 / med:.1f} img/s ({med:.2f} ms/call, spread "
                        f"{100 * (max(ts) - min(ts)) / med:.1f}% over {len(ts)} x {iters[vname]} calls)")
        line.append(f"outputs agree: inv_pp {err:.1e}, metrics {merr:.1e}")
        print("  ".join(line), flush=True)


if __name__ == "__main__":
    main()
