"""Reconstruction throughput: the fusion kernel against the same algorithm in
torch ops, and reconstruct_sequence in frames per second.

Times, in one process and alternating, on seeded inputs (no dataset):
  (a) hip.fuse_depths -- one launch for all source views (csrc/reconstruct.hip);
  (b) the steps of the reference's reproject_with_depth_batch,
      check_geometric_consistency_batch and gemo_filter_fusion
      (scripts/infer_video.py:254-369) written in torch ops on the same GPU,
      per source view, with its two inverse calls per projection and its
      nearest grid_sample.
Workloads: one KITTI-size frame (192x640) and one ScanNet-size frame (240x320),
S=4 source views, the scene of tests/reconstruct_oracle.py.  Each variant is
warmed up, then timed with device events in `--repeats` chunks of about
`--seconds / --repeats` each, a chunk of (a) then a chunk of (b); the spread is
(max - min) / median over the chunks.  The kernel's bytes per second are its
compulsory traffic (8 + 4 S + 1) B H W over the median time of a call -- calls
issued back to back, so launch latency is in it.

Then models.reconstruct.reconstruct_sequence on T=32 KITTI-size frames
(it8-seq4-inter-out, deterministic weights), with and without the fusion.

    python tools/reconstruct_throughput.py > profiles/reconstruct_throughput.txt
"""
import argparse
import os
import statistics
import sys
from collections import OrderedDict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

WORKLOADS = (("kitti", dict(B=1, S=4, H=192, W=640, seed=9)), ("scannet", dict(B=1, S=4, H=240, W=320, seed=10)))


def fusion_torch(depth_ref, depth_src, K, extr_ref, extr_src, thres_p_dist=1.0, thres_d_diff=1e-3, thres_view=1):
    """The reference's fusion in torch ops, view by view."""
    B, H, W = depth_ref.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=depth_ref.device),
                            torch.arange(W, dtype=torch.float32, device=depth_ref.device), indexing="ij")
    xs, ys = xs.expand(B, H, W), ys.expand(B, H, W)
    ones = torch.ones(B, 1, H * W, device=depth_ref.device)
    pix = torch.cat([xs.reshape(B, 1, -1), ys.reshape(B, 1, -1), ones], 1)
    count = torch.zeros_like(depth_ref)
    total = torch.zeros_like(depth_ref)
    for depth_s, extr_s in zip(depth_src, extr_src):
        cam = torch.inverse(K) @ (pix * depth_ref.view(B, 1, -1))
        there = ((extr_s @ torch.inverse(extr_ref)) @ torch.cat([cam, ones], 1))[:, :3]
        proj = K @ there
        uv = proj[:, :2] / proj[:, 2:3].clamp(min=1e-10)
        grid = torch.stack([uv[:, 0].view(B, H, W) / ((W - 1) / 2) - 1, uv[:, 1].view(B, H, W) / ((H - 1) / 2) - 1], 3)
        sampled = torch.nn.functional.grid_sample(depth_s.unsqueeze(1), grid, mode="nearest", padding_mode="zeros",
                                                  align_corners=True).squeeze(1)
        cam_s = torch.inverse(K) @ (torch.cat([uv, ones], 1) * sampled.view(B, 1, -1))
        back = ((extr_ref @ torch.inverse(extr_s)) @ torch.cat([cam_s, ones], 1))[:, :3]
        d_re = back[:, 2].view(B, H, W) * (sampled > 0)
        proj_b = K @ back
        uv_b = proj_b[:, :2] / proj_b[:, 2:3].clamp(min=1e-10)
        dist = torch.sqrt((uv_b[:, 0].view(B, H, W) - xs) ** 2 + (uv_b[:, 1].view(B, H, W) - ys) ** 2)
        rel = (d_re - depth_ref).abs() / depth_ref.clamp(min=1e-10)
        mask = (dist < thres_p_dist) & (rel < thres_d_diff)
        d_re[~mask] = 0
        count += mask.float()
        total += d_re
    fused = (total + depth_ref) / (count + 1) * ((count - thres_view) >= 0)
    return fused, count.to(torch.uint8)


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


def describe(ts, iters):
    med = statistics.median(ts)
    return med, f"{med:.3f} ms/call (spread {100 * (max(ts) - min(ts)) / med:.1f}% over {len(ts)} x {iters} calls)"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seconds", type=float, default=2.5, help="timed seconds per variant and workload (>= 2)")
    ap.add_argument("--repeats", type=int, default=5, help="alternating chunks per variant")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=32, help="T of the reconstruct_sequence measurement (0: skip)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("reconstruct_throughput: needs a ROCm device (timings on a CPU say nothing)")
    import dro_sfm_amd.hip as hip
    from reconstruct_oracle import make_scene
    dev = torch.device("cuda", 0)
    for name, wl in WORKLOADS:
        scene = make_scene(wl["B"], wl["S"], wl["H"], wl["W"], wl["seed"])
        t = [torch.from_numpy(scene[k]).to(dev) for k in ("depth_ref", "depth_src", "K", "extr_ref", "extr_src")]
        variants = OrderedDict(fuse_depths=lambda: hip.fuse_depths(*t, check_skew=False),
                               torch_ops=lambda: fusion_torch(*t))
        (fa, ca), (fb, cb) = variants["fuse_depths"](), variants["torch_ops"]()
        # two fp32 evaluations may part at a rounding or a threshold: those pixels are counted, not compared
        same = ca == cb
        agree = (f"outputs: {int((~same).sum())} of {ca.numel()} counts differ, fused within "
                 f"{float(((fa - fb).abs() * same).max() / fb.abs().max()):.1e} of max where they agree")
        times, iters = alternate(variants, args)
        med_a, txt_a = describe(times["fuse_depths"], iters["fuse_depths"])
        med_b, txt_b = describe(times["torch_ops"], iters["torch_ops"])
        nbytes = (8 + 4 * wl["S"] + 1) * wl["B"] * wl["H"] * wl["W"]
        print(f"fusion {name} B={wl['B']} S={wl['S']} {wl['H']}x{wl['W']}:  fuse_depths {txt_a}  torch_ops {txt_b}  "
              f"ratio {med_b / med_a:.1f}x  compulsory {nbytes / 1e6:.2f} MB -> {nbytes / med_a / 1e6:.1f} GB/s  {agree}",
              flush=True)
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
        params = default_params(kitti=True)
        variants = OrderedDict(fused=lambda: reconstruct_sequence(model, frames, K, params),
                               unfused=lambda: reconstruct_sequence(model, frames, K, params, fuse=False))
        npts = {v: fn()["points"].shape[0] for v, fn in variants.items()}
        times, iters = alternate(variants, args)
        line = [f"reconstruct_sequence it8-seq4-inter-out T={T} {H}x{W} ({T - 2} frames reconstructed, 4 per forward):"]
        for v in variants:
            med, txt = describe(times[v], iters[v])
            line.append(f"{v} {(T - 2) * 1e3 / med:.1f} frames/s, {txt}, {npts[v]} points")
        print("  ".join(line), flush=True)


if __name__ == "__main__":
    main()
