"""Rendering throughput: hip.render_points against the same computation in
torch ops, and the splat kernel with and without its early skip.

Times, in one process and alternating, on a seeded scene (no dataset):
  (a)  hip.render_points (csrc/render.hip: fill, splat, resolve), every pair
       sending its atomic;
  (a') the same with the splat reading the pixel's key first and skipping an
       atomic that cannot win (DRO_RENDER_EARLY_SKIP=1);
  (b)  the same computation in torch ops on the same GPU: the projection of
       every (view, point) pair, int64 keys, scatter_reduce amin into the
       padded z-buffer, the window minimum as s*s shifted torch.minimum, the
       colour gather.
Workload: KITTI size (192x640), the cumulative cloud of 30 frames (depth maps
with 30 % holes, lifted by hip.backproject_points along a forward-moving
camera), point size 5, V = 30 pictures, frame i drawing the points of the
frames <= i; once from the chase camera and once from each frame's own.  Each
variant is warmed up, then timed with device events in `--repeats` chunks of
about `--seconds / --repeats` each, one chunk per variant in turn; the spread
is (max - min) / median over the chunks.  Times are whole calls issued back to
back (allocation of the outputs and launch latency included), not kernel times.

    python tools/render_throughput.py > profiles/render_throughput.txt
"""
import argparse
import os
import statistics
import sys
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

EMPTY = torch.iinfo(torch.int64).max


def render_torch(xyz, rgb, K, world2cam, limit, size, s, near=1e-6):
    """dro_render_points in torch ops.  Pairs that draw nothing go to a spare
    cell behind the z-buffer, so nothing synchronises."""
    H, W = size
    V, n = K.shape[0], xyz.shape[0]
    m = s // 2
    Hp, Wp = H + 2 * m, W + 2 * m
    cam = torch.einsum("vij,nj->vni", world2cam[:, :3, :3], xyz) + world2cam[:, None, :3, 3]
    x, y, z = cam.unbind(-1)
    ur = torch.round(K[:, 0, 0, None] * x / z + K[:, 0, 2, None])
    vr = torch.round(K[:, 1, 1, None] * y / z + K[:, 1, 2, None])
    idx = torch.arange(n, device=xyz.device)
    ok = (torch.isfinite(cam).all(-1) & (z >= near) & (idx[None, :] < limit[:, None])
          & (ur >= -m) & (ur <= W - 1 + m) & (vr >= -m) & (vr <= H - 1 + m))
    cell = ((vr.clamp(-m, H - 1 + m).long() + m) * Wp + (ur.clamp(-m, W - 1 + m).long() + m)
            + torch.arange(V, device=xyz.device)[:, None] * (Hp * Wp))
    cell = torch.where(ok, cell, torch.full_like(cell, V * Hp * Wp))
    key = (z.contiguous().view(torch.int32).long() << 32) | idx[None, :]
    buf = torch.full((V * Hp * Wp + 1,), EMPTY, dtype=torch.int64, device=xyz.device)
    buf.scatter_reduce_(0, cell.reshape(-1), key.reshape(-1), "amin")
    buf = buf[:-1].view(V, Hp, Wp)
    best = torch.full((V, H, W), EMPTY, dtype=torch.int64, device=xyz.device)
    for dy in range(-((s - 1) // 2), s // 2 + 1):
        for dx in range(-((s - 1) // 2), s // 2 + 1):
            best = torch.minimum(best, buf[:, m + dy:m + dy + H, m + dx:m + dx + W])
    empty = best == EMPTY
    bytes_ = torch.round(rgb * 255.0).clamp(0, 255).to(torch.uint8)
    image = bytes_[torch.where(empty, torch.zeros_like(best), best & 0xFFFFFFFF)]
    image[empty] = 0
    return image


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


def make_cloud(T, H, W, dev):
    """T frames along a camera moving 1 m per frame with a slow turn; depths
    5..30 m with 30 % holes.  Returns points, colours, per-frame counts
    (device), the poses (host) and K [3,3]."""
    import dro_sfm_amd.hip as hip
    from common import kitti_K, smooth_images
    from reconstruct_oracle import _rot
    g = torch.Generator().manual_seed(5)
    depth = 5.0 + 25.0 * smooth_images(T, H, W, 31, detail=0.03)[:, 0]
    depth[torch.rand(T, H, W, generator=g) < 0.3] = 0
    rgb = smooth_images(T, H, W, 32)
    K = kitti_K(1)[0]
    poses = np.tile(np.eye(4), (T, 1, 1))
    for i in range(T):
        poses[i, :3, :3] = _rot((0.0, 0.01 * i, 0.0))
        poses[i, :3, 3] = (0.05 * i, 0.0, 1.0 * i)
    depth, rgb = depth.to(dev), rgb.to(dev)
    xyz, col, n = hip.backproject_points(depth, rgb, K.to(dev).expand(T, 3, 3).contiguous(),
                                         torch.from_numpy(poses).float().to(dev))
    n = int(n)
    return xyz[:n].contiguous(), col[:n].contiguous(), (depth > 0).sum((1, 2)), poses, K.to(dev)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seconds", type=float, default=2.5, help="timed seconds per variant and workload (>= 2)")
    ap.add_argument("--repeats", type=int, default=5, help="alternating chunks per variant")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--point_size", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("render_throughput: needs a ROCm device (timings on a CPU say nothing)")
    import dro_sfm_amd.hip as hip
    from dro_sfm_amd.models import reconstruct as M
    dev = torch.device("cuda", 0)
    T, H, W, s = args.frames, 192, 640, args.point_size
    xyz, col, counts, poses, K = make_cloud(T, H, W, dev)
    limit = torch.cumsum(counts, 0).to(torch.int32)
    pairs = int(limit.sum())
    cameras = OrderedDict(
        chase=(torch.from_numpy(M.chase_camera(poses, kitti=True)).float().to(dev),
               torch.from_numpy(M.render_intrinsics(H, W)).float().to(dev).expand(T, 3, 3).contiguous()),
        first_person=(torch.from_numpy(M.rigid_inverse(poses)).float().to(dev), K.expand(T, 3, 3).contiguous()))
    for name, (world2cam, Kv) in cameras.items():
        def native(skip):
            os.environ["DRO_RENDER_EARLY_SKIP"] = skip
            return hip.render_points(xyz, col, Kv, world2cam, (H, W), limit=limit, point_size=s, check_skew=False)

        variants = OrderedDict(render_points=lambda: native("0"), early_skip=lambda: native("1"),
                               torch_ops=lambda: render_torch(xyz, col, Kv, world2cam, limit, (H, W), s))
        a, a0, b = (fn() for fn in variants.values())
        _, _, _, cell, _ = hip.render_points(xyz, col, Kv, world2cam, (H, W), limit=limit, point_size=s,
                                             check_skew=False, record=True)
        keys = int((cell != hip.RENDER_REJECTED).sum())
        del cell
        # two fp32 evaluations of the projection may part at a rounding: those pixels are counted
        agree = (f"render_points and early_skip differ at {int((a != a0).any(-1).sum())}, render_points and "
                 f"torch_ops at {int((a != b).any(-1).sum())} of {a.shape[0] * H * W} pixels; "
                 f"{100 * float((a != 0).any(-1).float().mean()):.1f} % of the pixels drawn")
        times, iters = alternate(variants, args)
        med = {}
        txt = []
        for v in variants:
            med[v], t = describe(times[v], iters[v])
            txt.append(f"{v} {t}")
        print(f"render {name} V={T} {H}x{W} s={s}, {xyz.shape[0]} points, {pairs} (view, point) pairs, {keys} keys "
              f"written:  {'  '.join(txt)}  torch_ops / render_points {med['torch_ops'] / med['render_points']:.1f}x  "
              f"early_skip / render_points {med['early_skip'] / med['render_points']:.2f}x  "
              f"{pairs / med['render_points'] / 1e6:.2f} G pairs/s, {keys / med['render_points'] / 1e6:.2f} G keys/s "
              f"(whole call)  {agree}", flush=True)
    os.environ.pop("DRO_RENDER_EARLY_SKIP", None)


if __name__ == "__main__":
    main()
