"""Visualisation throughput: viz_inv_depth plus the RGB-over-depth panel on the
GPU against the host path of the reference.

Times, in one process and alternating, on seeded inputs (no dataset, no model):
  (a) device       utils.depth.viz_panel -- hip.percentile (one block per
                   image, every radix pass in one launch) and hip.colorize with
                   the panel: two launches, nothing leaves the device;
  (b) device+copy  (a), then the uint8 panel copied to the host (what writing
                   files needs);
  (c) host         what scripts/infer.py:160-181 does per frame: the inverse
                   depth and the frame copied to the host, np.percentile,
                   division, clip, a 256-entry table lookup, concatenation,
                   conversion to bytes.
and the two launches of (a) on their own.  Workloads: KITTI 192x640 at B = 1
and B = 4.  Each variant is warmed up, then timed with device events in
`--repeats` chunks of about `--seconds / --repeats` each, one chunk of every
variant in turn; frames/s = B / median chunk time per call, the spread is
(max - min) / median over the chunks.

Only the one-block-per-image percentile was built; the multi-launch variant
(a histogram and a select launch per digit, as the median of csrc/metrics.hip)
was not, so there is no measurement of it.

    python tools/infer_viz_throughput.py > profiles/infer_viz_throughput.txt
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
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

H, W = 192, 640


def host_panel(rgb, inv, lut):
    """infer.py:160-181 with numpy: one frame at a time, as the reference."""
    out = []
    for b in range(inv.shape[0]):
        frame = rgb[b].permute(1, 2, 0).cpu().numpy() * 255
        x = inv[b, 0].cpu().numpy()
        x = x / (np.percentile(x, 95) + 1e-6)
        k = np.minimum((np.clip(x, 0.0, 1.0) * 256).astype(np.int64), 255)
        out.append(np.rint(np.concatenate([frame, lut[k] * 255], 0)).astype(np.uint8))
    return np.stack(out)


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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("infer_viz_throughput: needs a ROCm device (timings on a CPU say nothing)")
    import dro_sfm_amd.hip as hip
    from common import smooth_images
    from dro_sfm_amd.utils.colormaps import PLASMA
    from dro_sfm_amd.utils.depth import viz_panel
    dev = torch.device("cuda", 0)
    lut_host = np.array(PLASMA)
    lut = torch.tensor(PLASMA, dtype=torch.float32, device=dev)
    for B in (1, 4):
        rgb = smooth_images(B, H, W, 51).to(dev)
        # an inverse depth map: near at the bottom, smooth, with fine detail
        ramp = torch.linspace(0.0, 1.0, H, device=dev).view(1, 1, H, 1) ** 2
        inv = (0.02 + 0.5 * ramp + 0.1 * smooth_images(B, H, W, 52).to(dev)[:, :1]).contiguous()
        maps = inv[:, 0]
        norm = hip.percentile(maps.reshape(B, -1), 95)
        variants = OrderedDict(
            device=lambda: viz_panel(rgb, inv),
            device_copy=lambda: viz_panel(rgb, inv).cpu(),
            host=lambda: host_panel(rgb, inv, lut_host),
            percentile_only=lambda: hip.percentile(maps.reshape(B, -1), 95),
            colorize_only=lambda: hip.colorize(maps, norm, lut, rgb=rgb, color=False))
        a, c = variants["device"]().cpu().numpy(), variants["host"]()
        differ = int((a != c).any(-1).sum())
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        iters = {v: max(2, int(args.seconds * 1e3 / args.repeats / chunk_ms(fn, 3))) for v, fn in variants.items()}
        times = {v: [] for v in variants}
        for _ in range(args.repeats):
            for v, fn in variants.items():
                times[v].append(chunk_ms(fn, iters[v]))
        line = [f"viz_inv_depth + panel B={B} {H}x{W}:"]
        for v, ts in times.items():
            med = statistics.median(ts)
            line.append(f"{v} {B * 1e3 / med:.0f} frames/s ({med:.4f} ms/call, spread "
                        f"{100 * (max(ts) - min(ts)) / med:.1f}% over {len(ts)} x {iters[v]} calls)")
        line.append(f"device and host panels differ at {differ} of {a.shape[0] * a.shape[1] * a.shape[2]} pixels")
        print("  ".join(line), flush=True)


if __name__ == "__main__":
    main()
