"""From a trained model to depth maps a user can look at or load elsewhere:
what the reference's scripts/infer.py and the per-frame half of
scripts/infer_video.py (:139-226) produce for a sequence.

  per-frame inverse depth and relative poses (the forward loop of
  models/reconstruct.py) -> depth -> the RGB-over-colourised-inverse-depth
  panel of infer.py:160-181 -> files: panels as PNG, depths as .npz or as the
  KITTI 16-bit PNG of write_depth.

The percentile that normalises each map, the colour lookup with the panel and
the PNG scanlines are HIP launches for the whole sequence (hip.percentile,
hip.colorize, hip.depth_png16_rows; csrc/viz.hip): nothing is copied to the
host unless files are asked for, and then once per kind of file.  Out of
scope: the fp16 path, the video montage, colormaps other than plasma.
"""
import os

import numpy as np
import torch

from .. import hip
from ..datasets.png import encode_png
from ..utils.depth import inv2depth, viz_panel
from .reconstruct import predict_interior_frames, relative_poses_to_host


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)


def save_panels(out_dir, panels, first=1):
    """panels uint8 [n,H2,W,3] (RGB) -> out_dir/%06d.png, numbered from
    `first` (the index of the frame a panel shows).  One copy off the device."""
    host = panels.cpu().numpy()
    n, H2, W, _ = host.shape
    rows = np.zeros((n, H2, 1 + 3 * W), dtype=np.uint8)          # filter type None
    rows[:, :, 1:] = host.reshape(n, H2, 3 * W)
    for i in range(n):
        _write(os.path.join(out_dir, "%06d.png" % (first + i)), encode_png(rows[i], W, H2, 2))


def save_depths(out_dir, depths, K, save, first=1):
    """depths [n,1,H,W] -> out_dir/%06d.npz ('depth', 'intrinsics': what
    write_depth writes) or .png (16-bit, depth * 256), numbered from `first`.
    One copy off the device for all frames."""
    n, _, H, W = depths.shape
    if save == "npz":
        host, Kh = depths[:, 0].cpu().numpy(), K.reshape(3, 3).cpu().numpy()
        for i in range(n):
            np.savez_compressed(os.path.join(out_dir, "%06d.npz" % (first + i)), depth=host[i], intrinsics=Kh)
    else:
        rows = hip.depth_png16_rows(depths[:, 0]).cpu().numpy()
        for i in range(n):
            _write(os.path.join(out_dir, "%06d.png" % (first + i)), encode_png(rows[i], W, H, 16))


def infer_sequence(model, frames, K, out_dir=None, save=None, viz=True, frames_per_forward=4):
    """frames [T,3,H,W] float32 on the GPU (T >= 3), K [3,3] or [1,3,3] the
    intrinsics of those frames.  Every interior frame t = 1..T-2 is predicted
    with the references (t-1, t+1), exactly as reconstruct_sequence does,
    frames_per_forward frames per forward.

    Returns a dict:
      'inv_depths' [T-2,1,H,W]  the model's full-resolution inverse depths
      'depths'     [T-2,1,H,W]  inv2depth of them
      'poses'      [T-2,2,4,4]  float64 (host): per frame the predicted
                                transforms to the previous and to the next frame
      'panels'     [T-2,2H,W,3] uint8 (viz=True): the frame above its plasma
                                inverse depth, each map normalised by its own
                                95th percentile (utils.depth.viz_panel)
    With out_dir, frame t is written as out_dir/%06d.png % t (the panel, with
    viz=True) and, with save 'npz' or 'png', as out_dir/depth/%06d.<save>
    (utils.depth.write_depth's formats; load_depth reads them back).
    Runs under no_grad in eval mode and restores the model's training flags."""
    if frames.dim() != 4 or frames.shape[1] != 3 or frames.shape[0] < 3:
        raise RuntimeError(f"infer_sequence: frames [T>=3,3,H,W] expected, got {tuple(frames.shape)}")
    if save not in (None, "npz", "png"):
        raise ValueError(f"infer_sequence: save must be None, 'npz' or 'png', got {save!r}")
    if save is not None and out_dir is None:
        raise ValueError("infer_sequence: save needs an out_dir")
    hip.ops.require_device(frames, K, what="infer_sequence")
    T = frames.shape[0]
    K1 = K.reshape(1, 3, 3)
    modes = [(m, m.training) for m in model.modules()]
    model.eval()
    try:
        with torch.no_grad():
            inv, poses = predict_interior_frames(model, frames, K1, frames_per_forward, "infer_sequence")
            out = {"inv_depths": inv, "depths": inv2depth(inv), "poses": torch.from_numpy(relative_poses_to_host(poses))}
            if viz:
                out["panels"] = viz_panel(frames[1:T - 1], inv)
    finally:
        for m, training in modes:
            m.training = training
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        if viz:
            save_panels(out_dir, out["panels"])
        if save is not None:
            os.makedirs(os.path.join(out_dir, "depth"), exist_ok=True)
            save_depths(os.path.join(out_dir, "depth"), out["depths"], K1, save)
    return out
