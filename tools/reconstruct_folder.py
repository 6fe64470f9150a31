"""Reconstruction of a folder of frames from a reference checkpoint: the command
line of the reference's scripts/infer_video.py in its point-cloud mode.

    python tools/reconstruct_folder.py --checkpoint model.ckpt --input frames/ --output out/ \
        [--ply] [--renders chase|first_person] [--kitti] [--image_shape 192 640] [--intrinsics FX FY CX CY]
        [--session]

The frames (sorted by name, one size) are decoded with Pillow, resized on the
GPU and run through models.reconstruct.reconstruct_sequence.  out/pose.obj is
the camera path (the reference's *_pose.obj), out/cloud.ply the coloured point
cloud with --ply, out/renders/%06d.png one picture of the growing cloud per
frame with --renders: `chase` is the reference viewer's cinematic camera,
`first_person` each frame's own camera.  --kitti takes KITTI's intrinsics, depth
limit and chase distance; without it the intrinsics are made up as the
reference does (or given).  The first and the last frame only serve as
references.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--checkpoint", required=True, help="a reference .ckpt file")
    ap.add_argument("--input", required=True, help="folder of .png / .jpg frames")
    ap.add_argument("--output", required=True, help="output folder")
    ap.add_argument("--ply", action="store_true", help="write out/cloud.ply")
    ap.add_argument("--renders", choices=["chase", "first_person"], default=None, help="write out/renders/%%06d.png")
    ap.add_argument("--kitti", action="store_true", help="KITTI intrinsics, depth limit and chase camera")
    ap.add_argument("--image_shape", type=int, nargs=2, default=None, help="network input (H W); default: the checkpoint's")
    ap.add_argument("--intrinsics", type=float, nargs=4, default=None, metavar=("FX", "FY", "CX", "CY"),
                    help="the raw frames' camera")
    ap.add_argument("--render_size", type=int, nargs=2, default=None, help="picture size (H W); default: the network input")
    ap.add_argument("--point_size", type=int, default=5)
    ap.add_argument("--no_fusion", action="store_true", help="the reference's output as it stands (fusion disabled)")
    ap.add_argument("--frames_per_forward", type=int, default=4)
    ap.add_argument("--session", action="store_true",
                    help="run through models.session.InferenceSession: the forward replayed from a hipGraph, with the "
                         "fused eval BatchNorm (default: eager)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("reconstruct_folder: needs a ROCm device (there is no CPU path)")
    from PIL import Image
    from infer_folder import get_intrinsics
    from dro_sfm_amd.datasets.gpu_transforms import resize_to_tensor
    from dro_sfm_amd.models import reconstruct as M
    from dro_sfm_amd.models.SfmModelMF import SfmModelMF
    from dro_sfm_amd.networks.depth_pose.DepthPoseNet import DepthPoseNet
    from dro_sfm_amd.utils.load import load_checkpoint, load_network
    ckpt = load_checkpoint(args.checkpoint)
    cfg = ckpt["config"]
    params = cfg["model"].get("params", {})
    lo, hi = float(params.get("min_depth", 0.1)), float(params.get("max_depth", 80.0))
    shape = args.image_shape or tuple(cfg["datasets"]["augmentation"]["image_shape"])
    model = SfmModelMF(flip_lr_prob=0.0, min_depth=lo, max_depth=hi)
    net = DepthPoseNet(version=cfg["model"]["depth_net"]["version"], min_depth=lo, max_depth=hi)
    model.add_depth_net(load_network(net, ckpt["state_dict"], ["depth_net", "disp_network"]))
    dev = torch.device("cuda", 0)
    model = model.to(dev)
    if args.session:
        from dro_sfm_amd.models.session import InferenceSession
        model = InferenceSession(model)
    names = sorted(f for f in os.listdir(args.input) if f.lower().endswith((".png", ".jpg", ".jpeg")))
    if len(names) < 3:
        sys.exit("reconstruct_folder: at least 3 frames are needed (each frame is predicted with its two neighbours)")
    raw = np.stack([np.asarray(Image.open(os.path.join(args.input, f)).convert("RGB")) for f in names])
    frames = resize_to_tensor(torch.from_numpy(raw).to(dev), shape)
    K = torch.from_numpy(get_intrinsics((raw.shape[2], raw.shape[1]), shape, "kitti" if args.kitti else "other",
                                        args.intrinsics)).to(dev)
    out = M.reconstruct_sequence(model, frames, K, M.default_params(kitti=args.kitti), fuse=not args.no_fusion,
                                 frames_per_forward=args.frames_per_forward, render=args.renders,
                                 render_size=args.render_size, point_size=args.point_size)
    os.makedirs(args.output, exist_ok=True)
    M.save_trajectory_obj(os.path.join(args.output, "pose.obj"), out["poses"])
    written = ["pose.obj"]
    if args.ply:
        M.save_ply(os.path.join(args.output, "cloud.ply"), out["points"], out["colors"])
        written.append("cloud.ply")
    if args.renders:
        M.save_renders(args.output, out["renders"])
        written.append(f"renders/ ({out['renders'].shape[0]} pictures)")
    print(f"{out['points'].shape[0]} points of {out['depths'].shape[0]} frames ({names[1]} .. {names[-2]}): "
          f"{', '.join(written)} written to {args.output}")


if __name__ == "__main__":
    main()
