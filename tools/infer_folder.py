"""Depth maps of a folder of frames from a reference checkpoint: the command
line of the reference's scripts/infer_video.py up to its per-frame outputs.

    python tools/infer_folder.py --checkpoint model.ckpt --input frames/ --output out/ \
        [--image_shape 192 640] [--data_type kitti | --intrinsics FX FY CX CY] [--save npz|png] [--session]

The frames (sorted by name, one size) are decoded with Pillow, resized on the
GPU (datasets.gpu_transforms.resize_to_tensor) and run through
models.infer.infer_sequence: out/%06d.png is the frame above its colourised
inverse depth, out/depth/ holds the depth files with --save.  The first and
the last frame only serve as references.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (fx, fy, cx, cy) of the raw frames: KITTI's rectified colour camera (its public calibration files)
INTRINSICS = {"kitti": (721.5377, 721.5377, 609.5593, 172.854)}


def get_intrinsics(raw_wh, image_shape, data_type, pinhole=None):
    """The rule of infer_video.py:100-137: a known camera's intrinsics (here
    `pinhole` = (fx, fy, cx, cy), or the data set's), else fx = fy = 1.2 w and
    the image centre; then scaled from the raw to the network size."""
    w, h = raw_wh
    fx, fy, cx, cy = pinhole or INTRINSICS.get(data_type, (1.2 * w, 1.2 * w, w / 2.0, h / 2.0))
    K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=np.float32)
    K[0] *= image_shape[1] / w
    K[1] *= image_shape[0] / h
    return K


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--checkpoint", required=True, help="a reference .ckpt file")
    ap.add_argument("--input", required=True, help="folder of .png / .jpg frames")
    ap.add_argument("--output", required=True, help="output folder")
    ap.add_argument("--image_shape", type=int, nargs=2, default=None, help="network input (H W); default: the checkpoint's")
    ap.add_argument("--data_type", default="kitti", help="kitti, or anything else for made-up intrinsics")
    ap.add_argument("--intrinsics", type=float, nargs=4, default=None, metavar=("FX", "FY", "CX", "CY"),
                    help="the raw frames' camera, instead of --data_type")
    ap.add_argument("--save", choices=["npz", "png"], default=None, help="also write depth files")
    ap.add_argument("--frames_per_forward", type=int, default=4)
    ap.add_argument("--session", action="store_true",
                    help="run through models.session.InferenceSession: the forward replayed from a hipGraph, with the "
                         "fused eval BatchNorm (default: eager)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("infer_folder: needs a ROCm device (there is no CPU path)")
    from PIL import Image
    from dro_sfm_amd.datasets.gpu_transforms import resize_to_tensor
    from dro_sfm_amd.models.infer import infer_sequence
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
        sys.exit("infer_folder: at least 3 frames are needed (each frame is predicted with its two neighbours)")
    raw = np.stack([np.asarray(Image.open(os.path.join(args.input, f)).convert("RGB")) for f in names])
    frames = resize_to_tensor(torch.from_numpy(raw).to(dev), shape)
    K = torch.from_numpy(get_intrinsics((raw.shape[2], raw.shape[1]), shape, args.data_type, args.intrinsics)).to(dev)
    out = infer_sequence(model, frames, K, out_dir=args.output, save=args.save,
                         frames_per_forward=args.frames_per_forward)
    print(f"{out['depths'].shape[0]} frames of {names[1]} .. {names[-2]} written to {args.output}")


if __name__ == "__main__":
    main()
