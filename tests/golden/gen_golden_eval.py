"""Golden vectors of the evaluation step (test infrastructure; runs ONLY in the
build container, like gen_golden.py, whose shims and helpers it uses).

  post_process.npz        the reference's post_process_inv_depth and inv2depth
                          (dro_sfm/utils/depth.py:102-121, :202-256) at widths
                          2, 3, 20, 37, 96 for the three fuse methods.
  evaluate_depth_it8.npz  the reference's evaluation sequence
                          (ModelWrapper.evaluate_depth, model_wrapper.py:355-399)
                          on SfmModelMF + DepthPoseNet it8-seq4-inter-out.

dro_sfm.models.model_wrapper does not import under the shims (it needs
torchvision.transforms.functional, horovod and IPython), so evaluate_depth is
RESTATED here line by line from the reference's own functions: the model's
forward, flip_lr, flip_lr_intr, post_process_inv_depth, inv2depth,
compute_depth_metrics and compute_pose_metrics.  The pose errors are computed
per sample on B=1 slices (the formula's domain) and averaged.

Usage:  python tests/golden/gen_golden_eval.py
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from common import _gen, det_init, kitti_K, smooth_images  # noqa: E402
from gen_golden import REF, install_shims, save  # noqa: E402

WIDTHS = (2, 3, 20, 37, 96)
METHODS = ("mean", "max", "min")
MODES = ("", "_pp", "_gt", "_pp_gt")
THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)
MARGIN = 1e-5


def fill_bn_buffers(module):
    """Non-trivial BatchNorm running statistics, keyed by name like det_init's
    parameters: with det_init's 0 / 1 an evaluation that ignored the running
    statistics would go unnoticed.  The tests fill the product net the same way."""
    with torch.no_grad():
        for name, t in module.state_dict().items():
            if name.endswith("running_mean"):
                t.copy_(0.05 * torch.randn(t.shape, generator=_gen(name, 1)))
            elif name.endswith("running_var"):
                t.copy_(1.0 + 0.2 * torch.rand(t.shape, generator=_gen(name, 1)))
    return module


def gen_post_process():
    from dro_sfm.utils.depth import inv2depth, post_process_inv_depth
    g = torch.Generator().manual_seed(91)
    out = {}
    B, H = 2, 3
    for W in WIDTHS:
        inv = 0.01 + 0.49 * torch.rand(B, 1, H, W, generator=g)
        flipped = 0.01 + 0.49 * torch.rand(B, 1, H, W, generator=g)
        # the <= 0 and clamp branches of inv2depth, at both borders and on both inputs
        inv[0, 0, 0, 0], inv[1, 0, 1, W - 1], inv[1, 0, 2, 0] = 0.0, -0.1, 1e-7
        flipped[0, 0, 1, 0], flipped[1, 0, 0, W - 1], flipped[0, 0, 2, W - 1] = 0.0, -0.1, 1e-7
        out[f"inv_{W}"], out[f"flipped_{W}"] = inv, flipped
        out[f"depth_{W}"] = inv2depth(inv)
        for m in METHODS:
            pp = post_process_inv_depth(inv, flipped, method=m)
            out[f"pp_{m}_{W}"] = pp
            out[f"depth_pp_{m}_{W}"] = inv2depth(pp)
    save("post_process", **out)


def threshold_margin(cfg, gt, pred, use_gt_scale):
    """The smallest relative distance of any valid pixel's max(gt/pred, pred/gt)
    from an a1/a2/a3 threshold, following compute_depth_metrics
    (utils/depth.py:285-321) to the line that forms `thresh`."""
    pred = pred.clamp(min=1e-6)
    H, W = gt.shape[-2:]
    crop = torch.ones(H, W, dtype=torch.bool)
    if cfg.crop == "garg":
        crop[:] = False
        crop[int(0.40810811 * H):int(0.99189189 * H), int(0.03594771 * W):int(0.96405229 * W)] = True
    worst, nvalid = float("inf"), []
    for pred_i, gt_i in zip(pred, gt):
        gt_i, pred_i = gt_i.squeeze(), pred_i.squeeze()
        valid = (gt_i > cfg.min_depth) & (gt_i < cfg.max_depth) & crop
        gt_i, pred_i = gt_i[valid], pred_i[valid]
        nvalid.append(int(valid.sum()))
        if use_gt_scale:
            pred_i = torch.clamp(pred_i * torch.median(gt_i / pred_i), cfg.min_depth, cfg.max_depth)
        pred_i = pred_i.clamp(cfg.min_depth, cfg.max_depth)
        thresh = torch.max(gt_i / pred_i, pred_i / gt_i).double()
        for t in THRESHOLDS:
            worst = min(worst, float((thresh / t - 1.0).abs().min()))
    return worst, nvalid


def gen_evaluate():
    from dro_sfm.geometry.pose import Pose
    from dro_sfm.models.SfmModelMF import SfmModelMF
    from dro_sfm.networks.depth_pose.DepthPoseNet import DepthPoseNet
    from dro_sfm.utils.depth import (compute_depth_metrics, compute_pose_metrics, inv2depth,
                                     post_process_inv_depth)
    from dro_sfm.utils.image import flip_lr, flip_lr_intr
    B, N, H, W, mind, maxd = 2, 2, 64, 96, 0.5, 80.0
    cfg = SimpleNamespace(crop="garg", min_depth=mind, max_depth=maxd)
    net = fill_bn_buffers(det_init(DepthPoseNet(version="it8-seq4-inter-out", min_depth=mind, max_depth=maxd)))
    model = SfmModelMF(flip_lr_prob=0.0, rotation_mode="euler", min_depth=mind, max_depth=maxd)
    model.add_depth_net(net)
    model.eval()
    img = smooth_images(B, H, W, 31)
    refs = [smooth_images(B, H, W, 32 + j) for j in range(N)]
    K = kitti_K(B, W=W, H=H)
    gp = torch.Generator().manual_seed(6)
    gvec = torch.stack([torch.cat([0.1 * torch.randn(B, 3, generator=gp), 0.02 * torch.randn(B, 3, generator=gp)], 1)
                        for _ in range(N)], 1)
    gpose = [Pose.from_vec(gvec[:, j], "euler").mat for j in range(N)]

    # model_wrapper.py:357-372
    batch = {"rgb": img, "rgb_context": list(refs), "intrinsics": K.clone(), "pose_context": gpose}
    with torch.no_grad():
        output = model(batch)
        inv_depths, poses = output["inv_depths"], output["poses"]
        depth = inv2depth(inv_depths[0])
        batch["rgb"] = flip_lr(batch["rgb"])
        batch["rgb_context"] = [flip_lr(i) for i in batch["rgb_context"]]
        batch["intrinsics"] = flip_lr_intr(batch["intrinsics"], width=depth.shape[3])
        inv_depths_flipped = model(batch)["inv_depths"]
        inv_depth_pp = post_process_inv_depth(inv_depths[0], inv_depths_flipped[0], method="mean")
        depth_pp = inv2depth(inv_depth_pp)
    diff = float((flip_lr(inv_depths_flipped[0]) - inv_depths[0]).abs().max() / inv_depths[0].abs().max())
    print(f"  flipped pass differs from the plain one by up to {diff:.3f} of max|inv|")

    # model_wrapper.py:375-378, per sample
    pose_errs = torch.stack([compute_pose_metrics(cfg, gt=[p[b:b + 1] for p in gpose],
                                                  pred=[Pose(p.mat[b:b + 1]) for p in poses])
                             for b in range(B)]).mean(0)

    # ground truth from the prediction; the first seed whose a1/a2/a3 counts are
    # safe from rounding in every mode
    for seed in range(32):
        g = torch.Generator().manual_seed(seed)
        gt = (depth * (0.6 + 1.2 * torch.rand(depth.shape, generator=g))).clamp(mind + 0.1, maxd - 1.0)
        gt[torch.rand(depth.shape, generator=g) < 0.3] = 0.0
        margins = {m: threshold_margin(cfg, gt, depth_pp if "pp" in m else depth, "gt" in m) for m in MODES}
        worst = min(v[0] for v in margins.values())
        print(f"  gt seed {seed}: smallest threshold margin {worst:.2e}, valid pixels {margins[''][1]}")
        if worst > MARGIN:
            break
    else:
        raise SystemExit("no ground-truth seed below 32 keeps every pixel clear of the a1/a2/a3 thresholds")

    # model_wrapper.py:381-394
    metrics = {}
    for mode in MODES:
        m = compute_depth_metrics(cfg, gt=gt, pred=depth_pp if "pp" in mode else depth, use_gt_scale="gt" in mode)
        metrics["metrics" + mode] = torch.cat([m, pose_errs])
        print(f"  depth{mode}: " + " ".join(f"{float(v):.4f}" for v in metrics["metrics" + mode]))
    save("evaluate_depth_it8", image=img, refs=torch.stack(refs), K=K, gt_depth=gt, gt_poses=torch.stack(gpose, 1),
         inv=inv_depths[0], inv_flipped=inv_depths_flipped[0], inv_pp=inv_depth_pp,
         poses=torch.stack([p.mat for p in poses], 1), **metrics,
         min_depth=np.float32(mind), max_depth=np.float32(maxd), crop=np.int32(1), seed=np.int32(seed))


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("reference not present: golden fixtures can only be regenerated in the build container")
    torch.set_num_threads(8)
    install_shims()
    gen_post_process()
    gen_evaluate()
