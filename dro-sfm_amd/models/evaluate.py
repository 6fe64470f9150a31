"""Depth evaluation with test-time flip post-processing: the validation step
of the reference, ModelWrapper.evaluate_depth (dro_sfm/models/model_wrapper.py:355-399).

What changes versus the reference, never the math:
  * the unflipped and the flipped pass are ONE forward of batch 2B (eval-mode
    BatchNorm uses running statistics, so the samples of a batch are
    independent): half the launches of a launch-bound network;
  * flip back, fuse, border blend and both inv2depth calls are one HIP launch
    (hip.post_process_inv_depth, csrc/evalpost.hip);
  * the caller's batch is left as it was (the reference leaves
    batch['intrinsics'] and batch['rgb_context'] flipped);
  * the pose errors are the batch mean of the per-sample errors (the
    reference's formula holds at batch size 1, where the two agree);
  * no host synchronisation: every metric stays a device tensor.
"""
from collections import OrderedDict

import torch

from .. import hip
from ..geometry.pose import Pose
from ..utils.depth import compute_depth_metrics, compute_depth_metrics_demon, compute_pose_metrics

# the entries of every metrics vector (model_wrapper.py:50)
METRICS_KEYS = ("abs_rel", "sqr_rel", "rmse", "rmse_log", "a1", "a2", "a3", "SILog", "l1_inv",
                "rot_ang", "t_ang", "t_cm")
METRICS_MODES = ("", "_pp", "_gt", "_pp_gt")


def evaluate_from_inv_depths(inv, inv_flipped, batch, params, poses, demon=False, metrics_name="depth",
                             metrics_modes=METRICS_MODES):
    """Everything of evaluate_depth after the network (model_wrapper.py:361-399):
    inv [B,1,H,W] the prediction, inv_flipped the prediction on the flipped
    inputs (still flipped), poses the unflipped pass's list of N Pose.  One
    post-process launch, then per mode the nine depth metrics with the three
    pose errors appended.  Returns {'metrics': OrderedDict of float32 device
    tensors [12], 'inv_depth': inv_pp}."""
    inv_pp, depth, depth_pp = hip.post_process_inv_depth(inv, inv_flipped, method="mean")
    metrics = OrderedDict()
    if "depth" in batch:
        if "pose_context" in batch:
            pose_errs = compute_pose_metrics(params, gt=batch["pose_context"], pred=poses).to(inv_pp.device)
        else:
            pose_errs = torch.zeros(3, device=inv_pp.device)
        for mode in metrics_modes:
            pred = depth_pp if "pp" in mode else depth
            if demon:
                m = compute_depth_metrics_demon(params, gt=batch["depth"], gt_pose=batch["pose_context"], pred=pred,
                                                use_gt_scale="gt" in mode)
            else:
                m = compute_depth_metrics(params, gt=batch["depth"], pred=pred, use_gt_scale="gt" in mode)
            metrics[metrics_name + mode] = torch.cat([m.float(), pose_errs])
    return {"metrics": metrics, "inv_depth": inv_pp}


def evaluate_depth(model, batch, params, demon=False, metrics_name="depth", metrics_modes=METRICS_MODES):
    """ModelWrapper.evaluate_depth (model_wrapper.py:355-399) for an SfmModelMF
    family `model`: metrics[metrics_name + mode] is a float32 device tensor [12]
    in the order of METRICS_KEYS for mode '' (plain), '_pp' (flip
    post-processed), '_gt' (ground-truth median scaled) and '_pp_gt'; empty when
    the batch has no 'depth'.  `params` needs .min_depth, .max_depth and .crop;
    `demon` selects compute_depth_metrics_demon (the reference's Demon
    validation sets).  Runs under no_grad in eval mode and restores the
    model's mode; `batch` is not modified."""
    modes = [(m, m.training) for m in model.modules()]
    model.eval()
    try:
        with torch.no_grad():
            rgb, K = batch["rgb"], batch["intrinsics"]
            B, W = rgb.shape[0], rgb.shape[3]
            K_flipped = K.clone()                            # flip_lr_intr (utils/image.py:61-81) on a copy
            K_flipped[:, 0, 0] = -K[:, 0, 0]
            K_flipped[:, 0, 2] = W - K[:, 0, 2]
            both = dict(batch)
            both["rgb"] = torch.cat([rgb, torch.flip(rgb, [3])])
            both["rgb_context"] = [torch.cat([r, torch.flip(r, [3])]) for r in batch.get("rgb_context", [])]
            both["intrinsics"] = torch.cat([K, K_flipped])
            out = model(both)
            inv = out["inv_depths"][0]
            poses = [Pose(p.mat[:B]) for p in out["poses"]]
            return evaluate_from_inv_depths(inv[:B], inv[B:], batch, params, poses, demon=demon,
                                            metrics_name=metrics_name, metrics_modes=metrics_modes)
    finally:
        for m, training in modes:
            m.training = training
