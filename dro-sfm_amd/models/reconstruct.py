"""From a trained model to a reconstruction of a sequence: the loop of the
reference's scripts/infer_video.py:564-689 for an SfmModelMF.

  per-frame depth and relative poses -> chained camera poses -> cleaned depth
  maps -> multi-view consistency filter and fusion -> coloured world-space
  point cloud.

What changes versus the reference, never the per-frame math:
  * several frames go through ONE eval-mode forward (eval BatchNorm uses the
    running statistics, so the samples of a batch are independent; the
    argument of models/evaluate.py);
  * cleaning, fusion and back-projection are one HIP launch each for the whole
    sequence (hip.clean_depth, hip.fuse_depths, hip.backproject_points;
    csrc/reconstruct.hip), not ~70 ATen launches per frame and source view;
  * the fusion is ON.  In the reference the call is disabled (`and False`,
    infer_video.py:668) and passes the accumulated camera->world poses where
    its functions expect world->camera extrinsics; here the extrinsics are the
    inverses of the accumulated poses;
  * a zero crop means no crop (see hip.clean_depth);
  * the points of pixels without depth are dropped (keep_invalid=True keeps
    them, as the reference does);
  * host synchronisations: one read of K's skew before the loop, one copy of
    the relative poses off the device (they are chained on the host in fp64),
    and the final slice of the packed cloud to its length.
"""
from types import SimpleNamespace

import numpy as np
import torch

from .. import hip
from ..utils.depth import inv2depth


def default_params(kitti=False):
    """sfm_params of the reference (infer_video.py:860-868).  Two optional
    entries, fusion_thres_p_dist (1) and fusion_thres_d_diff (1e-3), override
    the thresholds gemo_filter_fusion hard-codes (:349)."""
    return SimpleNamespace(grad_max=0.05, depth_max=15.0 if kitti else 6.0, crop_h=32, crop_w=32,
                           fusion_view_num=5, fusion_thres_view=1)


def euler_vec_to_mat(vec):
    """[...,6] (tx,ty,tz, rx,ry,rz), R = Rx Ry Rz (geometry/pose_utils.py:40-85)
    -> [...,4,4] float64 on the host."""
    vec = np.asarray(vec, dtype=np.float64)
    x, y, z = vec[..., 3], vec[..., 4], vec[..., 5]
    cx, sx, cy, sy, cz, sz = np.cos(x), np.sin(x), np.cos(y), np.sin(y), np.cos(z), np.sin(z)
    T = np.zeros(vec.shape[:-1] + (4, 4))
    T[..., 0, 0], T[..., 0, 1], T[..., 0, 2] = cy * cz, -cy * sz, sy
    T[..., 1, 0], T[..., 1, 1], T[..., 1, 2] = sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy
    T[..., 2, 0], T[..., 2, 1], T[..., 2, 2] = -cx * sy * cz + sx * sz, cx * sy * sz + sx * cz, cx * cy
    T[..., :3, 3] = vec[..., :3]
    T[..., 3, 3] = 1.0
    return T


def rigid_inverse(T):
    """[...,4,4] -> [R^T | -R^T t]."""
    T = np.asarray(T, dtype=np.float64)
    out = np.zeros_like(T)
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -(Rt @ T[..., :3, 3:])[..., 0]
    out[..., 3, 3] = 1.0
    return out


def chain_poses(pose21, pose23):
    """The live branch of the reference's pose handling (infer_video.py:618-663).
    pose21, pose23 [n,4,4]: per frame the predicted transforms to the previous
    and to the next frame.  Both translations are negated; from the second
    frame on pose21's translation is rescaled to the length of the previous
    frame's pose23 translation; the camera poses are accumulated by right
    multiplication.  Returns the accumulated (camera->world) poses [n,4,4],
    float64."""
    pose21 = np.array(pose21, dtype=np.float64)
    pose23 = np.array(pose23, dtype=np.float64)
    out = np.empty_like(pose21)
    pose_prev, pose23_prev = None, None
    for i in range(pose21.shape[0]):
        p21, p23 = pose21[i], pose23[i]
        p21[:3, 3] = -p21[:3, 3]
        p23[:3, 3] = -p23[:3, 3]
        if pose23_prev is not None:
            p21[:3, 3] = p21[:3, 3] * (np.linalg.norm(pose23_prev[:3, 3]) / np.linalg.norm(p21[:3, 3]))
        pose23_prev = p23
        pose_prev = p21 if pose_prev is None else pose_prev @ p21
        out[i] = pose_prev
    return out


def _pose_tensor(poses):
    """The model's N Pose objects of one forward -> [b,N,6] euler vectors when
    it kept them, else [b,N,4,4] matrices (device tensors)."""
    if all(p.vec is not None and p.mode == "euler" for p in poses):
        return torch.stack([p.vec for p in poses], 1)
    return torch.stack([p.mat for p in poses], 1)


def relative_poses_to_host(t):
    """[n,N,6] euler vectors or [n,N,4,4] matrices -> [n,N,4,4] float64 on the
    host: the one device->host copy of the poses."""
    a = t.double().cpu().numpy()
    return euler_vec_to_mat(a) if a.shape[-1] == 6 else a


def fuse_sequence(depths, K, cam2world, params, check_skew=True):
    """Step 4: frame i >= fusion_view_num - 1 is fused with the previous
    fusion_view_num - 1 cleaned depths, all frames in one launch; the first
    frames keep their cleaned depth.  depths [n,H,W], K [n,3,3], cam2world
    [n,4,4] (host, float64)."""
    S = int(params.fusion_view_num) - 1
    n = depths.shape[0]
    if S < 1 or n <= S:
        return depths.clone()
    extr = torch.from_numpy(rigid_inverse(cam2world)).float().to(depths.device)
    m = n - S
    src = torch.stack([depths[s:s + m] for s in range(S)])
    esrc = torch.stack([extr[s:s + m] for s in range(S)])
    fused, _ = hip.fuse_depths(depths[S:], src, K[S:], extr[S:], esrc,
                               thres_p_dist=getattr(params, "fusion_thres_p_dist", 1.0),
                               thres_d_diff=getattr(params, "fusion_thres_d_diff", 1e-3),
                               thres_view=int(params.fusion_thres_view), check_skew=check_skew)
    return torch.cat([depths[:S], fused])


def predict_interior_frames(model, frames, K1, frames_per_forward, what):
    """Every interior frame t = 1..T-2 of frames [T,3,H,W] through `model`
    with the references (t-1, t+1), frames_per_forward frames per forward.
    Returns (inv_depths [T-2,1,H,W], relative poses [T-2,2,6] or [T-2,2,4,4],
    see _pose_tensor).  The caller sets eval mode and no_grad."""
    T = frames.shape[0]
    inv, poses = [], []
    for lo in range(1, T - 1, frames_per_forward):
        hi = min(lo + frames_per_forward, T - 1)
        out = model({"rgb": frames[lo:hi], "rgb_context": [frames[lo - 1:hi - 1], frames[lo + 1:hi + 1]],
                     "intrinsics": K1.expand(hi - lo, 3, 3).contiguous()})
        inv.append(out["inv_depths"][0])
        if len(out["poses"]) != 2:
            raise RuntimeError(f"{what}: the model must predict the two context poses")
        poses.append(_pose_tensor(out["poses"]))
    return torch.cat(inv), torch.cat(poses)


def reconstruct_sequence(model, frames, K, params=None, fuse=True, keep_invalid=False, frames_per_forward=4):
    """frames [T,3,H,W] float32 on the GPU (T >= 3), K [3,3] or [1,3,3] pinhole
    intrinsics of those frames.  Every interior frame t = 1..T-2 is predicted
    with the references (t-1, t+1), frames_per_forward frames per forward.

    Returns a dict:
      'points'  [n,3] float32 world-space points, frame-major then row-major
      'colors'  [n,3] float32, the frames' own values
      'poses'   [T-2,4,4] float64 (host): the accumulated camera poses
      'depths'  [T-2,H,W] the cleaned (and, with fuse=True, fused) depth maps
    fuse=False gives the reference's output as it stands (fusion disabled).
    Runs under no_grad in eval mode and restores the model's training flags."""
    params = default_params() if params is None else params
    if frames.dim() != 4 or frames.shape[1] != 3 or frames.shape[0] < 3:
        raise RuntimeError(f"reconstruct_sequence: frames [T>=3,3,H,W] expected, got {tuple(frames.shape)}")
    hip.ops.require_device(frames, K, what="reconstruct_sequence")
    T = frames.shape[0]
    n = T - 2
    K1 = K.reshape(1, 3, 3)
    if float(K1[0, 0, 1]) != 0.0:
        raise RuntimeError("reconstruct_sequence: K has a non-zero skew")
    modes = [(m, m.training) for m in model.modules()]
    model.eval()
    try:
        with torch.no_grad():
            inv, poses = predict_interior_frames(model, frames, K1, frames_per_forward, "reconstruct_sequence")
            depths = hip.clean_depth(inv2depth(inv)[:, 0], params.grad_max, params.depth_max,
                                     params.crop_h, params.crop_w)
            rel = relative_poses_to_host(poses)
            cam2world = chain_poses(rel[:, 0], rel[:, 1])
            Kn = K1.expand(n, 3, 3).contiguous()
            if fuse:
                depths = fuse_sequence(depths, Kn, cam2world, params, check_skew=False)
            xyz, colors, count = hip.backproject_points(depths, frames[1:T - 1], Kn,
                                                        torch.from_numpy(cam2world).float().to(frames.device),
                                                        keep_invalid=keep_invalid, check_skew=False)
            count = int(count)
            return {"points": xyz[:count], "colors": colors[:count], "poses": torch.from_numpy(cam2world),
                    "depths": depths}
    finally:
        for m, training in modes:
            m.training = training


def save_ply(path, xyz, rgb):
    """Binary little-endian PLY of a coloured point cloud.  xyz [n,3] float,
    rgb [n,3] uint8, or float in [0,1] (scaled by 255 and rounded).  Host code:
    tensors are copied off the device."""
    def host(a):
        return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)

    xyz, rgb = host(xyz), host(rgb)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or rgb.shape != xyz.shape:
        raise ValueError(f"save_ply: xyz and rgb [n,3] expected, got {xyz.shape} and {rgb.shape}")
    if rgb.dtype != np.uint8:
        rgb = np.rint(np.clip(rgb.astype(np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)
    rec = np.empty(xyz.shape[0], dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                                        ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {xyz.shape[0]}\n"
              "property float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())
