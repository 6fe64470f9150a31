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

After the cloud, the pictures of the reference's viewer (scripts/vis.py:259-360,
fed by infer_video.py:683-689): render_sequence draws the growing cloud once
per frame, all frames in one hip.render_points call (csrc/render.hip), from the
viewer's chase camera or from each frame's own; save_renders and
save_trajectory_obj write renders/%06d.png and the camera path.  A
deterministic software z-buffer, not vtk's OpenGL output, and a function of
the finished cloud rather than a viewer fed through a queue.
"""
import os
from types import SimpleNamespace

import numpy as np
import torch

from .. import hip
from ..datasets.png import encode_png
from ..utils.depth import inv2depth


def default_params(kitti=False):
    """sfm_params of the reference (infer_video.py:860-868).  Two optional
    entries, fusion_thres_p_dist (1) and fusion_thres_d_diff (1e-3), override
    the thresholds gemo_filter_fusion hard-codes (:349); kitti itself is kept
    for the chase camera of the renders."""
    return SimpleNamespace(grad_max=0.05, depth_max=15.0 if kitti else 6.0, crop_h=32, crop_w=32,
                           fusion_view_num=5, fusion_thres_view=1, kitti=bool(kitti))


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


def reconstruct_sequence(model, frames, K, params=None, fuse=True, keep_invalid=False, frames_per_forward=4,
                         render=None, render_size=None, point_size=5):
    """frames [T,3,H,W] float32 on the GPU (T >= 3), K [3,3] or [1,3,3] pinhole
    intrinsics of those frames.  Every interior frame t = 1..T-2 is predicted
    with the references (t-1, t+1), frames_per_forward frames per forward.

    Returns a dict:
      'points'  [n,3] float32 world-space points, frame-major then row-major
      'colors'  [n,3] float32, the frames' own values
      'poses'   [T-2,4,4] float64 (host): the accumulated camera poses
      'depths'  [T-2,H,W] the cleaned (and, with fuse=True, fused) depth maps
      'renders' [T-2,h,w,3] uint8, with render = "chase" or "first_person"
                only: frame i shows the cloud of the frames <= i
                (render_sequence; render_size = (h, w), default the frames';
                the chase camera keeps KITTI's distance with params.kitti)
    fuse=False gives the reference's output as it stands (fusion disabled).
    Runs under no_grad in eval mode and restores the model's training flags."""
    params = default_params() if params is None else params
    if render not in (None,) + CAMERAS:
        raise RuntimeError(f"reconstruct_sequence: render None, 'chase' or 'first_person' expected, got {render!r}")
    if frames.dim() != 4 or frames.shape[1] != 3 or frames.shape[0] < 3:
        raise RuntimeError(f"reconstruct_sequence: frames [T>=3,3,H,W] expected, got {tuple(frames.shape)}")
    if render == "first_person" and render_size is not None and tuple(render_size) != tuple(frames.shape[2:]):
        raise RuntimeError("reconstruct_sequence: first_person renders have the frames' size (K is theirs)")
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
            out = {"points": xyz[:count], "colors": colors[:count], "poses": torch.from_numpy(cam2world),
                   "depths": depths}
            if render is not None:
                H, W = frames.shape[2:]
                per_frame = (torch.full((n,), H * W, device=frames.device) if keep_invalid
                             else (depths > 0).sum((1, 2)))
                out["renders"] = render_sequence(out["points"], out["colors"], per_frame, cam2world, K1,
                                                 render_size or (H, W), camera=render, point_size=point_size,
                                                 kitti=getattr(params, "kitti", False))
            return out
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


# ------------------------------------------------------------------ rendering
CAMERAS = ("chase", "first_person")
# eye = c - a f + b up, focus = c + f - d up (scripts/vis.py:326-333)
CHASE = {False: (1.0, 0.5, 0.1), True: (5.0, 48.0, 1.0)}
VIEW_ANGLE = 30.0            # vtkCamera's default vertical view angle, degrees


def look_at(eye, focus, view_up):
    """World->camera [..,4,4] float64 of a camera at `eye` looking at `focus`
    in this project's axes (x right, y down, z forward): z = the direction of
    view, x = -view_up x z, y = z x x.  view_up must not be parallel to z."""
    eye, focus = np.asarray(eye, dtype=np.float64), np.asarray(focus, dtype=np.float64)
    z = focus - eye
    z = z / np.linalg.norm(z, axis=-1, keepdims=True)
    x = np.cross(-np.asarray(view_up, dtype=np.float64), z)
    x = x / np.linalg.norm(x, axis=-1, keepdims=True)
    y = np.cross(z, x)
    T = np.zeros(eye.shape[:-1] + (4, 4))
    T[..., 0, :3], T[..., 1, :3], T[..., 2, :3] = x, y, z
    T[..., :3, 3] = -(T[..., :3, :3] @ eye[..., None])[..., 0]
    T[..., 3, 3] = 1.0
    return T


def chase_camera(cam2world, kitti=False):
    """The cinematic camera of the reference's viewer (scripts/vis.py:319-333)
    for camera poses cam2world [..,4,4]: behind and above the current camera,
    looking just ahead of it.  c = the camera centre, f = the camera's z axis
    in the world, up = (0,-1,0): eye = c - a f + b up, focus = c + f - d up
    with (a, b, d) = (5, 48, 1) for KITTI, else (1, 0.5, 0.1); view-up is
    (0,-1,0).  Returns the look-at world->camera matrices, float64 (host)."""
    T = np.asarray(cam2world, dtype=np.float64)
    c, f = T[..., :3, 3], T[..., :3, 2]
    up = np.array([0.0, -1.0, 0.0])
    a, b, d = CHASE[bool(kitti)]
    return look_at(c - a * f + b * up, c + 1.0 * f + -d * up, up)


def render_intrinsics(H, W):
    """[3,3] float64: vtk's default camera for an H x W window -- a vertical
    view angle of 30 degrees, square pixels, the principal point at the image
    centre ((W-1)/2, (H-1)/2: integer coordinates are pixel centres)."""
    f = 0.5 * H / np.tan(np.radians(0.5 * VIEW_ANGLE))
    return np.array([[f, 0.0, 0.5 * (W - 1)], [0.0, f, 0.5 * (H - 1)], [0.0, 0.0, 1.0]])


def render_sequence(points, colors, counts, cam2world, K, size, camera="chase", point_size=5, kitti=False):
    """The growing cloud of a sequence, one picture per frame, in ONE
    hip.render_points call: points / colors [n,3] (device) in frame-major
    order, counts [T] (device, integer) the points of each frame, cam2world
    [T,4,4] (host).  Frame i draws the points of the frames <= i: the limit is
    the running sum of counts, taken on the device (no synchronisation).

    camera="chase": the reference viewer's cinematic camera (chase_camera)
    with render_intrinsics(*size); K is not used.  camera="first_person": each
    frame's own pose with K ([3,3], [1,3,3] or [T,3,3], the intrinsics of
    images of `size`).  Returns [T,H,W,3] uint8 on a black background, as the
    reference's renderer has it."""
    if camera not in CAMERAS:
        raise RuntimeError(f"render_sequence: camera 'chase' or 'first_person' expected, got {camera!r}")
    cam2world = np.asarray(cam2world, dtype=np.float64)
    T = cam2world.shape[0]
    if cam2world.shape != (T, 4, 4) or counts.shape != (T,):
        raise RuntimeError(f"render_sequence: cam2world [T,4,4] and counts [T] expected, got "
                           f"{cam2world.shape} and {tuple(counts.shape)}")
    H, W = (int(v) for v in size)
    dev = points.device
    if camera == "chase":
        world2cam = chase_camera(cam2world, kitti)
        Kv = torch.from_numpy(render_intrinsics(H, W)).float().to(dev).expand(T, 3, 3)
    else:
        world2cam = rigid_inverse(cam2world)
        Kv = K.reshape(-1, 3, 3).expand(T, 3, 3)
    limit = torch.cumsum(counts, 0).to(torch.int32)
    return hip.render_points(points, colors, Kv.contiguous(), torch.from_numpy(world2cam).float().to(dev), (H, W),
                             limit=limit, point_size=point_size, check_skew=camera != "chase")


def save_renders(out_dir, renders):
    """renders uint8 [n,H,W,3] (RGB) -> out_dir/renders/%06d.png, numbered from
    0 as the reference's viewer numbers them (scripts/vis.py:353).  One copy off
    the device."""
    host = renders.cpu().numpy() if torch.is_tensor(renders) else np.asarray(renders)
    n, H, W = host.shape[:3]
    rows = np.zeros((n, H, 1 + 3 * W), dtype=np.uint8)           # filter type None
    rows[:, :, 1:] = host.reshape(n, H, 3 * W)
    folder = os.path.join(out_dir, "renders")
    os.makedirs(folder, exist_ok=True)
    for i in range(n):
        with open(os.path.join(folder, "%06d.png" % i), "wb") as f:
            f.write(encode_png(rows[i], W, H, 2))


def save_trajectory_obj(path, poses):
    """The camera path as the reference writes it (scripts/infer_video.py:
    711-719): one `v x y z` line per pose (its translation, printed as Python
    prints a float64) and an `f` line for every second consecutive triple."""
    poses = poses.numpy() if torch.is_tensor(poses) else np.asarray(poses)
    poses = poses.astype(np.float64)
    with open(path, "w") as f:
        for item in poses:
            f.write(f"v {item[0, 3]} {item[1, 3]} {item[2, 3]}\n")
        for i in range(1, len(poses) - 1, 2):
            f.write(f"f {i} {i + 1} {i + 2}\n")
