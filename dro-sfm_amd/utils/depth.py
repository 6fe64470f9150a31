"""Depth encodings (dro_sfm/utils/depth.py:102-144, networks/layers/resnet/layers.py:11-20),
depth files and the inverse-depth visualisation (dro_sfm/utils/depth.py:11-99).

Written with torch.where instead of the reference's boolean index_put so
they never synchronise with the host (graph-capturable).
"""
import math

import numpy as np
import torch


_LUTS = {}


def _lut(colormap, device):
    """The [256,3] float32 table of `colormap` on `device` (uploaded once)."""
    from .colormaps import TABLES
    if colormap not in TABLES:
        raise NotImplementedError(f"viz_inv_depth: colormap {colormap!r} is not built in (only 'plasma')")
    key = (colormap, str(device))
    if key not in _LUTS:
        _LUTS[key] = torch.tensor(TABLES[colormap], dtype=torch.float32, device=device)
    return _LUTS[key]


def _inv_depth_maps(inv_depth):
    """[H,W], [1,H,W] or [B,1,H,W] -> ([B,H,W] contiguous view, batched?)."""
    if inv_depth.dim() == 4 and inv_depth.shape[1] == 1:
        return inv_depth[:, 0], True
    if inv_depth.dim() == 3 and inv_depth.shape[0] == 1:
        return inv_depth, False
    if inv_depth.dim() == 2:
        return inv_depth[None], False
    raise RuntimeError(f"viz_inv_depth: [H,W], [1,H,W] or [B,1,H,W] expected, got {tuple(inv_depth.shape)}")


def _normalizer(maps, normalizer, percentile, filter_zeros):
    from .. import hip
    B = maps.shape[0]
    if normalizer is None:
        return hip.percentile(maps.reshape(B, -1), percentile, filter_zeros=filter_zeros)
    if torch.is_tensor(normalizer):
        return normalizer.to(device=maps.device, dtype=torch.float32).reshape(-1).expand(B).contiguous()
    return torch.full((B,), float(normalizer), dtype=torch.float32, device=maps.device)


def viz_inv_depth(inv_depth, normalizer=None, percentile=95, colormap='plasma', filter_zeros=False):
    """viz_inv_depth (dro_sfm/utils/depth.py:65-99 of the reference), same
    signature: the colour map of an inverse depth map normalised by its
    `percentile` (of the values > 0 with filter_zeros), or by `normalizer`.
    [H,W] or [1,H,W] -> [H,W,3]; a batch [B,1,H,W] -> [B,H,W,3], each image
    with its own percentile.  Unlike the reference it stays on the GPU (two
    launches: csrc/viz.hip percentile and lookup; no host round trip), returns
    a float32 device tensor, leaves its input unmodified (the reference
    divides a CPU tensor's storage in place), and knows 'plasma' only."""
    from .. import hip
    maps, batched = _inv_depth_maps(inv_depth.detach())
    lut = _lut(colormap, maps.device)
    color = hip.colorize(maps, _normalizer(maps, normalizer, percentile, filter_zeros), lut)
    return color if batched else color[0]


def viz_panel(rgb, inv_depth, normalizer=None, percentile=95, colormap='plasma', filter_zeros=False):
    """The picture scripts/infer.py:160-181 writes: the frame above the colour
    map of its inverse depth, as bytes.  rgb [B,3,H,W] in [0,1], inv_depth
    [B,1,H,W] -> uint8 [B,2H,W,3] (RGB order) on the device: rint(255 v),
    saturated, half to even as in the conversion of imwrite."""
    from .. import hip
    maps, _ = _inv_depth_maps(inv_depth.detach())
    lut = _lut(colormap, maps.device)
    return hip.colorize(maps, _normalizer(maps, normalizer, percentile, filter_zeros), lut, rgb=rgb.detach(),
                        color=False)[1]


def write_depth(filename, depth, intrinsics=None):
    """write_depth (dro_sfm/utils/depth.py:34-62 of the reference), same
    signature.  '.npz': keys 'depth' (squeezed) and 'intrinsics'.  '.png': the
    KITTI 16-bit encoding depth * 256, truncated, clamped to 0..65535 as Pillow
    clamps a mode-I image; the scanlines are made on the GPU
    (hip.depth_png16_rows) and deflated on the host.  depth: a device tensor
    with H x W elements after squeezing (a numpy array is uploaded for '.png')."""
    if filename.endswith('.npz'):
        d = depth.detach().squeeze().cpu().numpy() if torch.is_tensor(depth) else depth
        if torch.is_tensor(intrinsics):
            intrinsics = intrinsics.detach().cpu().numpy()
        np.savez_compressed(filename, depth=d, intrinsics=intrinsics)
    elif filename.endswith('.png'):
        from .. import hip
        from ..datasets.png import encode_png
        if not torch.is_tensor(depth):
            depth = torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32)).to("cuda")
        d = depth.detach().squeeze()
        if d.dim() < 2 and depth.dim() >= 2:  # a map of one row or one column: squeeze took it
            d = d.reshape(depth.shape[-2:])
        if d.dim() != 2:
            raise RuntimeError(f"write_depth: one [H,W] map expected, got {tuple(depth.shape)}")
        rows = hip.depth_png16_rows(d[None])[0].cpu().numpy()
        with open(filename, "wb") as f:
            f.write(encode_png(rows, d.shape[1], d.shape[0], 16))
    else:
        raise NotImplementedError('Depth filename not valid.')


def load_depth(file):
    """load_depth (dro_sfm/utils/depth.py:11-31 of the reference): the [H,W]
    depth map of a '.npz' ('depth') or of a 16-bit '.png' (value / 256, float64;
    invalid pixels are 0).  Host code."""
    if file.endswith('npz'):
        return np.load(file)['depth']
    elif file.endswith('png'):
        from PIL import Image
        with Image.open(file) as im:
            depth_png = np.array(im, dtype=int)
        assert np.max(depth_png) > 255, 'Wrong .png depth file'
        return depth_png.astype(np.float64) / 256.
    raise NotImplementedError('Depth extension not supported.')


def inv2depth(inv_depth):
    if isinstance(inv_depth, (list, tuple)):
        return [inv2depth(x) for x in inv_depth]
    d = 1.0 / inv_depth.clamp(min=1e-6)
    return torch.where(inv_depth <= 0.0, torch.zeros_like(d), d)


def depth2inv(depth):
    if isinstance(depth, (list, tuple)):
        return [depth2inv(x) for x in depth]
    i = 1.0 / depth.clamp(min=1e-6)
    return torch.where(depth <= 0.0, torch.zeros_like(i), i)


def disp_to_depth(disp, min_depth, max_depth):
    lo, hi = 1.0 / max_depth, 1.0 / min_depth
    scaled = lo + (hi - lo) * disp
    return scaled, 1.0 / scaled


def fuse_inv_depth(inv_depth, inv_depth_hat, method='mean'):
    """fuse_inv_depth (dro_sfm/utils/depth.py:202-227 of the reference), same
    signature: the mean / max / min of an inverse depth map and the flipped-back
    map of the flipped pass."""
    if method == 'mean':
        return 0.5 * (inv_depth + inv_depth_hat)
    elif method == 'max':
        return torch.max(inv_depth, inv_depth_hat)
    elif method == 'min':
        return torch.min(inv_depth, inv_depth_hat)
    raise ValueError('Unknown post-process method {}'.format(method))


def post_process_inv_depth(inv_depth, inv_depth_flipped, method='mean'):
    """post_process_inv_depth (dro_sfm/utils/depth.py:230-256 of the reference),
    same signature and return value: the post-processed inverse depth map
    [B,1,H,W].  One HIP launch (csrc/evalpost.hip); GPU tensors only."""
    if method not in ('mean', 'max', 'min'):
        raise ValueError('Unknown post-process method {}'.format(method))
    from .. import hip
    return hip.post_process_inv_depth(inv_depth, inv_depth_flipped, method=method)[0]


def compute_depth_metrics(config, gt, pred, use_gt_scale=True):
    """compute_depth_metrics (dro_sfm/utils/depth.py:259-343 of the reference),
    same signature and return value: a tensor [9] of abs_rel, sq_rel, rmse,
    rmse_log, a1, a2, a3, SILog, iabs_diff averaged over the batch.  `config`
    needs .crop ('garg', 'eigen_nyu' or other), .min_depth and .max_depth.
    Computed by the HIP metrics kernels (csrc/metrics.hip); GPU tensors only."""
    from .. import hip
    return hip.depth_metrics(gt, pred, config.min_depth, config.max_depth, crop=config.crop,
                             use_gt_scale=use_gt_scale).type_as(gt)


def _first_ref_poses(gt_pose, B):
    """The per-image transform the reference's loop pairs with image b
    (`zip(pred, gt, gt_pose)`, utils/depth.py:353): a [B,N,4,4] tensor gives
    image b its first reference; a list of N [B,4,4] tensors (the collated
    batch['pose_context']) gives image b element 0 of reference b, and images
    b >= N are not evaluated (they still count in the batch mean)."""
    if torch.is_tensor(gt_pose):
        return gt_pose, B
    n = min(B, len(gt_pose))
    return torch.stack([gt_pose[b][0] for b in range(n)]).unsqueeze(1), n


def compute_depth_metrics_demon(config, gt, gt_pose, pred, use_gt_scale=True):
    """compute_depth_metrics_demon (dro_sfm/utils/depth.py:343-398 of the
    reference), same signature and return value: tensor [9] of abs_rel, sq_rel,
    rmse, rmse_log, a1, a2, a3, SILog, iabs_diff.  `config` needs .min_depth
    and .max_depth.  HIP metrics kernels (csrc/metrics.hip); GPU tensors only."""
    from .. import hip
    B = gt.shape[0]
    poses, n = _first_ref_poses(gt_pose, B)
    out = hip.depth_metrics_demon(gt[:n], poses.to(gt.device), pred[:n], config.min_depth, config.max_depth,
                                  use_gt_scale=use_gt_scale)
    if n != B:
        out = out * (n / B)
    return out.type_as(gt)


def compute_pose_metrics(config, gt, pred):
    """compute_pose_metrics (dro_sfm/utils/depth.py:400-421 of the reference):
    [rotation error (deg), translation direction error (deg), scale-fitted
    translation error (cm)] of the first reference's pose (gt[0], pred[0] a
    Pose or a [B,4,4] tensor).  The reference takes the pair to the host and
    computes in numpy float32; here the same formulas run in float64 on the
    pair's device (no host synchronisation), returned as float32.  The
    reference's formula holds for one sample (its validation loaders use
    batch size 1); a larger batch gives the mean of the per-sample errors."""
    pm = pred[0].mat if hasattr(pred[0], "mat") else pred[0]
    pr = pm.detach().double().reshape(-1, 4, 4)
    g = gt[0].detach().to(pr.device).double().reshape(-1, 4, 4)
    R1, t1, R2, t2 = g[:, :3, :3], g[:, :3, 3], pr[:, :3, :3], pr[:, :3, 3]
    cos_r = torch.clamp_max(((R1 * R2).sum((1, 2)) - 1.0) / 2.0, 1.0)    # trace(R1^T R2)
    rdeg = torch.arccos(cos_r) * (180.0 / math.pi)
    cos_t = (t1 * t2).sum(1) / (t1.norm(dim=1) * t2.norm(dim=1))
    tdeg = torch.arccos(cos_t) * (180.0 / math.pi)
    a = (t1 * t2).sum(1) / (t2 * t2).sum(1)
    tcm = 100.0 * torch.sqrt(((t1 - a.unsqueeze(1) * t2) ** 2).sum(1))
    return torch.stack([rdeg, tdeg, tcm], 1).mean(0).float()
