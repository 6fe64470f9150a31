"""Restatements of the reconstruction ops (csrc/reconstruct.hip) in numpy, and
the synthetic scene their tests share.  Test infrastructure only.

fusion() follows dro_depth_fusion step by step in the dtype it is given:
float64 is the oracle, float32 is used once, on the CPU, to measure how far an
fp32 evaluation can drift from it (measure_bands, the TOL_* constants of
tests/test_reconstruct.py).

The fusion's decisions are discontinuous in three places: the rounding of
(u, v) to a source pixel and the two thresholds.  fusion() takes a recorded
decision of the kernel for a (pixel, view) pair ONLY where its own float64
quantity lies inside a band around that discontinuity; everywhere else it
decides for itself.  A recorded pixel is taken only if it is one of the
roundings the band allows.
"""
import numpy as np

OUTSIDE = -2


def unpack_pixel(rec):
    """int32 ((y + 32768) << 16) | (x + 32768) -> x, y, outside."""
    r = rec.astype(np.int64) & 0xFFFFFFFF
    return (r & 0xFFFF) - 32768, (r >> 16) - 32768, rec == OUTSIDE


def rigid_inv(E):
    R, t = E[..., :3, :3], E[..., :3, 3:]
    Rt = np.swapaxes(R, -1, -2)
    return Rt, -(Rt @ t)


def relative(A, B):
    """[R | t] of A B^-1 for rigid [...,4,4] A and B."""
    Rbi, tbi = rigid_inv(B)
    return A[..., :3, :3] @ Rbi, A[..., :3, :3] @ tbi + A[..., :3, 3:]


def lift(u, v, d, K, R, t):
    """Pixel (u, v) [B,H,W] at depth d into its camera, moved by [R | t] [B,3,3], [B,3,1]."""
    fx, fy, cx, cy = (K[:, i, j][:, None, None] for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)))
    X = np.stack([((u - cx) / fx) * d, ((v - cy) / fy) * d, d], 1)            # [B,3,H,W]
    B, _, H, W = X.shape
    return (R @ X.reshape(B, 3, -1) + t).reshape(B, 3, H, W)


def project(P, K, tiny):
    fx, fy, cx, cy = (K[:, i, j][:, None, None] for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)))
    z = np.maximum(P[:, 2], tiny)
    return (fx * P[:, 0] + cx * P[:, 2]) / z, (fy * P[:, 1] + cy * P[:, 2]) / z


def view(depth_ref, depth_src, K, E_ref, E_src, thres_p_dist, thres_d_diff, dtype=np.float64, rec_pixel=None,
         rec_consistent=None, tol_round=0.0, tol_dist=0.0, tol_rel=0.0):
    """One source view.  Returns a dict of [B,H,W] arrays: u, v, px, py, inside,
    d_re, dist, rel, ok and the in-band flags band_round, band_thres."""
    f = dtype
    depth_ref, depth_src, K, E_ref, E_src = (np.asarray(a, dtype=f) for a in (depth_ref, depth_src, K, E_ref, E_src))
    B, H, W = depth_ref.shape
    tiny = f(1e-10)
    with np.errstate(all="ignore"):
        y, x = np.meshgrid(np.arange(H, dtype=f), np.arange(W, dtype=f), indexing="ij")
        x, y = np.broadcast_to(x, (B, H, W)), np.broadcast_to(y, (B, H, W))
        R, t = relative(E_src, E_ref)
        Rb, tb = relative(E_ref, E_src)
        u, v = project(lift(x, y, depth_ref, K, R, t), K, tiny)
        ur, vr = np.rint(u), np.rint(v)
        inside = (ur >= 0) & (ur <= W - 1) & (vr >= 0) & (vr <= H - 1)
        band_round = np.zeros((B, H, W), bool)
        if rec_pixel is not None:
            fu, fv = u - np.floor(u), v - np.floor(v)
            band_round = (np.abs(fu - 0.5) <= tol_round) | (np.abs(fv - 0.5) <= tol_round)
            kx, ky, kout = unpack_pixel(rec_pixel)
            k_in = ~kout & (kx >= 0) & (kx <= W - 1) & (ky >= 0) & (ky <= H - 1)
            near = (np.abs(kx - u) <= 0.5 + tol_round) & (np.abs(ky - v) <= 0.5 + tol_round)
            may_be_out = np.zeros((B, H, W), bool)
            for su in (-tol_round, tol_round):
                for sv in (-tol_round, tol_round):
                    a, b = np.rint(u + su), np.rint(v + sv)
                    may_be_out |= ~((a >= 0) & (a <= W - 1) & (b >= 0) & (b <= H - 1))
            take_in = band_round & k_in & near
            take_out = band_round & kout & may_be_out
            ur, vr = np.where(take_in, kx, ur), np.where(take_in, ky, vr)
            inside = np.where(take_in, True, np.where(take_out, False, inside))
        px = np.where(inside, ur, 0).astype(np.int64)
        py = np.where(inside, vr, 0).astype(np.int64)
        sampled = np.where(inside, depth_src[np.arange(B)[:, None, None], py, px], f(0))
        Q = lift(u, v, sampled, K, Rb, tb)
        d_re = Q[:, 2] * (sampled > 0)
        u_re, v_re = project(Q, K, tiny)
        dist = np.sqrt((u_re - x) ** 2 + (v_re - y) ** 2)
        rel = np.abs(d_re - depth_ref) / np.maximum(depth_ref, tiny)
        ok_p, ok_d = dist < thres_p_dist, rel < thres_d_diff
        ok = ok_p & ok_d
        band_thres = np.zeros((B, H, W), bool)
        if rec_consistent is not None:
            in_p, in_d = np.abs(dist - thres_p_dist) <= tol_dist, np.abs(rel - thres_d_diff) <= tol_rel
            band_thres = in_p | in_d
            # a clear failure of either test decides, whatever the other's band says
            clear_fail = (~in_p & ~ok_p) | (~in_d & ~ok_d)
            ok = np.where(band_thres & ~clear_fail, rec_consistent.astype(bool), ok)
    return dict(u=u, v=v, px=px, py=py, inside=inside, d_re=d_re, dist=dist, rel=rel, ok=ok,
                band_round=band_round, band_thres=band_thres)


def fusion(depth_ref, depth_src, K, E_ref, E_src, thres_p_dist=1.0, thres_d_diff=1e-3, thres_view=1,
           dtype=np.float64, rec_pixel=None, rec_consistent=None, tols=(0.0, 0.0, 0.0)):
    """dro_depth_fusion.  Returns count [B,H,W] int, fused [B,H,W], the list of
    per-view dicts and the share of (pixel, view) pairs inside a band."""
    S = depth_src.shape[0]
    depth_ref = np.asarray(depth_ref, dtype=dtype)
    total = np.zeros(depth_ref.shape, dtype)
    count = np.zeros(depth_ref.shape, np.int64)
    views, banded = [], 0
    for s in range(S):
        w = view(depth_ref, depth_src[s], K, E_ref, E_src[s], thres_p_dist, thres_d_diff, dtype,
                 None if rec_pixel is None else rec_pixel[s], None if rec_consistent is None else rec_consistent[s],
                 *tols)
        with np.errstate(all="ignore"):
            total = total + np.where(w["ok"], w["d_re"], dtype(0))
        count += w["ok"]
        banded += int((w["band_round"] | w["band_thres"]).sum())
        views.append(w)
    with np.errstate(all="ignore"):
        fused = np.where(count >= thres_view, (total + depth_ref) / (count + 1).astype(dtype), dtype(0))
    return count, fused, views, banded / float(S * depth_ref.size)


def measure_bands(scene, thres_p_dist=1.0, thres_d_diff=1e-3):
    """max |fp32 - fp64| of the restatement's u/v, dist and rel over the (pixel,
    view) pairs where both precisions pick the same source pixel (and the
    quantities are finite)."""
    args = (scene["depth_ref"], scene["depth_src"], scene["K"], scene["extr_ref"], scene["extr_src"])
    _, _, v64, _ = fusion(*args, thres_p_dist, thres_d_diff, dtype=np.float64)
    _, _, v32, _ = fusion(*args, thres_p_dist, thres_d_diff, dtype=np.float32)
    out = dict(uv=0.0, dist=0.0, rel=0.0)
    for a, b in zip(v64, v32):
        same = (a["px"] == b["px"]) & (a["py"] == b["py"]) & (a["inside"] == b["inside"])
        for key, names in (("uv", ("u", "v")), ("dist", ("dist",)), ("rel", ("rel",))):
            for nme in names:
                with np.errstate(all="ignore"):
                    d = np.abs(a[nme] - b[nme].astype(np.float64))
                    keep = same & np.isfinite(d)
                    # far from its threshold a quantity decides nothing (a hole reprojects to
                    # the camera centre: dist ~ 1e4; a pixel without depth has rel ~ 1e10)
                    if key == "rel":
                        keep &= a["rel"] < 10.0 * thres_d_diff
                    if key == "dist":
                        keep &= a["dist"] < 10.0 * thres_p_dist
                if keep.any():
                    out[key] = max(out[key], float(d[keep].max()))
    return out


# ---------------------------------------------------------------- the other two ops
def clean_depth(depth, grad_max, depth_max, crop_h, crop_w):
    """dro_depth_clean in numpy float32, operation by operation."""
    d = np.asarray(depth, dtype=np.float32)
    pad = np.pad(d, [(0, 0), (0, 1), (0, 1)], "constant")
    with np.errstate(all="ignore"):
        gy, gx = pad[:, 1:, :-1] - pad[:, :-1, :-1], pad[:, :-1, 1:] - pad[:, :-1, :-1]
        g = gy * gy + gx * gx
        out = d.copy()
        out[g > np.float32(grad_max)] = 0
        out[d > np.float32(depth_max)] = 0
    if crop_h > 0 and crop_w > 0:
        out[:, :crop_h, :crop_w] = 0
        out[:, -crop_h:, -crop_w:] = 0
    return out


def backproject(depth, rgb, K, cam2world, keep_invalid=False):
    """dro_backproject_points in float64: xyz [n,3], colours [n,3] (the input's
    dtype), frame-major then row-major."""
    depth, K, T = (np.asarray(a, dtype=np.float64) for a in (depth, K, cam2world))
    B, H, W = depth.shape
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    x, y = np.broadcast_to(x, (B, H, W)), np.broadcast_to(y, (B, H, W))
    P = lift(x, y, depth, K, T[:, :3, :3], T[:, :3, 3:])
    xyz = P.transpose(0, 2, 3, 1).reshape(-1, 3)
    col = np.asarray(rgb).transpose(0, 2, 3, 1).reshape(-1, 3)
    if keep_invalid:
        return xyz, col
    keep = (depth > 0).reshape(-1)
    return xyz[keep], col[keep]


# ---------------------------------------------------------------- scene
def _rot(r):
    x, y, z = r
    cx, sx, cy, sy, cz, sz = np.cos(x), np.sin(x), np.cos(y), np.sin(y), np.cos(z), np.sin(z)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rx @ Ry @ Rz


def _pose(rng, r_max, t_max):
    E = np.eye(4)
    E[:3, :3] = _rot(rng.uniform(-r_max, r_max, 3))
    E[:3, 3] = rng.uniform(-t_max, t_max, 3)
    return E


def render_plane(normal, offset, K, E, H, W):
    """Depth of the world plane normal . X = offset seen by the world->camera E."""
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack([(x - K[0, 2]) / K[0, 0], (y - K[1, 2]) / K[1, 1], np.ones_like(x)], 0).reshape(3, -1)
    R, t = E[:3, :3], E[:3, 3]
    # X = R^T (d ray - t):  d = (offset + n . R^T t) / (n . R^T ray)
    return ((offset + normal @ (R.T @ t)) / (normal @ (R.T @ ray))).reshape(H, W)


def make_scene(B, S, H, W, seed):
    """A slanted plane per sample seen by a reference camera and S source
    cameras within 0.02 rad and 0.15 units of it.  The source depths carry
    multiplicative noise of 2e-5 on the left half and 1e-2 on the right half,
    and 5 % holes.  float32 arrays, as the ops take them."""
    rng = np.random.RandomState(seed)
    K = np.zeros((B, 3, 3))
    depth_ref = np.zeros((B, H, W))
    depth_src = np.zeros((S, B, H, W))
    extr_ref = np.zeros((B, 4, 4))
    extr_src = np.zeros((S, B, 4, 4))
    for b in range(B):
        K[b] = [[0.58 * W * (1 + 0.03 * b), 0, 0.49 * W], [0, 1.92 * H * (1 - 0.02 * b), 0.46 * H], [0, 0, 1]]
        normal = np.array([0.25 - 0.4 * b, 0.12, 1.0])
        normal /= np.linalg.norm(normal)
        offset = 2.5 + 0.8 * b
        extr_ref[b] = _pose(rng, 0.3, 0.5)
        depth_ref[b] = render_plane(normal, offset, K[b], extr_ref[b], H, W)
        for s in range(S):
            extr_src[s, b] = _pose(rng, 0.02, 0.15) @ extr_ref[b]
            d = render_plane(normal, offset, K[b], extr_src[s, b], H, W)
            sigma = np.where(np.arange(W) < W // 2, 2e-5, 1e-2)[None, :]
            d = d * (1.0 + sigma * rng.standard_normal((H, W)))
            d[rng.uniform(size=(H, W)) < 0.05] = 0.0
            depth_src[s, b] = d
    f = np.float32
    return dict(depth_ref=depth_ref.astype(f), depth_src=depth_src.astype(f), K=K.astype(f),
                extr_ref=extr_ref.astype(f), extr_src=extr_src.astype(f))
