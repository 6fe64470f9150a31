"""Sequence reconstruction on the GPU: hip.clean_depth, hip.fuse_depths,
hip.backproject_points (csrc/reconstruct.hip) and
models.reconstruct.reconstruct_sequence.

fuse_depths is checked against the reference's own outputs
(tests/golden/fusion_b2_s4.npz, gen_golden_fusion.py) and against the float64
restatement of tests/reconstruct_oracle.py.  Its decisions are discontinuous
at the rounding to a source pixel and at the two thresholds; the restatement
takes the kernel's recorded decision for a (pixel, view) pair only where its
OWN float64 quantity lies within a band of the discontinuity:

  TOL_ROUND  the fraction of u or v within this of 1/2
  TOL_DIST   |dist - thres_p_dist|
  TOL_REL    |rel - thres_d_diff|

Each band is 4x the largest |fp32 - fp64| of the restatement's own u / v, dist
and rel (reconstruct_oracle.measure_bands: a numpy float32 evaluation against
the float64 one, on the CPU, over the pairs where both pick the same source
pixel and the quantity is within 10x of its threshold), at the largest shape
tested here.  Measured:

  scene (B, S, H, W, seed)   u / v      dist       rel
  (2, 4, 37, 53, 5)          9.6e-6     1.2e-5     1.32e-7
  (1, 1, 37, 53, 6)          7.0e-6     1.3e-5     1.02e-7
  (1, 8, 37, 53, 13)         1.0e-5     1.1e-5     1.17e-7
  (1, 4, 192, 640, 9)        1.50e-4    2.06e-4    1.12e-7      <- the bands

tests/test_reconstruct_capi.py repeats the measurement (no GPU needed) and
fails if a band is not between 4x and 5x what it finds, or if more than 2 % of
the pairs of any scene lie inside a band (0.17-0.25 % with an empty record).
Bounds: count equal everywhere, fused within 1e-4 of max|ref| (the project's
parity bar); everything else as stated per test.
"""
import os

import numpy as np
import pytest
import torch

import reconstruct_oracle as R
from common import DAMPED, det_init, load_fixture, smooth_images

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
TOL = 1e-4
TOL_ROUND = 6.1e-4      # 4 x 1.50e-4 px, the largest of the u / v column
TOL_DIST = 8.4e-4       # 4 x 2.06e-4 px
TOL_REL = 5.4e-7        # 4 x 1.32e-7
TOLS = (TOL_ROUND, TOL_DIST, TOL_REL)
MAX_BAND_SHARE = 0.02
SCENES = {"b2_s4": (2, 4, 37, 53, 5), "s1": (1, 1, 37, 53, 6), "s8": (1, 8, 37, 53, 13), "kitti": (1, 4, 192, 640, 9)}
KEYS = ("depth_ref", "depth_src", "K", "extr_ref", "extr_src")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel_err(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


def run_fusion(scene, record=True, **kw):
    import dro_sfm_amd.hip as hip
    out = hip.fuse_depths(*(dev(scene[k]) for k in KEYS), record=record, **kw)
    return [o.cpu().numpy() for o in out]


def check_against_restatement(name, scene, **kw):
    fused, count, pixel, consistent = run_fusion(scene, **kw)
    want_count, want_fused, views, share = R.fusion(*(scene[k] for k in KEYS), rec_pixel=pixel,
                                                    rec_consistent=consistent, tols=TOLS, **kw)
    S = scene["depth_src"].shape[0]
    err = rel_err(fused, want_fused)
    print(f"fuse_depths {name}: pinned-pair share {100 * share:.3f} % (limit {100 * MAX_BAND_SHARE:.0f} %), count "
          f"histogram {np.bincount(count.ravel(), minlength=S + 1).tolist()}, count mismatches "
          f"{int((count != want_count).sum())}, fused max|d|/max|ref| {err:.2e}")
    assert share <= MAX_BAND_SHARE
    assert np.array_equal(count.astype(np.int64), want_count)
    assert err < TOL
    # the recorded decisions are the ones the outputs were made from
    assert np.array_equal(consistent.sum(0), count)
    # the test hooks change nothing
    plain = run_fusion(scene, record=False, **kw)
    assert np.array_equal(plain[0], fused, equal_nan=True) and np.array_equal(plain[1], count)
    return fused, count, pixel, consistent, views


# ------------------------------------------------------------------ 1. fuse_depths
@pytest.fixture(scope="module")
def golden():
    return {k: v.numpy() for k, v in load_fixture(os.path.join(G, "fusion_b2_s4.npz")).items()}


def test_fuse_depths_golden(golden):
    """Against the reference's check_geometric_consistency_batch and the sums of
    gemo_filter_fusion.  Two fp32 evaluations may part at a discontinuity, so
    per view the masks are compared outside the float64 restatement's bands,
    count and fused at the pixels none of whose views is in a band; the number
    of pixels that differ at all is printed (observed on MI355X: see
    DESIGN.md §10)."""
    kw = dict(thres_p_dist=float(golden["thres_p_dist"]), thres_d_diff=float(golden["thres_d_diff"]),
              thres_view=int(golden["thres_view"]))
    fused, count, pixel, consistent, views = check_against_restatement("golden", golden, **kw)
    S = golden["depth_src"].shape[0]
    assert np.bincount(golden["count"].ravel(), minlength=S + 1).min() > 0      # every count 0..S occurs
    banded = np.stack([w["band_round"] | w["band_thres"] for w in views])
    clear = ~banded.any(0)
    print(f"fuse_depths vs the reference: {int((count != golden['count']).sum())} of {count.size} pixels differ in "
          f"count, {int((~clear).sum())} pixels have a view in a band")
    assert np.array_equal(consistent.astype(bool)[~banded], golden["masks"].astype(bool)[~banded])
    assert np.array_equal(count[clear], golden["count"][clear])
    assert rel_err(fused[clear], golden["fused"][clear]) < TOL
    # the reprojected depths of the consistent views, through the recorded sample
    for s, w in enumerate(views):
        both = consistent[s].astype(bool) & golden["masks"][s].astype(bool) & ~banded[s]
        assert rel_err(w["d_re"][both], golden["reprojected"][s][both]) < TOL


@pytest.mark.parametrize("name", list(SCENES))
def test_fuse_depths_restatement(name):
    """More than one block per image, a partial last block, B = 2 with different
    poses per sample, S = 1, 4 and 8, the KITTI size."""
    B, S, H, W, seed = SCENES[name]
    check_against_restatement(name, R.make_scene(B, S, H, W, seed))


@pytest.fixture(scope="module")
def small():
    return R.make_scene(2, 4, 37, 53, 5)


def test_fuse_depths_no_source_depth(small):
    scene = dict(small, depth_src=np.zeros_like(small["depth_src"]))
    fused, count = run_fusion(scene, record=False)
    assert not count.any() and not fused.any()
    # thres_view = 0: every pixel passes the view filter, and with no consistent view fused is the depth itself
    fused, count = run_fusion(scene, record=False, thres_view=0)
    assert not count.any() and np.array_equal(fused, small["depth_ref"])


def test_fuse_depths_thres_view_zero(small):
    fused, count = run_fusion(small, record=False, thres_view=0)
    fused1, count1 = run_fusion(small, record=False, thres_view=1)
    assert np.array_equal(count, count1)
    assert (count == 0).any() and np.array_equal(fused[count == 0], small["depth_ref"][count == 0])
    assert np.array_equal(fused[count > 0], fused1[count > 0]) and not fused1[count == 0].any()
    # a view threshold above S leaves nothing
    assert not run_fusion(small, record=False, thres_view=5)[0].any()


def test_fuse_depths_identity(small):
    """Identity poses and equal depths: every view is consistent, fused is the depth."""
    S, B = small["depth_src"].shape[:2]
    eye = np.broadcast_to(np.eye(4, dtype=np.float32), (S, B, 4, 4)).copy()
    scene = dict(small, depth_src=np.broadcast_to(small["depth_ref"], small["depth_src"].shape).copy(),
                 extr_ref=eye[0], extr_src=eye)
    fused, count = run_fusion(scene, record=False)
    assert (count == S).all()
    err = rel_err(fused, small["depth_ref"])
    print(f"identity: fused vs depth {err:.2e}")
    assert err < 1e-6


def test_fuse_depths_source_turned_away(small):
    """A source camera looking the other way: every z <= 0 is clamped, every sample is off the image."""
    turn = np.diag([-1.0, 1.0, -1.0, 1.0]).astype(np.float32)                # half a turn about y
    scene = dict(small, extr_src=np.einsum("ij,sbjk->sbik", turn, small["extr_src"]))
    fused, count, pixel, consistent = run_fusion(scene)
    assert (pixel == R.OUTSIDE).all() and not consistent.any()
    assert not count.any() and not fused.any() and np.isfinite(fused).all()


def test_fuse_depths_nan_stays_local(small):
    """A NaN in one source pixel reaches only the reference pixels that sample it, as an inconsistent view."""
    base = run_fusion(small)
    s, b, y, x = 1, 1, 17, 20
    src = small["depth_src"].copy()
    src[s, b, y, x] = np.nan
    fused, count, pixel, consistent = run_fusion(dict(small, depth_src=src))
    px, py, outside = R.unpack_pixel(pixel)
    hit = np.zeros(count.shape, bool)
    hit[b] = ~outside[s, b] & (px[s, b] == x) & (py[s, b] == y)
    assert hit.any()
    assert np.isfinite(fused).all()
    assert not consistent[s][hit].any()
    for a, c in zip((fused, count, pixel), base):
        assert np.array_equal(a[..., ~hit] if a.ndim == 4 else a[~hit], c[..., ~hit] if c.ndim == 4 else c[~hit])
    others = np.ones(len(src), bool)
    others[s] = False
    assert np.array_equal(consistent[others], base[3][others])


def test_fuse_depths_deterministic_and_capturable(small):
    import dro_sfm_amd.hip as hip
    args = [dev(small[k]) for k in KEYS]
    first = hip.fuse_depths(*args)
    again = hip.fuse_depths(*args)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip.fuse_depths(*args)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = hip.fuse_depths(*args)
    for _ in range(2):
        for o in out:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, first))


def test_fuse_depths_refuses_skew(small):
    import dro_sfm_amd.hip as hip
    args = [dev(small[k]) for k in KEYS]
    args[2][1, 0, 1] = 0.5
    with pytest.raises(RuntimeError, match="skew"):
        hip.fuse_depths(*args)


# ------------------------------------------------------------------ 2. clean_depth
def _depth_map(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    d = 1.0 + 2.5 * smooth_images(B, H, W, seed, detail=0.03)[:, 0] + 0.02 * torch.rand(B, H, W, generator=g)
    return d.numpy().astype(np.float32)


@pytest.mark.parametrize("shape", [(2, 37, 53), (1, 192, 640)])
@pytest.mark.parametrize("crop", [(0, 0), (0, 5), (8, 6), (32, 32), (40, 700)])
def test_clean_depth_bit_identical(shape, crop):
    """Crop 0 (no crop), a crop larger than the map, values exactly at both
    thresholds (kept: the tests are strict), the last row and column against
    the zero padding."""
    import dro_sfm_amd.hip as hip
    B, H, W = shape
    d = _depth_map(B, H, W, 3)
    grad_max, depth_max = 0.05, 2.5
    d[0, 5, 7] = np.float32(depth_max)                     # exactly at depth_max: kept
    d[0, 5, 9] = np.nextafter(np.float32(depth_max), np.float32(np.inf))
    # a gradient of exactly float32(grad_max): 0.05f is not a square of a float difference in general, so
    # use a threshold that is: (0.25)^2 + 0^2 = 0.0625 in a flat patch
    d[0, 20:23, 30:34] = 2.0
    d[0, 20, 31] = 1.75                                    # pixel (20,30): gx = -0.25, gy = 0
    for gm in (grad_max, 0.0625):
        want = R.clean_depth(d, gm, depth_max, *crop)
        got = hip.clean_depth(dev(d), gm, depth_max, *crop).cpu().numpy()
        assert np.array_equal(got, want), (gm, int((got != want).sum()))
    want = R.clean_depth(d, 0.0625, depth_max, *crop)
    inside_crop = want[0, 20, 30] == 0 and crop[0] > 20 and crop[1] > 30
    assert inside_crop or want[0, 20, 30] == 2.0           # g == grad_max is kept
    zeroed = int((want == 0).sum())
    assert 0 < zeroed and (zeroed < want.size or crop == (40, 700))
    if crop[0] == 0 or crop[1] == 0:                       # no crop: the thresholds alone
        assert np.array_equal(want, R.clean_depth(d, 0.0625, depth_max, 0, 0))


def test_clean_depth_propagates_nothing_from_nan():
    """NaN compares false: a NaN pixel and its upper / left neighbours are kept as they are."""
    import dro_sfm_amd.hip as hip
    d = _depth_map(1, 37, 53, 4)
    d[0, 10, 10] = np.nan
    got = hip.clean_depth(dev(d), 0.05, 2.5, 4, 4).cpu().numpy()
    assert np.array_equal(got, R.clean_depth(d, 0.05, 2.5, 4, 4), equal_nan=True)


# ------------------------------------------------------------------ 3. backproject_points
def _cloud_inputs(B, H, W, holes):
    g = np.random.RandomState(B * H + W)
    depth = _depth_map(B, H, W, 8)
    if holes == "none":
        depth[:] = 0
    elif holes == "half":
        depth[g.uniform(size=depth.shape) < 0.5] = 0
        depth[0, 0, :5] = -1.0                              # a negative depth is no depth
    rgb = smooth_images(B, H, W, 9).numpy()
    K = np.stack([np.array([[0.58 * W, 0, 0.49 * W], [0, 1.92 * H, 0.46 * H], [0, 0, 1]], np.float32)] * B)
    pose = np.stack([R._pose(g, 0.5, 2.0) for _ in range(B)]).astype(np.float32)
    return depth, rgb, K, pose


@pytest.mark.parametrize("shape", [(1, 37, 53), (2, 37, 53), (2, 192, 640)])
@pytest.mark.parametrize("holes", ["all", "none", "half"])
def test_backproject_points(shape, holes):
    """The count, the order and every point: all-valid, all-invalid and half
    holes; 37x53 is 2 tiles of 1024 pixels per frame with a partial one, B = 2
    puts a frame boundary inside a tile, 192x640 B = 2 crosses 240 blocks."""
    import dro_sfm_amd.hip as hip
    depth, rgb, K, pose = _cloud_inputs(*shape, holes)
    want_xyz, want_rgb = R.backproject(depth, rgb, K, pose)
    xyz, col, n = hip.backproject_points(dev(depth), dev(rgb), dev(K), dev(pose))
    assert n.dtype == torch.int32 and n.is_cuda and xyz.shape == (depth.size, 3) and col.shape == xyz.shape
    n = int(n)
    assert n == want_xyz.shape[0] == {"all": depth.size, "none": 0}.get(holes, n)
    if n == 0:
        return
    extent = float(np.abs(want_xyz).max())
    err = float(np.abs(xyz[:n].cpu().numpy() - want_xyz).max()) / extent
    print(f"backproject_points {shape} {holes}: n {n}, xyz max|d|/extent {err:.2e}")
    assert err < TOL                                        # a point out of order is off by ~1 pixel's footprint
    assert np.array_equal(col[:n].cpu().numpy(), want_rgb)  # and its colour is another pixel's
    again = hip.backproject_points(dev(depth), dev(rgb), dev(K), dev(pose))
    assert torch.equal(again[0][:n], xyz[:n]) and torch.equal(again[1][:n], col[:n]) and int(again[2]) == n


def test_backproject_points_keep_invalid():
    import dro_sfm_amd.hip as hip
    depth, rgb, K, pose = _cloud_inputs(2, 37, 53, "half")
    want_xyz, want_rgb = R.backproject(depth, rgb, K, pose, keep_invalid=True)
    xyz, col, n = hip.backproject_points(dev(depth), dev(rgb), dev(K), dev(pose), keep_invalid=True)
    assert int(n) == depth.size == want_xyz.shape[0]
    assert float(np.abs(xyz.cpu().numpy() - want_xyz).max()) / float(np.abs(want_xyz).max()) < TOL
    assert np.array_equal(col.cpu().numpy(), want_rgb)
    # a pixel without depth lands on the camera centre
    b, y, x = np.argwhere(depth == 0)[0]
    assert np.allclose(xyz.cpu().numpy().reshape(2, 37, 53, 3)[b, y, x], pose[b, :3, 3], atol=1e-6)


# ------------------------------------------------------------------ 4. the ops refuse the CPU
def test_ops_refuse_cpu_tensors(small):
    import dro_sfm_amd.hip as hip
    t = [torch.from_numpy(small[k]) for k in KEYS]
    with pytest.raises(RuntimeError, match="ROCm device"):
        hip.clean_depth(t[0])
    with pytest.raises(RuntimeError, match="ROCm device"):
        hip.fuse_depths(*t)
    with pytest.raises(RuntimeError, match="ROCm device"):
        hip.backproject_points(t[0], torch.zeros(2, 3, 37, 53), t[2], t[3])
    with pytest.raises(RuntimeError, match="float32"):
        hip.clean_depth(t[0].double().to(DEV))


# ------------------------------------------------------------------ 5. reconstruct_sequence
def gap_threshold(values, q=0.7):
    """A threshold near the q-quantile of `values` that no value is close to:
    the middle of the widest gap between neighbours in the tenth of the sorted
    values around it.  The batched and the single-frame forwards agree to ~1e-6,
    not bit for bit; a threshold inside a gap keeps rounding from deciding."""
    v = np.sort(np.asarray(values, dtype=np.float64).ravel())
    lo, hi = int((q - 0.05) * v.size), int((q + 0.05) * v.size)
    i = lo + int(np.argmax(np.diff(v[lo:hi + 1])))
    return 0.5 * (v[i] + v[i + 1])


@pytest.fixture(scope="module")
def sequence():
    from types import SimpleNamespace
    import dro_sfm_amd.hip as hip
    from dro_sfm_amd.models import reconstruct as M
    from dro_sfm_amd.models.SfmModelMF import SfmModelMF
    from dro_sfm_amd.networks.depth_pose.DepthPoseNet import DepthPoseNet
    from dro_sfm_amd.utils.depth import inv2depth
    T, H, W = 7, 64, 96
    net = det_init(DepthPoseNet(version="it4-seq4-out", min_depth=0.1, max_depth=10.0))
    # At random init the net predicts translations of 0.56 at depths of 0.27: no view of any frame is consistent
    # with another and the fusion would return zeros.  The pose heads' output convolutions are damped (as
    # common.condition_params damps them) so that neighbouring cameras are ~0.1 px of parallax apart: views are
    # consistent, and every (u, v) stays far from a half-integer, where the ~4e-7 by which a batched and a
    # single-frame forward differ could pick another source pixel.
    with torch.no_grad():
        for k, v in net.state_dict().items():
            if k.startswith(DAMPED) and "pose" in k and v.is_floating_point():
                v.mul_(0.002)
    model = SfmModelMF(flip_lr_prob=0.0, min_depth=0.1, max_depth=10.0)
    model.add_depth_net(net)
    model = model.to(DEV).train()
    frames = smooth_images(T, H, W, 21).to(DEV)
    K = torch.tensor([[0.58 * W, 0.0, 0.49 * W], [0.0, 1.92 * H, 0.46 * H], [0.0, 0.0, 1.0]], device=DEV)
    # by hand: one frame per forward, one op call per frame
    model.eval()
    raw, rel = [], []
    with torch.no_grad():
        for t in range(1, T - 1):
            out = model({"rgb": frames[t:t + 1], "rgb_context": [frames[t - 1:t], frames[t + 1:t + 2]],
                         "intrinsics": K[None]})
            raw.append(inv2depth(out["inv_depths"][0])[:, 0])
            rel.append(torch.stack([p.mat[0] for p in out["poses"]]).double().cpu().numpy())
    model.train()
    raw = torch.cat(raw)
    r = raw.cpu().numpy().astype(np.float64)
    pad = np.pad(r, [(0, 0), (0, 1), (0, 1)])
    grad = (pad[:, 1:, :-1] - r) ** 2 + (pad[:, :-1, 1:] - r) ** 2
    params = SimpleNamespace(grad_max=gap_threshold(grad), depth_max=gap_threshold(r), crop_h=10, crop_w=12,
                             fusion_view_num=3, fusion_thres_view=1, fusion_thres_p_dist=2.0,
                             fusion_thres_d_diff=0.25)
    rel = np.stack(rel)
    poses = M.chain_poses(rel[:, 0], rel[:, 1])
    extr = torch.from_numpy(M.rigid_inverse(poses)).float().to(DEV)
    c2w = torch.from_numpy(poses).float().to(DEV)
    clean = torch.cat([hip.clean_depth(raw[i:i + 1], params.grad_max, params.depth_max, params.crop_h, params.crop_w)
                       for i in range(T - 2)])
    S = params.fusion_view_num - 1
    fused, counts = [clean[i] for i in range(S)], []
    for i in range(S, T - 2):
        f, c = hip.fuse_depths(clean[i:i + 1], clean[i - S:i, None], K[None], extr[i:i + 1], extr[i - S:i, None],
                               thres_p_dist=params.fusion_thres_p_dist, thres_d_diff=params.fusion_thres_d_diff,
                               thres_view=params.fusion_thres_view)
        fused.append(f[0])
        counts.append(c)
    fused = torch.stack(fused)

    def cloud(depths):
        pts, cols = [], []
        for i in range(T - 2):
            xyz, col, n = hip.backproject_points(depths[i:i + 1], frames[i + 1:i + 2], K[None], c2w[i:i + 1])
            pts.append(xyz[:int(n)])
            cols.append(col[:int(n)])
        return torch.cat(pts), torch.cat(cols)

    return SimpleNamespace(model=model, frames=frames, K=K, params=params, poses=poses, clean=clean, fused=fused,
                           counts=torch.cat(counts), cloud=cloud, M=M)


@pytest.mark.parametrize("fuse", [True, False])
def test_reconstruct_sequence_wiring(sequence, fuse):
    """Batched forwards (4 + 1 frames), one launch per stage for the whole
    sequence, against one frame at a time."""
    q = sequence
    out = q.M.reconstruct_sequence(q.model, q.frames, q.K, q.params, fuse=fuse)
    assert q.model.training and all(m.training for m in q.model.modules())
    want_depths = q.fused if fuse else q.clean
    want_pts, want_cols = q.cloud(want_depths)
    hist = np.bincount(q.counts.cpu().numpy().ravel(), minlength=q.params.fusion_view_num).tolist()
    perr = rel_err(out["poses"].numpy(), q.poses)
    derr = rel_err(out["depths"].cpu().numpy(), want_depths.cpu().numpy())
    print(f"reconstruct_sequence fuse={fuse}: {out['points'].shape[0]} points (by hand {want_pts.shape[0]}), poses "
          f"{perr:.2e}, depths {derr:.2e}, kept pixels {int((want_depths > 0).sum())} of {want_depths.numel()}, "
          f"count histogram of the fused frames {hist}")
    assert out["poses"].dtype == torch.float64 and out["poses"].shape == (5, 4, 4)
    assert perr < 1e-6
    assert derr < 1e-5
    assert out["points"].shape == want_pts.shape and out["colors"].shape == want_cols.shape
    assert rel_err(out["points"].cpu().numpy(), want_pts.cpu().numpy()) < 1e-5
    assert torch.equal(out["colors"], want_cols)
    # the stages did something: cleaning removed and kept pixels, fusion found consistent views and changed depths
    kept = float((q.clean > 0).float().mean())
    assert 0.1 < kept < 0.9
    assert hist[1] + hist[2] > 0 and not torch.equal(q.fused, q.clean)
