"""hip.render_points (csrc/render.hip) and the sequence renders on the GPU.

How the picture is checked (tests/render_oracle.py is the restatement):
  * reduction, exactly: from the (cell, z bits) the splat kernel recorded per
    (view, point), the oracle's integer z-buffer and window minimum must give
    image, depth and index equal at every pixel -- atomics, ties, limits,
    margin and colour rule, no tolerance;
  * arithmetic: the recorded cell is the float64 oracle's, except where u or v
    lies within TOL_ROUND of a half-integer, where either rounding is taken;
    the recorded z is within 1e-6 relative.
TOL_ROUND is 4x to 5x the largest |fp32 - fp64| of the oracle's own u / v over
these scenes and at most 2 % of the pairs may lie in the band
(tests/test_render_host.py measures both again on the CPU).
"""
import functools
import os

import numpy as np
import pytest
import torch

import render_oracle as R
from common import smooth_images
from reconstruct_oracle import _pose
from test_reconstruct import sequence  # noqa: F401  (the small model setup: it4-seq4-out, T = 7, 64x96, damped)

DEV = "cuda"
SIZE = (37, 53)
TOL_ROUND = 3.2e-5        # 4.5 x 7.05e-6 px, the largest |fp32 - fp64| of u / v (test_render_host.py prints it)
TOL_Z = 1e-6
MAX_BAND_SHARE = 0.02
# name: (n, V, H, W, seed)
SCENES = {"n1": (1, 1) + SIZE + (3,), "n63": (63, 3) + SIZE + (4,), "n257": (257, 1) + SIZE + (5,),
          "n4000": (4003, 3) + SIZE + (6,)}
# (scene, point size, limit): absent, 0 for every view, differing per view
CASES = [(name, s, "none") for name in SCENES for s in (1, 2, 5)] + [
    ("n4000", 5, "zero"), ("n257", 1, "zero"), ("n4000", 2, "per_view"), ("n63", 5, "per_view"),
    ("n257", 5, "per_view")]
BACKGROUND = (7, 200, 90)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def limit_of(mode, n, V):
    if mode == "none":
        return None
    if mode == "zero":
        return np.zeros(V, np.int32)
    return np.array([n, 0, n // 3][:V] if V > 1 else [n // 2], np.int32)


def host(ts):
    return [None if t is None else t.cpu().numpy() for t in ts]


@functools.lru_cache(maxsize=None)
def run(name, s, mode):
    import dro_sfm_amd.hip as hip
    scene = R.make_scene(*SCENES[name])
    n, V = SCENES[name][:2]
    limit = limit_of(mode, n, V)
    out = hip.render_points(dev(scene["xyz"]), dev(scene["rgb"]), dev(scene["K"]), dev(scene["world2cam"]), SIZE,
                            limit=None if limit is None else dev(limit), point_size=s, background=BACKGROUND,
                            want_depth=True, want_index=True, record=True)
    return scene, limit, host(out)


# ------------------------------------------------------------------ 1. reduction, exact
@pytest.mark.gpu
@pytest.mark.parametrize("name,s,mode", CASES)
def test_reduction_exact(name, s, mode):
    scene, limit, (image, depth, index, cell, zbits) = run(name, s, mode)
    n, V = SCENES[name][:2]
    assert image.shape == (V,) + SIZE + (3,) and image.dtype == np.uint8
    assert cell.shape == (V, n) and zbits.shape == (V, n)
    want = R.render(None, scene["rgb"], None, None, SIZE, s, background=BACKGROUND, cell=cell,
                    zbits=zbits.view(np.uint32))
    drawn = int((index >= 0).sum())
    print(f"{name} s={s} limit={mode}: {int((cell != R.REJECTED).sum())} keys of {V * n} pairs, {drawn} of "
          f"{index.size} pixels drawn")
    assert np.array_equal(index, want[2])
    assert np.array_equal(depth.view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(image, want[0])
    if limit is not None:
        beyond = np.arange(n)[None, :] >= limit[:, None]
        assert (cell[beyond] == R.REJECTED).all() and (zbits[beyond] == 0).all()
        for v in range(V):
            assert index[v].max() < limit[v]
    if mode == "zero":
        assert (image == np.array(BACKGROUND, np.uint8)).all() and (depth == 0).all() and (index == -1).all()
    elif n > 1:
        assert drawn > 0


# ------------------------------------------------------------------ 2. arithmetic
@pytest.mark.gpu
@pytest.mark.parametrize("name,s,mode", CASES)
def test_arithmetic(name, s, mode):
    scene, limit, (_, _, _, cell, zbits) = run(name, s, mode)
    _, _, w = R.splat(scene["xyz"], scene["K"], scene["world2cam"], SIZE, s, limit=limit, dtype=np.float64)
    exact = R.allowed_cells(w, SIZE, s, 0.0)[0]
    allowed = R.allowed_cells(w, SIZE, s, TOL_ROUND)
    ok = np.logical_or.reduce([cell == a for a in allowed])
    in_band = np.logical_or.reduce([a != exact for a in allowed])
    share = float(in_band.mean())
    print(f"{name} s={s} limit={mode}: {int((cell != exact).sum())} of {cell.size} cells differ from float64's, "
          f"{100 * share:.3f} % of the pairs in the band")
    assert share <= MAX_BAND_SHARE
    assert ok.all(), np.argwhere(~ok)[:5]
    assert (cell[~in_band] == exact[~in_band]).all()
    hit = cell != R.REJECTED
    if hit.any():
        z = zbits.view(np.uint32).view(np.float32)[hit].astype(np.float64)
        err = float(np.abs(z / w["z"][hit] - 1.0).max())
        print(f"  z max relative error {err:.2e}")
        assert err < TOL_Z
    assert (zbits[~hit] == 0).all()


# ------------------------------------------------------------------ 3. edge cases in one scene
def edge_scene(s):
    """Identity pose, fx = fy = 8, depths powers of two: every coordinate is
    exact in float32 and the expected picture is known pixel by pixel."""
    H, W = SIZE
    m = R.margin(s)
    K = np.array([[[8.0, 0, 26.0], [0, 8.0, 18.0], [0, 0, 1]]], np.float32)

    def at(px, py, z):
        return [(px - 26.0) * z / 8.0, (py - 18.0) * z / 8.0, z]

    nan, inf = float("nan"), float("inf")
    pts = [at(26, 18, -1.0),                    # 0 behind the camera
           at(26, 18, 0.125),                   # 1 z < near (0.25)
           [nan, 0, 1], [0, inf, 1], [0, 0, -inf], [0, 0, nan],      # 2-5 not finite
           [1e30, 0, 1], [0, -1e30, 1], [3e38, 3e38, 1],              # 6-8 project to +-1e30 and to inf
           at(10, 10, 2.0), at(10, 10, 2.0),    # 9, 10 coincident: 9 wins
           at(20, 10, 4.0), at(20, 10, 2.0),    # 11, 12 the same pixel at two depths: 12 wins
           at(26, 18, 0.25)]                    # 13 exactly at near: drawn
    edges = []                                  # (index, edge pixel (y, x), steps off the edge, side)
    for k in range(1, m + 2):
        row, col = 3 + 7 * (k - 1), 25 + 7 * (k - 1)
        for side, (px, py, ey, ex) in dict(left=(-k, row, row, 0), right=(W - 1 + k, row, row, W - 1),
                                           top=(col, -k, 0, col), bottom=(col, H - 1 + k, H - 1, col)).items():
            edges.append((len(pts), (ey, ex), k, side))
            pts.append(at(px, py, 1.0))
    xyz = np.array(pts, np.float32)
    g = np.random.RandomState(17)
    rgb = g.uniform(0, 1, xyz.shape).astype(np.float32)
    rgb[9], rgb[10] = (1.0, 0.5, 0.0), (0.0, 0.0, 1.0)            # 0.5 * 255 = 127.5 -> 128 (half to even)
    rgb[12] = (-0.3, 1.7, nan)                                     # saturated; NaN -> 0
    return dict(xyz=xyz, rgb=rgb, K=K, world2cam=np.eye(4, dtype=np.float32)[None]), edges


@pytest.mark.gpu
@pytest.mark.parametrize("s", [1, 2, 5])
def test_edge_cases(s):
    import dro_sfm_amd.hip as hip
    H, W = SIZE
    m = R.margin(s)
    scene, edges = edge_scene(s)
    image, depth, index, cell, zbits = host(hip.render_points(
        dev(scene["xyz"]), dev(scene["rgb"]), dev(scene["K"]), dev(scene["world2cam"]), SIZE, point_size=s,
        near=0.25, background=BACKGROUND, want_depth=True, want_index=True, record=True))
    want = R.render(scene["xyz"], scene["rgb"], scene["K"], scene["world2cam"], SIZE, s, near=0.25,
                    background=BACKGROUND, dtype=np.float32)
    assert np.array_equal(index, want[2]) and np.array_equal(image, want[0])
    assert np.array_equal(depth.view(np.uint32), want[1].view(np.uint32))
    assert (cell[0, :9] == R.REJECTED).all() and (zbits[0, :9] == 0).all()
    assert (cell[0, 9:14] != R.REJECTED).all()
    assert index[0, 10, 10] == 9 and tuple(image[0, 10, 10]) == (255, 128, 0) and depth[0, 10, 10] == 2.0
    assert index[0, 10, 20] == 12 and tuple(image[0, 10, 20]) == (0, 255, 0) and depth[0, 10, 20] == 2.0
    assert index[0, 18, 26] == 13 and depth[0, 18, 26] == 0.25
    for i, (ey, ex), k, side in edges:
        reach = (s - 1) // 2 if side in ("left", "top") else s // 2     # the square spans -(s//2) .. +((s-1)//2)
        assert (cell[0, i] != R.REJECTED) == (k <= m), (i, side, k)
        assert (index[0, ey, ex] == i) == (k <= reach), (i, side, k)
        assert (index == i).sum() == s * max(reach - k + 1, 0), (i, side, k)
    assert (index == -1).any() and (image[index == -1] == np.array(BACKGROUND, np.uint8)).all()
    assert (depth[index == -1] == 0).all()


@pytest.mark.gpu
def test_empty_cloud():
    import dro_sfm_amd.hip as hip
    K = dev(np.array([[[8.0, 0, 26.0], [0, 8.0, 18.0], [0, 0, 1]]] * 2, np.float32))
    E = dev(np.stack([np.eye(4, dtype=np.float32)] * 2))
    empty = torch.zeros(0, 3, device=DEV)
    image, depth, index = hip.render_points(empty, empty, K, E, SIZE, point_size=5, background=BACKGROUND,
                                            want_depth=True, want_index=True)
    assert image.shape == (2,) + SIZE + (3,)
    assert (image.cpu().numpy() == np.array(BACKGROUND, np.uint8)).all()
    assert (depth == 0).all() and (index == -1).all()
    plain = hip.render_points(empty, empty, K, E, SIZE)
    assert torch.is_tensor(plain) and int(plain.max()) == 0


# ------------------------------------------------------------------ 4. round trip through backproject_points
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 37, 53), (2, 192, 640)])
def test_round_trip(shape):
    """A depth map with holes lifted by backproject_points and rendered back
    with the same K and the inverse pose at point size 1: every pixel with
    depth shows its own colour, rint(255 rgb), and its depth; the holes show
    the background.  Each point returns to an integer pixel to ~1e-3 px, so no
    rounding band is involved.  192x640 is 480 resolve blocks per view."""
    import dro_sfm_amd.hip as hip
    from dro_sfm_amd.models.reconstruct import rigid_inverse
    B, H, W = shape
    g = np.random.RandomState(B * H + W)
    depth = (1.0 + 2.5 * smooth_images(B, H, W, 8, detail=0.03)[:, 0]).numpy()
    depth[g.uniform(size=depth.shape) < 0.3] = 0
    rgb = smooth_images(B, H, W, 9).numpy()
    K = np.stack([np.array([[0.58 * W, 0, 0.49 * W], [0, 1.92 * H, 0.46 * H], [0, 0, 1]], np.float32)] * B)
    pose = np.stack([_pose(g, 0.5, 2.0) for _ in range(B)])
    xyz, col, n = hip.backproject_points(dev(depth), dev(rgb), dev(K), dev(pose, torch.float32))
    counts = (depth > 0).reshape(B, -1).sum(1)
    assert int(n) == counts.sum()
    world2cam = dev(rigid_inverse(pose), torch.float32)
    start = 0
    for b in range(B):
        pts = slice(start, start + int(counts[b]))
        start += int(counts[b])
        image, z, index = host(hip.render_points(xyz[pts], col[pts], dev(K[b:b + 1]), world2cam[b:b + 1], (H, W),
                                                 background=BACKGROUND, want_depth=True, want_index=True))
        valid = depth[b] > 0
        assert np.array_equal(index[0] >= 0, valid)
        assert np.array_equal(index[0][valid], np.arange(int(counts[b])))           # row-major, each its own pixel
        assert np.array_equal(image[0][valid], R.to_byte(rgb[b].transpose(1, 2, 0))[valid])
        assert (image[0][~valid] == np.array(BACKGROUND, np.uint8)).all() and (z[0][~valid] == 0).all()
        err = float(np.abs(z[0][valid] / depth[b][valid] - 1.0).max())
        print(f"round trip {shape} frame {b}: {int(valid.sum())} points, depth max relative error {err:.2e}")
        assert err < 1e-5


# ------------------------------------------------------------------ 5. determinism, hooks, capture
@pytest.mark.gpu
def test_deterministic_hooks_and_capture():
    import dro_sfm_amd.hip as hip
    scene = R.make_scene(*SCENES["n4000"])
    limit = dev(limit_of("per_view", 4003, 3))
    args = [dev(scene[k]) for k in ("xyz", "rgb", "K", "world2cam")] + [SIZE]
    kw = dict(limit=limit, point_size=5, want_depth=True, want_index=True)
    first = hip.render_points(*args, **kw)
    again = hip.render_points(*args, **kw)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    recorded = hip.render_points(*args, record=True, **kw)
    assert len(recorded) == 5 and all(torch.equal(a, b) for a, b in zip(first, recorded))
    assert torch.equal(hip.render_points(*args, limit=limit, point_size=5), first[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip.render_points(*args, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = hip.render_points(*args, **kw)
    for _ in range(2):
        for o in out:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, first))


@pytest.mark.gpu
def test_wrapper_refuses():
    import dro_sfm_amd.hip as hip
    scene = R.make_scene(*SCENES["n63"])
    xyz, rgb, K, E = (dev(scene[k]) for k in ("xyz", "rgb", "K", "world2cam"))
    skewed = K.clone()
    skewed[1, 0, 1] = 0.5
    with pytest.raises(RuntimeError, match="skew"):
        hip.render_points(xyz, rgb, skewed, E, SIZE)
    with pytest.raises(RuntimeError, match="point_size"):
        hip.render_points(xyz, rgb, K, E, SIZE, point_size=16)
    with pytest.raises(RuntimeError, match=r"\[n,3\]"):
        hip.render_points(xyz, rgb[:5], K, E, SIZE)
    with pytest.raises(RuntimeError, match="limit"):
        hip.render_points(xyz, rgb, K, E, SIZE, limit=torch.zeros(3, device=DEV))
    with pytest.raises(RuntimeError, match="near"):
        hip.render_points(xyz, rgb, K, E, SIZE, near=0.0)


# ------------------------------------------------------------------ 6. the sequence
@pytest.mark.gpu
def test_reconstruct_sequence_renders(sequence, tmp_path):  # noqa: F811
    from PIL import Image
    q = sequence
    M = q.M
    plain = M.reconstruct_sequence(q.model, q.frames, q.K, q.params)
    out = M.reconstruct_sequence(q.model, q.frames, q.K, q.params, render="first_person", point_size=3)
    assert set(out) == set(plain) | {"renders"}
    for k in plain:
        assert torch.equal(out[k], plain[k]), k
    T, H, W = q.frames.shape[0], q.frames.shape[2], q.frames.shape[3]
    assert out["renders"].shape == (T - 2, H, W, 3) and out["renders"].dtype == torch.uint8
    counts = (out["depths"] > 0).sum((1, 2))
    by_hand = M.render_sequence(out["points"], out["colors"], counts, out["poses"].numpy(), q.K, (H, W),
                                camera="first_person", point_size=3)
    assert torch.equal(out["renders"], by_hand)
    # frame i, one call at a time: the cloud of the frames <= i from frame i's own camera
    import dro_sfm_amd.hip as hip
    ends = torch.cumsum(counts, 0).tolist()
    world2cam = torch.from_numpy(M.rigid_inverse(out["poses"].numpy())).float().to(DEV)
    for i in (0, T - 3):
        one = hip.render_points(out["points"][:ends[i]], out["colors"][:ends[i]], q.K[None], world2cam[i:i + 1],
                                (H, W), point_size=3)
        assert torch.equal(one[0], out["renders"][i]), i
    drawn = (out["renders"] != 0).any(-1).float().mean((1, 2)).tolist()
    print(f"share of drawn pixels per frame {[round(d, 3) for d in drawn]}")
    assert min(drawn) > 0.05
    chase = M.reconstruct_sequence(q.model, q.frames, q.K, q.params, render="chase", render_size=(48, 80))
    assert chase["renders"].shape == (T - 2, 48, 80, 3) and torch.equal(chase["points"], plain["points"])
    with pytest.raises(RuntimeError, match="render"):
        M.reconstruct_sequence(q.model, q.frames, q.K, q.params, render="orbit")
    M.save_renders(str(tmp_path), out["renders"])
    M.save_trajectory_obj(str(tmp_path / "pose.obj"), out["poses"])
    want = out["renders"].cpu().numpy()
    assert sorted(os.listdir(tmp_path / "renders")) == ["%06d.png" % i for i in range(T - 2)]
    for i in range(T - 2):
        with Image.open(tmp_path / "renders" / ("%06d.png" % i)) as im:
            assert im.mode == "RGB" and np.array_equal(np.array(im), want[i]), i
    assert open(tmp_path / "pose.obj").read().count("v ") == T - 2
