"""The renderer's entry points and its host-side parts without a GPU: the
exports and their argument checks (nothing is launched), the chase camera
against a transcription of the reference viewer's rule, the trajectory file,
the render intrinsics, the rounding band of tests/test_render.py measured
again, and the window-minimum resolve against brute-force square splatting."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import render_oracle as R
from test_render import CASES, MAX_BAND_SHARE, SCENES, SIZE, TOL_ROUND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dro_amd.h")
LIB = os.path.join(ROOT, "dro-sfm_amd", "libdro_amd.so")
NEW = ("dro_render_points_workspace_bytes", "dro_render_points")
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("libdro_amd.so not built: run `make -C dro-sfm_amd/csrc`")
    from dro_sfm_amd.hip import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def p():
    buf = (ctypes.c_float * 64)()
    yield ctypes.cast(buf, ctypes.c_void_p)


# ------------------------------------------------------------------ C ABI
def test_exports_declared(lib):
    from dro_sfm_amd.hip import _lib
    declared = set(re.findall(r"\b(dro_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    for n in NEW:
        assert n in declared and n in _lib.EXPORTED and hasattr(lib, n), n
    assert lib.dro_abi_version() == 10


def call(lib, p, xyz="p", rgb="p", n=4, K="p", pose="p", limit=None, V=1, H=4, W=4, s=1, near=1e-6, image="p",
         ws="p", ws_bytes=1 << 20):
    a = {k: (p if v == "p" else v) for k, v in dict(xyz=xyz, rgb=rgb, K=K, pose=pose, image=image, ws=ws).items()}
    return lib.dro_render_points(a["xyz"], a["rgb"], n, a["K"], a["pose"], limit, V, H, W, s, near, 0, a["image"],
                                 None, None, None, None, a["ws"], ws_bytes, None)


def test_render_points_arguments_rejected(lib, p):
    """Every refusal comes before the first launch: the pointers are host
    memory, a launch would fault."""
    for name in ("xyz", "rgb", "K", "pose", "image", "ws"):
        assert call(lib, p, **{name: None}) == -1, name
        assert b"NULL" in lib.dro_last_error()
    for kw in (dict(s=0), dict(s=16), dict(s=-1), dict(V=0), dict(V=-2), dict(V=65536), dict(H=0), dict(W=0),
               dict(H=-3), dict(W=-1), dict(H=32769), dict(W=32769), dict(n=1 << 31), dict(n=-1)):
        assert call(lib, p, **kw) == -2, kw
        assert b"sizes" in lib.dro_last_error()
    assert call(lib, p, ws_bytes=8 * 16 - 1) == -2
    assert b"workspace" in lib.dro_last_error()
    for near in (0.0, -1.0, NAN, float("inf")):
        assert call(lib, p, near=near) == -3, near
        assert b"near" in lib.dro_last_error()


def test_render_points_workspace_bytes(lib):
    """One 64-bit key per cell of the image padded by s // 2 on every side."""
    f = lib.dro_render_points_workspace_bytes
    assert f(1, 37, 53, 1) == 8 * 37 * 53
    assert f(3, 37, 53, 2) == 8 * 3 * 39 * 55
    assert f(3, 37, 53, 5) == 8 * 3 * 41 * 57
    assert f(30, 192, 640, 15) == 8 * 30 * 206 * 654
    assert f(2, 32768, 32768, 15) == 8 * 2 * 32782 * 32782            # beyond 32 bits
    for V, H, W, s in ((0, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, 4, 4, 0), (1, 4, 4, 16), (1, 32769, 4, 1),
                       (65536, 4, 4, 1)):
        assert f(V, H, W, s) == 0, (V, H, W, s)


def test_wrapper_refuses_cpu_tensors_and_shapes():
    import dro_sfm_amd.hip as hip
    xyz, K, E = torch.zeros(5, 3), torch.eye(3)[None], torch.eye(4)[None]
    with pytest.raises(RuntimeError, match="ROCm device"):
        hip.render_points(xyz, xyz, K, E, (4, 4))


# ------------------------------------------------------------------ chase camera
def reference_chase(pose, is_kitti):
    """scripts/vis.py:319-333, line by line; `pose` is what the reference feeds
    its viewer: the inverse of the accumulated camera pose."""
    R_, T = pose[:3, :3], pose[:3, 3:4]
    pos_our = -1 * np.matmul(R_.transpose(), T)
    pos_our = pos_our[:, 0]
    forward = np.matmul(np.array([0, 0, 1]).reshape(1, 3), R_)[0]
    up = np.array([0, -1, 0])
    if not is_kitti:
        position = pos_our - 1 * forward + 0.5 * up
        focal = pos_our + 1 * forward + -0.1 * up
    else:
        position = pos_our - 5 * forward + 48 * up
        focal = pos_our + 1 * forward + -1 * up
    return position, focal, up


def reference_look_at(position, focal, view_up):
    """A camera at `position` looking at `focal`: right = direction x view-up
    (vtkCamera's), down = direction x right; rows x, y, z."""
    d = (focal - position) / np.linalg.norm(focal - position)
    right = np.cross(d, view_up)
    right = right / np.linalg.norm(right)
    down = np.cross(d, right)
    E = np.eye(4)
    E[:3, :3] = np.stack([right, down, d])
    E[:3, 3] = -E[:3, :3] @ position
    return E


@pytest.mark.parametrize("kitti", [False, True])
def test_chase_camera_matches_the_reference_rule(kitti):
    from dro_sfm_amd.models.reconstruct import chase_camera, render_intrinsics, rigid_inverse
    from reconstruct_oracle import _pose
    g = np.random.RandomState(11)
    cam2world = np.stack([_pose(g, 0.6, 3.0) for _ in range(9)])
    got = chase_camera(cam2world, kitti=kitti)
    assert got.dtype == np.float64 and got.shape == (9, 4, 4)
    K = render_intrinsics(37, 53)
    for i in range(9):
        position, focal, up = reference_chase(np.linalg.inv(cam2world[i]), kitti)
        want = reference_look_at(position, focal, up)
        assert np.abs(got[i] - want).max() < 1e-12, i
        Rm = got[i, :3, :3]
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-13 and abs(np.linalg.det(Rm) - 1.0) < 1e-13
        assert np.array_equal(got[i, 3], [0, 0, 0, 1])
        assert np.abs(Rm @ position + got[i, :3, 3]).max() < 1e-12           # the eye is the origin
        f = Rm @ focal + got[i, :3, 3]
        assert f[2] > 0
        uv = (K @ (f / f[2]))[:2]
        assert np.abs(uv - [26.0, 18.0]).max() < 1e-10                        # the focus at the image centre
        # the world's up (-y) is up in the picture: a point above the focus has a smaller v
        a = Rm @ (focal + 0.1 * up) + got[i, :3, 3]
        assert (K @ (a / a[2]))[1] < uv[1]
    # the eye sits behind and above the camera: on its -z side, on the world's -y side of it
    cam = rigid_inverse(cam2world)
    a, b, _ = (5.0, 48.0, 1.0) if kitti else (1.0, 0.5, 0.1)
    eye = -np.einsum("nji,nj->ni", got[:, :3, :3], got[:, :3, 3])
    eye_cam = np.einsum("nij,nj->ni", cam[:, :3, :3], eye) + cam[:, :3, 3]
    assert np.abs(eye - (cam2world[:, :3, 3] - a * cam2world[:, :3, 2] + b * np.array([0, -1.0, 0]))).max() < 1e-12
    assert (eye_cam[:, 2] < 0).all() or kitti


def test_render_intrinsics():
    from dro_sfm_amd.models.reconstruct import render_intrinsics
    K = render_intrinsics(600, 800)
    assert K.dtype == np.float64 and K.shape == (3, 3)
    assert K[0, 0] == K[1, 1] and K[0, 1] == 0 and np.array_equal(K[2], [0, 0, 1])
    assert (K[0, 2], K[1, 2]) == (399.5, 299.5)
    # the rays through the top and the bottom EDGE of the picture (half a pixel beyond the outer centres)
    # are 30 degrees apart
    top, bottom = np.arctan((-0.5 - K[1, 2]) / K[1, 1]), np.arctan((599.5 - K[1, 2]) / K[1, 1])
    assert abs(np.degrees(bottom - top) - 30.0) < 1e-12
    assert abs(K[1, 1] - 300.0 / np.tan(np.radians(15.0))) < 1e-10


# ------------------------------------------------------------------ trajectory file
def test_save_trajectory_obj(tmp_path):
    from dro_sfm_amd.models.reconstruct import save_trajectory_obj
    from reconstruct_oracle import _pose
    g = np.random.RandomState(3)
    for n in (1, 2, 3, 6, 7):
        pose_list = [_pose(g, 0.5, 4.0) for _ in range(n)]
        # scripts/infer_video.py:711-719
        want = str(tmp_path / "want.obj")
        with open(want, 'w') as f_ou:
            for item in pose_list:
                f_ou.write(f'v {item[0, 3]} {item[1, 3]} {item[2, 3]}\n')

            n_pose = len(pose_list)
            for idx_p in range(1, n_pose-1, 2):
                f_ou.write(f'f {idx_p} {idx_p+1} {idx_p+2}\n')
        got = str(tmp_path / "got.obj")
        save_trajectory_obj(got, torch.from_numpy(np.stack(pose_list)))
        assert open(got, "rb").read() == open(want, "rb").read(), n
        save_trajectory_obj(got, np.stack(pose_list))
        assert open(got, "rb").read() == open(want, "rb").read(), n
    assert open(got).read().count("\nf ") == 3                   # 7 poses: f 1 2 3, f 3 4 5, f 5 6 7


def test_save_renders_round_trip(tmp_path):
    from PIL import Image
    from dro_sfm_amd.models.reconstruct import save_renders
    g = np.random.RandomState(5)
    renders = g.randint(0, 256, size=(3, 7, 11, 3)).astype(np.uint8)
    save_renders(str(tmp_path), torch.from_numpy(renders))
    assert sorted(os.listdir(tmp_path / "renders")) == ["000000.png", "000001.png", "000002.png"]
    for i in range(3):
        with Image.open(tmp_path / "renders" / ("%06d.png" % i)) as im:
            assert im.mode == "RGB" and np.array_equal(np.array(im), renders[i])


# ------------------------------------------------------------------ the band
def test_band_is_what_is_measured():
    """TOL_ROUND of tests/test_render.py is 4x to 5x the largest |fp32 - fp64|
    of the restatement's own u / v over the scenes and point sizes of the GPU
    tests, and at most 2 % of the (view, point) pairs of any of them have a u
    or v fraction within the band of 1/2 (the seeds are chosen so)."""
    worst = 0.0
    for name, s, _ in CASES:
        scene = R.make_scene(*SCENES[name])
        d, pairs = R.measure_band(scene, SIZE, s)
        share = R.band_share(scene, SIZE, s, TOL_ROUND)
        print(f"{name} s={s}: {pairs} pairs near the image, |fp32 - fp64| u/v {d:.3e}, in the band "
              f"{100 * share:.3f} %")
        assert share <= MAX_BAND_SHARE, (name, s)
        worst = max(worst, d)
    print(f"largest |fp32 - fp64| {worst:.3e}, band {TOL_ROUND:.3e} = {TOL_ROUND / worst:.2f} x")
    assert 4.0 * worst <= TOL_ROUND <= 5.0 * worst


def test_float32_restatement_agrees_with_float64_outside_the_band():
    """The two precisions of the oracle pick the same cell wherever the float64
    position is outside the band: the band is wide enough for fp32."""
    for name, s, _ in CASES:
        scene = R.make_scene(*SCENES[name])
        c32, z32, _ = R.splat(scene["xyz"], scene["K"], scene["world2cam"], SIZE, s, dtype=np.float32)
        _, _, w = R.splat(scene["xyz"], scene["K"], scene["world2cam"], SIZE, s, dtype=np.float64)
        allowed = R.allowed_cells(w, SIZE, s, TOL_ROUND)
        assert np.logical_or.reduce([c32 == a for a in allowed]).all(), (name, s)
        drawn = c32 != R.REJECTED
        z = z32.view(np.float32)[drawn].astype(np.float64)
        assert np.abs(z / w["z"][drawn] - 1.0).max() < 1e-6


# ------------------------------------------------------------------ window minimum == square splatting
@pytest.mark.parametrize("s", [1, 2, 5, 15])
def test_window_minimum_equals_square_splatting(s):
    """The resolve's minimum over the s x s window of centres is the picture of
    every key painted over its s x s square, on random keys: cells anywhere in
    the padded map (the margin included), several keys per cell, equal depths."""
    g = np.random.RandomState(100 + s)
    H, W = 13, 17
    m = R.margin(s)
    V, n = 2, max(6, 200 // (s * s))                                    # some pixels stay empty
    cell = g.randint(0, (H + 2 * m) * (W + 2 * m), size=(V, n)).astype(np.int32)
    cell[:, ::7] = R.REJECTED
    shared = cell[:, 2::9].shape[1]
    cell[:, 1::9][:, :shared] = cell[:, 2::9]                            # shared cells
    zbits = g.randint(1, 6, size=(V, n)).astype(np.uint32) + np.uint32(0x3F800000)   # few depths: many ties
    zbits[cell == R.REJECTED] = 0
    buf = R.zbuffer(cell, zbits, (H, W), s)
    got = R.resolve_window(buf, (H, W), s)
    want = R.resolve_squares(cell, R.keys_of(zbits), (H, W), s)
    assert np.array_equal(got, want)
    assert (got != R.EMPTY).any() and ((got == R.EMPTY).any() or s == 15)
    # the corners of the margin paint the corners of the image
    one = np.full((1, 1), 0, np.int32)
    far = np.full((1, 1), (H + 2 * m) * (W + 2 * m) - 1, np.int32)
    z1 = np.full((1, 1), 0x3F800000, np.uint32)
    a = R.resolve_window(R.zbuffer(one, z1, (H, W), s), (H, W), s)[0] != R.EMPTY
    b = R.resolve_window(R.zbuffer(far, z1, (H, W), s), (H, W), s)[0] != R.EMPTY
    assert bool(a[0, 0]) == ((s - 1) // 2 >= m) and a.sum() == a[0, 0]     # the top-left margin corner: odd s only
    assert b[H - 1, W - 1] and b.sum() == 1
