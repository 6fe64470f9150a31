"""Depth inference outputs on the GPU: hip.percentile, hip.colorize,
hip.depth_png16_rows (csrc/viz.hip), utils.depth.viz_inv_depth / write_depth /
load_depth and models.infer.infer_sequence.

Bounds, none of them taken from what the kernels give:

  percentile   against np.percentile of the same fp32 data evaluated in
               float64: |out - ref| <= 1e-6 max(|a_lo|, |a_hi|).  The order
               statistics are exact (integer counts) and the interpolation
               a_lo + (a_hi - a_lo) frac is rounded to fp32 once (< 6e-8
               relative; three fp32 roundings would still be < 1.8e-7).  q = 0
               and q = 100 are the minimum and the maximum bit for bit, but for
               the sign of a zero: the kernel orders -0.0 below +0.0, numpy
               returns whichever it met first.
  colours      bin edges move with the last bit of the divisor and numpy
               versions differ on float32 + 1e-6, so the check is on the lookup
               index: every pixel equals lut[k] with k one of the two indices
               obtained in float64 from t (1 - 1e-5) and t (1 + 1e-5), t =
               x / (norm + 1e-6) 256 (fp32 division and sum: 2e-7).  NaN gives
               (0, 0, 0).  No pixel is left out.
  bytes        panels and PNG scanlines are integers: exact.
  sequence     inverse depths bit for bit against the model called by hand on
               the same groups; 1 against 4 frames per forward within 1e-6 of
               max|ref| (the forwards differ by ~4e-7, tests/test_reconstruct.py).
"""
import os

import numpy as np
import pytest
import torch

from common import DAMPED, det_init, smooth_images
from test_viz_host import rows16

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
QS = (0, 37.5, 50, 95, 100)
KITTI = 192 * 640


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def bits(a):
    """int32 view of float32 values with -0.0 taken to +0.0."""
    return (np.asarray(a, dtype=np.float32) + np.float32(0.0)).view(np.int32)


# ------------------------------------------------------------------ percentile
def rows_of(n, seed):
    """Three rows of length n with different numbers of values > 0: 16 levels
    around zero (heavy ties, negatives), all equal, and a mix of negatives,
    zeros of both signs and a few distinct positives."""
    g = np.random.RandomState(seed)
    ties = (np.round(g.standard_normal(n) * 4) / 8).clip(-1, 0.875)
    equal = np.full(n, 0.37)
    mixed = g.standard_normal(n) * 3
    mixed[g.uniform(size=n) < 0.3] = 0.0
    mixed[g.uniform(size=n) < 0.2] = -0.0
    return np.stack([ties, equal, mixed]).astype(np.float32)


def kitti_rows():
    """192x640 rows: a smooth inverse depth map, its 16-level quantisation, and
    the mix of rows_of."""
    g = np.random.RandomState(77)
    y, x = np.mgrid[0:192, 0:640].astype(np.float64)
    smooth = (0.02 + 0.5 * (y / 192) ** 2 + 0.05 * np.sin(x / 40) ** 2 + 0.01 * g.uniform(size=(192, 640))).ravel()
    return np.stack([smooth, np.round(smooth * 16) / 16, rows_of(KITTI, 78)[2]]).astype(np.float32)


def reference_percentile(row, q, filter_zeros):
    """(np.percentile in float64, max(|a_lo|, |a_hi|)) of one fp32 row."""
    kept = (row[row > 0] if filter_zeros else row).astype(np.float64)
    m = kept.size
    if m == 0:
        return np.nan, 0.0
    a = np.sort(kept)
    lo = int(np.floor((m - 1) * q / 100))
    hi = min(lo + 1, m - 1)
    return float(np.percentile(kept, q)), max(abs(a[lo]), abs(a[hi]))


def check_percentile(rows, label):
    import dro_sfm_amd.hip as hip
    t = dev(rows)
    worst = 0.0
    for filter_zeros in (False, True):
        for q in QS:
            got = hip.percentile(t, q, filter_zeros=filter_zeros).cpu().numpy()
            assert got.dtype == np.float32 and got.shape == (rows.shape[0],)
            for b, row in enumerate(rows):
                ref, scale = reference_percentile(row, q, filter_zeros)
                if np.isnan(ref):
                    assert np.isnan(got[b]), (label, b, q, filter_zeros)
                    continue
                err = abs(float(got[b]) - ref)
                worst = max(worst, err / scale if scale > 0 else err)
                assert err <= 1e-6 * scale, (label, b, q, filter_zeros, float(got[b]), ref)
                kept = row[row > 0] if filter_zeros else row
                if q == 0:
                    assert bits(got[b]) == bits(kept.min()), (label, b, filter_zeros)
                if q == 100:
                    assert bits(got[b]) == bits(kept.max()), (label, b, filter_zeros)
    print(f"percentile {label}: worst |out - ref| / max(|a_lo|, |a_hi|) = {worst:.2e}")


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1000])
def test_percentile_small_rows(n):
    rows = rows_of(n, n)
    kept = [(r > 0).sum() for r in rows]
    assert n < 255 or len(set(kept)) == 3                     # three different kept counts in one call
    check_percentile(rows, f"n={n}")


def test_percentile_kitti_rows_and_determinism():
    import dro_sfm_amd.hip as hip
    rows = kitti_rows()
    check_percentile(rows, "192x640")
    t = dev(rows)
    for q in (37.5, 95):
        a, b = hip.percentile(t, q, filter_zeros=True), hip.percentile(t, q, filter_zeros=True)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # a row of a larger batch gives what it gives alone
    alone = torch.cat([hip.percentile(t[i:i + 1], 95) for i in range(3)])
    assert torch.equal(alone.view(torch.int32), hip.percentile(t, 95).view(torch.int32))


def test_percentile_empty_rows_give_nan():
    import dro_sfm_amd.hip as hip
    rows = np.zeros((4, 300), dtype=np.float32)
    rows[1] = -0.0
    rows[2] = -1.5
    rows[3, 17] = 2.5                                          # one value kept
    got = hip.percentile(dev(rows), 95, filter_zeros=True).cpu().numpy()
    assert np.isnan(got[:3]).all() and got[3] == 2.5
    got = hip.percentile(dev(rows), 50, filter_zeros=False).cpu().numpy()
    assert np.array_equal(got, np.array([0.0, 0.0, -1.5, 0.0], dtype=np.float32))
    with pytest.raises(RuntimeError, match="q outside"):
        hip.percentile(dev(rows), 101)


# ------------------------------------------------------------------ colours
def lut32():
    from dro_sfm_amd.utils.colormaps import PLASMA
    return np.array(PLASMA, dtype=np.float64).astype(np.float32)


def check_colors(color, x, norm, label):
    """color [B,H,W,3], x [B,H,W], norm [B] (the fp32 normaliser used): every
    pixel is lut[k] for one of the two float64 indices around its quotient."""
    lut = lut32()
    color, x = np.asarray(color), np.asarray(x, dtype=np.float64)
    assert color.dtype == np.float32 and color.shape == x.shape + (3,)
    second = 0
    for b in range(x.shape[0]):
        u = x[b] / (float(norm[b]) + 1e-6)
        nan = np.isnan(u)
        ok = np.zeros(x[b].shape, dtype=bool)
        for i, s in enumerate((1.0 - 1e-5, 1.0 + 1e-5)):
            k = np.minimum(np.floor(np.clip(np.where(nan, 0.0, u) * s, 0.0, 1.0) * 256.0), 255).astype(np.int64)
            hit = (color[b] == lut[k]).all(-1)
            second += int((hit & ~ok).sum()) if i else 0
            ok |= hit
        ok = np.where(nan, (color[b] == 0).all(-1), ok)
        assert ok.all(), (label, b, int((~ok).sum()), np.argwhere(~ok)[:4].tolist())
    print(f"colours {label}: {x.size} pixels, {second} took the second index")


def special_maps(B, H, W, seed, nan):
    g = np.random.RandomState(seed)
    norm = np.array([0.7, 1.3], dtype=np.float32)[:B]
    x = (g.uniform(-0.2, 1.2, size=(B, H, W)) * norm[:, None, None]).astype(np.float32)
    for b in range(B):
        flat = x[b].reshape(-1)
        flat[0], flat[1], flat[2], flat[3], flat[4] = 0.0, norm[b], 3.0 * norm[b], -norm[b], -0.0
        if nan:
            flat[5] = flat[-1] = np.nan
        # values on and next to the edges of table entries
        edges = np.float32(norm[b] + np.float32(1e-6)) * np.array([1, 2, 128, 255], dtype=np.float32) / np.float32(256)
        flat[6:10] = edges
        flat[10:14] = np.nextafter(edges, np.float32(0))
    return x, norm


@pytest.mark.parametrize("H,W", [(5, 7), (37, 96)])
def test_colorize_given_normaliser_and_panel(H, W):
    import dro_sfm_amd.hip as hip
    from dro_sfm_amd.utils.depth import viz_inv_depth, viz_panel
    x, norm = special_maps(2, H, W, H, nan=True)
    lut = dev(lut32())
    color = hip.colorize(dev(x), dev(norm), lut)
    check_colors(color.cpu().numpy(), x, norm, f"{H}x{W} given")
    assert float(color[0].reshape(-1, 3)[2].sub(lut[255]).abs().max()) == 0.0     # above the normaliser: last entry
    assert float(color[0].reshape(-1, 3)[3].sub(lut[0]).abs().max()) == 0.0       # negative: first entry
    # the panel: bytes of the frame above bytes of the colours
    g = np.random.RandomState(W)
    rgb = g.uniform(-0.1, 1.1, size=(2, 3, H, W)).astype(np.float32)
    rgb.reshape(-1)[:6] = (0.0, 1.0, 0.5, 1.5 / 255, 2.5 / 255, 254.5 / 255)      # ends and ties of the rounding
    color2, panel = hip.colorize(dev(x), dev(norm), lut, rgb=dev(rgb))
    assert torch.equal(color2, color) and panel.dtype == torch.uint8 and panel.shape == (2, 2 * H, W, 3)
    top = np.clip(np.rint(np.float32(255) * rgb), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1)
    bottom = np.rint(np.float32(255) * color.cpu().numpy()).astype(np.uint8)
    assert np.array_equal(panel.cpu().numpy(), np.concatenate([top, bottom], 1))
    # the public functions with a scalar normaliser, per image
    for b in range(2):
        single = viz_inv_depth(dev(x[b]), normalizer=float(norm[b]))
        assert single.shape == (H, W, 3) and single.is_cuda and torch.equal(single, color[b])
        assert torch.equal(viz_inv_depth(dev(x[b:b + 1]), normalizer=float(norm[b])), color[b])
        only = viz_panel(dev(rgb[b:b + 1]), dev(x[b:b + 1, None]), normalizer=float(norm[b]))
        assert torch.equal(only[0], panel[b])


@pytest.mark.parametrize("H,W", [(5, 7), (37, 96)])
def test_viz_inv_depth_automatic_normaliser(H, W):
    import dro_sfm_amd.hip as hip
    from dro_sfm_amd.utils.depth import viz_inv_depth
    x, _ = special_maps(2, H, W, H + 1, nan=False)
    for filter_zeros in (False, True):
        t = dev(x[:, None])
        before = t.clone()
        color = viz_inv_depth(t, filter_zeros=filter_zeros)
        assert color.shape == (2, H, W, 3) and color.is_cuda and torch.equal(t, before)
        norm = hip.percentile(dev(x.reshape(2, -1)), 95, filter_zeros=filter_zeros).cpu().numpy()
        for b in range(2):                                     # each image by its own percentile
            kept = x[b][x[b] > 0] if filter_zeros else x[b]
            want = np.percentile(kept.astype(np.float64), 95)
            assert abs(norm[b] - want) <= 1e-6 * abs(want)
        assert norm[0] != norm[1]
        check_colors(color.cpu().numpy(), x, norm, f"{H}x{W} automatic filter_zeros={filter_zeros}")


def test_viz_inv_depth_against_the_reference():
    """tests/golden/viz_inv_depth.npz: the reference's viz_inv_depth and the
    normaliser numpy computed, on a 37x96 map and on one with zeros."""
    import dro_sfm_amd.hip as hip
    from dro_sfm_amd.utils.depth import viz_inv_depth
    with np.load(os.path.join(G, "viz_inv_depth.npz")) as z:
        gold = {k: z[k] for k in z.files}
    for name, filter_zeros in (("plain", False), ("zeros", True)):
        inv, want, want_norm = gold[name + "_inv"], gold[name + "_color"], float(gold[name + "_norm"])
        assert inv.shape == (37, 96) and want.shape == (37, 96, 3)
        norm = hip.percentile(dev(inv.reshape(1, -1)), 95, filter_zeros=filter_zeros).cpu().numpy()
        assert abs(float(norm[0]) - want_norm) <= 1e-6 * want_norm
        got = viz_inv_depth(dev(inv[None]), filter_zeros=filter_zeros).cpu().numpy()
        assert got.shape == (37, 96, 3)
        check_colors(want[None], inv[None], [want_norm], f"reference {name}")
        check_colors(got[None], inv[None], norm, f"product {name}")
        same = (got == want).all(-1)
        print(f"reference {name}: {int(same.sum())} of {same.size} pixels have the reference's colour exactly")
        # a pixel can differ only within 2e-7 (relative) of one of 256 edges: ~1e-4 of the pixels; 1 % is 100x that
        assert same.mean() > 0.99


# ------------------------------------------------------------------ PNG rows, write_depth, load_depth
SPECIAL = (0.0, 0.0039, 1.5, 255.999, 300.0, -1.0, float("nan"))


def depth_map(H, W, seed):
    g = np.random.RandomState(seed)
    d = g.uniform(0.0, 80.0, size=(H, W)).astype(np.float32)
    d.reshape(-1)[:len(SPECIAL)] = SPECIAL
    return d


def png_integers(d):
    """Pillow's value of a mode-I image of trunc(d * 256) saved as 16-bit."""
    v = np.nan_to_num(d.astype(np.float64) * 256.0, nan=0.0)
    return np.clip(np.trunc(v), 0, 65535).astype(np.int64)


@pytest.mark.parametrize("W", [1, 3, 640])
def test_depth_png_rows_and_files(W, tmp_path):
    from PIL import Image
    import dro_sfm_amd.hip as hip
    from dro_sfm_amd.utils.depth import load_depth, write_depth
    H = 9
    d = np.stack([depth_map(H, W, W), depth_map(H, W, W + 1)[::-1].copy()])
    want = png_integers(d)
    assert [int(v) for v in want[0].reshape(-1)[:7]] == [0, 0, 384, 65535, 65535, 0, 0]
    rows = hip.depth_png16_rows(dev(d))
    assert rows.dtype == torch.uint8 and rows.shape == (2, H, 1 + 2 * W)
    assert np.array_equal(rows.cpu().numpy(), np.stack([rows16(want[0]), rows16(want[1])]))
    for b, shape in enumerate(((H, W), (1, 1, H, W))):
        path = str(tmp_path / f"d{b}.png")
        write_depth(path, dev(d[b]).reshape(shape))
        with Image.open(path) as im:
            assert im.mode == "I;16" and im.size == (W, H)
            assert np.array_equal(np.array(im, dtype=int), want[b])
        assert np.array_equal(load_depth(path), want[b] / 256.0)
    # 255.999 * 256 = 65535.74 truncates to the largest value, 300 * 256 is clamped to it
    npz = str(tmp_path / "d.npz")
    K = torch.eye(3, device=DEV)
    write_depth(npz, dev(d[0])[None, None], intrinsics=K)
    assert np.array_equal(load_depth(npz), d[0].squeeze(), equal_nan=True)     # squeezed, as the reference writes it


def test_kitti_depth_png_round_trip(tmp_path):
    from PIL import Image
    from dro_sfm_amd.utils.depth import load_depth, write_depth
    src = os.path.join(G, "png_kitti_depth16.png")
    with Image.open(src) as im:
        first = np.array(im, dtype=int)
    depth = load_depth(src)
    assert np.array_equal(depth * 256, first) and first.max() > 255
    path = str(tmp_path / "again.png")
    write_depth(path, depth.astype(np.float32))                # a host array is uploaded
    with Image.open(path) as im:
        assert im.mode == "I;16" and np.array_equal(np.array(im, dtype=int), first)


# ------------------------------------------------------------------ infer_sequence
@pytest.fixture(scope="module")
def sequence():
    from types import SimpleNamespace
    from dro_sfm_amd.models.SfmModelMF import SfmModelMF
    from dro_sfm_amd.networks.depth_pose.DepthPoseNet import DepthPoseNet
    T, H, W = 7, 64, 96
    net = det_init(DepthPoseNet(version="it4-seq4-out", min_depth=0.1, max_depth=10.0))
    with torch.no_grad():
        for k, v in net.state_dict().items():
            if k.startswith(DAMPED) and "pose" in k and v.is_floating_point():
                v.mul_(0.002)
    model = SfmModelMF(flip_lr_prob=0.0, min_depth=0.1, max_depth=10.0)
    model.add_depth_net(net)
    model = model.to(DEV).train()
    frames = smooth_images(T, H, W, 21).to(DEV)
    K = torch.tensor([[0.58 * W, 0.0, 0.49 * W], [0.0, 1.92 * H, 0.46 * H], [0.0, 0.0, 1.0]], device=DEV)
    # by hand, in the groups infer_sequence forms with 4 frames per forward: frames 1-4, then frame 5
    model.eval()
    inv, poses = [], []
    with torch.no_grad():
        for lo, hi in ((1, 5), (5, 6)):
            out = model({"rgb": frames[lo:hi], "rgb_context": [frames[lo - 1:hi - 1], frames[lo + 1:hi + 1]],
                         "intrinsics": K[None].expand(hi - lo, 3, 3).contiguous()})
            inv.append(out["inv_depths"][0])
            poses.append(torch.stack([p.mat for p in out["poses"]], 1))
    model.train()
    return SimpleNamespace(model=model, frames=frames, K=K, T=T, H=H, W=W, inv=torch.cat(inv),
                           poses=torch.cat(poses).double().cpu().numpy())


def test_infer_sequence_wiring(sequence, tmp_path):
    from PIL import Image
    from dro_sfm_amd.models.infer import infer_sequence
    from dro_sfm_amd.utils.depth import inv2depth, load_depth, viz_inv_depth
    q = sequence
    n, H, W = q.T - 2, q.H, q.W
    out_dir = str(tmp_path / "npz")
    out = infer_sequence(q.model, q.frames, q.K, out_dir=out_dir, save="npz")
    assert q.model.training and all(m.training for m in q.model.modules())
    assert out["inv_depths"].shape == (n, 1, H, W)
    assert torch.equal(out["inv_depths"].view(torch.int32), q.inv.view(torch.int32))
    assert torch.equal(out["depths"], inv2depth(q.inv))
    assert out["poses"].dtype == torch.float64 and out["poses"].shape == (n, 2, 4, 4)
    assert rel_err(out["poses"].numpy(), q.poses) < 1e-6
    # the panels: the frames above viz_inv_depth of the maps, as bytes
    panels = out["panels"]
    assert panels.dtype == torch.uint8 and panels.shape == (n, 2 * H, W, 3) and panels.is_cuda
    top = torch.round(255 * q.frames[1:q.T - 1]).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
    bottom = torch.round(255 * viz_inv_depth(q.inv)).to(torch.uint8)
    assert torch.equal(panels, torch.cat([top, bottom], 1))
    assert len(torch.unique(bottom.reshape(-1, 3), dim=0)) > 16          # a picture, not one colour
    # files: one panel per interior frame, named by the frame, and the depths
    assert sorted(os.listdir(out_dir)) == ["%06d.png" % t for t in range(1, q.T - 1)] + ["depth"]
    assert sorted(os.listdir(os.path.join(out_dir, "depth"))) == ["%06d.npz" % t for t in range(1, q.T - 1)]
    host = panels.cpu().numpy()
    depths = out["depths"].cpu().numpy()
    for i, t in enumerate(range(1, q.T - 1)):
        with Image.open(os.path.join(out_dir, "%06d.png" % t)) as im:
            assert im.mode == "RGB" and np.array_equal(np.array(im), host[i])
        path = os.path.join(out_dir, "depth", "%06d.npz" % t)
        assert np.array_equal(load_depth(path), depths[i, 0])
        with np.load(path) as z:
            assert np.array_equal(z["intrinsics"], q.K.cpu().numpy())
    # 16-bit depth files, no panels
    png_dir = str(tmp_path / "png")
    out16 = infer_sequence(q.model, q.frames, q.K, out_dir=png_dir, save="png", viz=False)
    assert "panels" not in out16 and os.listdir(png_dir) == ["depth"]
    assert torch.equal(out16["inv_depths"], out["inv_depths"])
    # this untrained net's depths stay below 1: load_depth, like the reference's, takes a file without a value
    # above 255 for an 8-bit image and refuses it (test_depth_png_rows_and_files reads files back with it)
    assert depths.max() < 1.0
    for i, t in enumerate(range(1, q.T - 1)):
        path = os.path.join(png_dir, "depth", "%06d.png" % t)
        with Image.open(path) as im:
            assert im.mode == "I;16" and im.size == (W, H)
            assert np.array_equal(np.array(im, dtype=int), np.trunc(depths[i, 0].astype(np.float64) * 256))
        with pytest.raises(AssertionError, match="Wrong .png depth file"):
            load_depth(path)
    # one frame per forward: the same maps to rounding
    q.model.eval()
    one = infer_sequence(q.model, q.frames, q.K, viz=False, frames_per_forward=1)
    assert not q.model.training and not any(m.training for m in q.model.modules())
    q.model.train()
    err = rel_err(one["inv_depths"].cpu().numpy(), out["inv_depths"].cpu().numpy())
    perr = rel_err(one["poses"].numpy(), out["poses"].numpy())
    print(f"infer_sequence 1 against 4 frames per forward: inverse depths {err:.2e}, poses {perr:.2e}")
    assert err < 1e-6 and perr < 1e-6
    with pytest.raises(ValueError):
        infer_sequence(q.model, q.frames, q.K, save="npz")
    with pytest.raises(RuntimeError, match="frames"):
        infer_sequence(q.model, q.frames[:2], q.K)


def test_ops_refuse_cpu_tensors():
    import dro_sfm_amd.hip as hip
    x = torch.ones(1, 4, 4)
    with pytest.raises(RuntimeError, match="ROCm device"):
        hip.percentile(x.reshape(1, 16), 95)
    with pytest.raises(RuntimeError, match="ROCm device"):
        hip.colorize(x, torch.ones(1, device=DEV), torch.zeros(256, 3, device=DEV))
    with pytest.raises(RuntimeError, match="ROCm device"):
        hip.depth_png16_rows(x)
