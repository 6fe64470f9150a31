"""numpy restatement of csrc/render.hip (dro_render_points).

The projection is written operation by operation -- in float32 it follows the
kernel's roundings one for one (the object is built with -ffp-contract=off),
in float64 it is the value the kernel's pixel is judged against.  The z-buffer
and the window minimum are exact integer arithmetic on the 64-bit keys
(float_bits(z) << 32) | point_index, so everything after the splat's pixel
choice is compared bit for bit.
"""
import numpy as np

from reconstruct_oracle import _pose

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
REJECTED = -1


def margin(s):
    return s // 2


def window(s):
    """Offsets from a pixel to the centres whose square covers it."""
    return -((s - 1) // 2), s // 2


# ------------------------------------------------------------------ projection
def project(xyz, K, world2cam, dtype=np.float64):
    """Camera points and pixel coordinates of every (view, point) pair:
    x, y, z, u, v [V,n] in `dtype`, each product and sum rounded on its own in
    the kernel's order."""
    f = dtype
    p = np.asarray(xyz, dtype=f)
    K = np.asarray(K, dtype=f)
    E = np.asarray(world2cam, dtype=f)
    p0, p1, p2 = p[None, :, 0], p[None, :, 1], p[None, :, 2]
    with np.errstate(all="ignore"):
        cam = [E[:, r, 0, None] * p0 + E[:, r, 1, None] * p1 + E[:, r, 2, None] * p2 + E[:, r, 3, None]
               for r in range(3)]
        x, y, z = cam
        u = K[:, 0, 0, None] * x / z + K[:, 0, 2, None]
        v = K[:, 1, 1, None] * y / z + K[:, 1, 2, None]
    return x, y, z, u, v


def accepted(x, y, z, near, n, limit=None):
    """[V,n] bool: below the view's limit, finite, z >= near."""
    V = x.shape[0]
    lim = np.full(V, n, np.int64) if limit is None else np.asarray(limit, dtype=np.int64)
    with np.errstate(all="ignore"):
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (z >= x.dtype.type(near))
    return ok & (np.arange(n)[None, :] < lim[:, None])


def cell_of(ur, vr, H, W, s):
    """Rounded pixel -> padded z-buffer cell, REJECTED outside the margin; the
    range test in float before any integer conversion."""
    m = margin(s)
    with np.errstate(all="ignore"):
        inside = (ur >= -m) & (ur <= W - 1 + m) & (vr >= -m) & (vr <= H - 1 + m)
    xi = np.where(inside, ur, 0).astype(np.int64)
    yi = np.where(inside, vr, 0).astype(np.int64)
    return np.where(inside, (yi + m) * (W + 2 * m) + (xi + m), REJECTED).astype(np.int32)


def splat(xyz, K, world2cam, size, s=1, near=1e-6, limit=None, dtype=np.float64):
    """What the splat kernel records: cell [V,n] int32 (REJECTED when the pair
    writes no key), zbits [V,n] uint32 (the bits of float32(z), 0 when
    rejected), and the dict of the projection."""
    H, W = size
    n = np.asarray(xyz).shape[0]
    x, y, z, u, v = project(xyz, K, world2cam, dtype)
    ok = accepted(x, y, z, near, n, limit)
    with np.errstate(all="ignore"):
        cell = cell_of(np.rint(u), np.rint(v), H, W, s)       # np.rint: half to even, as rintf
    cell = np.where(ok, cell, REJECTED).astype(np.int32)
    with np.errstate(all="ignore"):
        zbits = np.where(cell != REJECTED, z.astype(np.float32).view(np.uint32), 0).astype(np.uint32)
    return cell, zbits, dict(x=x, y=y, z=z, u=u, v=v, ok=ok)


# ------------------------------------------------------------------ z-buffer (exact)
def keys_of(zbits):
    V, n = zbits.shape
    return (zbits.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)[None, :]


def zbuffer(cell, zbits, size, s):
    """The padded z-buffer [V, H+2m, W+2m] uint64 after every (view, point)
    pair took the minimum of its key into its cell."""
    H, W = size
    m = margin(s)
    V = cell.shape[0]
    buf = np.full((V, (H + 2 * m) * (W + 2 * m)), EMPTY, np.uint64)
    keys = keys_of(zbits)
    for v in range(V):
        hit = cell[v] != REJECTED
        np.minimum.at(buf[v], cell[v][hit].astype(np.int64), keys[v][hit])
    return buf.reshape(V, H + 2 * m, W + 2 * m)


def resolve_window(buf, size, s):
    """[V,H,W] uint64: the minimum key over the s x s window of centres."""
    H, W = size
    m = margin(s)
    lo, hi = window(s)
    best = np.full((buf.shape[0], H, W), EMPTY, np.uint64)
    for dy in range(lo, hi + 1):
        for dx in range(lo, hi + 1):
            best = np.minimum(best, buf[:, m + dy:m + dy + H, m + dx:m + dx + W])
    return best


def resolve_squares(cell, keys, size, s):
    """The same picture by brute force: every key painted over its s x s
    square (pixels -(s//2) .. +((s-1)//2) around the centre), clipped to the
    image.  cell, keys [V,n]."""
    H, W = size
    m = margin(s)
    Wp = W + 2 * m
    best = np.full((cell.shape[0], H, W), EMPTY, np.uint64)
    for v in range(cell.shape[0]):
        for c, k in zip(cell[v].tolist(), keys[v].tolist()):
            if c == REJECTED:
                continue
            cy, cx = c // Wp - m, c % Wp - m
            y0, y1 = max(cy - s // 2, 0), min(cy + (s - 1) // 2, H - 1)
            x0, x1 = max(cx - s // 2, 0), min(cx + (s - 1) // 2, W - 1)
            if y0 <= y1 and x0 <= x1:
                best[v, y0:y1 + 1, x0:x1 + 1] = np.minimum(best[v, y0:y1 + 1, x0:x1 + 1], np.uint64(k))
    return best


def to_byte(c):
    """rint(255 c) saturated in float32, half to even; NaN -> 0 (fmaxf)."""
    with np.errstate(all="ignore"):
        return np.fmin(np.fmax(np.rint(np.float32(255.0) * np.asarray(c, np.float32)), np.float32(0)),
                       np.float32(255)).astype(np.uint8)


def shade(best, rgb, background=(0, 0, 0)):
    """Winning keys [V,H,W] -> image [V,H,W,3] uint8, depth [V,H,W] float32 (0
    where empty), index [V,H,W] int32 (-1 where empty)."""
    empty = best == EMPTY
    idx = np.where(empty, 0, best & np.uint64(0xFFFFFFFF)).astype(np.int64)
    rgb = np.asarray(rgb, np.float32)
    if rgb.shape[0] == 0:
        image = np.zeros(best.shape + (3,), np.uint8)
    else:
        image = to_byte(rgb)[idx]
    image[empty] = np.asarray(background, np.uint8)
    depth = np.where(empty, 0, best >> np.uint64(32)).astype(np.uint32).view(np.float32)
    index = np.where(empty, -1, idx).astype(np.int32)
    return image, depth, index


def render(xyz, rgb, K, world2cam, size, s=1, near=1e-6, limit=None, background=(0, 0, 0), dtype=np.float32,
           cell=None, zbits=None):
    """dro_render_points; with cell / zbits the splat's recorded decisions are
    taken and only the exact part is restated."""
    if cell is None:
        cell, zbits, _ = splat(xyz, K, world2cam, size, s, near, limit, dtype)
    return shade(resolve_window(zbuffer(cell, zbits, size, s), size, s), rgb, background)


# ------------------------------------------------------------------ the rounding band
def near_image(w, size, s, pad=1.0):
    """Pairs whose float64 position lies on the padded image or within `pad`
    pixels of it: the only ones whose rounding the kernel's range test can
    turn into a cell (far outside, |fp32 - fp64| grows with |u| and decides
    nothing)."""
    H, W = size
    m = margin(s) + 0.5 + pad
    with np.errstate(all="ignore"):
        return w["ok"] & (w["u"] >= -m) & (w["u"] <= W - 1 + m) & (w["v"] >= -m) & (w["v"] <= H - 1 + m)


def measure_band(scene, size, s, near=1e-6):
    """(largest |fp32 - fp64| of u and v, number of pairs) over near_image."""
    _, _, w64 = splat(scene["xyz"], scene["K"], scene["world2cam"], size, s, near, scene.get("limit"), np.float64)
    _, _, w32 = splat(scene["xyz"], scene["K"], scene["world2cam"], size, s, near, scene.get("limit"), np.float32)
    sel = near_image(w64, size, s) & w32["ok"]
    if not sel.any():
        return 0.0, 0
    d = max(float(np.abs(w32[k][sel].astype(np.float64) - w64[k][sel]).max()) for k in ("u", "v"))
    return d, int(sel.sum())


def band_share(scene, size, s, band, near=1e-6):
    """Share of the near_image pairs whose u or v fraction lies within `band`
    of 1/2 (float64 oracle alone)."""
    _, _, w = splat(scene["xyz"], scene["K"], scene["world2cam"], size, s, near, scene.get("limit"), np.float64)
    sel = near_image(w, size, s)
    if not sel.any():
        return 0.0
    fu = np.abs(w["u"][sel] - np.floor(w["u"][sel]) - 0.5)
    fv = np.abs(w["v"][sel] - np.floor(w["v"][sel]) - 0.5)
    return float(((fu <= band) | (fv <= band)).mean())


def allowed_cells(w, size, s, band):
    """Per pair the set of cells the kernel may record, as a list of [V,n]
    int32 arrays: the float64 pixel, and where u or v lies within `band` of a
    half-integer the other rounding too (4 combinations at most)."""
    H, W = size
    out = []
    for du in (-band, band):
        for dv in (-band, band):
            with np.errstate(all="ignore"):
                c = cell_of(np.rint(w["u"] + du), np.rint(w["v"] + dv), H, W, s)
            out.append(np.where(w["ok"], c, REJECTED).astype(np.int32))
    return out


# ------------------------------------------------------------------ scenes
def make_scene(n, V, H, W, seed, spread=1.4):
    """n coloured points 1..6 in front of V nearby cameras (rotations <= 0.1
    rad, translations <= 0.3: every z stays >= 0.5, far from `near`), spread
    so that a share of them projects off the image on every side."""
    g = np.random.RandomState(seed)
    K = np.stack([np.array([[0.9 * W + 0.7 * i, 0, 0.49 * W - 0.3 * i], [0, 1.3 * H - 0.5 * i, 0.46 * H + 0.2 * i],
                            [0, 0, 1]], np.float32) for i in range(V)])
    z = g.uniform(1.0, 6.0, n)
    x = (g.uniform(-0.5, 0.5, n) * spread * W / K[0, 0, 0]) * z
    y = (g.uniform(-0.5, 0.5, n) * spread * H / K[0, 1, 1]) * z
    xyz = np.stack([x, y, z], 1).astype(np.float32)
    rgb = g.uniform(0, 1, (n, 3)).astype(np.float32)
    world2cam = np.stack([_pose(g, 0.1, 0.3) for _ in range(V)]).astype(np.float32)
    return dict(xyz=xyz, rgb=rgb, K=K, world2cam=world2cam)
