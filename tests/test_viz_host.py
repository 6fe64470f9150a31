"""The depth-output entry points (csrc/viz.hip) and their host-side parts
without a GPU: the committed plasma table against matplotlib's, the PNG
encoder against Pillow, bad arguments rejected before any launch with a status
code and a message, and the new symbols in the header and in the library."""
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dro-sfm_amd", "libdro_amd.so")
HEADER = os.path.join(ROOT, "include", "dro_amd.h")
NEW = ("dro_percentile", "dro_colorize", "dro_depth_png16_rows")
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


def test_plasma_table_is_matplotlibs():
    matplotlib = pytest.importorskip("matplotlib")
    from dro_sfm_amd.utils.colormaps import PLASMA, TABLES
    want = matplotlib.colormaps["plasma"].colors
    assert len(PLASMA) == 256 == len(want) and TABLES["plasma"] is PLASMA
    assert [tuple(float(v) for v in row) for row in want] == [tuple(row) for row in PLASMA]


def test_product_does_not_import_matplotlib():
    import ast
    seen = 0
    for folder, _, files in os.walk(os.path.join(ROOT, "dro-sfm_amd")):
        for name in files:
            if not name.endswith(".py"):
                continue
            seen += 1
            with open(os.path.join(folder, name)) as f:
                tree = ast.parse(f.read())
            for node in ast.walk(tree):
                mods = ([a.name for a in node.names] if isinstance(node, ast.Import)
                        else [node.module or ""] if isinstance(node, ast.ImportFrom) else [])
                assert not any(m.split(".")[0] == "matplotlib" for m in mods), os.path.join(folder, name)
    assert seen > 20


# ------------------------------------------------------------------ encode_png
def rows16(values):
    """[H,W] integers -> the filtered scanlines of a 16-bit grey PNG, in numpy."""
    H, W = values.shape
    rows = np.zeros((H, 1 + 2 * W), dtype=np.uint8)
    rows[:, 1::2] = values >> 8
    rows[:, 2::2] = values & 255
    return rows


@pytest.mark.parametrize("W", [1, 2, 3, 640])
def test_encode_png_opens_in_pillow_as_16_bit(W):
    from PIL import Image
    from dro_sfm_amd.datasets.png import encode_png, parse_png
    H = 5
    g = np.random.RandomState(W)
    values = g.randint(0, 65536, size=(H, W))
    values.flat[0], values.flat[-1] = 65535, 0
    blob = encode_png(rows16(values), W, H, 16)
    with Image.open(io.BytesIO(blob)) as im:
        assert im.mode == "I;16" and im.size == (W, H)
        assert np.array_equal(np.array(im, dtype=int), values)
    info = parse_png(blob)                                   # the package's own reader checks every CRC
    assert (info.width, info.height, info.kind) == (W, H, 16)


def test_encode_png_rgb_and_bad_arguments():
    from PIL import Image
    from dro_sfm_amd.datasets.png import encode_png
    g = np.random.RandomState(0)
    img = g.randint(0, 256, size=(4, 7, 3)).astype(np.uint8)
    rows = np.zeros((4, 1 + 21), dtype=np.uint8)
    rows[:, 1:] = img.reshape(4, 21)
    with Image.open(io.BytesIO(encode_png(rows, 7, 4, 2))) as im:
        assert im.mode == "RGB" and np.array_equal(np.array(im), img)
    assert encode_png(rows.tobytes(), 7, 4, 2) == encode_png(rows, 7, 4, 2)
    with pytest.raises(ValueError, match="kind"):
        encode_png(rows, 7, 4, 3)
    with pytest.raises(ValueError, match="rows"):
        encode_png(rows, 7, 5, 2)
    with pytest.raises(ValueError, match="rows"):
        encode_png(rows, 0, 4, 2)


# ------------------------------------------------------------------ C ABI
def test_exports_declared(lib):
    from dro_sfm_amd.hip import _lib
    declared = set(re.findall(r"\b(dro_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    for n in NEW:
        assert n in declared and n in _lib.EXPORTED and hasattr(lib, n), n
    assert _lib.EXPORTED[-len(NEW):] == NEW                  # appended, nothing reordered
    assert lib.dro_abi_version() == 10


def test_percentile_arguments_rejected(lib, p):
    for values, out in ((None, p), (p, None)):
        assert lib.dro_percentile(values, 1, 4, 95.0, 0, out, None) == -1
        assert b"NULL" in lib.dro_last_error()
    for B, n in ((0, 4), (-1, 4), (65536, 4), (1, 0), (1, -3), (1, 1 << 31)):
        assert lib.dro_percentile(p, B, n, 95.0, 0, p, None) == -2, (B, n)
        assert b"sizes" in lib.dro_last_error()
    for q in (-0.5, 100.5, NAN):
        assert lib.dro_percentile(p, 1, 4, q, 0, p, None) == -3, q
        assert b"q outside" in lib.dro_last_error()


def test_colorize_arguments_rejected(lib, p):
    # x, norm, lut are needed; one of color and panel; rgb with a panel
    for x, norm, lut, rgb, color, panel in ((None, p, p, None, p, None), (p, None, p, None, p, None),
                                            (p, p, None, None, p, None), (p, p, p, None, None, None),
                                            (p, p, p, p, None, None), (p, p, p, None, p, p),
                                            (p, p, p, None, None, p)):
        assert lib.dro_colorize(x, norm, lut, rgb, 1, 2, 2, color, panel, None) == -1
        assert b"NULL" in lib.dro_last_error()
    for B, H, W in ((0, 2, 2), (65536, 2, 2), (1, 0, 2), (1, 2, 0), (1, -1, 2), (1, 65536, 32768)):
        assert lib.dro_colorize(p, p, p, None, B, H, W, p, None, None) == -2, (B, H, W)
        assert b"sizes" in lib.dro_last_error()


def test_depth_png16_rows_arguments_rejected(lib, p):
    for depth, rows in ((None, p), (p, None)):
        assert lib.dro_depth_png16_rows(depth, 1, 2, 2, rows, None) == -1
        assert b"NULL" in lib.dro_last_error()
    for B, H, W in ((0, 2, 2), (65536, 2, 2), (1, 0, 2), (1, 2, 0), (1, 2, -1), (1, 32768, 65536)):
        assert lib.dro_depth_png16_rows(p, B, H, W, p, None) == -2, (B, H, W)
        assert b"sizes" in lib.dro_last_error()


def test_wrappers_refuse_cpu_tensors_and_colormaps():
    import dro_sfm_amd.hip as hip
    from dro_sfm_amd.models.infer import infer_sequence
    from dro_sfm_amd.utils.depth import viz_inv_depth, write_depth
    x = torch.ones(1, 4, 4)
    with pytest.raises(RuntimeError, match="ROCm device"):
        hip.percentile(x.reshape(1, 16), 95)
    with pytest.raises(RuntimeError, match="ROCm device"):
        hip.colorize(x, torch.ones(1), torch.zeros(256, 3))
    with pytest.raises(RuntimeError, match="ROCm device"):
        hip.depth_png16_rows(x)
    with pytest.raises(RuntimeError, match="ROCm device"):
        viz_inv_depth(x, normalizer=1.0)
    with pytest.raises(RuntimeError, match="ROCm device"):
        write_depth("unused.png", x)
    with pytest.raises(RuntimeError, match="ROCm device"):
        infer_sequence(torch.nn.Identity(), torch.zeros(3, 3, 4, 4), torch.eye(3))
    with pytest.raises(NotImplementedError, match="plasma"):
        viz_inv_depth(x, colormap="viridis")
    with pytest.raises(NotImplementedError):
        write_depth("unused.tiff", x)


def test_depth_files_round_trip_on_the_host(tmp_path):
    """The .npz branch needs no device: the reference's keys, and load_depth."""
    from dro_sfm_amd.utils.depth import load_depth, write_depth
    depth = torch.arange(12, dtype=torch.float32).reshape(1, 1, 3, 4) / 7
    K = torch.tensor([[50.0, 0.0, 2.0], [0.0, 51.0, 1.5], [0.0, 0.0, 1.0]])
    path = str(tmp_path / "d.npz")
    write_depth(path, depth, intrinsics=K)
    with np.load(path) as z:
        assert sorted(z.files) == ["depth", "intrinsics"]
        assert np.array_equal(z["depth"], depth[0, 0].numpy()) and np.array_equal(z["intrinsics"], K.numpy())
    assert np.array_equal(load_depth(path), depth[0, 0].numpy())
    with pytest.raises(NotImplementedError):
        load_depth(str(tmp_path / "d.exr"))
