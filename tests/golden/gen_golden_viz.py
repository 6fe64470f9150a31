"""Golden vectors of the inverse-depth visualisation (test infrastructure; runs
ONLY in the build container, like gen_golden.py).

  viz_inv_depth.npz  the reference's own viz_inv_depth (dro_sfm/utils/depth.py
                     :65-99) on a 37x96 inverse depth map, and on a map with
                     zeros with filter_zeros=True: the inputs, the colours and
                     the normaliser numpy computed for each.

The reference imports `get_cmap` from matplotlib.cm, which newer matplotlib
versions no longer have: it is put back as a lookup in matplotlib.colormaps.
torchvision is absent (gen_golden's stand-in lets the module import), so the
reference's write_depth cannot run; the PNG tests compare with Pillow instead.

Usage:  python tests/golden/gen_golden_viz.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import install_shims, save  # noqa: E402

H, W = 37, 96


def inverse_depth(seed, zeros):
    """A smooth positive map with a few flat steps (ties), float32."""
    g = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    inv = 0.05 + 0.6 * (y / H) ** 2 + 0.1 * np.sin(x / 7.0) ** 2 + 0.02 * g.uniform(size=(H, W))
    inv[5:9, 10:40] = 0.25
    inv[30:, 80:] = 1.7                       # beyond the 95th percentile: clipped to the last entry
    if zeros:
        inv[g.uniform(size=(H, W)) < 0.3] = 0.0
    return inv.astype(np.float32)


def main():
    install_shims()
    import matplotlib
    import matplotlib.cm
    if not hasattr(matplotlib.cm, "get_cmap"):
        matplotlib.cm.get_cmap = lambda name: matplotlib.colormaps[name]
    from dro_sfm.utils.depth import viz_inv_depth
    out = {}
    for name, zeros in (("plain", False), ("zeros", True)):
        inv = inverse_depth(3 if zeros else 2, zeros)
        norm = np.percentile(inv[inv > 0] if zeros else inv, 95)
        # the reference divides the array it is given in place: hand it a copy
        color = viz_inv_depth(torch.from_numpy(inv.copy())[None], filter_zeros=zeros)
        assert color.shape == (H, W, 3)
        out[name + "_inv"] = inv
        out[name + "_color"] = color
        assert norm.dtype == np.float32       # numpy's percentile of float32 data is a float32
        out[name + "_norm"] = norm
        print(f"  {name}: normaliser {float(norm):.9g}, {len(np.unique(color.reshape(-1, 3), axis=0))} colours")
    # save() rounds float64 to float32: the colours are table entries and are compared as float32
    save("viz_inv_depth", **out)


if __name__ == "__main__":
    main()
