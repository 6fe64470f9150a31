"""Golden vectors of the multi-view depth fusion (test infrastructure; runs ONLY
in the build container, like gen_golden.py).

  fusion_b2_s4.npz  the reference's own get_coordinate_xy and
                    check_geometric_consistency_batch (scripts/infer_video.py
                    :240-335) on CPU tensors, B=2 (different poses per sample),
                    S=4 source views, 37x53: the inputs, the per-view masks and
                    reprojected depths, count and fused.

scripts/infer_video.py does not import here (it needs git, cv2 and vtk at
import time), so the three function definitions are compiled out of the file at
generation time.  gemo_filter_fusion moves its inputs to "cuda"; its five
summing lines (:351-367) are restated below.  The extrinsics are world->camera,
which is what those functions expect (the reference's disabled call passes
camera->world poses; tests/reconstruct_oracle.py and DESIGN.md §10).

Usage:  python tests/golden/gen_golden_fusion.py
"""
import ast
import logging
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import REF, save  # noqa: E402
from reconstruct_oracle import make_scene  # noqa: E402

WANTED = ("get_coordinate_xy", "reproject_with_depth_batch", "check_geometric_consistency_batch")
B, S, H, W, SEED = 2, 4, 37, 53, 5
THRES_P_DIST, THRES_D_DIFF, THRES_VIEW = 1, 0.001, 1      # gemo_filter_fusion's values, sfm_params' thres_view


def reference_functions():
    path = os.path.join(REF, "scripts", "infer_video.py")
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(d.name for d in defs) == sorted(WANTED)
    ns = {"torch": torch, "logging": logging}
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns


def main():
    logging.disable(logging.WARNING)
    ref = reference_functions()
    scene = make_scene(B, S, H, W, SEED)
    depth_ref = torch.from_numpy(scene["depth_ref"])
    intr = torch.from_numpy(scene["K"])
    extr_ref = torch.from_numpy(scene["extr_ref"])
    xy = ref["get_coordinate_xy"](depth_ref.shape, device=depth_ref.device)
    geo_mask_sum = torch.zeros_like(depth_ref)
    all_srcview_depth_ests = torch.zeros_like(depth_ref)
    masks, reprojected = [], []
    for s in range(S):
        geo_mask, depth_reprojected = ref["check_geometric_consistency_batch"](
            depth_ref, torch.from_numpy(scene["depth_src"][s]),
            ref_pose={"intr": intr, "extr": extr_ref},
            src_pose={"intr": intr, "extr": torch.from_numpy(scene["extr_src"][s])},
            xy_coords=xy, thres_p_dist=THRES_P_DIST, thres_d_diff=THRES_D_DIFF)
        geo_mask_sum += geo_mask.float()
        all_srcview_depth_ests += depth_reprojected
        masks.append(geo_mask.to(torch.uint8))
        reprojected.append(depth_reprojected)
    geo_mask = (geo_mask_sum - THRES_VIEW) >= 0
    fused = (all_srcview_depth_ests + depth_ref) / (geo_mask_sum + 1)
    fused = fused * geo_mask
    count = geo_mask_sum.to(torch.uint8)
    print("  count histogram:", np.bincount(count.numpy().ravel(), minlength=S + 1).tolist())
    save("fusion_b2_s4", masks=torch.stack(masks), reprojected=torch.stack(reprojected), count=count, fused=fused,
         thres_p_dist=np.float32(THRES_P_DIST), thres_d_diff=np.float32(THRES_D_DIFF),
         thres_view=np.int32(THRES_VIEW), **scene)


if __name__ == "__main__":
    main()
