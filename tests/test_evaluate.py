"""The evaluation step on the GPU: hip.post_process_inv_depth (csrc/evalpost.hip),
models.evaluate.evaluate_depth and DataParallelTrainer.validate against the
reference's own outputs (tests/golden/gen_golden_eval.py: post_process.npz,
evaluate_depth_it8.npz) and against restatements written here.

Bounds: 1e-4 relative (max|a-b| / max|b|, the project's parity bar) for maps;
tests/test_metrics.py's close() (1e-4 relative + 1e-7) for metric vectors.  The
a1/a2/a3 counts are safe under that bound because the generator keeps every
valid pixel's ratio at least 1e-5 (relative) away from the thresholds.
"""
import os
from types import SimpleNamespace

import pytest
import torch

from common import det_init, fval, load_fixture
from gen_golden_eval import METHODS, MODES, WIDTHS, fill_bn_buffers
from oracle import dro_oracle as O
from test_metrics import close

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-4
DEV = "cuda"


def rel(a, b):
    return O.rel_err(a.cpu(), b.cpu())


@pytest.fixture(scope="module")
def post():
    return load_fixture(os.path.join(G, "post_process.npz"))


@pytest.fixture(scope="module")
def ev():
    d = load_fixture(os.path.join(G, "evaluate_depth_it8.npz"))
    d["params"] = SimpleNamespace(crop={0: "", 1: "garg", 2: "eigen_nyu"}[int(d["crop"])],
                                  min_depth=fval(d["min_depth"]), max_depth=fval(d["max_depth"]))
    return d


# ------------------------------------------------------------------ 1. kernel vs the reference's outputs
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("W", WIDTHS)
def test_post_process_golden(post, W, method):
    """Every width class (no ramp column: 2, 3 -- at 3 the centre column is its
    own mirror; one ramp column per side: 20; odd with two: 37; five: 96) and
    fuse method.  Not bit-exact by construction (the kernel forms
    linspace(0, 1, W)[x] itself); observed on MI355X: see DESIGN.md."""
    import dro_sfm_amd.hip as hip
    inv, flipped = post[f"inv_{W}"].to(DEV), post[f"flipped_{W}"].to(DEV)
    inv_pp, depth, depth_pp = hip.post_process_inv_depth(inv, flipped, method=method)
    want = {"inv_pp": post[f"pp_{method}_{W}"], "depth": post[f"depth_{W}"], "depth_pp": post[f"depth_pp_{method}_{W}"]}
    got = {"inv_pp": inv_pp, "depth": depth, "depth_pp": depth_pp}
    for k in want:
        assert got[k].shape == want[k].shape and got[k].is_cuda
        # the 1e-7 entries give depths of 1e6, which would hide the other
        # entries in max|ref|: the same bound over the entries below 1e3 as well
        small = want[k].abs() < 1e3
        errs = (rel(got[k], want[k]), rel(got[k].cpu()[small], want[k][small]))
        print(f"post_process W={W} {method} {k}: max|d|/max|ref| {errs[0]:.2e} (entries < 1e3: {errs[1]:.2e})")
        assert max(errs) < TOL, (k, errs)
    # inv2depth's `<= 0` branch: exactly 0
    assert bool((inv.cpu() <= 0).any()) and bool((want["inv_pp"] <= 0).any())
    assert torch.equal(depth.cpu()[inv.cpu() <= 0], torch.zeros(int((inv.cpu() <= 0).sum())))
    neg = want["inv_pp"] <= 0
    assert bool((inv_pp.cpu()[neg] <= 0).all())
    assert torch.equal(depth_pp.cpu()[neg], torch.zeros(int(neg.sum())))


# ------------------------------------------------------------------ 2. indexing at size
def _restated(inv, flipped, method):
    """post_process_inv_depth + inv2depth (utils/depth.py:102-121, :202-256) in torch ops."""
    B, C, H, W = inv.shape
    hat = torch.flip(flipped, [3])
    fused = {"mean": lambda: 0.5 * (inv + hat), "max": lambda: torch.max(inv, hat),
             "min": lambda: torch.min(inv, hat)}[method]()
    xs = torch.linspace(0.0, 1.0, W, device=inv.device, dtype=inv.dtype).repeat(B, C, H, 1)
    mask = 1.0 - torch.clamp(20.0 * (xs - 0.05), 0.0, 1.0)
    mask_hat = torch.flip(mask, [3])
    pp = mask_hat * inv + mask * hat + (1.0 - mask - mask_hat) * fused

    def inv2depth(v):
        d = 1.0 / v.clamp(min=1e-6)
        d[v <= 0.0] = 0.0
        return d

    return pp, inv2depth(inv), inv2depth(pp)


@pytest.mark.parametrize("shape", [(3, 5, 641), (1, 192, 640)])
@pytest.mark.parametrize("method", METHODS)
def test_post_process_indexing_at_size(shape, method):
    """More than one block per image and per row, a width that is no multiple
    of the block, a partial last block, several images; deterministic."""
    import dro_sfm_amd.hip as hip
    B, H, W = shape
    g = torch.Generator().manual_seed(17)
    inv = (0.01 + 0.49 * torch.rand(B, 1, H, W, generator=g)).to(DEV)
    flipped = (0.01 + 0.49 * torch.rand(B, 1, H, W, generator=g)).to(DEV)
    inv[0, 0, H // 2, ::7] = 0.0
    flipped[B - 1, 0, 0, ::5] = -0.1
    got = hip.post_process_inv_depth(inv, flipped, method=method)
    want = _restated(inv, flipped, method)
    for name, a, b in zip(("inv_pp", "depth", "depth_pp"), got, want):
        err = rel(a, b)
        print(f"post_process {shape} {method} {name}: {err:.2e}")
        assert err < TOL, (name, err)
    again = hip.post_process_inv_depth(inv, flipped, method=method)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


# ------------------------------------------------------------------ 3. everything after the network
def _batch(ev, *drop):
    N = ev["refs"].shape[0]
    b = {"rgb": ev["image"].to(DEV), "rgb_context": [ev["refs"][j].to(DEV) for j in range(N)],
         "intrinsics": ev["K"].to(DEV), "depth": ev["gt_depth"].to(DEV),
         "pose_context": [ev["gt_poses"][:, j].to(DEV) for j in range(N)]}
    for k in drop:
        del b[k]
    return b


def test_pipeline_after_network_golden(ev):
    """evaluate_from_inv_depths on the REFERENCE's predictions against the
    reference's post-processed map and its four metric vectors."""
    from dro_sfm_amd.geometry.pose import Pose
    from dro_sfm_amd.models.evaluate import METRICS_KEYS, evaluate_from_inv_depths
    poses = [Pose(ev["poses"][:, j].to(DEV)) for j in range(ev["poses"].shape[1])]
    out = evaluate_from_inv_depths(ev["inv"].to(DEV), ev["inv_flipped"].to(DEV), _batch(ev), ev["params"], poses)
    err = rel(out["inv_depth"], ev["inv_pp"])
    print(f"inv_pp vs reference: {err:.2e}")
    assert err < TOL
    assert list(out["metrics"]) == ["depth" + m for m in MODES]
    for mode in MODES:
        got, want = out["metrics"]["depth" + mode], ev["metrics" + mode]
        print(f"depth{mode}: " + " ".join(f"{k} {float(a):.6g}/{float(b):.6g}" for k, a, b in zip(METRICS_KEYS, got, want)))
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == (12,)
        assert close(got, want), (mode, got.cpu(), want)


def test_pipeline_after_network_demon(ev):
    """demon=True reads compute_depth_metrics_demon with the batch's
    pose_context as its gt_pose (model_wrapper.py:383-387)."""
    import dro_sfm_amd.hip as hip
    from dro_sfm_amd.geometry.pose import Pose
    from dro_sfm_amd.models.evaluate import evaluate_from_inv_depths
    from dro_sfm_amd.utils.depth import compute_depth_metrics_demon
    inv, inv_flipped, batch = ev["inv"].to(DEV), ev["inv_flipped"].to(DEV), _batch(ev)
    poses = [Pose(ev["poses"][:, j].to(DEV)) for j in range(ev["poses"].shape[1])]
    out = evaluate_from_inv_depths(inv, inv_flipped, batch, ev["params"], poses, demon=True, metrics_name="d",
                                   metrics_modes=("_pp", "_gt"))
    _, depth, depth_pp = hip.post_process_inv_depth(inv, inv_flipped)
    assert list(out["metrics"]) == ["d_pp", "d_gt"]
    for name, pred, scaled in (("d_pp", depth_pp, False), ("d_gt", depth, True)):
        want = compute_depth_metrics_demon(ev["params"], batch["depth"], batch["pose_context"], pred,
                                           use_gt_scale=scaled)
        assert close(out["metrics"][name][:9], want), (name, out["metrics"][name].cpu(), want.cpu())
        assert close(out["metrics"][name][9:], ev["metrics"][9:])
    assert not close(out["metrics"]["d_gt"][:9], ev["metrics_gt"][:9])     # not the KITTI metric


# ------------------------------------------------------------------ 4. end to end
@pytest.fixture(scope="module")
def e2e(ev):
    """The product model filled as the generator fills the reference's, one
    evaluate_depth call, and the two passes made by hand."""
    import dro_sfm_amd.hip as hip
    from dro_sfm_amd.models.evaluate import evaluate_depth
    from dro_sfm_amd.models.SfmModelMF import SfmModelMF
    from dro_sfm_amd.networks.depth_pose.DepthPoseNet import DepthPoseNet
    p = ev["params"]
    net = fill_bn_buffers(det_init(DepthPoseNet(version="it8-seq4-inter-out", min_depth=p.min_depth,
                                                max_depth=p.max_depth)))
    model = SfmModelMF(flip_lr_prob=0.0, min_depth=p.min_depth, max_depth=p.max_depth)
    model.add_depth_net(net)
    model = model.to(DEV).train()
    batch = _batch(ev)
    before = {"intrinsics": batch["intrinsics"].clone(), "rgb": batch["rgb"].clone(),
              "rgb_context": [r.clone() for r in batch["rgb_context"]]}
    out = evaluate_depth(model, batch, p)
    assert model.training
    W = batch["rgb"].shape[3]
    model.eval()
    with torch.no_grad():
        plain = model(dict(batch))
        Kf = batch["intrinsics"].clone()
        Kf[:, 0, 0] = -Kf[:, 0, 0]
        Kf[:, 0, 2] = W - Kf[:, 0, 2]
        flipped = model(dict(batch, rgb=torch.flip(batch["rgb"], [3]),
                             rgb_context=[torch.flip(r, [3]) for r in batch["rgb_context"]], intrinsics=Kf))
        inv_pp, depth, depth_pp = hip.post_process_inv_depth(plain["inv_depths"][0], flipped["inv_depths"][0])
    model.train()
    return SimpleNamespace(model=model, batch=batch, before=before, out=out, poses=plain["poses"], inv_pp=inv_pp,
                           depth=depth, depth_pp=depth_pp)


def test_evaluate_depth_matches_reference(ev, e2e):
    err = rel(e2e.out["inv_depth"], ev["inv_pp"])
    print(f"evaluate_depth inv_depth vs the reference's inv_pp: {err:.2e}")
    assert err < TOL


def test_evaluate_depth_wiring(ev, e2e):
    """The batched 2B forward equals the two passes, and each mode reads the
    prediction and scaling it names."""
    from dro_sfm_amd.geometry.pose import Pose
    from dro_sfm_amd.utils.depth import compute_depth_metrics, compute_pose_metrics
    err = rel(e2e.inv_pp, e2e.out["inv_depth"])
    print(f"two passes vs one batched forward, inv_pp: {err:.2e}")
    assert err < TOL
    B = e2e.batch["rgb"].shape[0]
    gt_pose = e2e.batch["pose_context"]
    pose_errs = torch.stack([compute_pose_metrics(ev["params"], [g[b:b + 1] for g in gt_pose],
                                                  [Pose(q.mat[b:b + 1]) for q in e2e.poses])
                             for b in range(B)]).mean(0)
    metrics = e2e.out["metrics"]
    assert list(metrics) == ["depth" + m for m in MODES]
    for mode in MODES:
        pred = e2e.depth_pp if "pp" in mode else e2e.depth
        want = compute_depth_metrics(ev["params"], e2e.batch["depth"], pred, use_gt_scale="gt" in mode)
        got = metrics["depth" + mode]
        assert got.shape == (12,) and got.dtype == torch.float32 and got.is_cuda
        assert close(got[:9], want), (mode, got.cpu(), want.cpu())
        assert close(got[9:], pose_errs), (mode, got.cpu(), pose_errs.cpu())
    # the plain and post-processed predictions really differ
    assert not close(metrics["depth"][:9], metrics["depth_pp"][:9])
    assert not close(metrics["depth"][:9], metrics["depth_gt"][:9])


def test_evaluate_depth_leaves_the_batch_alone(e2e):
    assert torch.equal(e2e.batch["intrinsics"], e2e.before["intrinsics"])
    assert torch.equal(e2e.batch["rgb"], e2e.before["rgb"])
    assert len(e2e.batch["rgb_context"]) == len(e2e.before["rgb_context"])
    assert all(torch.equal(a, b) for a, b in zip(e2e.batch["rgb_context"], e2e.before["rgb_context"]))


def test_evaluate_depth_without_ground_truth(ev, e2e):
    from dro_sfm_amd.models.evaluate import evaluate_depth
    out = evaluate_depth(e2e.model, _batch(ev, "depth"), ev["params"])
    assert len(out["metrics"]) == 0
    assert rel(out["inv_depth"], e2e.out["inv_depth"]) < TOL
    out = evaluate_depth(e2e.model, _batch(ev, "pose_context"), ev["params"])
    for mode in MODES:
        assert torch.equal(out["metrics"]["depth" + mode][9:].cpu(), torch.zeros(3))
        assert close(out["metrics"]["depth" + mode][:9], e2e.out["metrics"]["depth" + mode][:9])


# ------------------------------------------------------------------ 5. validation between graph replays
def test_validate_does_not_disturb_graphed_training():
    """tests/test_graph_step.py::_graph_vs_eager's set-up: a replayed step after a
    validate() gives the loss and gradient of the same step without it, the
    BatchNorm buffers are untouched and the model is back in train mode."""
    with torch.backends.cudnn.flags(enabled=False):
        _validate_between_replays()


def _validate_between_replays():
    from test_graph_step import _batch as train_batch, _setup
    from dro_sfm_amd.models.evaluate import METRICS_KEYS
    from dro_sfm_amd.trainers.dp_trainer import DataParallelTrainer, GraphedTrainStep
    batch = train_batch()
    K0 = batch["intrinsics"].clone()
    m = _setup()
    tr = DataParallelTrainer(m, capturable=True)
    gs = GraphedTrainStep(tr, batch, warmup=3)
    snap_m = {k: v.clone() for k, v in m.state_dict().items()}
    snap_s = [{k: v.clone() for k, v in st.items()} for st in tr.optimizer.state.values()]

    def restore():
        with torch.no_grad():
            for k, v in m.state_dict().items():
                v.copy_(snap_m[k])
            for st, sv in zip(tr.optimizer.state.values(), snap_s):
                for k in st:
                    st[k].copy_(sv[k])
        batch["intrinsics"].copy_(K0)

    restore()
    l0 = gs.step(batch, flip=False)[0].clone()
    g0 = tr.grads.flat.clone()

    restore()
    g = torch.Generator(device=DEV).manual_seed(4)
    B, _, H, W = batch["rgb"].shape
    vbatch = dict(batch, depth=1.0 + 30.0 * torch.rand(B, 1, H, W, generator=g, device=DEV),
                  pose_context=[torch.eye(4, device=DEV).repeat(B, 1, 1) for _ in batch["rgb_context"]])
    for p in vbatch["pose_context"]:
        p[:, :3, 3] = 0.1 * torch.rand(B, 3, generator=g, device=DEV)
    bn = {k: v.clone() for k, v in m.state_dict().items()
          if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    assert len(bn) > 30
    out = tr.validate([vbatch], SimpleNamespace(crop="garg", min_depth=0.5, max_depth=80.0))
    assert m.training and all(mod.training for mod in m.modules())
    assert list(out) == ["depth" + mode for mode in MODES]
    assert all(v.shape == (len(METRICS_KEYS),) and bool(torch.isfinite(v).all()) for v in out.values())
    after = m.state_dict()
    for k, v in bn.items():
        assert torch.equal(after[k], v), k
    assert torch.equal(batch["intrinsics"], K0)
    l1 = gs.step(batch, flip=False)[0].clone()
    g1 = tr.grads.flat.clone()
    torch.cuda.synchronize()
    le, ge = O.rel_err(l1.cpu(), l0.cpu()), float((g1 - g0).norm() / g0.norm())
    print(f"replay after validate vs replay: loss {le:.2e}, gradient L2 {ge:.2e}")
    assert le < 1e-5
    assert ge < 1e-4
