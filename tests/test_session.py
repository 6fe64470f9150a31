"""models.session.InferenceSession on the GPU: graph replays of the eval forward
against the eager forward (it4-seq4-out, 64x96, B = 2, N = 2; weights as
tests/test_reconstruct.py sets them up).

The comparisons are bitwise (torch.equal): every kernel of the eval forward is
deterministic and a replay launches the kernels the eager forward launches, on
the same arguments.  The eager side runs under fused_eval_batchnorm(True), the
BatchNorm formula the session captures.  One row is not bitwise: the graphed
TRAINING step after a validate().  The backward's fp32 atomics arrive in any
order, and two trajectories of two steps part further than that (Adam turns an
all-noise gradient into an all-noise update, and the second step's
min-reprojection selection is discontinuous in the parameters), so the
comparison is made where only the validate differs: after the first step the
whole state is saved; the second step is taken from those bits, and again from
those bits with the validate in between.  It is then bounded as
tests/test_graph_step.py and tests/test_evaluate.py bound one step from one
state: loss within 1e-5 relative, gradient within 1e-4 relative L2, parameters
within 1e-5 absolute.  That validate() itself changes nothing is checked
bitwise (parameters, buffers, Adam state, gradients, the batch)."""
from types import SimpleNamespace

import pytest
import torch

from common import DAMPED, det_init, smooth_images

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W = 64, 96


def make_batch(B, seed, N=2):
    g = torch.Generator().manual_seed(seed)
    K = torch.tensor([[0.58 * W, 0.0, 0.49 * W], [0.0, 1.92 * H, 0.46 * H], [0.0, 0.0, 1.0]])
    return {"rgb": torch.rand(B, 3, H, W, generator=g).to(DEV),
            "rgb_context": [torch.rand(B, 3, H, W, generator=g).to(DEV) for _ in range(N)],
            "intrinsics": K.repeat(B, 1, 1).to(DEV)}


@pytest.fixture(scope="module")
def model():
    from dro_sfm_amd.models.SfmModelMF import SfmModelMF
    from dro_sfm_amd.networks.depth_pose.DepthPoseNet import DepthPoseNet
    net = det_init(DepthPoseNet(version="it4-seq4-out", min_depth=0.1, max_depth=10.0))
    with torch.no_grad():
        for k, v in net.state_dict().items():
            if k.startswith(DAMPED) and "pose" in k and v.is_floating_point():
                v.mul_(0.002)
    m = SfmModelMF(flip_lr_prob=0.0, min_depth=0.1, max_depth=10.0)
    m.add_depth_net(net)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def batches():
    """Read-only: the two B = 2 batches and the B = 1 batch the tests share."""
    return SimpleNamespace(a=make_batch(2, 1), b=make_batch(2, 2), one=make_batch(1, 3))


def eager(model, batch):
    from dro_sfm_amd.networks.optim.extractor import fused_eval_batchnorm
    with torch.no_grad(), fused_eval_batchnorm(True):
        return model(batch)


def tensors(out):
    assert len(out["inv_depths"]) == 1 and len(out["poses"]) == 2
    return [out["inv_depths"][0]] + [p.mat for p in out["poses"]]


def same(a, b):
    ta, tb = tensors(a), tensors(b)
    for i, (x, y) in enumerate(zip(ta, tb)):
        assert x.shape == y.shape
        assert torch.equal(x, y), (i, float((x - y).abs().max()))
    return True


def session_of(model, **kw):
    from dro_sfm_amd.models.session import InferenceSession
    from dro_sfm_amd.networks.optim import extractor as E
    assert not E._FUSED_EVAL_BN[0]
    return InferenceSession(model, **kw)


def test_replay_and_second_input(model, batches):
    from dro_sfm_amd.networks.optim import extractor as E
    want_a, want_b = eager(model, batches.a), eager(model, batches.b)
    assert not torch.equal(want_a["inv_depths"][0], want_b["inv_depths"][0])
    s = session_of(model)
    got_a = s(batches.a)
    assert s.captures == 1 and not E._FUSED_EVAL_BN[0]
    assert same(got_a, want_a)
    assert got_a["inv_depths"][0].shape == (2, 1, H, W) and not got_a["inv_depths"][0].requires_grad
    kept = [t.clone() for t in tensors(got_a)]
    got_b = s(batches.b)
    assert same(got_b, want_b)
    assert all(torch.equal(x, y) for x, y in zip(tensors(got_a), kept))      # the first result is a copy
    assert same(s(batches.a), want_a)
    assert s.captures == 1
    # the fused BN is what was captured: the ATen formula differs in rounding (reported)
    with torch.no_grad():
        aten = model(batches.a)
    d = float((aten["inv_depths"][0] - want_a["inv_depths"][0]).abs().max() / aten["inv_depths"][0].abs().max())
    print(f"eval forward, fused BN against ATen BN: inv_depth max|d|/max|ref| {d:.2e}")


def test_refuses_training_mode_and_eager_modes(model, batches):
    s = session_of(model, graph=False)
    assert same(s(batches.a), eager(model, batches.a)) and s.captures == 0
    with torch.no_grad():
        aten = model(batches.a)
    assert same(session_of(model, graph=False, fused_eval_bn=False)(batches.a), aten)
    assert same(session_of(model, fused_eval_bn=False)(batches.a), aten)        # a graph of the ATen formula
    model.train()
    try:
        with pytest.raises(RuntimeError, match="training mode"):
            s(batches.a)
    finally:
        model.eval()


def test_in_place_changes_reach_the_replay(model, batches):
    s = session_of(model)
    before = s(batches.a)
    net = model.depth_net
    touched = (net.update_block_depth.depth_gru.convq1.weight, net.fnet.bn1.running_mean,
               net.cnet_depth.layer1[0].bn2.running_var)
    saved = [t.detach().clone() for t in touched]
    try:
        with torch.no_grad():
            touched[0].mul_(1.01)
            touched[1].add_(0.05)
            touched[2].mul_(1.5)
        want = eager(model, batches.a)
        assert not torch.equal(want["inv_depths"][0], before["inv_depths"][0])
        assert same(s(batches.a), want)
        assert s.captures == 1
        # load_state_dict copies in place as well
        model.load_state_dict({k: v.clone() for k, v in model.state_dict().items()})
        assert same(s(batches.a), want) and s.captures == 1
    finally:
        with torch.no_grad():
            for t, v in zip(touched, saved):
                t.copy_(v)
    assert same(s(batches.a), before) and s.captures == 1


def test_replaced_tensor_is_captured_again(model, batches):
    s = session_of(model)
    want = eager(model, batches.a)
    assert same(s(batches.a), want) and s.captures == 1
    p = model.depth_net.update_block_pose.pose_gru.convz1.weight
    old = p.data
    p.data = p.data.clone()
    assert p.data_ptr() != old.data_ptr()
    old.zero_()                                      # the captured graph still reads this storage
    assert same(s(batches.a), want)
    assert s.captures == 2
    assert same(s(batches.b), eager(model, batches.b)) and s.captures == 2


def test_new_shape_graph_limit_and_release(model, batches):
    want_a, want_one = eager(model, batches.a), eager(model, batches.one)
    s = session_of(model)
    assert same(s(batches.a), want_a) and s.captures == 1
    assert same(s(batches.one), want_one) and s.captures == 2      # a second graph
    assert same(s(batches.a), want_a) and same(s(batches.one), want_one) and s.captures == 2
    s.release()
    assert same(s(batches.one), want_one) and s.captures == 3      # afresh
    lim = session_of(model, max_graphs=1)
    assert same(lim(batches.a), want_a) and lim.captures == 1
    assert same(lim(batches.one), want_one) and lim.captures == 1  # eager beyond the limit, nothing evicted
    assert same(lim(batches.a), want_a) and lim.captures == 1


@pytest.mark.parametrize("T", [7, 5])
def test_sequences(model, T):
    """T = 7 with four frames per forward: chunks of 4 and 1, two signatures."""
    from dro_sfm_amd.models.infer import infer_sequence
    from dro_sfm_amd.models.reconstruct import reconstruct_sequence
    from dro_sfm_amd.networks.optim.extractor import fused_eval_batchnorm
    frames = smooth_images(T, H, W, 21).to(DEV)
    K = torch.tensor([[0.58 * W, 0.0, 0.49 * W], [0.0, 1.92 * H, 0.46 * H], [0.0, 0.0, 1.0]], device=DEV)
    params = SimpleNamespace(grad_max=10.0, depth_max=10.0, crop_h=4, crop_w=6, fusion_view_num=3,
                             fusion_thres_view=1, fusion_thres_p_dist=2.0, fusion_thres_d_diff=0.25)
    s = session_of(model)
    s.train()                                        # the functions set eval mode and restore what they found
    try:
        with fused_eval_batchnorm(True):
            want = infer_sequence(model, frames, K, viz=False, frames_per_forward=4)
            want_r = reconstruct_sequence(model, frames, K, params, frames_per_forward=4)
        got = infer_sequence(s, frames, K, viz=False, frames_per_forward=4)
        assert s.captures == (2 if T == 7 else 1)
        assert s.training and model.training and all(m.training for m in model.modules())
        got_r = reconstruct_sequence(s, frames, K, params, frames_per_forward=4)
        assert s.captures == (2 if T == 7 else 1)
    finally:
        s.eval()
    assert got["inv_depths"].shape == (T - 2, 1, H, W)
    assert torch.equal(got["inv_depths"], want["inv_depths"]) and torch.equal(got["poses"], want["poses"])
    assert got_r["points"].shape == want_r["points"].shape and got_r["points"].shape[0] > 0
    assert torch.equal(got_r["points"], want_r["points"]) and torch.equal(got_r["colors"], want_r["colors"])
    assert torch.equal(got_r["poses"], want_r["poses"]) and torch.equal(got_r["depths"], want_r["depths"])


def ground_truth(batch, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    B = batch["rgb"].shape[0]
    out = dict(batch, depth=0.2 + 8.0 * torch.rand(B, 1, H, W, generator=g, device=DEV),
               pose_context=[torch.eye(4, device=DEV).repeat(B, 1, 1) for _ in batch["rgb_context"]])
    for p in out["pose_context"]:
        p[:, :3, 3] = 0.1 * torch.rand(B, 3, generator=g, device=DEV)
    return out


def test_evaluate_depth(model, batches):
    from dro_sfm_amd.models.evaluate import evaluate_depth
    from dro_sfm_amd.networks.optim.extractor import fused_eval_batchnorm
    batch = ground_truth(batches.a, 4)
    params = SimpleNamespace(crop="", min_depth=0.1, max_depth=10.0)
    with fused_eval_batchnorm(True):
        want = evaluate_depth(model, batch, params)
    s = session_of(model)
    got = evaluate_depth(s, batch, params)
    assert s.captures == 1 and list(got["metrics"]) == list(want["metrics"]) and len(got["metrics"]) == 4
    for k in want["metrics"]:
        assert bool(torch.isfinite(want["metrics"][k]).all())
        assert torch.equal(got["metrics"][k], want["metrics"][k]), k
    assert torch.equal(got["inv_depth"], want["inv_depth"])


def test_validate_with_a_session_between_graphed_steps():
    with torch.backends.cudnn.flags(enabled=False):
        _validate_between_replays()


def _validate_between_replays():
    from test_graph_step import _batch as train_batch, _setup
    from dro_sfm_amd.models.session import InferenceSession
    from dro_sfm_amd.trainers.dp_trainer import DataParallelTrainer, GraphedTrainStep
    batch = train_batch()
    K0 = batch["intrinsics"].clone()
    m = _setup()
    tr = DataParallelTrainer(m, capturable=True)
    gs = GraphedTrainStep(tr, batch, warmup=3)

    def snapshot():
        return ({k: v.clone() for k, v in m.state_dict().items()},
                [{k: v.clone() for k, v in st.items()} for st in tr.optimizer.state.values()])

    def restore(snap):
        with torch.no_grad():
            for k, v in m.state_dict().items():
                v.copy_(snap[0][k])
            for st, sv in zip(tr.optimizer.state.values(), snap[1]):
                for k in st:
                    st[k].copy_(sv[k])
        batch["intrinsics"].copy_(K0)

    def step():
        loss = gs.step(batch, flip=False)[0].clone()
        return loss, tr.grads.flat.clone(), [p.detach().clone() for p in m.parameters()]

    first = step()[0]
    after_first = snapshot()                         # both second steps start from these bits
    restore(after_first)
    l0, g0, p0 = step()

    session = InferenceSession(m)
    params = SimpleNamespace(crop="garg", min_depth=0.5, max_depth=80.0)
    restore(after_first)
    loader = [ground_truth(train_batch(), 4), ground_truth(train_batch(), 5)]
    state, adam = snapshot()
    assert sum(k.endswith(("running_mean", "running_var", "num_batches_tracked")) for k in state) > 30
    grads = tr.grads.flat.clone()
    out = tr.validate(loader, params, session=session)
    assert m.training and all(mod.training for mod in m.modules())
    after = m.state_dict()
    for k, v in state.items():                           # every parameter and BN buffer, bit for bit
        assert torch.equal(after[k], v), k
    for st, sv in zip(tr.optimizer.state.values(), adam):
        assert all(torch.equal(st[k], sv[k]) for k in sv)
    assert torch.equal(tr.grads.flat, grads) and torch.equal(batch["intrinsics"], K0)
    l1, g1, p1 = step()
    torch.cuda.synchronize()
    assert session.captures == 1                     # both validation batches: one signature (2B = 4)
    assert len(out) == 4 and all(bool(torch.isfinite(v).all()) for v in out.values())
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    worst = max(float((a - b).abs().max()) for a, b in zip(p1, p0))
    ge = float((g1 - g0).norm() / g0.norm())
    print(f"step, validate with a session, step against step, step: first loss {float(first):.6f}, second loss "
          f"{rel(l1, l0):.2e}, second gradient L2 {ge:.2e}, parameters max|d| {worst:.2e}")
    assert rel(l1, l0) < 1e-5
    assert ge < 1e-4
    assert worst < 1e-5
    # the session follows the parameters Adam moved: a replay now equals the eager forward now
    from dro_sfm_amd.networks.optim.extractor import fused_eval_batchnorm
    vb = ground_truth(train_batch(), 4)
    both = {"rgb": torch.cat([vb["rgb"], vb["rgb"]]), "rgb_context": [torch.cat([r, r]) for r in vb["rgb_context"]],
            "intrinsics": torch.cat([vb["intrinsics"], vb["intrinsics"]])}
    m.eval()
    try:
        with torch.no_grad(), fused_eval_batchnorm(True):
            want = m(both)
        got = session(both)
    finally:
        m.train()
    assert session.captures == 1 and same(got, want)
