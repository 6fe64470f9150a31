"""models.session.InferenceSession and the eval-BN switch without a GPU.

The package's model has no CPU path (hip.warp_cost, hip.bilinear_upsample2x
and the other ops refuse CPU tensors: tests/test_capi.py::test_no_cpu_fallback),
and infer_sequence refuses CPU frames, so the session's host logic is checked
here on a stand-in with SfmModelMF's eval interface, built from the encoders'
own BasicBlocks (every eval BatchNorm site kind: BN -> ReLU, BN + skip -> ReLU,
the downsample's BN alone), through predict_interior_frames -- the loop that
infer_sequence and reconstruct_sequence share.  The same cases on the real
it4-seq4-out model at 64x96 run on the GPU: tests/test_session.py."""
import pytest
import torch
import torch.nn as nn

from dro_sfm_amd.geometry.pose import Pose
from dro_sfm_amd.models.reconstruct import predict_interior_frames
from dro_sfm_amd.models.session import InferenceSession
from dro_sfm_amd.networks.optim import extractor as E

T, H, W = 5, 64, 96


class Standin(nn.Module):
    """{"inv_depths": [inv [B,1,H,W]], "poses": [Pose, Pose]} from rgb, the two
    context frames and the intrinsics, like SfmModelMF in eval mode."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(9, 8, 3, 1, 1, bias=False)
        self.bn = E.BatchNorm2d(8)
        self.layer = nn.Sequential(E.BasicBlock(8, 8, 1), E.BasicBlock(8, 12, 2))
        self.head = nn.Conv2d(12, 13, 3, 1, 1)
        self.calls = 0

    def forward(self, batch):
        self.calls += 1
        x = torch.cat([batch["rgb"], *batch["rgb_context"]], 1)
        x = self.layer(self.bn.act(E.conv3x3(self.conv, x)))
        y = self.head(x)
        inv = torch.sigmoid(nn.functional.interpolate(y[:, :1], scale_factor=2.0)) * batch["intrinsics"][:, :1, :1, None]
        vec = 0.01 * y[:, 1:].mean((2, 3)).view(-1, 2, 6)
        return {"inv_depths": [inv], "poses": [Pose.from_vec(vec[:, j], "euler") for j in range(2)]}


@pytest.fixture()
def model():
    torch.manual_seed(0)
    m = Standin()
    g = torch.Generator().manual_seed(1)
    for mod in m.modules():                         # statistics and affine parameters away from 0 / 1
        if isinstance(mod, nn.BatchNorm2d):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g))
            mod.running_var.copy_(0.5 + torch.rand(mod.num_features, generator=g))
            mod.weight.data.copy_(torch.randn(mod.num_features, generator=g))
            mod.bias.data.copy_(torch.randn(mod.num_features, generator=g))
    return m.eval()


@pytest.fixture()
def frames():
    return torch.rand(T, 3, H, W, generator=torch.Generator().manual_seed(2))


K = torch.tensor([[[0.58 * W, 0.0, 0.49 * W], [0.0, 1.92 * H, 0.46 * H], [0.0, 0.0, 1.0]]])


def batch_of(frames, lo=1, hi=3):
    return {"rgb": frames[lo:hi], "rgb_context": [frames[lo - 1:hi - 1], frames[lo + 1:hi + 1]],
            "intrinsics": K.expand(hi - lo, 3, 3).contiguous()}


def same(a, b):
    assert len(a["inv_depths"]) == len(b["inv_depths"]) == 1 and len(a["poses"]) == len(b["poses"]) == 2
    assert torch.equal(a["inv_depths"][0], b["inv_depths"][0])
    for p, q in zip(a["poses"], b["poses"]):
        assert isinstance(p, Pose) and torch.equal(p.vec, q.vec) and torch.equal(p.mat, q.mat)


def test_session_is_a_module_holding_the_model(model):
    s = InferenceSession(model)
    assert isinstance(s, nn.Module) and s.model is model and model in list(s.modules())
    s.train()
    assert model.training
    s.eval()
    assert not model.training and not any(m.training for m in s.modules())


def test_cpu_pass_through_equals_the_model(model, frames):
    s = InferenceSession(model)
    with torch.no_grad():
        want = model(batch_of(frames))
    got = s(batch_of(frames))
    same(got, want)
    assert s.captures == 0
    assert not got["inv_depths"][0].requires_grad            # under no_grad although the caller was not
    assert not E._FUSED_EVAL_BN[0]


def test_refuses_a_model_in_training_mode(model, frames):
    s = InferenceSession(model)
    model.train()
    calls = model.calls
    with pytest.raises(RuntimeError, match="training mode"):
        s(batch_of(frames))
    assert model.calls == calls


def test_refuses_frames_of_another_dtype_or_shape(model, frames):
    s = InferenceSession(model)
    calls = model.calls
    b = batch_of(frames)
    with pytest.raises(RuntimeError, match="float32"):
        s(dict(b, rgb=b["rgb"].double()))
    with pytest.raises(RuntimeError, match="float32"):
        s(dict(b, intrinsics=b["intrinsics"].long()))
    with pytest.raises(RuntimeError, match="does not match rgb"):
        s(dict(b, rgb_context=[b["rgb_context"][0], b["rgb_context"][1][:1]]))
    assert model.calls == calls


def test_interior_frames_through_the_session(model, frames):
    """T = 5, two frames per forward: chunks of 2 and 1."""
    with torch.no_grad():
        want = predict_interior_frames(model, frames, K, 2, "test")
    s = InferenceSession(model)
    s.eval()
    got = predict_interior_frames(s, frames, K, 2, "test")
    assert got[0].shape == (T - 2, 1, H, W) and got[1].shape == (T - 2, 2, 6)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert s.captures == 0


def test_switch_leaves_cpu_tensors_on_aten(model, frames, monkeypatch):
    import dro_sfm_amd.hip as hip

    def boom(*a, **k):
        raise AssertionError("hip.batchnorm_eval_act called for a CPU tensor")

    monkeypatch.setattr(hip, "batchnorm_eval_act", boom)
    with torch.no_grad():
        want = model(batch_of(frames))
        with E.fused_eval_batchnorm(True):
            assert E._FUSED_EVAL_BN[0]
            got = model(batch_of(frames))
    assert not E._FUSED_EVAL_BN[0]
    same(got, want)


def test_switch_function_and_context_manager():
    assert E._FUSED_EVAL_BN[0] is False                      # default off
    assert E.set_fused_eval_batchnorm(True) is False and E._FUSED_EVAL_BN[0] is True
    with E.fused_eval_batchnorm(False):
        assert E._FUSED_EVAL_BN[0] is False
    assert E._FUSED_EVAL_BN[0] is True
    assert E.set_fused_eval_batchnorm(False) is True and E._FUSED_EVAL_BN[0] is False


@pytest.mark.parametrize("before", [False, True])
def test_switch_restored_after_an_exception_inside_the_session(model, frames, before):
    seen = []

    def broken(batch):
        seen.append(E._FUSED_EVAL_BN[0])
        raise ValueError("inside the forward")

    model.forward = broken
    E.set_fused_eval_batchnorm(before)
    try:
        with pytest.raises(ValueError, match="inside the forward"):
            InferenceSession(model)(batch_of(frames))
        assert seen == [True] and E._FUSED_EVAL_BN[0] is before
        seen.clear()
        with pytest.raises(ValueError, match="inside the forward"):
            InferenceSession(model, fused_eval_bn=False)(batch_of(frames))
        assert seen == [before] and E._FUSED_EVAL_BN[0] is before
    finally:
        E.set_fused_eval_batchnorm(False)


def test_op_refuses_what_it_cannot_run():
    import dro_sfm_amd.hip as hip
    bn = E.BatchNorm2d(4).eval()
    with pytest.raises(RuntimeError, match="float32 NCHW"):
        hip.batchnorm_eval_act(torch.zeros(2, 4, 3), bn)
    with pytest.raises(RuntimeError, match="float32 NCHW"):
        hip.batchnorm_eval_act(torch.zeros(2, 4, 3, 3, dtype=torch.float64), bn)
    with pytest.raises(RuntimeError, match="running statistics"):
        hip.batchnorm_eval_act(torch.zeros(2, 4, 3, 3), nn.BatchNorm2d(4, track_running_stats=False).eval())
    with pytest.raises(RuntimeError, match="requires grad"):
        hip.batchnorm_eval_act(torch.zeros(2, 4, 3, 3), bn)              # bn.weight requires grad, grad enabled
    with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm device"):
        hip.batchnorm_eval_act(torch.zeros(2, 4, 3, 3), bn)              # no CPU fallback


def test_fake_kernel_and_schema():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert str(torch.ops.dro.batchnorm_eval_act.default._schema) == (
        "dro::batchnorm_eval_act(Tensor x, Tensor? weight, Tensor? bias, Tensor running_mean, Tensor running_var, "
        "Tensor? skip, bool relu, float eps) -> Tensor")
    with FakeTensorMode():
        x, v = torch.empty(2, 4, 5, 7), torch.empty(4)
        y = torch.ops.dro.batchnorm_eval_act(x, None, None, v, v, x, True, 1e-5)
        assert y.shape == x.shape and y.dtype == torch.float32


def test_validate_hands_the_session_to_evaluate(model):
    from collections import OrderedDict
    from dro_sfm_amd.trainers.dp_trainer import DataParallelTrainer
    model.train()
    tr = DataParallelTrainer(model)
    s = InferenceSession(model)
    got = []

    def fake(m, batch, params, demon=False):
        got.append((m, m.training, model.training))
        return {"metrics": OrderedDict(depth=torch.arange(12.0)), "inv_depth": None}

    out = tr.validate([{"rgb": torch.zeros(2, 3, 4, 4)}], None, evaluate=fake, session=s)
    assert got == [(s, False, False)] and torch.equal(out["depth"], torch.arange(12.0))
    assert model.training and s.training and all(m.training for m in model.modules())
    with pytest.raises(RuntimeError, match="this trainer's model"):
        tr.validate([], None, evaluate=fake, session=InferenceSession(Standin()))
