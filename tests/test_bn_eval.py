"""Eval-mode BatchNorm + skip + ReLU in one launch (csrc/batchnorm.hip
bn_eval_kernel, hip.batchnorm_eval_act) against a float64 restatement, and the
encoders' eval path with networks.optim.extractor.set_fused_eval_batchnorm.

Bound: the project's parity bound, |y - ref| <= 1e-4 * max|ref|.  What the
kernel can differ by: x - mean is one fp32 rounding of the RESULT (relative
6e-8 of |x - mean|, whatever |mean| is), k = gamma / sqrtf(var + eps) three
roundings (~2e-7 relative), the fma and the add one each -- a few 1e-7 of
the largest term, which max|ref| bounds from above up to the cancellation
between k (x - mean), beta and skip that the inputs here do not provoke.
The same bound is also asked of every channel on its own, there against the
channel's largest |k (x - mean)| + |beta| + |skip| (what the roundings are
relative to): with two elements per channel, as in the 600 000-channel shape,
a channel's own max|ref| cancels to nearly 0 somewhere.
With ReLU, outputs whose float64 pre-activation lies below -1e-4 * max|ref|
must be exactly 0.  Largest errors observed on MI355X: DESIGN.md §13."""
import functools

import pytest
import torch

import dro_sfm_amd.hip  # noqa: F401  (registers the ops)

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
EPS = 1e-5
SHAPES = [(1, 1, 1, 1),            # smallest input
          (2, 3, 5, 7),            # HW = 35: scalar path, odd tail
          (2, 5, 3, 3),            # HW = 9: planes not 16-byte aligned
          (3, 64, 6, 20),          # vector path
          (6, 64, 48, 160),        # 8 vector rounds per plane over 6 blocks: crosses the grid's stride within a plane
          (2, 600000, 1, 1)]       # 1.2 M planes, more than the grid's 2^20 blocks: a block takes a second plane


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """x, skip and per-channel statistics / affine parameters (shared by the
    cases of a shape, never modified): channel 0 has running_var 1e-8 beside
    eps 1e-5, odd channels a negative gamma, channel 2 (where there is one;
    channel 0 of a single-channel input) a mean far from the data."""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(N * 1000003 + C * 1009 + H * 31 + W)
    x = torch.randn(shape, generator=g)
    skip = torch.randn(shape, generator=g)
    mean = 0.5 * torch.randn(C, generator=g)
    var = 0.25 + torch.rand(C, generator=g)
    gamma = 0.5 + torch.rand(C, generator=g)
    beta = torch.randn(C, generator=g)
    var[0] = 1e-8
    gamma[1::2] *= -1.0
    mean[2 if C > 2 else 0] = 57.0
    return tuple(t.to(DEV) for t in (x, skip, mean, var, gamma, beta))


def restated(x, skip, mean, var, gamma, beta, relu):
    """float64: (pre-activation, output, |k (x - mean)| + |beta| + |skip|: the size of what is summed)."""
    d = lambda t: t.double().view(1, -1, 1, 1)
    k = (d(gamma) if gamma is not None else 1.0) / torch.sqrt(d(var) + float(torch.tensor(EPS, dtype=torch.float32)))
    pre = (x.double() - d(mean)) * k
    if beta is not None:
        pre = pre + d(beta)
    if skip is not None:
        pre = pre + skip.double()
    terms = ((x.double() - d(mean)) * k).abs() + (d(beta).abs() if beta is not None else 0.0)
    if skip is not None:
        terms = terms + skip.double().abs()
    return pre, (pre.clamp_min(0.0) if relu else pre), terms


WORST = {}


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("with_skip", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_against_float64(shape, with_skip, relu, affine):
    x, skip, mean, var, gamma, beta = inputs(shape)
    skip = skip if with_skip else None
    gamma, beta = (gamma, beta) if affine else (None, None)
    keep = [t.clone() for t in (x, mean, var)]
    y = torch.ops.dro.batchnorm_eval_act(x, gamma, beta, mean, var, skip, relu, EPS)
    torch.cuda.synchronize()
    pre, ref, terms = restated(x, skip, mean, var, gamma, beta, relu)
    scale = float(ref.abs().max())
    err = float((y.double() - ref).abs().max())
    rel = err / scale if scale > 0 else 0.0
    WORST[shape] = max(WORST.get(shape, 0.0), rel)
    cerr, cscale = (y.double() - ref).abs().amax((0, 2, 3)), terms.amax((0, 2, 3))
    chan = float((cerr / cscale.clamp_min(1e-300)).max())
    print(f"batchnorm_eval_act {shape} skip={with_skip} relu={relu} affine={affine}: max|d| {err:.3e}, "
          f"max|ref| {scale:.3e}, ratio {rel:.2e} (worst of this shape so far {WORST[shape]:.2e}), "
          f"worst channel against its own largest summed terms {chan:.2e}")
    assert y.shape == x.shape and y.dtype == torch.float32 and y.is_contiguous()
    assert bool(torch.isfinite(y).all())
    assert err <= TOL * scale
    # channel by channel as well (the 1e-8 variance channel sets max|ref| of the whole tensor), against the
    # channel's largest |k (x - mean)| + |beta| + |skip|: a channel's max|ref| itself can cancel to nearly 0
    assert bool((cerr <= TOL * cscale).all()), chan
    if relu:
        off = pre < -TOL * scale
        assert torch.equal(y[off], torch.zeros_like(y[off]))
        assert float(y.min()) >= 0.0
        if x.numel() > 100:
            assert bool(off.any()) and bool((pre > TOL * scale).any())
    # inputs untouched, and the same bits again (no atomics, nothing cached)
    assert all(torch.equal(a, b) for a, b in zip(keep, (x, mean, var)))
    assert torch.equal(y, torch.ops.dro.batchnorm_eval_act(x, gamma, beta, mean, var, skip, relu, EPS))


def test_statistics_are_read_on_each_launch():
    """In-place updates of the statistics and of the affine parameters reach the
    next call: nothing is folded or cached on the host."""
    import dro_sfm_amd.hip as hip
    from dro_sfm_amd.networks.optim.extractor import BatchNorm2d
    x, skip, mean, var, gamma, beta = inputs((3, 64, 6, 20))
    bn = BatchNorm2d(64).to(DEV).eval()
    with torch.no_grad():
        y0 = hip.batchnorm_eval_act(x, bn, skip=skip)
        for dst, src in ((bn.running_mean, mean), (bn.running_var, var), (bn.weight, gamma), (bn.bias, beta)):
            dst.copy_(src)
        y1 = hip.batchnorm_eval_act(x, bn, skip=skip)
    assert not torch.equal(y0, y1)
    assert torch.equal(y1, torch.ops.dro.batchnorm_eval_act(x, gamma, beta, mean, var, skip, True, bn.eps))
    assert int(bn.num_batches_tracked) == 0


def test_op_makes_strided_inputs_contiguous():
    import dro_sfm_amd.hip as hip
    from dro_sfm_amd.networks.optim.extractor import BatchNorm2d
    x, skip, mean, var, gamma, beta = inputs((3, 64, 6, 20))
    bn = BatchNorm2d(64).to(DEV).eval()
    with torch.no_grad():
        bn.running_mean.copy_(mean)
        bn.running_var.copy_(var)
        want = hip.batchnorm_eval_act(x, bn, skip=skip, relu=False)
        xs = x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
        ss = skip.to(memory_format=torch.channels_last)
        assert not xs.is_contiguous() and not ss.is_contiguous()
        assert torch.equal(hip.batchnorm_eval_act(xs, bn, skip=ss, relu=False), want)
        with pytest.raises(RuntimeError, match="skip"):
            hip.batchnorm_eval_act(x, bn, skip=skip[:, :, :3])


def test_opcheck():
    x, skip, mean, var, gamma, beta = inputs((2, 3, 5, 7))
    tests = ("test_schema", "test_faketensor")
    torch.library.opcheck(torch.ops.dro.batchnorm_eval_act.default, (x, gamma, beta, mean, var, skip, True, EPS),
                          test_utils=tests)
    torch.library.opcheck(torch.ops.dro.batchnorm_eval_act.default, (x, None, None, mean, var, None, False, EPS),
                          test_utils=tests)


# ------------------------------------------------------------------ the encoders' eval path
def randomised_encoder(stride):
    from dro_sfm_amd.networks.optim.extractor import ResNetEncoder
    torch.manual_seed(stride)
    enc = ResNetEncoder(out_chs=32, stride=stride)
    g = torch.Generator().manual_seed(100 + stride)
    with torch.no_grad():
        for m in enc.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(0.2 * torch.randn(m.num_features, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
                m.weight.copy_(0.75 + 0.5 * torch.rand(m.num_features, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.num_features, generator=g))
    return enc.to(DEV).eval()


def aten_names(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        out = fn()
    torch.cuda.synchronize()
    return out, {e.key for e in prof.key_averages()}


@pytest.mark.parametrize("stride", [8, 4])
def test_encoder_eval_path(stride, monkeypatch):
    import dro_sfm_amd.hip as hip
    from dro_sfm_amd.networks.optim import extractor as E
    enc = randomised_encoder(stride)
    x = torch.rand(2, 3, 32, 48, generator=torch.Generator().manual_seed(5)).to(DEV)
    calls = []
    real = hip.batchnorm_eval_act
    monkeypatch.setattr(hip, "batchnorm_eval_act",
                        lambda x, bn, skip=None, relu=True: (calls.append((skip is not None, relu)),
                                                             real(x, bn, skip=skip, relu=relu))[1])
    with torch.no_grad():
        off, names_off = aten_names(lambda: enc(x))
        assert not calls and any("batch_norm" in n for n in names_off)
        with E.fused_eval_batchnorm(True):
            on, names_on = aten_names(lambda: enc(x))
        assert not E._FUSED_EVAL_BN[0]
    assert not any("batch_norm" in n for n in names_on), sorted(n for n in names_on if "batch_norm" in n)
    # the stem and six bn1 (BN -> ReLU), six bn2 (BN + skip -> ReLU), two downsample BNs (BN alone)
    assert sorted(calls) == sorted([(False, True)] * 7 + [(True, True)] * 6 + [(False, False)] * 2)
    scale = float(off.abs().max())
    err = float((on - off).abs().max())
    print(f"ResNetEncoder stride {stride} eval, fused BN against ATen: max|d| {err:.3e}, max|ref| {scale:.3e}, "
          f"ratio {err / scale:.2e}")
    assert on.shape == off.shape == (2, 32, 32 // stride, 48 // stride)
    assert err <= TOL * scale
    # training mode and a forward that needs gradients keep the present paths
    with E.fused_eval_batchnorm(True):
        calls.clear()
        enc(x)                                               # eval, grad enabled, parameters require grad
        assert not calls
        enc.train()
        with torch.no_grad():
            enc(x)
        assert not calls
