"""ResNet-18 trunk (layers 1-3) with the stride-8 fusion head.

State-dict compatible with the reference ResNetEncoder
(dro_sfm/networks/optim/extractor.py:7-107): conv1/bn1, layer1..layer3 of
BasicBlocks (conv1/bn1/conv2/bn2[/downsample.0,1]), upconv1.0,
upconv1_fusion.0, out_conv (+ upconv2*, stride 4).  Pretrained ImageNet
weights are never downloaded -- load a checkpoint instead.

Training-mode batch normalisation (round 6) runs INSIDE the 3x3 stride-1
convolutions at the sites whose channels hold more than 16 K elements (the
layer1 blocks of fnet and cnet_pose at KITTI size; hip.bnconv's size policy,
"all" for every stride-1 site) (hip.bnconv, csrc/conv.hip BnFuse): the
producing conv's epilogue takes the batch statistics, the consuming conv
stages relu(bn(.) [+ skip]) and stores it once, the consumer's data gradient
takes the BN backward's statistics; a stage's first block output is staged by
the second block's conv1 (run_stage).  After the stride-2 convs (stage
entries, downsamples, stems) BN runs as hip.batchnorm_act (csrc/batchnorm.hip:
one launch each way where a channel fits one block, two otherwise) -- both
with fixed-order fp64 statistics, against 6-9 PyTorch launches per site
(DRO_BN_FUSION=0|large|all / hip.bnconv.set_bn_fusion: A/B runs).  Not MIOpen's BN: measured on MI355X
in round 2, its one-pass variance put 1e-2 relative error on encoder gradients
against the fp64 oracle.  Eval mode and CPU tensors use PyTorch's native
kernels; with set_fused_eval_batchnorm(True) (default off; InferenceSession
switches it on) eval-mode BN + skip + ReLU on the GPU is one launch of
hip.batchnorm_eval_act per site, which reads the running statistics itself.
The 2x bilinear upsampling of the fusion head is a HIP kernel
(hip.bilinear_upsample2x): ATen's loops over all planes per output pixel.  So
is the stem's 3x3/s2 max pooling (hip.maxpool3x3s2, bit-identical to
F.max_pool2d forward and backward; ATen's backward took 55 us per call).
The stride-1 3x3 convolutions (layer1-3, the fusion head with its concat read
in place, out_conv) run on the HIP conv engine's halo-tiled kernels
(conv3x3); on the trainer path their weight gradients -- one use each -- are
launched in groups of up to 8 weights per stream (hip/conv.py, grouped weight
gradients).  The 7x7/s2 stems, 3x3/s2 stage entries and 1x1/s2 downsamples
run on the flattened implicit GEMM with the stride (forward), its
parity-class form (data gradient: each input-pixel parity class takes only
its own taps) and the generic weight-gradient kernel -- no MIOpen in the
encoders, so the training step is bitwise repeatable (round 4: MIOpen's
stride-2 forward differed run to run by ~1e-6, which the untrained recurrence
amplified to 2e-4 in the loss).  set_native_strided_convs(False) puts them on
MIOpen for A/B runs.
"""
import contextlib
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import hip
from ...hip import bnconv


_FUSED_BN = [True]
_NATIVE_POOL = [True]
_NATIVE_CONV = [True]
# DRO_NATIVE_STRIDED=0: the stride-2 convolutions on MIOpen from the start
# (A/B parity runs of the whole suite on that path)
_NATIVE_STRIDED = [os.environ.get("DRO_NATIVE_STRIDED", "1") == "1"]


def set_native_strided_convs(enabled):
    """The stride-2 stems / stage entries / 1x1 downsamples on the HIP engine
    (True, default) or MIOpen (False, A/B runs).  Measured round 4 (KITTI
    metric step): 15.0-15.2 ms native vs 14.95 ms with these on MIOpen, whose
    forward is not run-to-run deterministic; parity is tested either way
    (tests/test_conv_engine.py, DRO_NATIVE_STRIDED=0 for the whole suite)."""
    _NATIVE_STRIDED[0] = bool(enabled)


def set_native_convs(enabled):
    """Every encoder convolution on the HIP f32-MFMA engine (default True) or
    on MIOpen (False, A/B runs): stride-1 3x3 on the halo kernels, the stride-2
    stems / stage entries / 1x1 downsamples on the flattened implicit GEMM."""
    _NATIVE_CONV[0] = bool(enabled)


def conv3x3(m, srcs, act=None):
    """act(m(cat(srcs))) for an nn.Conv2d m on the HIP conv engine
    (csrc/conv.hip): stride-1 3x3 'same' convolutions on the halo kernels
    (sources read as a virtual concatenation, bias + ReLU in the epilogue);
    stride-1/2 convolutions of one source (the 7x7/s2 stems, 3x3/s2 stage
    entries, 1x1/s2 downsamples) on the flattened implicit GEMM; weight
    gradients in place into the trainer's flat buffer.  CPU tensors (and the
    MIOpen A/B switch) go through m."""
    srcs = list(srcs) if isinstance(srcs, (list, tuple)) else [srcs]
    if (_NATIVE_CONV[0] and srcs[0].is_cuda and m.kernel_size == (3, 3) and m.stride == (1, 1)
            and m.padding == (1, 1) and m.dilation == (1, 1) and m.groups == 1):
        return hip.conv2d(srcs, m.weight, m.bias, act=act)
    if (_NATIVE_CONV[0] and _NATIVE_STRIDED[0] and srcs[0].is_cuda and len(srcs) == 1 and m.stride[0] == m.stride[1]
            and m.stride[0] in (1, 2) and m.padding[0] == m.padding[1] and m.dilation == (1, 1)
            and m.groups == 1 and m.padding_mode == "zeros" and (act is None or not torch.is_grad_enabled())):
        # the stride-2 stems / stage entries / downsamples (no activation follows
        # them in the encoders: BatchNorm does)
        return hip.conv2d_strided(srcs[0], m.weight, m.bias, m.stride[0], m.padding[0], act)
    y = m(srcs[0] if len(srcs) == 1 else torch.cat(srcs, 1))
    return F.relu(y, inplace=True) if act == "relu" else y


def set_native_maxpool(enabled):
    """hip.maxpool3x3s2 for the stem pooling on the GPU (default True)."""
    _NATIVE_POOL[0] = bool(enabled)


def set_fused_batchnorm(enabled):
    """hip.batchnorm_act for training-mode BN+ReLU on the GPU (default True)."""
    _FUSED_BN[0] = bool(enabled)


_FUSED_EVAL_BN = [False]


def set_fused_eval_batchnorm(enabled):
    """hip.batchnorm_eval_act for eval-mode BN (+ skip) (+ ReLU) on the GPU: one
    launch per site instead of ATen's batch_norm, add and relu (default False:
    the eval path is then exactly the ATen one).  models.session.InferenceSession
    switches it on around its forwards.  Returns the previous setting."""
    prev = _FUSED_EVAL_BN[0]
    _FUSED_EVAL_BN[0] = bool(enabled)
    return prev


@contextlib.contextmanager
def fused_eval_batchnorm(enabled=True):
    """set_fused_eval_batchnorm(enabled) for the duration of a with block; the
    previous setting is restored on the way out, also after an exception."""
    prev = set_fused_eval_batchnorm(enabled)
    try:
        yield
    finally:
        _FUSED_EVAL_BN[0] = prev


def _needs_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _fused_bn_ok(bn, conv, x, stride=1):
    """BN inside the conv launches (hip.bnconv) for this site: the native conv
    engine and the fused BN are on, the conv is 3x3 stride 1 and the site is
    inside hip.bnconv's size policy (x: the block input, `stride` the block's)."""
    if x.dim() != 4:
        return False
    elems = x.shape[0] * ((x.shape[2] - 1) // stride + 1) * ((x.shape[3] - 1) // stride + 1)
    return _FUSED_BN[0] and _NATIVE_CONV[0] and bnconv.supported(bn, conv, x, elems)


class BatchNorm2d(nn.BatchNorm2d):
    """nn.BatchNorm2d (same state_dict) computed by the native kernels."""

    def forward(self, x):
        with torch.backends.cudnn.flags(enabled=False):
            return super().forward(x)

    def act(self, x, skip=None, relu=True):
        """relu(bn(x) + skip): one fused op in training mode on the GPU."""
        if _FUSED_BN[0] and self.training and x.is_cuda and self.momentum is not None:
            y = hip.batchnorm_act(x, self, skip=skip, relu=relu)
            if relu:   # parity tests: the ReLU branch this site took (hip.record_bilinear_cells)
                hip.ops.record_branch(("relu", getattr(self, "_dro_tag", None)), lambda: (y > 0).to(torch.uint8), x)
            return y
        if (_FUSED_EVAL_BN[0] and not self.training and x.is_cuda
                and not _needs_grad(x, skip, self.weight, self.bias)):
            # eval mode (inference): BN on the running statistics, the skip and
            # the ReLU in one launch (set_fused_eval_batchnorm, default off)
            return hip.batchnorm_eval_act(x, self, skip=skip, relu=relu)
        y = self(x)
        if skip is not None:
            y = y + skip
        return F.relu(y, inplace=True) if relu else y


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, cin, cout, stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False),
                                            BatchNorm2d(cout))

    def fused_ok(self, x):
        """BN inside the 3x3 stride-1 convs (hip.bnconv) for this block."""
        return _fused_bn_ok(self.bn2, self.conv2, x, self.conv1.stride[0])

    def forward_z2(self, x):
        """(z2, skip): conv2's output with bn2's statistics taken (hip.bnconv)
        and the skip -- relu(bn2(z2) + skip) is the block's output.  In a
        stride-1 block conv1 takes bn1's statistics and conv2 stages
        relu(bn1(.)) itself; a stride-2 block keeps bn1 / the downsample's BN
        after the strided convs (hip.batchnorm_act)."""
        x = hip.grad_sink(x)
        if self.downsample is None and bnconv.supported(self.bn1, self.conv1, x):
            z1 = bnconv.conv_bn_stats(x, self.conv1, self.bn1)
            return bnconv.bn_relu_conv_stats(z1, self.bn1, self.conv2, self.bn2), x
        y = self.bn1.act(conv3x3(self.conv1, x))
        skip = x if self.downsample is None else self.downsample[1].act(conv3x3(self.downsample[0], x), relu=False)
        return bnconv.conv_bn_stats(y, self.conv2, self.bn2), skip

    def forward_after(self, z2p, skipp, bn2p):
        """This (stride-1) block on the previous block's (z2, skip, bn2): its
        conv1 stages the previous output relu(bn2p(z2p) + skipp) and stores it
        (it is this block's skip) -- no apply launch for the previous block."""
        x, z1 = bnconv.bn_add_relu_conv_stats(z2p, bn2p, skipp, self.conv1, self.bn1)
        z2 = bnconv.bn_relu_conv_stats(z1, self.bn1, self.conv2, self.bn2)
        return bnconv.bn_apply(z2, self.bn2, skip=x)

    def forward(self, x):
        # conv1, the skip (or the downsample) all read x: their input gradients
        # meet in place in a sink (the skip's BN backward writes it first)
        if self.fused_ok(x):
            z2, skip = self.forward_z2(x)
            return bnconv.bn_apply(z2, self.bn2, skip=skip)
        x = hip.grad_sink(x)
        y = self.bn1.act(conv3x3(self.conv1, x))
        if self.downsample is None:
            skip = x
        else:
            skip = self.downsample[1].act(conv3x3(self.downsample[0], x), relu=False)
        return self.bn2.act(conv3x3(self.conv2, y), skip=skip)


def _stage(cin, cout, stride):
    return nn.Sequential(BasicBlock(cin, cout, stride), BasicBlock(cout, cout, 1))


def run_stage(stage, x):
    """stage(x) for a ResNet stage of two BasicBlocks; with the fused BN path
    the first block's output is staged by the second block's conv1
    (BasicBlock.forward_after) instead of being applied by its own launch."""
    b0, b1 = stage[0], stage[1]
    if (len(stage) == 2 and b0.fused_ok(x) and b1.downsample is None
            and bnconv.supported(b1.bn1, b1.conv1, x) and b1.fused_ok(x)):
        z2, skip = b0.forward_z2(x)
        return b1.forward_after(z2, skip, b0.bn2)
    return stage(x)


class ResNetEncoder(nn.Module):
    """Feature/context encoder; input [B, 3*num_input_images, H, W] or a list
    of such tensors (batched along dim 0, split back on return)."""

    def __init__(self, num_layers=18, num_input_images=1, pretrained=False, out_chs=32, stride=8):
        super().__init__()
        if num_layers != 18:
            raise NotImplementedError("only the ResNet-18 trunk is used by DepthPoseNet")
        if stride not in (4, 8):
            raise NotImplementedError("stride must be 4 or 8 (extractor.py:28-41)")
        self.stride = stride
        self.conv1 = nn.Conv2d(3 * num_input_images, 64, 7, 2, 3, bias=False)
        self.bn1 = BatchNorm2d(64)
        self.layer1 = _stage(64, 64, 1)
        self.layer2 = _stage(64, 128, 2)
        self.layer3 = _stage(128, 256, 2)
        self.upconv1 = nn.Sequential(nn.Conv2d(256, 128, 3, 1, 1), nn.ReLU(inplace=True))
        self.upconv1_fusion = nn.Sequential(nn.Conv2d(256, 128, 3, 1, 1), nn.ReLU(inplace=True))
        if stride == 4:
            self.upconv2 = nn.Sequential(nn.Conv2d(128, 64, 3, 1, 1), nn.ReLU(inplace=True))
            self.upconv2_fusion = nn.Sequential(nn.Conv2d(128, 64, 3, 1, 1), nn.ReLU(inplace=True))
            self.out_conv = nn.Conv2d(64, out_chs, 3, 1, 1)
        else:
            self.out_conv = nn.Conv2d(128, out_chs, 3, 1, 1)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        chunks = None
        if isinstance(x, (list, tuple)):
            chunks = len(x)
            x = torch.cat(list(x), 0)
        x = self.bn1.act(conv3x3(self.conv1, x))
        x = (hip.maxpool3x3s2(x, getattr(self, "_dro_tag", None)) if (x.is_cuda and _NATIVE_POOL[0])
             else F.max_pool2d(x, 3, 2, 1))
        s4 = run_stage(self.layer1, x)
        s8 = run_stage(self.layer2, s4)
        x = run_stage(self.layer3, s8)
        rec = hip.ops.record_relu         # parity tests: the ReLU branch of each decoder conv
        x = rec(conv3x3(self.upconv1[0], hip.bilinear_upsample2x(x), "relu"), self.upconv1[0])
        x = rec(conv3x3(self.upconv1_fusion[0], [x, s8], "relu"), self.upconv1_fusion[0])   # concat read in place
        if self.stride == 4:
            x = rec(conv3x3(self.upconv2[0], hip.bilinear_upsample2x(x), "relu"), self.upconv2[0])
            x = rec(conv3x3(self.upconv2_fusion[0], [x, s4], "relu"), self.upconv2_fusion[0])
        x = conv3x3(self.out_conv, x)
        if chunks is not None:
            return torch.chunk(x, chunks, 0)
        return x
