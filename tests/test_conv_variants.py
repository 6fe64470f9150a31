"""Every conv-engine kernel variant pinned to a kernel-level fp64 case
(tests/conv_variants.py holds the table and the runners).

* routing (CPU): each case's declared plan classes are what dro_conv2d_plan_cin /
  dro_conv2d_strided_plan return for its shape, and a plain fp32 F.conv2d
  evaluation of the case stays below 2.5e-5 of the fp64 one on both error
  measures -- the 1e-4 bound of the GPU test then has a 4x margin that comes
  from the reference, not from the kernels;
* parity (GPU): forward + backward with the launch log on; the expected
  instantiations were launched, and the output, every source gradient and the
  weight / bias gradients are within 1e-4 of fp64 F.conv2d, globally
  (max|a - b| / max|ref|) and per channel (each output channel of the output,
  each source channel of a data gradient, each output-channel row of a weight
  gradient against that channel's own max|ref|);
* closure (GPU): every instantiation one eager KITTI (it8-seq4-inter-out,
  B=2, 192x640) or it12-h-out training step launches is in the table's
  `expect` sets (or is the grouped weight gradient of test_wgrad_group*.py).
"""
import ctypes
import os

import pytest
import torch

import conv_variants as V

CASE_IDS = [c.name for c in V.CASES]


@pytest.fixture(scope="module")
def lib():
    from dro_sfm_amd.hip import _lib
    return _lib.load()


def _plan(lib, rows, kch, c):
    info = (ctypes.c_longlong * 16)()
    assert lib.dro_conv2d_plan_cin(rows, kch, c.k[0], c.k[1], c.B, c.H, c.W, c.wcin, info) == 0
    halo, bm, ks, kin = bool(info[0]), int(info[1]), int(info[4]), int(info[15])
    return V.Plan(halo, bm, kin, ks > 1), ks


# ------------------------------------------------------------------ routing (CPU)
@pytest.mark.parametrize("name", CASE_IDS)
def test_routing(lib, name):
    c = V.BY_NAME[name]
    if c.call == "strided":
        info = (ctypes.c_longlong * 8)()
        assert lib.dro_conv2d_strided_plan(c.B, c.H, c.W, c.cin, c.cout, c.k[0], c.k[1], c.stride, c.pad, info) == 0
        got = {"fwd": V.Fl(int(info[0]), info[1] > 1), "dgrad": V.Fl(int(info[2]), info[3] > 1)}
        assert got == c.plans, (name, got)
        assert bool(info[4]) == (c.stride == 2)
        assert bool(info[5]) == V._k7_wgrad(c)
    else:
        for label, (rows, kch) in c.gemms().items():
            got, ks = _plan(lib, rows, kch, c)
            assert got == c.plans[label], (name, label, got)
            if c.thin and label == "dgrad":
                assert (4 if ks >= 4 else 2 if ks >= 2 else 1) == c.spans, (name, ks)
    bad, worst = V.calibrate(c)
    assert not bad, (name, "fp32 F.conv2d vs fp64 over 2.5e-5: change the case's inputs", bad)


def test_table_reaches_every_plan_class():
    """Every reachable (kernel shape, BM, kin) of the halo kernel in both modes,
    split-K per shape and mode, both BM and split classes of the flat kernel
    in both modes, the thin data gradient's CINP x span classes."""
    names = set().union(*(c.expect for c in V.CASES))
    for kh, kw in V.HALO_SHAPES:
        for bm, kin in ((32, 4), (32, 2), (32, 1), (64, 2), (64, 1)):
            for mode in (0, 1):
                pre, suf = f"dconv_kernel<{bm}, {kh}, {kw}, {mode}, ", f", {kin}>"
                assert any(n.startswith(pre) and n.endswith(suf) for n in names), (pre, suf)
        assert any(c.k == (kh, kw) and c.call == "conv2d" and c.plans["fwd"].split and c.plans["dgrad"].split
                   for c in V.CASES), (kh, kw)
    flat = {(c.plans[m].bm, c.plans[m].split, m) for c in V.CASES if c.call == "conv2d" and not c.thin
            for m in ("fwd", "dgrad") if not c.plans[m].halo}
    assert flat == {(bm, sp, m) for bm in (32, 64) for sp in (False, True) for m in ("fwd", "dgrad")}
    thin = [c for c in V.CASES if c.thin]
    assert {V._cinp(c.cin) for c in thin} == {1, 2, 4, 8} and {c.spans for c in thin} == {1, 2, 4}
    for n in ("igemm_kernel<32, 1, 0, 0> parity classes", "igemm_kernel<64, 1, 0, 0> parity classes", "wgrad_kernel(",
              "wgrad_k7_kernel<1, 1>", "wgrad_k7_kernel<1, 6>", "wgrad_k7_kernel<2, 3>", "wgrad_k7_kernel<2, 6>"):
        assert n in names, n
    for kh, kw in V.HALO_SHAPES:
        for multi in ("false", "true"):
            assert f"wgrad2_kernel<{kh}, {kw}, 0, {multi}, 1>" in names


def test_table_is_ragged():
    """Within each halo class: H and W no multiples of the tile, rows no
    multiple of BM, kch no multiple of CK (where Cin % 4 == 0 allows), and
    (split cases) a chunk count that kin x ksplit does not divide."""
    for c in V.CASES:
        if c.call != "conv2d" or not c.plans["fwd"].halo:
            continue
        assert c.cin % 4 == 0, c.name      # weight rows a multiple of 4 long (T is odd)
        th, tw = (4, 16) if c.k == (1, 5) else (8, 8)
        assert c.H % th and c.W % tw, c.name
        for label, (rows, kch) in c.gemms().items():
            p = c.plans[label]
            ck = (16 if p.bm == 32 else 8) * (2 if c.k == (1, 1) else 1) // (2 if c.k == (3, 3) else 1)
            # (Cin % 4 == 0: the forward's kch is always a multiple of a CK of 4)
            assert rows % p.bm and (kch % ck or (label == "fwd" and ck == 4)), (c.name, label)
            if p.split:
                assert -(-kch // ck) % (p.kin * 2), (c.name, label)


# (nuse, B, H, W, Cin, Cout, KH, KW) -> (splits, bytes): the halo weight
# gradient's split plan (csrc/conv.hip plan_wgrad2), one shape per clamp;
# bytes = align256(splits * Cout * Cin * KH * KW * 4) + align256(splits * Cout * 4)
WGRAD_PLAN_PINS = [
    ((1, 6, 48, 160, 64, 64, 3, 3), 240, 35450880),     # the benchmark's roofline call: the 256-split cap
    ((1, 2, 24, 80, 128, 128, 3, 3), 60, 35420160),     # tile-count bound
    ((1, 2, 24, 80, 256, 256, 1, 1), 15, 3947520),      # block-target bound
    ((8, 2, 24, 80, 256, 128, 1, 5), 32, 20987904),     # multi-use: tiles over (use, image, tile)
]


def test_wgrad_multi_workspace_pinned(lib):
    def align256(n):
        return (n + 255) // 256 * 256
    for shape, splits, nbytes in WGRAD_PLAN_PINS:
        nuse, B, H, W, Cin, Cout, KH, KW = shape
        assert nbytes == align256(splits * Cout * Cin * KH * KW * 4) + align256(splits * Cout * 4), shape
        assert lib.dro_conv2d_weight_grad_multi_workspace_bytes(*shape) == nbytes, shape


# ------------------------------------------------------------------ parity (GPU)
def _engines(c):
    """Both engines where the split-bf16 one (csrc/xconv.hip) takes the call."""
    both = c.call in ("conv2d", "gru_half") and c.k in V.HALO_SHAPES
    return ("f32", "split") if both else ("f32",)


@pytest.mark.gpu
@pytest.mark.parametrize("name,engine", [(c.name, e) for c in V.CASES for e in _engines(c)])
def test_parity(name, engine):
    from dro_sfm_amd.hip import conv as C
    c = V.BY_NAME[name]
    prev = C._XCONV[0]
    C.set_split_engine(engine == "split")
    try:
        names, bad, worst = V.check_gpu(c)
    finally:
        C.set_split_engine(prev)
    print(f"{name} [{engine}]: worst error {worst:.3e}; launched {sorted(names)}")
    if engine == "f32":
        assert c.expect <= names, (name, "not launched", sorted(c.expect - names), "launched", sorted(names))
    assert not bad, (name, "(label, global, per channel) over 1e-4", bad)


# ------------------------------------------------------------------ closure (GPU)
def _step_names(case):
    import test_hip_parity as T
    from common import condition_params, load_spec, params_from_spec
    tag, version, kind, mind, maxd, batch = T.full_size_case(case)
    params = condition_params(params_from_spec(load_spec(os.path.join(T.G, f"depthposenet_{tag}_keys.json"))),
                              T.FULL_DAMP)
    model = (T._selfsup_model if kind == "selfsup" else T._sup_model)(mind, maxd, tag, version, params)
    gb = {k: (v.to(V.DEV) if torch.is_tensor(v) else [t.to(V.DEV) for t in v]) for k, v in batch.items()}
    with V.conv_log() as names:
        out = model(gb)
        out["loss"].sum().backward()
        torch.cuda.synchronize()
    return names


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["kitti", "sup_view3"])
def test_step_launches_only_covered_variants(case):
    """One eager training step of the KITTI metric configuration / the
    it12-h-out configuration: every conv-engine instantiation it launches has a
    kernel-level case in the table.  A change that makes the step launch a new
    one must add a case for it to tests/conv_variants.py."""
    covered = set().union(*(c.expect for c in V.CASES)) | V.GROUP_COVERED
    names = _step_names(case)
    assert names, "the launch log is empty"
    missing = sorted(names - covered)
    assert not missing, ("instantiations without a kernel-level case in tests/conv_variants.py", missing)
