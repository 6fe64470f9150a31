"""Grouped weight gradients at the trainer level (GPU): one
DataParallelTrainer.step with the grouped launches off and one with them on,
on the small model and batch of test_graph_step.py, within the bounds of
test_direct_weight_grads_match_autograd_path (loss 1e-6 relative, flat
gradient 1e-4 relative L2: a reassociated weight-gradient sum)."""
import pytest
import torch

from oracle import dro_oracle as O
from test_graph_step import _batch, _setup

pytestmark = pytest.mark.gpu


def test_grouped_step_matches_ungrouped_step():
    import dro_sfm_amd.hip.conv as hc
    from dro_sfm_amd.trainers.dp_trainer import DataParallelTrainer
    batch = _batch()
    K0 = batch["intrinsics"].clone()
    out = {}
    prev = hc._GROUPED[0]
    hc.GROUP_LOG[0] = True
    try:
        with torch.backends.cudnn.flags(enabled=False):
            for grouped in (False, True):
                hc.set_grouped_weight_grads(grouped)
                del hc.GROUP_LAUNCHES[:]
                m = _setup()
                tr = DataParallelTrainer(m)
                batch["intrinsics"].copy_(K0)
                loss = tr.step(batch, flip=False)[0].clone()
                torch.cuda.synchronize()
                used = sum(bool(getattr(p, "_dro_direct_used", False)) for p in m.parameters())
                out[grouped] = (loss, tr.grads.flat.clone(), used, [len(g[3]) for g in hc.GROUP_LAUNCHES])
                assert not hc._READY and not hc._PENDING
    finally:
        hc.set_grouped_weight_grads(prev)
        hc.GROUP_LOG[0] = False
        del hc.GROUP_LAUNCHES[:]
    (l0, g0, u0, n0), (l1, g1, u1, n1) = out[False], out[True]
    print(f"grouped launches (members each): {n1}; loss rel {O.rel_err(l1.cpu(), l0.cpu()):.2e}, "
          f"gradient rel L2 {float((g1 - g0).norm() / g0.norm()):.2e}")
    assert n0 == [] and len(n1) > 0 and max(n1) > 1      # groups of several weights did form
    assert u0 == u1 and u1 > 20
    assert O.rel_err(l1.cpu(), l0.cpu()) < 1e-6
    assert float((g1 - g0).norm() / g0.norm()) < 1e-4
