"""DataParallelTrainer.validate without a GPU: with a fake `evaluate` that
returns known per-batch metric vectors, the epoch result is the size-weighted
mean over all batches -- of one process, and of both ranks of a gloo group
(one packed all-reduce) -- and the model's mode is restored."""
import os
import socket
from collections import OrderedDict

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

# batch sizes per rank: unequal sizes, and a different number of batches per rank
SIZES = {0: (3, 1, 4), 1: (2, 5)}
NAMES = ("depth", "depth_pp")


def vector(rank, i, mode):
    return torch.arange(12, dtype=torch.float32) * 0.25 + 10.0 * rank + i + 100.0 * mode


def loader(rank):
    return [{"rgb": torch.zeros(b, 3, 4, 4), "tag": (rank, i)} for i, b in enumerate(SIZES[rank])]


def expected(ranks):
    total = sum(b for r in ranks for b in SIZES[r])
    return [sum(vector(r, i, m).double() * b for r in ranks for i, b in enumerate(SIZES[r])) / total
            for m in range(len(NAMES))]


class Fake:
    """Stands in for evaluate_depth: known vectors, and a record of how it was called."""

    def __init__(self):
        self.calls = []

    def __call__(self, model, batch, params, demon=False):
        self.calls.append((model.training, model.bn.training, params, demon))
        rank, i = batch["tag"]
        return {"metrics": OrderedDict((n, vector(rank, i, m)) for m, n in enumerate(NAMES)), "inv_depth": None}


class Toy(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 4, 3)
        self.bn = nn.BatchNorm2d(4)


def check(out, ranks):
    assert list(out) == list(NAMES)
    for v, want in zip(out.values(), expected(ranks)):
        assert v.shape == (12,) and v.dtype == torch.float32
        assert torch.allclose(v.double(), want, rtol=1e-6, atol=0), (v, want)


def test_validate_single_process_weighted_mean():
    from dro_sfm_amd.trainers.dp_trainer import DataParallelTrainer
    model = Toy().train()
    model.bn.eval()                       # a frozen submodule keeps its own mode
    tr = DataParallelTrainer(model)
    fake, params = Fake(), object()
    out = tr.validate(loader(0), params, demon=True, evaluate=fake)
    check(out, (0,))
    assert len(fake.calls) == len(SIZES[0])
    assert all(c == (False, False, params, True) for c in fake.calls)      # eval mode inside, arguments passed on
    assert model.training and model.conv.training and not model.bn.training


def test_validate_without_ground_truth_is_empty():
    from dro_sfm_amd.trainers.dp_trainer import DataParallelTrainer
    tr = DataParallelTrainer(Toy().train())
    out = tr.validate(loader(0), None, evaluate=lambda *a, **k: {"metrics": OrderedDict(), "inv_depth": None})
    assert isinstance(out, OrderedDict) and not out
    assert tr.model.training


def test_validate_restores_mode_when_evaluate_raises():
    from dro_sfm_amd.trainers.dp_trainer import DataParallelTrainer
    tr = DataParallelTrainer(Toy().train())

    def broken(*a, **k):
        raise KeyError("depth")

    with pytest.raises(KeyError):
        tr.validate(loader(0), None, evaluate=broken)
    assert tr.model.training and tr.model.bn.training


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from dro_sfm_amd.trainers.dp_trainer import DataParallelTrainer, init_distributed
    init_distributed("gloo")
    model = Toy().train()
    tr = DataParallelTrainer(model)
    res = tr.validate(loader(rank), None, evaluate=Fake())
    out[rank] = ({k: v.clone() for k, v in res.items()}, model.training)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_validate_two_rank_gloo_weighted_mean():
    with mp.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
        res = dict(out)
    for rank in (0, 1):
        metrics, training = res[rank]
        check(OrderedDict((n, metrics[n]) for n in NAMES), (0, 1))
        assert training
    for n in NAMES:
        assert torch.equal(res[0][0][n], res[1][0][n]), "ranks disagree"
