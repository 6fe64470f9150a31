"""bench.py --dump-outputs and the plain / --full split.

The CPU tests check the dump's format on host tensors (float32 arrays, one
file per name, large arrays cut to a fixed sample that is the same on every
call) and the state snapshot that the last timed step starts from.  The GPU
test starts two short plain benchmark runs with --dump-outputs side by side
and checks the result line (the headline keys, none of the --full
measurements), the files, and that the two runs wrote the same outputs.
"""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_array_small_is_whole_and_float32():
    t = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    a = bench._dump_array(t)
    assert a.dtype == np.float32 and a.shape == (3, 4)
    assert np.array_equal(a, t.numpy().astype(np.float32))


def test_dump_array_large_is_a_fixed_sample(monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    t = torch.arange(5000, dtype=torch.float32)
    a, b = bench._dump_array(t), bench._dump_array(t.clone())
    assert a.dtype == np.float32 and a.shape == (1000,)
    assert np.array_equal(a, b)                          # the same positions on every call
    assert len(np.unique(a)) == 1000 and np.all(np.diff(a) > 0)   # distinct positions, in order
    torch.manual_seed(123)                               # independent of the global generator
    assert np.array_equal(bench._dump_array(t), a)


def _fake_trainer():
    flat = {"step": torch.zeros(()), "exp_avg": torch.zeros(50), "exp_avg_sq": torch.zeros(50)}
    model = torch.nn.BatchNorm1d(4)
    return types.SimpleNamespace(flat_params=torch.linspace(0, 1, 50), model=model,
                                 grads=types.SimpleNamespace(flat=torch.linspace(-1, 0, 50)),
                                 optimizer=types.SimpleNamespace(state={"flat": flat}))


def test_dump_outputs_writes_named_float32_files(tmp_path):
    trainer = _fake_trainer()
    metrics = {"photometric_loss": torch.tensor(0.5), "a/b": torch.tensor([1.0, 2.0]), "note": "text"}
    out = tmp_path / "dump"
    names = bench.dump_outputs(str(out), torch.tensor([0.25]), metrics, trainer)
    assert names == ["grads", "loss", "metrics_a_b", "metrics_photometric_loss", "params"]
    assert sorted(os.listdir(out)) == [n + ".npy" for n in names]
    for n in names:
        assert np.load(out / (n + ".npy")).dtype == np.float32
    assert np.load(out / "loss.npy").tolist() == [0.25]
    assert np.array_equal(np.load(out / "params.npy"), trainer.flat_params.numpy())
    assert np.array_equal(np.load(out / "grads.npy"), trainer.grads.flat.numpy())


def test_snapshot_restores_training_state_in_place():
    trainer = _fake_trainer()
    st = trainer.optimizer.state["flat"]
    live = [trainer.flat_params, st["exp_avg"], st["exp_avg_sq"], st["step"]] + list(trainer.model.buffers())
    before = [t.clone() for t in live]
    ptrs = [t.data_ptr() for t in live]
    snap = bench.snapshot_state(trainer)
    with torch.no_grad():                                # a few "training steps"
        trainer.flat_params.add_(1.0)
        st["exp_avg"].fill_(3.0)
        st["exp_avg_sq"].fill_(4.0)
        st["step"].add_(7)
        trainer.model.train()(torch.randn(8, 4))         # moves running stats and num_batches_tracked
    assert not all(torch.equal(t, b) for t, b in zip(live, before))
    bench.restore_state(snap)
    assert all(torch.equal(t, b) for t, b in zip(live, before))
    assert [t.data_ptr() for t in live] == ptrs          # in place: a captured graph keeps the addresses


def _rel_l2(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((a ** 2).sum()), 1e-300))


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_plain_bench_runs_dump_the_same_outputs(tmp_path):
    """Two runs with the same arguments write the same outputs.  Bounds: the
    forward has no atomics, so the loss and the metrics agree to a few fp32 ulp
    (1e-6 relative; eps = 1.2e-7).  The warp-cost backward accumulates with
    atomic adds in no fixed order: each gradient element is a sum of up to
    thousands of fp32 terms, whose order-dependent rounding is about
    eps * sqrt(terms) ~ 1e-5 relative at the worst and far less in the L2
    norm over the tensor; 1e-5 relative L2 bounds the gradients, and the
    parameters, which move by at most lr = 2e-4 in the step, with it."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    outs = [tmp_path / "a", tmp_path / "b"]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                               "--warmup", "1", "--dump-outputs", str(o)],
                              env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for o in outs]
    results = []
    for p in procs:
        stdout, stderr = p.communicate(timeout=240)
        assert p.returncode == 0, stderr[-4000:]
        lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, stdout[-2000:]
        results.append(json.loads(lines[0]))
    for res, out in zip(results, outs):
        assert res["steps"] == 3 and res["warmup"] == 1
        assert res["metric"] == bench.METRIC and res["unit"] == "images/s" and res["dtype"] == "f32"
        assert res["higher_is_better"] is True and res["value"] > 0
        # images/s and ms/step describe the same timed steps
        assert res["ms_per_step"] > 0
        assert res["value"] == pytest.approx(1000.0 * res["config"]["global_batch"] / res["ms_per_step"],
                                             rel=1e-3)
        # a plain run takes none of the measurements that need runs of their own
        assert not [k for k in res if k.startswith("roofline") or k == "cpu_baseline"]
        files = sorted(os.listdir(out))
        assert files == [n + ".npy" for n in res["dumped_outputs"]]
        assert {"loss.npy", "grads.npy", "params.npy"} <= set(files)
        total = 0
        for f in files:
            a = np.load(out / f)
            assert a.dtype == np.float32 and np.isfinite(a).all(), f
            total += a.nbytes
        assert total <= 64 << 20
        assert float(np.load(out / "loss.npy").reshape(-1)[0]) == pytest.approx(res["final_loss"], abs=1e-6)
    assert sorted(os.listdir(outs[0])) == sorted(os.listdir(outs[1]))
    for f in sorted(os.listdir(outs[0])):
        a, b = np.load(outs[0] / f), np.load(outs[1] / f)
        assert a.shape == b.shape, f
        err = _rel_l2(a, b)
        print(f"{f}: relative L2 between the two runs {err:.3e}")
        assert err <= (1e-5 if f in ("grads.npy", "params.npy") else 1e-6), (f, err)
    assert np.linalg.norm(np.load(outs[0] / "grads.npy")) > 0
