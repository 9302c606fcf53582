"""CPU tests of bench.py's --dump-outputs machinery on a stand-in for the training step: the writer (file set, dtypes, the seeded
sample of the flat weights, size bound) and the snapshot / restore of the training state the last timed step starts from."""
import inspect
import os
import types
from unittest import mock

import numpy as np
import torch


def _bench():
    with mock.patch.dict(os.environ):            # importing bench.py points MIOpen's user database at a temporary directory
        import bench
    return bench


def _step():
    g = torch.Generator().manual_seed(5)
    groups = [types.SimpleNamespace(param=torch.randn(n, generator=g), grad=torch.randn(n, generator=g)) for n in (7000, 300, 2500)]
    opt = types.SimpleNamespace(flat=types.SimpleNamespace(groups=groups), grad_norm=lambda: torch.tensor(2.5, dtype=torch.float64))
    return types.SimpleNamespace(optimizer=opt), groups


def test_dump_outputs_writes_the_last_steps_arrays(tmp_path):
    bench = _bench()
    step, groups = _step()
    losses = {"loss_ce": torch.tensor(1.25), "loss_mask_0": torch.tensor(0.5), "loss_dice_9": torch.tensor(0.75)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), step, losses, sample=1000)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(["loss_ce.npy", "loss_mask_0.npy", "loss_dice_9.npy", "grad_norm.npy", "params_sample.npy"])
    for n in names:                                                       # same arguments, same files
        x = np.load(tmp_path / "a" / n)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, np.load(tmp_path / "b" / n)), n
    for k, v in losses.items():
        assert np.load(tmp_path / "a" / (k + ".npy")) == v.item()
    gn = np.load(tmp_path / "a" / "grad_norm.npy")
    assert gn.dtype == np.float64 and gn == 2.5
    # one fixed, seeded set of positions of the groups laid end to end
    flat_p = torch.cat([g.param for g in groups])
    idx = torch.randint(flat_p.numel(), (1000,), generator=torch.Generator().manual_seed(0)).unique()
    p = np.load(tmp_path / "a" / "params_sample.npy")
    assert p.dtype == np.float32 and 900 < p.size <= 1000 and np.array_equal(p, flat_p[idx].numpy())
    # at most `sample` elements in all: every one of them
    bench.dump_outputs(str(tmp_path / "c"), step, losses, sample=1 << 20)
    assert np.array_equal(np.load(tmp_path / "c" / "params_sample.npy"), flat_p.numpy())


def test_restore_training_state_returns_weights_moments_and_counters():
    bench = _bench()
    step, groups = _step()
    moments = [torch.zeros_like(g.param) for g in groups]
    applied = []
    step._flat_state = lambda: [g.param for g in groups] + moments
    step.optimizer.steps, step.iter = 0, 0
    step.scheduler = types.SimpleNamespace(last_iter=0, _apply=lambda: applied.append(step.scheduler.last_iter))
    want = [t.clone() for t in step._flat_state()]
    snap = bench.snapshot_training_state(step)
    for t in step._flat_state():                                          # a few training steps later
        t.add_(1.0)
    step.optimizer.steps, step.iter, step.scheduler.last_iter = 7, 7, 7
    bench.restore_training_state(step, snap)
    assert all(torch.equal(t, w) for t, w in zip(step._flat_state(), want))
    assert (step.optimizer.steps, step.iter, step.scheduler.last_iter) == (0, 0, 0) and applied == [0]
    assert all(s.data_ptr() != t.data_ptr() for s, t in zip(snap[0], step._flat_state()))     # the snapshot is a copy


def test_dump_outputs_default_sample_stays_within_64_mb():
    sample = inspect.signature(_bench().dump_outputs).parameters["sample"].default
    assert sample * 8 <= 64 * 10 ** 6 - 10 ** 6                           # the weights even in float64, 1 MB left for the losses
