"""Gradient accumulation (accum.py), host side: the config key, its validation and the group schedule of the training loop --
which micro-batch folds, the partial group's 1/m, the optimizer-step index the cosine scheduler receives."""
import glob
import os

import pytest

from tubelet_transformer_amd.accum import GradAccumulator, GroupSchedule, steps_per_epoch
from tubelet_transformer_amd.config import load_cfg
from tubelet_transformer_amd.training import accum_steps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_published_configs_do_not_accumulate():
    paths = sorted(glob.glob(os.path.join(ROOT, "configuration", "*.yaml")))
    assert len(paths) == 4
    for p in paths:
        cfg = load_cfg(p)
        assert cfg.CONFIG.TRAIN.ACCUM_STEPS == 1, p
        assert accum_steps(cfg) == 1


@pytest.mark.parametrize("k", [0, -3])
def test_accum_steps_below_one_raise(k):
    cfg = load_cfg(os.path.join(ROOT, "configuration", "TubeR_CSN152_AVA21.yaml"))
    cfg.CONFIG.TRAIN.ACCUM_STEPS = k
    with pytest.raises(ValueError):
        accum_steps(cfg)
    with pytest.raises(ValueError):
        GroupSchedule(k)


def test_one_micro_batch_allocates_nothing():
    class _Store:                                   # k = 1 never touches the device
        device = None
        total = 1 << 30
    a = GradAccumulator(_Store(), 1)
    assert a.acc is None and a.bn_arena is None and a.begin_micro() is None


def _epoch(n_iter, k, sched, epoch=0):
    """the training loop's bookkeeping (training.train_tuber_detection) around a fake step function: returns the per-batch roles, the
    fold scales and the scheduler indices"""
    roles, scales, sched_calls = [], [], []
    n_steps = steps_per_epoch(n_iter, k)
    first_step = sched.steps

    def fake_step(role):
        if role == "last":
            scales.append(1.0 / sched.m())
        elif role is None:
            scales.append(1.0)

    for idx in range(n_iter):
        role = sched.role(last=idx + 1 == n_iter)
        roles.append(role)
        fake_step(role)
        before = sched.steps
        sched.advance(role)
        if sched.steps != before:
            sched_calls.append(epoch * n_steps + sched.steps - 1 - first_step)
    return roles, scales, sched_calls


def test_group_schedule_with_a_partial_group():
    s = GroupSchedule(2)
    roles, scales, calls = _epoch(5, 2, s)
    assert roles == ["first", "last", "first", "last", None]          # 2 + 2 + a group of one (a plain step)
    assert scales == [0.5, 0.5, 1.0]
    assert calls == [0, 1, 2] and s.steps == 3 and s.micro == 0
    roles, scales, calls = _epoch(5, 2, s, epoch=1)                 # next epoch: indices continue at epoch * steps_per_epoch
    assert calls == [3, 4, 5]


def test_group_schedule_partial_scale_is_one_over_m():
    s = GroupSchedule(3)
    roles, scales, calls = _epoch(8, 3, s)
    assert roles == ["first", "middle", "last", "first", "middle", "last", "first", "last"]
    assert scales == [1.0 / 3, 1.0 / 3, 0.5]
    assert calls == [0, 1, 2] and steps_per_epoch(8, 3) == 3


def test_group_schedule_k1_is_the_plain_loop():
    s = GroupSchedule(1)
    roles, scales, calls = _epoch(4, 1, s, epoch=2)
    assert roles == [None] * 4 and scales == [1.0] * 4
    assert calls == [8, 9, 10, 11]                                    # epoch * n_iter + idx, as without accumulation
