"""Gradient accumulation: the published 8-GPU x 2-clip step on fewer GPUs, exactly.

The reference trains with ``GPU_WORLD_SIZE: 8`` and ``TRAIN.BATCH_SIZE: 2`` (configuration/TubeR_CSN152_AVA21.yaml).  Its
BatchNorm3d is not synchronised and ``SetCriterionAVA`` normalises by the rank's own box count, so one 8-rank step is the MEAN of 8
independent 2-clip forward / backward passes -- which is what accumulating over 8 micro-batches of 2 clips computes.
``CONFIG.TRAIN.ACCUM_STEPS = k`` (default 1 = off) makes the training loop step the optimizer every k batches.

A group of m micro-batches (m = k, or fewer for the trailing partial group of an epoch):

    micro 0        zero_grad, forward, BN snapshot, backward, acc = g           (role "first")
    micro 1..m-2   zero_grad, forward, BN restore, backward, acc += g           (role "middle")
    micro m-1      zero_grad, forward, BN restore, backward, g = (acc + g) / m  (role "last"), then clip + AdamW as usual
    m = 1          the plain step                                               (role None)

``tuber_grad_accum`` (csrc/grad_accum.hip) runs each pass over the trainable windows of the flat gradient buffer in one launch; the fold
writes the mean back into ``gflat``, so the optimizer, clipping and the reducer read it unchanged.  Only micro-batch 0 updates the
BatchNorm running statistics (the snapshot / restore of ``tuber_bn_stats_copy``): a checkpoint of the 8-rank run holds rank 0's.

With a reducer (ddp.py) the micro-batches before the last issue no collective (DDP's ``no_sync``); on the last one each window is
folded on the backward stream right before its all-reduce is issued (``FlatGradReducer.pre_reduce``).
"""
import numpy as np
import torch

class GroupSchedule:
    """Which micro-batch of a group the next call is, and what it does.  Pure host bookkeeping (no device)."""

    def __init__(self, k):
        k = int(k)
        if k < 1:
            raise ValueError("ACCUM_STEPS must be >= 1, got %d" % k)
        self.k = k
        self.micro = 0                   # index of the next micro-batch inside the current group
        self.steps = 0                   # optimizer steps taken

    def role(self, last=False):
        """role of the next micro-batch; ``last``: it ends the group whatever its index (trailing partial group).  None = a plain step
        (k = 1, or a group of one)."""
        ends = last or self.micro + 1 >= self.k
        if self.micro == 0:
            return None if ends else "first"
        return "last" if ends else "middle"

    def m(self):
        """size of the group the next micro-batch ends (meaningful for role 'last')"""
        return self.micro + 1

    def advance(self, role):
        """the micro-batch of ``role`` has been issued.  Returns True when it stepped the optimizer."""
        if role in (None, "last"):
            self.micro = 0
            self.steps += 1
            return True
        self.micro += 1
        return False


def steps_per_epoch(n_iter, k):
    """optimizer steps of an epoch of n_iter batches (the trailing partial group steps too)"""
    return (int(n_iter) + int(k) - 1) // int(k)


def _bn_modules(model):
    return [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.track_running_stats
            and m.running_mean is not None]


class GradAccumulator:
    """Device state of the accumulation for one ParamStore: the fp32 ``acc`` buffer (only when k > 1), the window table, the fold
    scale (device, so a captured fold reads the current group's 1/m), and the BatchNorm snapshot arena + table."""

    def __init__(self, store, k):
        self.store = store
        self.sched = GroupSchedule(k)
        self.k = self.sched.k
        self.acc = None
        self.scale_dev = None
        self.bn_arena = None
        self._tables = {}
        self.role = None
        if self.k > 1:
            dev = store.device
            self.acc = torch.zeros(store.total, dtype=torch.float32, device=dev)
            self.scale_dev = torch.ones(1, dtype=torch.float32, device=dev)
            rows, off = [], 0
            for m in _bn_modules(store.module):
                for b in (m.running_mean, m.running_var, m.num_batches_tracked):
                    if b.device != dev or not b.is_contiguous() or b.element_size() * b.numel() % 4:
                        raise ValueError("BatchNorm buffer not snapshot-able (%s, %s)" % (b.dtype, b.device))
                    words = b.element_size() * b.numel() // 4
                    rows.append((b.data_ptr(), off, words))
                    off += words
            self.bn_rows = len(rows)
            self._bn_mods = _bn_modules(store.module)
            if rows:
                self.bn_arena = torch.zeros(max(off, 1), dtype=torch.float32, device=dev)
                self.bn_table = torch.tensor(rows, dtype=torch.int64).to(dev)
                self.bn_max = max(r[2] for r in rows)
                self._bn_ptrs = [r[0] for r in rows]

    @property
    def micro(self):
        return self.sched.micro

    @property
    def steps(self):
        return self.sched.steps

    # -- schedule ----------------------------------------------------------------------------------------------------------
    def begin_micro(self, last=False):
        """role of the next micro-batch (see module doc); for 'last' the fold scale 1/m is set on the device.  Does not advance:
        ``end_micro`` does, once the micro-batch has been issued (a failed capture can repeat it)."""
        role = self.sched.role(last)
        if role is not None:
            self._check_bn()
        if role == "last":
            self.scale_dev.fill_(1.0 / self.sched.m())
        self.role = role
        return role

    def end_micro(self):
        """returns True when the micro-batch just issued stepped the optimizer"""
        return self.sched.advance(self.role)

    def _check_bn(self):
        """the BatchNorm table holds raw buffer addresses: refuse to run if a buffer was re-allocated since it was built"""
        if self.bn_arena is None:
            return
        live = [b.data_ptr() for m in self._bn_mods for b in (m.running_mean, m.running_var, m.num_batches_tracked)]
        if live != self._bn_ptrs:
            raise RuntimeError("BatchNorm buffers were re-allocated or replaced after the GradAccumulator was built (model.to(), buffers "
                               "replaced by a checkpoint load): build a new accumulator / GraphedTrainStep")

    # -- device passes -----------------------------------------------------------------------------------------------------
    def windows(self):
        return self.store.trainable_ranges()

    def _table(self, wins):
        key = tuple(wins)
        t = self._tables.get(key)
        if t is None:
            if len(self._tables) > 64:
                self._tables.clear()
            t = self._tables[key] = torch.tensor(np.asarray(wins, dtype=np.int64).reshape(-1, 2)).to(self.store.device)
        return t

    def _launch(self, mode, wins=None):
        from . import lib
        wins = self.windows() if wins is None else list(wins)
        if not wins:
            return
        lib.call("tuber_grad_accum", self.store.gflat, self.acc, self._table(wins), len(wins), mode,
                 self.scale_dev if mode == 2 else None, 1.0)

    def init(self):
        self._launch(0)

    def add(self):
        self._launch(1)

    def fold(self, wins=None):
        """g[w] = (acc[w] + g[w]) * (1/m) over ``wins`` (default: every trainable window)"""
        self._launch(2, wins)

    def after_forward(self, role=None):
        """BatchNorm running statistics: snapshot after micro-batch 0's forward, restore after every later one (one launch each)"""
        role = self.role if role is None else role
        if role is None or self.bn_arena is None:
            return
        from . import lib
        lib.call("tuber_bn_stats_copy", self.bn_table, self.bn_rows, self.bn_arena, self.bn_max, 0 if role == "first" else 1)

    def after_backward(self, role=None):
        """first: acc = g; middle: acc += g; last / plain: nothing (the fold: ``fold``, per window through the reducer, or ``flush``)"""
        role = self.role if role is None else role
        if role == "first":
            self.init()
        elif role == "middle":
            self.add()

    def flush(self, step_fn):
        """close a pending partial group after its last micro-batch already ran as 'first' / 'middle' (a loader of unknown length):
        g = (acc + 0) / m = the mean, then the optimizer step.  Returns True when a step was taken.  Not for use with a reducer (the
        pending micro-batches issued no collective)."""
        if self.sched.micro == 0:
            return False
        if getattr(self.store, "reducer", None) is not None:
            raise RuntimeError("GradAccumulator.flush with a reducer: mark the group's last batch instead (train_step(..., last=True))")
        m = self.sched.micro
        self.scale_dev.fill_(1.0 / m)
        self.store.gflat.zero_()
        self.fold()
        step_fn()
        self.sched.micro = 0
        self.sched.steps += 1
        return True
