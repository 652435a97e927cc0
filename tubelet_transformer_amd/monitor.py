"""Step monitor: per-tensor gradient, parameter and update statistics, inside the captured training step.

``StepMonitor`` runs ONE segmented reduction over the flat buffers (csrc/tensor_stats.hip, ``tuber_tensor_stats``: three launches, no
atomics, deterministic) behind the AdamW launches of ``FusedClipAdamW.step()`` -- inside whichever hipGraph holds the optimizer step --
and leaves one 8-float row per parameter tensor in device memory:

    col 0  sum g^2 over the finite gradient elements (the gradient as it sits in ``gflat``: unclipped)
    col 1  max |g| over the finite elements          col 2  number of non-finite g          col 3  number of g == +-0
    col 4  sum p^2 over the finite parameter elements (the parameters AFTER this step's update)
    col 5  max |p| over the finite elements          col 6  number of non-finite p
    col 7  sum u^2, u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps): the AdamW direction before lr, without the decay term

Cadence and the non-finite case are decided on the device.  A good step t records iff ``t % every == 0``, into slot ``(t / every) %
history`` of a ring; a step the optimizer skipped (non-finite gradient norm) writes the separate BAD slot, once: the first failure is kept,
later ones are only counted.  The host reads nothing until ``rows()`` / ``bad()`` is called; ``configure(every=...)`` is one small copy and
needs no new capture.

The launch rides in ``step()``, so under gradient accumulation it exists only in the stepping micro-batch's graph and sees the folded mean
gradient, and under data parallelism it sees the all-reduced gradient: every rank records the same rows.  BatchNorm buffers are not
monitored.  The monitor is diagnostic: it holds no checkpoint state.
"""
import itertools

import numpy as np
import torch

from . import lib

KEY = "_tuber_step_monitor"        # where the training loop caches a model's monitor (model.__dict__)
COLUMNS = ("grad_sumsq", "grad_absmax", "grad_nonfinite", "grad_zeros", "param_sumsq", "param_absmax", "param_nonfinite", "update_sumsq")
REFERENCE_GROUPS = ("transformer", "backbone", "class_embed", "query_embed")      # optim.build_param_groups' order
STATE_WORDS = 4                    # device state: {every, history, bad_count, bad_step}
TENSOR = np.dtype([("chunk0", "<i4"), ("nchunks", "<i4"), ("beta1", "<f4"), ("beta2", "<f4"), ("eps", "<f4")])
CHUNK = np.dtype([("off", "<i8"), ("n", "<i4"), ("tensor", "<i4")])
_serial = itertools.count(1)


def chunk_table(offsets, numels, chunk):
    """the chunk table of tensors at ``offsets`` with ``numels`` elements: a tensor of n elements gets ceil(n / chunk) runs of at most
    ``chunk`` elements, in layout order -> structured array of (off, n, tensor).  No run crosses a tensor; together a tensor's runs tile it."""
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be >= 1, got %d" % chunk)
    rows = []
    for ti, (o, n) in enumerate(zip(offsets, numels)):
        for b in range(0, int(n), chunk):
            rows.append((int(o) + b, min(chunk, int(n) - b), ti))
    return np.array(rows, dtype=CHUNK)


def check_settings(every, history, prefix=""):
    """validated (every, history); a bad value raises ValueError naming ``prefix`` + its key"""
    if isinstance(every, bool) or not isinstance(every, int) or every < 1:
        raise ValueError("%sEVERY must be an integer >= 1, got %r" % (prefix, every))
    if isinstance(history, bool) or not isinstance(history, int) or history < 1:
        raise ValueError("%sHISTORY must be an integer >= 1, got %r" % (prefix, history))
    return int(every), int(history)


def monitor_settings(cfg):
    """CONFIG.TRAIN.MONITOR, validated -> dict(enable, every, history)"""
    M = cfg.CONFIG.TRAIN.MONITOR
    pre = "CONFIG.TRAIN.MONITOR."
    if not isinstance(M.ENABLE, bool):
        raise ValueError("%sENABLE must be a bool, got %r" % (pre, M.ENABLE))
    every, history = check_settings(M.EVERY, M.HISTORY, prefix=pre)
    return dict(enable=M.ENABLE, every=every, history=history)


def _bare(model):
    return model.module if hasattr(model, "module") else model


def monitor_of(model):
    """the monitor the training loop cached on this model, or None"""
    return _bare(model).__dict__.get(KEY)


def group_names(n_groups):
    """names of an optimizer's parameter groups in the logs: the four reference groups by role, anything else by index"""
    return list(REFERENCE_GROUPS) if n_groups == len(REFERENCE_GROUPS) else ["group%d" % i for i in range(n_groups)]


# -- reading a table (host; no device needed) ----------------------------------------------------------------------------------------
def summarize(table, numels, groups, lrs, names=None):
    """per parameter group and for the whole model ("all"): grad_norm, param_norm, update_ratio, nonfinite_grads, nonfinite_params,
    zero_grad_fraction of a ``[T, 8]`` table.  ``groups[i]``: the group of tensor i (-1: none), ``lrs[g]``: that group's learning rate.
    ``update_ratio = lr * sqrt(sum col 7) / sqrt(sum col 4)`` is the size of the AdamW step relative to the weights; it IGNORES weight decay
    (the ``lr * wd * p`` term of the update) and the whole-model value adds the groups' steps in quadrature."""
    table = np.asarray(table, dtype=np.float64)
    numels, groups = np.asarray(numels, dtype=np.float64), np.asarray(groups)
    names = group_names(len(lrs)) if names is None else list(names)

    def block(sel, step_sq):
        s = table[sel].sum(axis=0) if sel.any() else np.zeros(8)
        n = numels[sel].sum()
        return {"grad_norm": float(np.sqrt(s[0])), "param_norm": float(np.sqrt(s[4])),
                "update_ratio": float(np.sqrt(step_sq)) / float(np.sqrt(s[4])) if s[4] > 0 else 0.0,
                "nonfinite_grads": int(s[2]), "nonfinite_params": int(s[6]), "zero_grad_fraction": float(s[3] / n) if n > 0 else 0.0}

    out, total = {}, 0.0
    for gi, (name, lr) in enumerate(zip(names, lrs)):
        sel = groups == gi
        step_sq = float(lr) ** 2 * float(table[sel, 7].sum())
        total += step_sq
        out[name] = block(sel, step_sq)
    out["all"] = block(np.ones(len(table), dtype=bool), total)
    return out


def worst_tensors(table, names, k, by, groups=None, lrs=None):
    """the ``k`` tensor names with the largest per-tensor value of column ``by`` (an index, a COLUMNS name) or of "update_ratio", largest
    first, as (name, value) pairs"""
    table = np.asarray(table, dtype=np.float64)
    if by == "update_ratio":
        lr = np.array([lrs[g] if g >= 0 else 0.0 for g in groups], dtype=np.float64)
        val = np.where(table[:, 4] > 0, lr * np.sqrt(table[:, 7]) / np.sqrt(np.where(table[:, 4] > 0, table[:, 4], 1.0)), 0.0)
    else:
        val = table[:, COLUMNS.index(by) if isinstance(by, str) else int(by)]
    order = np.argsort(-val, kind="stable")[:max(int(k), 0)]
    return [(names[i], float(val[i])) for i in order]


def nonfinite_tensors(table, names, what="any"):
    """names of the tensors with a non-finite gradient (``what="grad"``), parameter ("param") or either ("any"), in flat-buffer order.

    How to read it after a skipped step (``bad()``): a NaN born in the backward reaches every tensor whose gradient the backward computes
    AFTER it, so the tensors whose gradient is still finite are those whose gradient was complete before the NaN appeared -- the NaN was
    born between the last finite and the first non-finite tensor in backward order.  A non-finite PARAMETER (or input) poisons the forward
    instead: then the loss and every gradient it reaches are non-finite, and the parameter list names the culprit."""
    table = np.asarray(table)
    bad = {"grad": table[:, 2] > 0, "param": table[:, 6] > 0, "any": (table[:, 2] > 0) | (table[:, 6] > 0)}[what]
    return [names[i] for i in np.nonzero(bad)[0]]


class StepMonitor:
    def __init__(self, model, every=50, history=8):
        self.every, self.history = check_settings(every, history)
        self.model = _bare(model)
        self.store, _ = self.model.engine()
        st = self.store
        dev = st.device
        if lib.query("tuber_tensor_stats_tensor_bytes") != TENSOR.itemsize or lib.query("tuber_tensor_stats_chunk_bytes") != CHUNK.itemsize:
            raise RuntimeError("tensor-statistics table layout drift between monitor.py and libtuber_hip.so")
        self.chunk = lib.query("tuber_tensor_stats_chunk")
        self.names = list(st.names)
        self.numels = [int(p.numel()) for p in st.params]
        chunks = chunk_table([st.offsets[n] for n in self.names], self.numels, self.chunk)
        self._tensors_host = np.zeros(len(self.names), dtype=TENSOR)
        count = np.bincount(chunks["tensor"], minlength=len(self.names)).astype(np.int32)
        self._tensors_host["nchunks"] = count
        self._tensors_host["chunk0"] = np.cumsum(count) - count
        self.groups = [-1] * len(self.names)                 # parameter group of every tensor (attach)
        self.n_tensors, self.n_chunks = len(self.names), len(chunks)
        self.chunks = torch.from_numpy(chunks.view(np.uint8).copy()).to(dev)
        self.tensors = torch.from_numpy(self._tensors_host.view(np.uint8).copy()).to(dev)
        self.partial = torch.zeros(self.n_chunks * 8, dtype=torch.float32, device=dev)
        # everything the launches write, in ONE buffer (one device-to-host read, one entry in the capture's snapshot):
        # state[4] | row_step[history] | row_norm[history][2] | pad to 4 words | ring[history][T][8] | bad[T][8]
        H, T = self.history, self.n_tensors
        self._o_step = STATE_WORDS
        self._o_norm = self._o_step + H
        self._o_ring = (self._o_norm + 2 * H + 3) // 4 * 4
        self._o_bad = self._o_ring + H * T * 8
        self.mem = torch.zeros(self._o_bad + T * 8, dtype=torch.int32, device=dev)
        fmem = self.mem.view(torch.float32)
        self.state = self.mem[:STATE_WORDS]
        self.row_step = self.mem[self._o_step:self._o_norm]
        self.row_norm = fmem[self._o_norm:self._o_norm + 2 * H]
        self.ring = fmem[self._o_ring:self._o_bad]
        self.bad_table = fmem[self._o_bad:]
        self.optimizer = None            # the optimizer object attach() was given
        self.fused = None                # its FusedClipAdamW (None: another optimizer, train_step probes eagerly)
        self.serial = next(_serial)      # part of GraphedTrainStep's key: a captured step bakes this monitor's addresses in
        self.reset()

    # -- settings ------------------------------------------------------------------------------------------------------------
    def settings(self):
        return dict(every=self.every, history=self.history)

    def configure(self, every):
        """change the cadence: one small copy into the device state, no new capture (``history`` sizes the ring: build a new monitor)"""
        self.every, _ = check_settings(every, self.history)
        self.state[:1].copy_(torch.tensor([self.every], dtype=torch.int32))

    @torch.no_grad()
    def reset(self):
        """forget every recorded row and the bad slot"""
        host = np.zeros(self.mem.numel(), dtype=np.int32)
        host[:2] = (self.every, self.history)
        host[self._o_step:self._o_norm] = -1             # row_step -1: the slot holds nothing
        self.mem.copy_(torch.from_numpy(host))

    @torch.no_grad()
    def clear_bad(self):
        """re-arm the bad slot: the next skipped step is recorded again"""
        self.state[2:4].zero_()
        self.bad_table.zero_()

    # -- launches ------------------------------------------------------------------------------------------------------------
    def _launch(self, m, v, step_ptr, clip):
        st = self.store
        if self.model._store is not st:
            raise RuntimeError("StepMonitor: the model's parameters were re-allocated after the monitor was built; build a new one")
        lib.call("tuber_tensor_stats", st.gflat, st.flat, m, v, self.tensors, self.n_tensors, self.chunks, self.n_chunks, self.partial,
                 self.state, self.history, self.row_step, self.row_norm, self.ring, self.bad_table, step_ptr, clip)

    @torch.no_grad()
    def probe(self):
        """record now, unconditionally, into ring slot 0, without the moments (column 7 = 0): an optimizer this module does not drive"""
        self._launch(None, None, None, None)

    @torch.no_grad()
    def step_update(self, fused, clip):
        """the launch behind an AdamW step: cadence from the device step count, the bad slot for a step the optimizer skipped"""
        self._launch(fused.exp_avg, fused.exp_avg_sq, fused.t_dev, clip)

    def attach(self, optimizer):
        """record behind every step of ``optimizer``.  An AdamW (``FusedClipAdamW`` or the stock object it adopts) launches the kernels
        inside ``FusedClipAdamW.step()``, so a captured step holds them; ``train_step`` calls ``probe()`` after any other optimizer's step.
        The tensor-to-group map and the betas / eps of column 7 come from the optimizer's ``param_groups``."""
        from .optim import adopt
        self.detach()
        fused = adopt(optimizer, self.model)
        if fused is not None:
            if fused.store is not self.store:
                raise ValueError("StepMonitor.attach: the optimizer drives another parameter store")
            fused.monitor = self
        by_ptr = {p.data_ptr(): gi for gi, g in enumerate(optimizer.param_groups) for p in g["params"]}
        self.groups = [by_ptr.get(p.data_ptr(), -1) for p in self.store.params]
        host = self._tensors_host
        for i, gi in enumerate(self.groups):
            g = optimizer.param_groups[gi] if gi >= 0 else {}
            b1, b2 = g.get("betas", (0.0, 0.0))
            host["beta1"][i], host["beta2"][i], host["eps"][i] = b1, b2, g.get("eps", 0.0)
        self.tensors.copy_(torch.from_numpy(host.view(np.uint8).copy()))
        self.optimizer, self.fused = optimizer, fused
        self.model.__dict__[KEY] = self
        return self

    def detach(self):
        if self.fused is not None and getattr(self.fused, "monitor", None) is self:
            self.fused.monitor = None
        self.optimizer = self.fused = None

    def drives(self, optimizer):
        """True when train_step has to call probe() itself after ``optimizer.step()`` (attached, and not an AdamW)"""
        return self.fused is None and self.optimizer is not None and self.optimizer is optimizer

    # -- reading -------------------------------------------------------------------------------------------------------------
    def _read(self):
        """the whole device buffer in ONE device-to-host read (syncs)"""
        host = self.mem.cpu().numpy()
        return host, host.view(np.float32)

    def _rows(self, host, fhost):
        H, T = self.history, self.n_tensors
        out = []
        for slot in range(H):
            t = int(host[self._o_step + slot])
            if t < 0:
                continue
            table = fhost[self._o_ring + slot * T * 8:self._o_ring + (slot + 1) * T * 8].reshape(T, 8).copy()
            out.append((t, float(fhost[self._o_norm + 2 * slot]), float(fhost[self._o_norm + 2 * slot + 1]), table))
        out.sort(key=lambda r: -r[0])
        return out

    def _bad(self, host, fhost):
        if int(host[2]) == 0:
            return None
        return int(host[3]), int(host[2]), fhost[self._o_bad:].reshape(self.n_tensors, 8).copy()

    def rows(self):
        """the recorded ring rows, newest first, as (t, norm, clip_coef, table[n_tensors, 8]) -- one device-to-host read"""
        return self._rows(*self._read())

    def bad(self):
        """None, or (bad_step, bad_count, table) of the FIRST step the optimizer skipped since ``clear_bad()``; ``bad_step`` is the AdamW
        step count at that moment (the number of good steps before it), ``bad_count`` the number of skipped steps since"""
        return self._bad(*self._read())

    def read(self):
        """(rows(), bad()) from one device-to-host read"""
        host, fhost = self._read()
        return self._rows(host, fhost), self._bad(host, fhost)

    def _lrs(self):
        return [] if self.optimizer is None else [float(g["lr"]) for g in self.optimizer.param_groups]

    def summary(self, row):
        """``summarize`` of a row of ``rows()`` (or a bare table) with this monitor's groups and the optimizer's CURRENT learning rates;
        ``update_ratio`` ignores weight decay"""
        table = row[3] if isinstance(row, tuple) else row
        return summarize(table, self.numels, self.groups, self._lrs())

    def worst(self, row, k=5, by="grad_sumsq"):
        """the ``k`` tensors with the largest value of a column (index or COLUMNS name) or of "update_ratio": (name, value) pairs"""
        table = row[3] if isinstance(row, tuple) else row
        return worst_tensors(table, self.names, k, by, self.groups, self._lrs())

    def nonfinite_names(self, table, what="any"):
        """``nonfinite_tensors`` with this monitor's names (see there for how to read the list)"""
        return nonfinite_tensors(table, self.names, what)


def monitor_for(cfg, model, optimizer):
    """the training loop's monitor: None unless CONFIG.TRAIN.MONITOR.ENABLE; else the one cached on the model (created on first use, its
    cadence following the config), attached to ``optimizer``"""
    if getattr(cfg.CONFIG.TRAIN, "MONITOR", None) is None:      # a config node built without this module's defaults
        return None
    s = monitor_settings(cfg)
    if not s["enable"]:
        return None
    model = _bare(model)
    m = model.__dict__.get(KEY)
    if m is None or m.store is not model.engine()[0] or m.history != s["history"]:
        m = StepMonitor(model, every=s["every"], history=s["history"])
    elif m.every != s["every"]:
        m.configure(every=s["every"])
    if m.optimizer is not optimizer:
        m.attach(optimizer)
    model.__dict__[KEY] = m
    return m
