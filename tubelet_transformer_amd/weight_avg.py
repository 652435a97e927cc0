"""Weight averaging (EMA / SWA) of the flat parameter buffer, inside the captured training step.

``WeightAverage`` keeps ``avg``, an fp32 twin of ``ParamStore.flat``, and updates it with ONE streaming launch
(csrc/weight_avg.hip, ``tuber_weight_average``): ``avg += w * (flat - avg)``.  Attached to an AdamW optimizer the launch sits behind
the AdamW segment launches of ``FusedClipAdamW.step()`` -- inside whichever hipGraph holds the optimizer step -- and reads the AdamW
step count, the skip flag of a non-finite step, the decay table and its own update count from DEVICE memory: a replayed graph averages
with the right weight every step, a step the optimizer skipped is not averaged, and ``set_decay()`` needs no new capture.

    mode "ema"   w = 1 - decay                              (timm ModelEmaV2: ema = decay * ema + (1 - decay) * p)
                 w = 1 - min(decay, (1 + n) / (10 + n))     with ``warmup`` (n = number of this update, from 1)
    mode "swa"   w = 1 / n                                  (torch.optim.swa_utils.AveragedModel's default avg_fn; update 1 copies)

``effective_weight`` states the weight on the host.  The average starts as a copy of the parameters (so the EMA sequence is the one
``AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(d))`` produces from its second update on).  Updates happen at the optimizer steps t
with ``t >= start`` and ``(t - start) % period == 0``; ``update()`` averages unconditionally (a per-epoch SWA cadence).

BatchNorm running statistics are NOT averaged: under ``applied()`` the averaged parameters run with the live running statistics, unless
statistics recomputed for them were kept (``applied(keep_bn=True)`` around ``bn_stats.recompute_bn_stats`` -- the
``AveragedModel(use_buffers=False)`` + ``update_bn`` recipe).

Data parallel: every rank applies the same all-reduced gradient to the same parameters, so every rank's average is bit-identical without
a collective of its own.
"""
import contextlib
import itertools

import numpy as np
import torch

from . import lib

MODES = ("ema", "swa")
KEY = "_tuber_weight_avg"          # where the training loop caches a model's averager (model.__dict__)
_serial = itertools.count(1)


def effective_weight(mode, decay, warmup, n):
    """the weight w of update number ``n`` (counted from 1) in ``avg += w * (p - avg)``, as the kernel forms it: in fp64 from the fp32
    decay, rounded to fp32 once"""
    if mode not in MODES:
        raise ValueError("mode must be one of %s, got %r" % (" | ".join(MODES), mode))
    n = int(n)
    if n < 1:
        raise ValueError("updates are counted from 1, got n = %d" % n)
    if mode == "swa":
        return float(np.float32(1.0 / n))
    d = float(np.float32(decay))
    if warmup:
        d = min(d, (1.0 + n) / (10.0 + n))
    return float(np.float32(1.0 - d))


def check_settings(mode, decay, warmup, start, period, prefix=""):
    """validated (mode, decay, warmup, start, period); a bad value raises ValueError naming ``prefix`` + its key"""
    if mode not in MODES:
        raise ValueError("%sMODE must be one of %s, got %r" % (prefix, " | ".join(MODES), mode))
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= float(decay) <= 1.0:
        raise ValueError("%sDECAY must lie in [0, 1], got %r" % (prefix, decay))
    if not isinstance(warmup, (bool, int)) or warmup not in (0, 1):
        raise ValueError("%sWARMUP must be a bool, got %r" % (prefix, warmup))
    if isinstance(start, bool) or not isinstance(start, int) or start < 0:
        raise ValueError("%sSTART must be an integer >= 0, got %r" % (prefix, start))
    if isinstance(period, bool) or not isinstance(period, int) or period < 1:
        raise ValueError("%sPERIOD must be an integer >= 1, got %r" % (prefix, period))
    return mode, float(decay), bool(warmup), int(start), int(period)


def ema_settings(cfg):
    """CONFIG.TRAIN.EMA, validated -> dict(enable, eval, mode, decay, warmup, start, period)"""
    E = cfg.CONFIG.TRAIN.EMA
    pre = "CONFIG.TRAIN.EMA."
    for k in ("ENABLE", "EVAL"):
        if not isinstance(E[k], bool):
            raise ValueError("%s%s must be a bool, got %r" % (pre, k, E[k]))
    mode, decay, warmup, start, period = check_settings(E.MODE, E.DECAY, E.WARMUP, E.START, E.PERIOD, prefix=pre)
    return dict(enable=E.ENABLE, eval=E.EVAL, mode=mode, decay=decay, warmup=warmup, start=start, period=period)


def _bare(model):
    return model.module if hasattr(model, "module") else model


def averager_of(model):
    """the averager the training loop cached on this model, or None"""
    return _bare(model).__dict__.get(KEY)


class WeightAverage:
    def __init__(self, model, mode="ema", decay=0.9999, warmup=False, start=0, period=1):
        self.mode, self.decay, self.warmup, self.start, self.period = check_settings(mode, decay, warmup, start, period)
        self.model = _bare(model)
        self.store, _ = self.model.engine()
        dev = self.store.device
        self.avg = self.store.flat.detach().clone()
        self.table = torch.zeros(5, dtype=torch.int32, device=dev)       # {decay (float bits), mode, warmup, start, period}: read by the kernel
        self.n_avg = torch.zeros(1, dtype=torch.int32, device=dev)       # updates applied so far (advanced on the device)
        self.bn = None                   # {buffer name: tensor}: BatchNorm statistics recomputed FOR the averaged weights (applied(keep_bn=True))
        self.optimizer = None            # the optimizer object attach() was given
        self.fused = None                # its FusedClipAdamW (None: another optimizer, train_step updates eagerly)
        self.serial = next(_serial)      # part of GraphedTrainStep's key: a captured step bakes this averager's addresses in
        self._active = False
        self._write_table()

    # -- settings ------------------------------------------------------------------------------------------------------------
    def settings(self):
        return dict(mode=self.mode, decay=self.decay, warmup=self.warmup, start=self.start, period=self.period)

    def configure(self, **kw):
        """change any of mode / decay / warmup / start / period: one small copy into the device table, no new capture"""
        s = dict(self.settings(), **kw)
        self.mode, self.decay, self.warmup, self.start, self.period = check_settings(s["mode"], s["decay"], s["warmup"], s["start"], s["period"])
        self._write_table()

    def set_decay(self, decay):
        self.configure(decay=decay)

    def _write_table(self):
        host = np.array([0, MODES.index(self.mode), int(self.warmup), self.start, self.period], dtype=np.int32)
        host[:1].view(np.float32)[0] = self.decay
        self.table.copy_(torch.from_numpy(host))

    @property
    def updates(self):
        """number of updates applied (host copy of the device counter; syncs)"""
        return int(self.n_avg.item())

    # -- updates -------------------------------------------------------------------------------------------------------------
    def _launch(self, step_ptr, clip):
        st = self.store
        if self.model._store is not st:
            raise RuntimeError("WeightAverage: the model's parameters were re-allocated after the averager was built; build a new one")
        lib.call("tuber_weight_average", self.avg, st.flat, st.total, self.table, self.n_avg, step_ptr, clip)

    @torch.no_grad()
    def update(self):
        """average now, unconditionally (a per-epoch SWA cadence, or an optimizer this module does not drive)"""
        self._launch(None, None)

    @torch.no_grad()
    def step_update(self, t_dev, clip):
        """the launch behind an AdamW step: cadence from the device step count, nothing for a step the optimizer skipped"""
        self._launch(t_dev, clip)

    def attach(self, optimizer):
        """average behind every step of ``optimizer``.  An AdamW (``FusedClipAdamW`` or the stock object it adopts) launches the kernel
        inside ``FusedClipAdamW.step()``, so a captured step holds it; ``train_step`` calls ``update()`` after any other optimizer's step."""
        from .optim import adopt
        self.detach()
        fused = adopt(optimizer, self.model)
        if fused is not None:
            if fused.store is not self.store:
                raise ValueError("WeightAverage.attach: the optimizer drives another parameter store")
            fused.averager = self
        self.optimizer, self.fused = optimizer, fused
        self.model.__dict__[KEY] = self
        return self

    def detach(self):
        if self.fused is not None and getattr(self.fused, "averager", None) is self:
            self.fused.averager = None
        self.optimizer = self.fused = None

    def drives(self, optimizer):
        """True when train_step has to call update() itself after ``optimizer.step()`` (attached, and not an AdamW)"""
        return self.fused is None and self.optimizer is not None and self.optimizer is optimizer

    # -- the averaged weights ------------------------------------------------------------------------------------------------
    def _buffers(self):
        return {n: b for n, b in self.model.named_buffers()}

    @torch.no_grad()
    def state_dict(self):
        """the model's ``state_dict()`` with every parameter replaced by its average (same names, same shapes: a checkpoint of the
        averaged model); buffers are the kept BatchNorm statistics when there are any, else the live ones"""
        flat, out = self.store.flat, {}
        lo, hi = flat.data_ptr(), flat.data_ptr() + 4 * flat.numel()
        for k, v in self.model.state_dict().items():
            p = v.data_ptr()
            if v.dtype == torch.float32 and lo <= p < hi:
                o = (p - lo) // 4
                out[k] = self.avg[o:o + v.numel()].view(v.shape).clone()
            elif self.bn is not None and k in self.bn:
                out[k] = self.bn[k].clone()
            else:
                out[k] = v.detach().clone()
        return out

    @torch.no_grad()
    def load_state_dict(self, sd, buffers=False):
        """averaged weights from a ``state_dict`` of the model's names (a leading ``module.`` is accepted).  Every parameter must be there
        with its shape.  ``buffers``: also keep the file's BatchNorm statistics as the ones the averaged weights run with."""
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
        missing = [n for n in self.store.names if n not in sd]
        if missing:
            raise KeyError("averaged weights: %d parameters missing, e.g. %s" % (len(missing), missing[:4]))
        for n, p in zip(self.store.names, self.store.params):
            v = torch.as_tensor(sd[n])
            if tuple(v.shape) != tuple(p.shape):
                raise ValueError("averaged weights: %s has shape %s, the model %s" % (n, tuple(v.shape), tuple(p.shape)))
            o = self.store.offsets[n]
            self.avg[o:o + p.numel()].view(p.shape).copy_(v.to(self.avg.device, torch.float32))
        if buffers:
            live = self._buffers()
            self.bn = {n: torch.as_tensor(sd[n]).to(b.device, b.dtype).clone() for n, b in live.items() if n in sd}

    def state(self):
        """everything a resume needs: the flat average, the update count, the settings, kept BatchNorm statistics (host tensors)"""
        return {"avg": self.avg.detach().cpu(), "n_avg": self.updates, "settings": self.settings(),
                "names": list(self.store.names), "offsets": [self.store.offsets[n] for n in self.store.names],
                "bn": None if self.bn is None else {n: b.detach().cpu() for n, b in self.bn.items()}}

    @torch.no_grad()
    def load_state(self, state):
        if list(state["names"]) != list(self.store.names) or list(state["offsets"]) != [self.store.offsets[n] for n in self.store.names] \
                or tuple(state["avg"].shape) != tuple(self.avg.shape):
            raise ValueError("weight-average state was saved for a different parameter layout")
        self.avg.copy_(state["avg"])
        self.n_avg.fill_(int(state["n_avg"]))
        self.configure(**state["settings"])
        live = self._buffers()
        bn = state.get("bn")
        self.bn = None if bn is None else {n: b.to(live[n].device, live[n].dtype).clone() for n, b in bn.items() if n in live}

    @contextlib.contextmanager
    def applied(self, model=None, keep_bn=False):
        """Run the model with the averaged parameters: on entry ``flat`` holds the average (the parameters are views, a captured step
        reads the same addresses), on exit the live parameters, every buffer (BatchNorm running statistics, their counters) and the
        dropout seed are back bit for bit -- ``bn_stats.recompute_bn_stats(model, loader)`` may run inside.  Kept statistics (an earlier
        ``keep_bn=True``) are installed on entry; ``keep_bn=True`` keeps what the buffers hold on exit.  The bf16 shadows the engine derives
        from ``flat`` are rebuilt on entry and exit.  Not re-entrant; no training step may run inside."""
        model = self.model if model is None else _bare(model)
        store, _ = model.engine()
        if store is not self.store:
            raise ValueError("WeightAverage.applied: this averager belongs to another model (or its parameters were re-allocated)")
        if self._active:
            raise RuntimeError("WeightAverage.applied is not re-entrant")
        with torch.no_grad():
            live = store.flat.clone()
            seed = store.seed.clone()
            bufs = self._buffers()
            saved = {n: b.clone() for n, b in bufs.items()}
            store.flat.copy_(self.avg)
            if self.bn is not None:
                for n, b in self.bn.items():
                    if n in bufs:
                        bufs[n].copy_(b)
            store.refresh()
        self._active = True
        try:
            yield model
        finally:
            self._active = False
            with torch.no_grad():
                bufs = self._buffers()
                if keep_bn:
                    self.bn = {n: b.clone() for n, b in bufs.items()}
                store.flat.copy_(live)
                store.seed.copy_(seed)
                for n, b in saved.items():
                    bufs[n].copy_(b)
                store.refresh()


def averager_for(cfg, model, optimizer):
    """the training loop's averager: None unless CONFIG.TRAIN.EMA.ENABLE; else the one cached on the model (created on first use, its
    settings following the config), attached to ``optimizer``"""
    if getattr(cfg.CONFIG.TRAIN, "EMA", None) is None:          # a config node built without this module's defaults
        return None
    s = ema_settings(cfg)
    if not s["enable"]:
        return None
    model = _bare(model)
    want = {k: s[k] for k in ("mode", "decay", "warmup", "start", "period")}
    a = model.__dict__.get(KEY)
    if a is None or a.store is not model.engine()[0]:
        a = WeightAverage(model, **want)
    elif a.settings() != want:
        a.configure(**want)
    if a.optimizer is not optimizer:
        a.attach(optimizer)
    model.__dict__[KEY] = a
    return a


def eval_context(cfg, model):
    """``applied()`` of the model's averager when CONFIG.TRAIN.EMA.ENABLE and .EVAL are set and it has one; else a null context"""
    E = getattr(cfg.CONFIG.TRAIN, "EMA", None)
    a = averager_of(model)
    if E is None or a is None:
        return contextlib.nullcontext()
    s = ema_settings(cfg)
    return a.applied(model) if s["enable"] and s["eval"] else contextlib.nullcontext()
