"""One optimisation step of TubeR on the MI355X path -- the body of the reference's hot loop
(``train_tuber_detection``, utils/video_action_recognition.py:96-157) without its per-step host syncs:

    outputs = model(samples) ; loss_dict = criterion(outputs, targets) ; losses = sum_k w_k * loss_k
    optimizer.zero_grad() ; losses.backward() ; clip_grad_norm_(0.1) ; optimizer.step()

The reference additionally copies ``pred_logits`` to the host every step as a NaN probe (:140) and calls ``.item()`` five
times on rank 0 (:182-193); here a step has no device->host transfer at all (the Hungarian assignment runs on the device) and
logging reads the (still on-device) loss tensors only when asked to.
"""
import collections
import contextlib
import os

import torch

from . import ab
from .ddp import attach_reducer, broadcast_parameters, cut_windows
from .optim import FusedClipAdamW, adopt, build_param_groups
from .monitor import KEY as _MON_KEY, monitor_for
from .weight_avg import KEY as _AVG_KEY, averager_for


def deploy_model(model, cfg, is_tuber=True, device=None):
    """Counterpart of utils/model_utils.py:39-63, same call form (``deploy_model(model, cfg, is_tuber=True)``): selects this
    rank's GPU (``torch.cuda.set_device(cfg.DDP_CONFIG.GPU)``), moves the model there, and -- instead of wrapping it in
    ``DistributedDataParallel`` -- broadcasts rank 0's parameters / buffers and attaches the flat-gradient reducer (ddp.py)
    when a process group with more than one rank exists.  Then initialises the transformer from the DETR checkpoint
    ``CONFIG.MODEL.PRETRAIN_TRANSFORMER_DIR`` like the reference (:60-61); a blank path skips that step (the reference would
    fail in ``torch.load``; there are no checkpoints in an offline image).  Returns the (unwrapped) model."""
    import torch.distributed as dist
    gpu = getattr(cfg.DDP_CONFIG, "GPU", None)
    if device is not None:
        dev = torch.device(device)
    elif gpu is not None:
        dev = torch.device("cuda", int(gpu))
    else:
        dev = torch.device("cuda", torch.cuda.current_device())
    if dev.type == "cuda":
        torch.cuda.set_device(dev)        # every launch goes to the CURRENT device's stream with raw pointers: pin it (model_utils.py:45)
    model.to(dev)
    store, _ = model.engine()
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        broadcast_parameters(store)
    attach_reducer(store, force=bool(os.environ.get("TUBER_FORCE_DDP")))      # None with a single rank (unless forced)
    path = getattr(cfg.CONFIG.MODEL, "PRETRAIN_TRANSFORMER_DIR", "")
    if is_tuber and path:
        from .checkpoint import load_detr_weights
        print("loading detr")
        load_detr_weights(model, path, cfg)
    return model


def build_optimizer(model, cfg):
    T = cfg.CONFIG.TRAIN
    return FusedClipAdamW(build_param_groups(model, cfg), lr=T.LR, weight_decay=T.W_DECAY, model=model)


def train_step(model, criterion, optimizer, samples, targets, max_norm, epoch=0, cfg=None, accum=None, last=False):
    """One eager optimisation step.  ``optimizer``: a ``FusedClipAdamW``, or the object the reference script builds --
    ``torch.optim.AdamW(param_dicts, lr=..., weight_decay=...)`` (train_tuber_ava.py:58), adopted transparently (optim.adopt: shared
    ``param_groups``, state exposed as views) -- or any other ``torch.optim.Optimizer``, driven by the reference's literal sequence
    ``clip_grad_norm_`` + ``optimizer.step()`` on the gradient views (video_action_recognition.py:152-154).
    ``accum``: an accum.GradAccumulator -- this call is one micro-batch of its group (``last``: it ends the group early); only the
    group's last micro-batch folds the mean gradient and steps the optimizer, clipping applies to the mean.
    Returns (total loss tensor, loss dict) -- all on the device, nothing synchronised."""
    store, _ = model.engine()
    reducer = getattr(store, "reducer", None)
    fused = adopt(optimizer, model)
    role = accum.begin_micro(last) if accum is not None else None
    outputs = model(samples)
    if role is not None:
        accum.after_forward(role)          # BatchNorm running statistics: only micro-batch 0 of a group updates them
    loss_dict = criterion(outputs, targets)
    weight_dict = criterion.weight_dict
    if cfg is not None and epoch > cfg.CONFIG.LOSS_COFS.WEIGHT_CHANGE:          # video_action_recognition.py:145-146
        weight_dict["loss_ce"] = cfg.CONFIG.LOSS_COFS.LOSS_CHANGE_COF
    losses = criterion.weighted_total(loss_dict, weight_dict)
    store.zero_grad()                      # optimizer.zero_grad() of a stock optimizer would drop the views into the flat buffer
    if role in ("first", "middle"):
        store.reducer = None               # no collective before the group's last micro-batch (DDP's no_sync)
        try:
            losses.backward()
        finally:
            store.reducer = reducer
        accum.after_backward(role)
        accum.end_micro()
        return losses.detach(), loss_dict
    if reducer is not None:
        with reducer.step(fold=accum.fold if role == "last" else None):    # each window folded right before its all-reduce is issued
            losses.backward()
            reducer.finish()
    else:
        losses.backward()
        if role == "last":
            accum.fold()
    if fused is not None:
        fused.step(max_norm=max_norm if max_norm and max_norm > 0 else None)
    else:
        if max_norm and max_norm > 0:
            torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)
        optimizer.step()
        avg = model.__dict__.get(_AVG_KEY)
        if avg is not None and avg.drives(optimizer):
            avg.update()                   # an optimizer the averaging launch cannot ride in: averaged eagerly behind its step
        mon = model.__dict__.get(_MON_KEY)
        if mon is not None and mon.drives(optimizer):
            mon.probe()                    # likewise the step monitor: the unconditional form, without moments
    if accum is not None:
        accum.end_micro()
    return losses.detach(), loss_dict


class _Snapshot:
    """Everything a training step mutates: parameters, BatchNorm buffers, Adam moments + step count, dropout seed.  The captured
    step needs eager warm-up passes (workspace sizing, reduce tables); they must not count as optimisation steps."""

    def __init__(self, model, store, opt, extra=()):
        self.items = [(store.flat, store.flat.clone()), (store.seed, store.seed.clone()), (opt.exp_avg, opt.exp_avg.clone()),
                      (opt.exp_avg_sq, opt.exp_avg_sq.clone()), (opt.t_dev, opt.t_dev.clone())]
        self.items += [(b, b.clone()) for b in model.buffers()]
        self.items += [(t, t.clone()) for t in extra if t is not None]       # gradient accumulation: acc, BatchNorm snapshot, fold scale
        avg = getattr(opt, "averager", None)
        if avg is not None:                                                  # weight averaging: the warm-up passes are no updates either
            self.items += [(t, t.clone()) for t in (avg.avg, avg.n_avg)]
        mon = getattr(opt, "monitor", None)
        if mon is not None:                                                  # step monitor: the warm-up passes record nothing
            self.items.append((mon.mem, mon.mem.clone()))

    def restore(self):
        with torch.no_grad():
            for live, saved in self.items:
                live.copy_(saved)


def _capture_plan(red):
    """(in_graph, split, cut_stages) of a capture, from the environment at capture time.  ``red``: the reducer the step all-reduces
    through, or None.
      TUBER_RCCL_IN_GRAPH=1      the collectives are captured into the one graph as a forked branch (own RCCL communicator only)
      TUBER_NO_SPLIT_GRAPH=1     a reducer without in-graph collectives: one graph, the all-reduce after it (else the graph is cut)
      TUBER_FORCE_SPLIT_GRAPH=1  cut the graph even without a reducer (tests: the cut graphs equal the single graph)
      TUBER_DDP_CUTS=4,3         the CSN stages whose backward ends at a cut (backbone.CSNRunner.cut_stages; (3,) when not cut)"""
    env = os.environ.get
    in_graph = red is not None and red.comm is not None and bool(env("TUBER_RCCL_IN_GRAPH"))
    split = (red is not None and not in_graph and not env("TUBER_NO_SPLIT_GRAPH")) or bool(env("TUBER_FORCE_SPLIT_GRAPH"))
    cut_stages = tuple(int(x) for x in env("TUBER_DDP_CUTS", "4,3").split(",") if x) if split else (3,)
    return in_graph, split, cut_stages


class _Captured:
    """One captured step of GraphedTrainStep: its graphs, the device buffers they read and write, and how its replay drives the reducer."""

    def __init__(self, red, in_graph, clips, mask, pt):
        self.red = red                  # ddp.FlatGradReducer the step all-reduces through (None: no reducer, or not a group's last micro-batch)
        self.in_graph = in_graph        # the collectives are part of graph A (TUBER_RCCL_IN_GRAPH); else the replay issues them
        self.clips = clips              # [B,3,T,H,W] fp32 input buffer the graphs read (GraphedTrainStep.input_buffers)
        self.mask = mask                # [B,H,W] bool padding mask buffer
        self.pt = pt                    # criterion.PaddedTargets: the padded [B, Tmax] targets, refilled before every replay
        self.A = None                   # first (or only) graph: weight refresh, forward, matching cost, ...
        self.B1 = None                  # host assignment only: criterion + backward (+ clip + AdamW), replayed after the host solve
        self.B2 = None                  # clip + AdamW behind the all-reduce (a reducer without in-graph collectives)
        self.parts = []                 # cut step: the graph parts after each cut, in replay order
        self.A2 = None                  # cut step: the last of ``parts`` (None: not cut)
        self.cuts = []                  # cut step: flat gradient offset of each cut, descending
        self.windows = None             # per issue point, the [lo, hi) windows of the flat gradient final there (ddp.cut_windows)
        self.flag_edges = frozenset()   # issue points ordered by a device counter instead of an event (FlatGradReducer.flag_points)
        self.on_device = True           # the Hungarian assignment runs on the device (cost within tuber_lsap_device's 128 x 128)
        self.logits_s = self.logits_b = self.boxes_s = self.cost = None     # forward outputs the criterion and matcher read
        self.match = None               # int32 [L, B, Tmax]: query matched to each target (-1: none)
        self.match_host = self.cost_host = None                            # host assignment only: pinned staging buffers
        self.loss = None                # total loss of the last replay (device)
        self.loss_dict = None           # its terms (device)


class CaptureFailed(RuntimeError):
    """the hipGraph capture of a training step did not complete (the eager step remains available)"""


_FROZEN_TAG = "frozen_bn"
_AVG_TAG = "weight_avg"
_MON_TAG = "step_monitor"


def _momenta(key):
    """the BatchNorm momentum part of a GraphedTrainStep key (a tuple behind the fixed five entries; the role is a string), or ()"""
    return next((e for e in key[5:] if isinstance(e, tuple) and e[:1] not in ((_FROZEN_TAG,), (_AVG_TAG,), (_MON_TAG,))), ())


def _frozen(key):
    """the frozen-BatchNorm part of a GraphedTrainStep key: (tag, layer indices) behind the fixed five entries, or ()"""
    return next((e for e in key[5:] if isinstance(e, tuple) and e[:1] == (_FROZEN_TAG,)), ())


def _averaged(key):
    """the weight-averaging part of a GraphedTrainStep key: (tag, averager serial) behind the fixed five entries, or ()"""
    return next((e for e in key[5:] if isinstance(e, tuple) and e[:1] == (_AVG_TAG,)), ())


def _monitored(key):
    """the step-monitor part of a GraphedTrainStep key: (tag, monitor serial) behind the fixed five entries, or ()"""
    return next((e for e in key[5:] if isinstance(e, tuple) and e[:1] == (_MON_TAG,)), ())


class GraphedTrainStep:
    """The same optimisation step replayed from ONE captured hipGraph (HIP graphs instead of a tracing compiler): bf16 weight
    refresh, forward of the whole model, matching-cost kernel, Hungarian assignment on the device (tuber_lsap_device), fused
    criterion (losses + output gradients), backward of the whole model, global-norm clip + AdamW.

    ~1600 kernel launches per step are issued by the GPU front-end instead of Python, so the step is GPU-bound.

    Everything that changes from batch to batch or epoch to epoch is read from DEVICE memory by the captured kernels and
    refreshed in ``__call__`` before the replay: the clips and their padding mask, the padded [B, Tmax] targets (boxes, labels,
    counts and -- JHMDB/UCF -- key-frame positions and visibility labels), the per-group learning rate / weight decay
    (``lr_scheduler.step()`` keeps working), the loss weights (the ``epoch > WEIGHT_CHANGE`` switch), the dropout seed and the
    AdamW step count.  A new clip shape or a changed set of frozen parameters captures a new graph (the eager warm-up passes of
    a capture are rolled back, so they are not optimisation steps); at most ``max_graphs`` graphs are kept (LRU).

    With > 1 rank (ddp.py) the step is graph A (refresh .. layer4's backward) -> RCCL all-reduce, on the reducer's own stream, of the
    ~58 % of the gradient buffer that is final at that point (transformer, heads, class branch, layer4, pool decoder) -> graph A1
    (layer3's backward, a latency-bound chain that leaves HBM and most CUs to the collective) -> all-reduce of layer3's 38 % ->
    graph A2 (layer2 / layer1 / stem backward) -> all-reduce of the remainder -> graph B2 (clip + AdamW), which waits for the side
    stream by event.  ``TUBER_DDP_CUTS=3`` restores the single cut of rounds 2-5 (97 % under layer2 / layer1 / stem); with
    ``TUBER_RCCL_IN_GRAPH=1`` the collectives are captured into ONE graph as a forked branch instead.

    ``accum_steps = k > 1`` (accum.py): every call is one micro-batch; its role in the group is part of the graph key.  "first":
    zero_grad, forward, BatchNorm snapshot, backward, acc = g; "middle": forward, BatchNorm restore, backward, acc += g (no collective);
    "last": forward, BatchNorm restore, backward, g = (acc + g) / m -- per window right before its all-reduce when a reducer is attached --
    then clip + AdamW + the bf16 refresh of the next forward.  ``last=True`` ends a group early (1/m is read from the device).
    """

    def __init__(self, model, criterion, optimizer, max_norm, tmax=16, max_graphs=4, accum_steps=1):
        fused = adopt(optimizer, model)
        if fused is None:
            raise TypeError("GraphedTrainStep needs AdamW (FusedClipAdamW or a stock torch.optim.AdamW); got %s" % type(optimizer).__name__)
        self.model, self.criterion, self.optimizer = model, criterion, fused
        self.max_norm, self.tmax, self.max_graphs = max_norm, tmax, max_graphs
        self.graphs = collections.OrderedDict()
        self.part_marks = None
        self.accum = None
        if int(accum_steps) != 1:
            from .accum import GradAccumulator
            self.accum = GradAccumulator(model.engine()[0], accum_steps)
            self.max_graphs = 4 * max_graphs          # per clip shape: the first / middle / last graphs and the group-of-one graph

    # -- capture -------------------------------------------------------------------------------------------------------------
    def _capture(self, clips, mask, targets, tmax, role=None):
        """capture with the cyclic garbage collector parked: a collection that runs INSIDE a stream capture may destroy the hipGraph /
        device tensors of an earlier step object (reference cycles through autograd nodes keep them until the collector runs), and the
        runtime aborts the process on such a call while a capture is open (seen in the GPU suite: "Fatal Python error: Aborted",
        Garbage-collecting, under test_deferred_weight_gradient_reductions_are_bit_identical).  Collected once up front instead."""
        import gc
        gc.collect()
        was_enabled = gc.isenabled()
        gc.disable()
        try:
            return self._capture_impl(clips, mask, targets, tmax, role)
        finally:
            if was_enabled:
                gc.enable()

    def _capture_impl(self, clips, mask, targets, tmax, role=None):
        from .criterion import PaddedTargets
        from .misc import NestedTensor
        model, crit, opt = self.model, self.criterion, self.optimizer
        store, runner = model.engine()
        dev = store.device
        acc = self.accum
        keep = getattr(store, "reducer", None)
        stepping = role not in ("first", "middle")
        red = keep if stepping else None             # no collective before a group's last micro-batch
        ddp = red is not None                        # N > 1 ranks (or a forced one-rank communicator): gradients are all-reduced
        in_graph, split, cut_stages = _capture_plan(red)
        own_step = not ddp or in_graph               # clip + AdamW inside the main graph (else graph B2, behind the all-reduce)
        fold = acc.fold if role == "last" else None  # with a reducer: each window folded right before its all-reduce (pre_reduce)
        g = _Captured(red, in_graph, clips.clone(), mask.clone(),
                      PaddedTargets(targets, crit.ava, crit.num_classes if crit.ava else crit.num_classes + 1, dev, tmax=tmax))
        max_norm = self.max_norm if self.max_norm and self.max_norm > 0 else None

        def head():
            outputs = model(NestedTensor(g.clips, g.mask))
            if role is not None:
                acc.after_forward(role)              # BatchNorm running statistics: snapshot (first) / restore (middle, last)
            logits, logits_b, boxes = crit.stacked(outputs)
            g.logits_s, g.boxes_s = crit.select(logits, boxes, g.pt)
            g.logits_b = logits_b
            with torch.no_grad():
                g.cost = crit.matcher.cost(g.logits_s.detach().contiguous(),
                                           (logits_b if crit.ava else g.logits_s).detach().contiguous(),
                                           g.boxes_s.detach().contiguous(), g.pt)

        def tail(step):
            g.loss_dict = crit.losses_from_match(g.logits_s, g.logits_b, g.boxes_s, g.pt, g.match)
            g.loss_dict["class_error"] = crit.class_error(g.logits_s[-1], g.pt, g.match[-1])
            g.loss = crit.weighted_total(g.loss_dict)
            opt.zero_grad()
            if in_graph:
                # the reducer's hooks fork its side stream off this stream inside the backward: the all-reduces (+ averaging) become a
                # parallel branch that joins before clip + AdamW
                with red.step(fold=fold):
                    g.loss.backward()
                    red.finish()
            else:
                g.loss.backward()
            if role in ("first", "middle"):
                acc.after_backward(role)
            elif role == "last" and not ddp:
                acc.fold()
            if step:
                opt.step(max_norm=max_norm)

        def step_body(step):
            head()
            g.match = crit.assign(g.cost, g.pt)
            tail(step)

        # eager warm-up with the reducer detached (its hooks must not fire inside a stream capture, and it flushes the deferred
        # reductions per bottleneck where the captured backward flushes twice): sizes every workspace, builds the reduce tables and
        # the loss-weight / hyper-parameter device tables.  Rolled back afterwards -- a capture is not an optimisation step.
        snap = _Snapshot(model, store, opt, () if acc is None else (acc.acc, acc.bn_arena, acc.scale_dev))
        store.reducer = red if in_graph else None
        # where the backward makes its gradient windows final (backbone.CSNRunner._backward_blocks): fixed BEFORE the warm-up passes so
        # that they and the capture issue the same weight-gradient groups and deferred-reduce tables
        runner.cut_stages = cut_stages
        if in_graph:
            red.dry = True                           # hooks fire (same deferred-reduce flush points as the capture), nothing is sent
        try:
            for _ in range(2):
                step_body(stepping)
            torch.cuda.synchronize()
        finally:
            snap.restore()
            if in_graph:
                red.dry = False
        opt.sync_hyper()
        crit.sync_weights(dev)
        g.on_device = g.cost.shape[2] <= 128 and g.cost.shape[3] <= 128      # the bound of tuber_lsap_device (criterion.assign)
        g.A = torch.cuda.CUDAGraph()
        if in_graph:
            with torch.cuda.graph(g.A, capture_error_mode="relaxed"):      # RCCL may touch the runtime while enqueuing
                step_body(own_step and stepping)
        elif split and g.on_device:
            # DDP: the graph is CUT inside the backward pass where a gradient window becomes final, so that window's RCCL all-reduce runs
            # on the reducer's stream under the backward of the stages below it.  Default cuts (TUBER_DDP_CUTS=4,3): (1) where layer4's
            # backward ends -- transformer + heads + class branch + layer4 + pool decoder, ~58 % of the bytes, go under layer3's
            # latency-bound chain, which leaves HBM and most CUs idle; (2) where layer3's backward ends -- layer3's 19 M parameters go
            # under layer2 / layer1 / stem; the ~1.5 M tail after the last graph.  (Until round 5 the only cut was (2): the whole 97 % ran
            # beside the bandwidth-bound layer2 / layer1 backward and cost a rank 0.77 ms of contention with nothing on the wire.)
            cut = []
            graphs = [g.A]
            # issue points ordered by a device-memory counter instead of an event (ddp.FlatGradReducer.flag_points): by default the FIRST
            flag_edges = red.flag_points() if red is not None else frozenset()
            torch.cuda.synchronize()
            cs = torch.cuda.Stream()
            cs.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(cs):
                g.A.capture_begin(capture_error_mode="relaxed")      # the cuts happen on autograd's worker thread

                def hook(off):
                    if len(cut) in flag_edges:
                        red.signal(len(cut))                         # last node of this part: the windows above are final
                    graphs[-1].capture_end()
                    cut.append(int(off))
                    nxt = torch.cuda.CUDAGraph()
                    nxt.capture_begin(pool=g.A.pool(), capture_error_mode="relaxed")
                    graphs.append(nxt)
                runner.split_hook = hook
                try:
                    step_body(own_step and stepping)
                finally:
                    runner.split_hook = None
                if len(cut) in flag_edges and not own_step and cut:  # (no cut -- a frozen body: one event-ordered window after the graph)
                    red.signal(len(cut))                             # end of backward: the remainder is final
                graphs[-1].capture_end()
            torch.cuda.current_stream().wait_stream(cs)
            g.parts, g.cuts = graphs[1:], cut
            g.A2 = graphs[-1] if cut else None
            g.flag_edges = flag_edges if cut else frozenset()
        elif g.on_device:
            with torch.cuda.graph(g.A):
                step_body(own_step and stepping)
        else:
            # assignment problems beyond the device solver's 128 x 128 bound: graph A (head) / tuber_lsap on the host / graph B1 (tail)
            with torch.cuda.graph(g.A):
                head()
            L, B = g.cost.shape[:2]
            g.match = torch.full((L, B, g.pt.tmax), -1, dtype=torch.int32, device=dev)
            g.match_host = torch.full((L, B, g.pt.tmax), -1, dtype=torch.int32).pin_memory()
            g.cost_host = torch.empty(g.cost.shape, dtype=torch.float32).pin_memory()
            g.B1 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g.B1, pool=g.A.pool()):
                tail(own_step and stepping)
        store.reducer = keep
        if not own_step:
            g.B2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g.B2, pool=g.A.pool()):
                opt.step(max_norm=max_norm)
        g.windows = cut_windows(g.cuts, runner.body_begin, store.total) if g.cuts else [[(0, store.total)]]
        return g

    def _key(self, shape, tmax, role=None):
        """graph key: clip shape, set of trainable tensors, train / eval criterion, padded target layout, the decoder's launch form (a
        captured step bakes it in: after a timed-out cooperative launch -- engine.coop_failed -- a new one is captured)[, the BatchNorm
        momenta that differ from the reference's 0.1 (baked into the finalisation launches: a changed momentum captures a new step; absent
        while every module has 0.1)][, the frozen BatchNorm layers (modules in eval mode: their launches differ; absent while every module
        trains, so freezing or unfreezing a layer captures a new step)][, the weight averager attached to the optimizer (its launch and
        addresses are part of the optimizer step; absent while none is attached)][, the step monitor attached to the optimizer (likewise)]
        [, accumulation role]"""
        store, runner = self.model.engine()
        key = (tuple(shape), store.trainable_signature(), self.criterion.training, tmax, store.coop_off)
        mom = runner.momentum_signature()
        if mom:
            key += (mom,)
        frz = runner.frozen_signature()
        if frz:
            key += ((_FROZEN_TAG, frz),)
        avg = getattr(getattr(self, "optimizer", None), "averager", None)
        if avg is not None:
            key += ((_AVG_TAG, avg.serial),)
        mon = getattr(getattr(self, "optimizer", None), "monitor", None)
        if mon is not None:
            key += ((_MON_TAG, mon.serial),)
        return key if role is None else key + (role,)

    def _wider(self, shape, tmax=0):
        """the first captured key for this clip shape whose padded target layout holds ``tmax`` boxes per clip (any role), or None"""
        want = self._key(shape, tmax)
        return next((k for k in self.graphs if k[:3] == want[:3] and k[3] >= tmax and k[4] == want[4] and _momenta(k) == _momenta(want)
                     and _frozen(k) == _frozen(want) and _averaged(k) == _averaged(want)
                     and _monitored(k) == _monitored(want)), None)

    def input_buffers(self, clips_shape):
        """(clips, mask) buffers the captured step for this clip shape reads, or None before its first call: a producer that fills them in
        place and passes them back to ``__call__`` saves the step its 67 MB device-to-device copy."""
        k = self._wider(clips_shape)
        return None if k is None else (self.graphs[k].clips, self.graphs[k].mask)

    # -- replay --------------------------------------------------------------------------------------------------------------
    def __call__(self, samples, targets, last=False):
        """``samples``: NestedTensor (clips + padding mask) or a plain [B,3,T,H,W] tensor (no padding).  ``last`` (accum_steps > 1): this
        micro-batch ends its group whatever its index."""
        store, _ = self.model.engine()
        acc = self.accum
        role = acc.begin_micro(last) if acc is not None else None
        if hasattr(samples, "tensors"):
            clips, mask = samples.tensors, samples.mask
        else:
            clips, mask = samples, None
        if mask is None:
            mask = torch.zeros(clips.shape[0], clips.shape[-2], clips.shape[-1], dtype=torch.bool, device=store.device)
        # the padded [B, Tmax] target layout is baked into the capture: a batch with more boxes per clip than any before (dense
        # AVA key frames) gets a graph with a wider layout instead of an error -- the reference has no such limit
        need = max([int(t["boxes"].shape[0]) for t in targets] + [1])
        tmax = max(self.tmax, (need + 15) // 16 * 16)
        wider = self._wider(clips.shape, tmax)                    # a captured wider layout serves narrower batches too
        key = self._key(clips.shape, tmax if wider is None else wider[3], role)
        g = self.graphs.get(key)
        if g is None:
            while len(self.graphs) >= self.max_graphs:            # LRU: a graph holds its own memory pool
                self.graphs.popitem(last=False)
            try:
                g = self._capture(clips.to(store.device, torch.float32), mask.to(store.device), targets, key[3], role)
            except (RuntimeError, ValueError) as e:
                raise CaptureFailed("%s: %s" % (type(e).__name__, e)) from e
            self.graphs[key] = g
        else:
            self.graphs.move_to_end(key)
        # a producer that writes straight into the captured buffers (``input_buffers``: the input pre-pass, bench.py's resident synthetic
        # clips) hands those very tensors back: nothing to copy then
        if clips.data_ptr() != g.clips.data_ptr():
            g.clips.copy_(clips, non_blocking=True)
        if mask.data_ptr() != g.mask.data_ptr():
            g.mask.copy_(mask, non_blocking=True)
        g.pt.refill(targets)
        self.optimizer.sync_hyper()
        if role in (None, "last"):
            self.optimizer.mark_stepped()
        self.criterion.sync_weights(store.device)
        sizes = g.pt.sizes
        red = None if g.in_graph else g.red                       # the replay drives the exchange (in-graph: graph A holds it)
        marks = self.part_marks                                   # bench.py: HIP-event stamps between the graph parts of the measured steps
        if marks is not None:
            marks.append([])
        with red.step(fold=acc.fold if role == "last" else None) if red is not None else contextlib.nullcontext():
            if marks is not None:
                self._mark()
            g.A.replay()
            if marks is not None:
                self._mark()
            if g.on_device:
                self.criterion._indices, self.criterion._match_dev = None, (g.match, sizes)
            else:
                g.cost_host.copy_(g.cost, non_blocking=True)
                torch.cuda.current_stream().synchronize()         # host assignment: the step's one host sync
                match, indices = self.criterion.matcher.solve(g.cost_host.numpy(), sizes)
                g.match_host.copy_(torch.from_numpy(match))
                g.match.copy_(g.match_host, non_blocking=True)
                L = len(indices)
                self.criterion.last_indices = [indices[L - 1]] + indices[:L - 1]
                g.B1.replay()
            # issue point i hands the windows final at cut i to the transport, then the backward of the stages below runs under it
            for i, part in enumerate(g.parts):
                if red is not None:
                    red.issue(i, g.windows[i], counter=i in g.flag_edges)
                part.replay()
                if marks is not None:
                    self._mark()
            if red is not None:
                red.issue(len(g.parts), g.windows[-1], counter=len(g.parts) in g.flag_edges)
                red.finish(rest=False)                            # the optimizer graph waits for the side stream (events only)
        if g.B2 is not None:
            g.B2.replay()
            if marks is not None:
                self._mark()
        if acc is not None:
            acc.end_micro()
        return g.loss, g.loss_dict

    def _mark(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.part_marks[-1].append(e)

    def part_ms(self):
        """mean duration (ms) of each graph part over the steps stamped since ``part_marks = []`` (syncs)"""
        torch.cuda.synchronize()
        rows = [[a.elapsed_time(b) for a, b in zip(m[:-1], m[1:])] for m in (self.part_marks or []) if len(m) > 1]
        self.part_marks = None
        if not rows:
            return None
        n = min(len(r) for r in rows)
        return [round(sum(r[i] for r in rows) / len(rows), 3) for i in range(n)]


class _DeviceMeters:
    """The reference's AverageMeters (class_err, losses_avg, losses_box, losses_giou, losses_ce, losses_ce_b:
    video_action_recognition.py:97-104,182-193), accumulated ON THE DEVICE -- every iteration contributes (weight = len(targets),
    like ``meter.update(value, len(targets))``), the host reads the six running averages only when it prints."""
    KEYS = ("class_error", "loss", "loss_bbox", "loss_giou", "loss_ce", "loss_ce_b")

    def __init__(self, device):
        self.sum = torch.zeros(len(self.KEYS), dtype=torch.float64, device=device)
        self.count = 0

    def update(self, loss, loss_dict, n):
        zero = loss.new_zeros(())
        vals = [loss if k == "loss" else loss_dict.get(k, zero) for k in self.KEYS]
        vals = [v.detach().reshape(()).to(loss.dtype) if torch.is_tensor(v) else loss.new_tensor(float(v)) for v in vals]
        self.sum.add_(torch.stack(vals).double(), alpha=float(n))
        self.count += n

    def averages(self):
        """{key: running average} -- ONE device->host read"""
        host = (self.sum / max(self.count, 1)).tolist()
        return dict(zip(self.KEYS, host))


def _graphed_for(model, criterion, optimizer, max_norm, accum_steps=1):
    """the cached GraphedTrainStep of (model, criterion, optimizer, max_norm[, accum_steps]), or None when the optimizer is not AdamW"""
    fused = adopt(optimizer, model)
    if fused is None:
        return None
    cache = model.__dict__.setdefault("_tuber_graphed", {})
    key = (id(criterion), id(fused), float(max_norm or 0.0))
    if accum_steps != 1:
        key = key + (int(accum_steps),)
    g = cache.get(key)
    if g is None:
        cache.clear()                       # one live training configuration per model: a graph owns its memory pool
        g = cache[key] = GraphedTrainStep(model, criterion, fused, max_norm, accum_steps=accum_steps)
    return g


def _accum_for(model, k):
    """the cached accum.GradAccumulator of the eager step for k micro-batches per optimizer step"""
    from .accum import GradAccumulator
    a = model.__dict__.get("_tuber_accum")
    if a is None or a.k != k or a.store is not model.engine()[0]:
        a = model.__dict__["_tuber_accum"] = GradAccumulator(model.engine()[0], k)
    return a


def accum_steps(cfg):
    """CONFIG.TRAIN.ACCUM_STEPS (micro-batches per optimizer step; 1 = off), validated"""
    k = int(getattr(cfg.CONFIG.TRAIN, "ACCUM_STEPS", 1))
    if k < 1:
        raise ValueError("CONFIG.TRAIN.ACCUM_STEPS must be >= 1, got %d" % k)
    return k


def train_tuber_detection(cfg, model, criterion, data_loader, optimizer, epoch, max_norm, lr_scheduler=None, writer=None,
                          graphed=None, print_freq=10):
    """One training epoch -- the reference's ``train_tuber_detection`` (utils/video_action_recognition.py:64-220), same argument
    list, on the HIP path.  ``optimizer`` is whatever the script built: the stock ``torch.optim.AdamW(param_dicts, ...)`` of
    train_tuber_ava.py:58 is adopted (optim.adopt), ``lr_scheduler`` stays bound to that object.

    Every batch is one replay of the captured hipGraph step (``GraphedTrainStep``, created on first use and cached on the model;
    ``graphed=False`` or ``TUBER_AB=eager_step`` forces the eager ``train_step``, which is also the fallback when a capture fails or
    the optimizer is not AdamW).  The six scalars the reference logs -- ``train/{class_error,totall_loss,loss_bbox,loss_giou,
    loss_ce,loss_ce_b}`` (:215-220), running averages weighted by ``len(targets)`` -- are accumulated on the device for EVERY
    iteration and read back every ``print_freq`` iterations, so the GPU queue stays full; a non-finite loss stops training like
    the reference (:195-198).  ``epoch > LOSS_COFS.WEIGHT_CHANGE`` switches ``loss_ce``'s weight (:145-146).

    ``CONFIG.TRAIN.ACCUM_STEPS = k > 1`` (accum.py): the optimizer steps every k batches on the mean gradient of the group -- an
    8-rank x 2-clip step on one GPU with k = 8 -- and once more on the trailing partial group (1/m) at the end of the epoch; the
    cosine ``lr_scheduler.step_update`` is called per optimizer step with the optimizer-step index.  Meters and the non-finite check
    stay per batch.

    ``CONFIG.TRAIN.EMA.ENABLE`` (weight_avg.py): an EMA / SWA of the weights is kept by one more launch behind every optimizer step -- in
    the captured step with AdamW, eagerly after any other optimizer; the averager is created on first use and cached on the model.

    ``CONFIG.TRAIN.MONITOR.ENABLE`` (monitor.py): per-tensor gradient / parameter / update statistics are recorded on the device every
    ``EVERY`` optimizer steps by launches behind the optimizer step; at the iterations where the loop syncs anyway (``print_freq``) rank 0
    writes the newest row's per-group ``monitor/{grad_norm,param_norm,update_ratio}/<group>`` and ``monitor/zero_grad_fraction`` to
    ``writer``, a row with non-finite parameters stops training on every rank, and the FloatingPointError of a non-finite loss names the
    tensors that were non-finite in the first skipped step."""
    import time
    k = accum_steps(cfg)
    averager_for(cfg, model, optimizer)
    monitor = monitor_for(cfg, model, optimizer)
    monitor_t = -1                                                # step count of the newest row already written to ``writer``
    model.train()
    criterion.train()
    dev = next(model.parameters()).device
    rank = getattr(cfg.DDP_CONFIG, "GPU_WORLD_RANK", 0)
    if epoch > cfg.CONFIG.LOSS_COFS.WEIGHT_CHANGE:
        criterion.weight_dict["loss_ce"] = cfg.CONFIG.LOSS_COFS.LOSS_CHANGE_COF
    if graphed is None and not ab.on("eager_step"):
        graphed = _graphed_for(model, criterion, optimizer, max_norm, accum_steps=k)
    elif graphed is False or graphed is None:
        graphed = None
    meters = _DeviceMeters(dev)
    end = time.time()
    loss = None
    store = model.engine()[0]
    tracker = _StepTracker(dev)
    import torch.distributed as _dist
    world = _dist.get_world_size() if _dist.is_available() and _dist.is_initialized() else 1
    n_iter = len(data_loader)
    if k > 1:
        from .accum import steps_per_epoch
        n_steps = steps_per_epoch(n_iter, k)
        if graphed is not None and getattr(graphed, "accum", None) is None:
            raise ValueError("ACCUM_STEPS = %d needs a GraphedTrainStep built with accum_steps=%d" % (k, k))
        accum = graphed.accum if graphed is not None else _accum_for(model, k)
        if accum.k != k:
            raise ValueError("ACCUM_STEPS = %d, but the step accumulates over %d micro-batches" % (k, accum.k))
        opt_step = accum.steps
    else:
        n_steps, accum = n_iter, None
    for idx, data in enumerate(data_loader):
        samples, targets = data[0], data[1]
        samples = samples.to(dev)            # reference :121; for an input_pipeline.ClipBatch this IS the HIP pre-pass (uint8 frames -> fp32 batch)
        targets = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in t.items() if k != "image_id"} for t in targets]
        last = idx + 1 == n_iter                                  # accumulation: the trailing partial group steps at the end of the epoch
        if accum is not None:
            steps_before = accum.steps
        if graphed is not None:
            try:
                loss, loss_dict = graphed(samples, targets, last=last)   # NestedTensor: clips AND padding mask go to the captured buffers
            except CaptureFailed as e:                            # a failed capture must not end the epoch
                if getattr(model.engine()[0], "reducer", None) is not None:
                    raise                                         # N > 1: every rank must stay on the same collective sequence
                import sys
                print("[tuber] hipGraph step unavailable (%s: %s); continuing with the eager step" % (type(e).__name__, e), file=sys.stderr, flush=True)
                graphed = None
                model.__dict__.pop("_tuber_graphed", None)
                loss, loss_dict = train_step(model, criterion, optimizer, samples, targets, max_norm, epoch=epoch, cfg=cfg, accum=accum, last=last)
        else:
            loss, loss_dict = train_step(model, criterion, optimizer, samples, targets, max_norm, epoch=epoch, cfg=cfg, accum=accum, last=last)
        if accum is None:
            stepped, opt_idx = True, idx
        else:
            stepped = accum.steps != steps_before
            opt_idx = accum.steps - 1 - opt_step
        if stepped and lr_scheduler is not None and cfg.CONFIG.TRAIN.LR_POLICY == "cosine":
            lr_scheduler.step_update(epoch * n_steps + opt_idx)
        if rank == 0:
            meters.update(loss, loss_dict, len(targets))
        # non-finite loss (reference :195-198 checks the rank-reduced loss on every rank, every iteration, BEFORE optimizer.step()): here the
        # optimizer's device-side guard skips the update of any step whose gradient norm is not finite (csrc/optim.hip), so nothing invalid is
        # ever applied, and the host learns about it from a device-side tracker updated on EVERY rank every step (no host-to-device copy, no
        # sync), MAX-reduced over the ranks and read on every rank, so that all ranks stop together instead of rank 0 raising while the
        # others wait in the next gradient all-reduce.  The collective is issued at iterations every rank reaches by
        # construction (idx % print_freq == 0 -- the same idx on every rank as long as the loaders have one length, which the gradient
        # all-reduce needs anyway) and once more after the loop; NOT at ``idx + 1 == n_iter``, which would pair with nothing on a rank whose
        # loader is longer.  The same tracker carries the cooperative decoder launch's error word: a timed-out
        # launch poisons its step with NaN (skipped like any other non-finite step); when ANY rank reports one, EVERY rank switches to
        # the launch chain at this same iteration and training continues.
        tracker.update(loss, store.coop_sync)
        if idx % print_freq == 0:
            if monitor is None:
                _check_tracker(tracker, store, loss_dict, epoch, idx, rank, world, _dist)  # (a captured step is keyed on store.coop_off: re-captured by itself)
            else:
                _check_tracker_monitored(monitor, tracker, store, loss_dict, epoch, idx, rank, world, _dist)
                monitor_t = _read_monitor(monitor, writer if rank == 0 else None, idx + epoch * n_iter, monitor_t, epoch, idx)
        if rank == 0 and (idx % print_freq == 0 or idx + 1 == n_iter):
            avg = meters.averages()
            lr = optimizer.param_groups[-1]["lr"]
            print("Epoch: [%d][%d/%d]" % (epoch, idx + 1, n_iter))
            print("lr: ", lr)
            print("batch time: %.3f" % (time.time() - end))
            print("class_error: {class_error:.3f}, loss: {loss:.3f}, loss_bbox: {loss_bbox:.3f}, loss_giou: {loss_giou:.3f}, "
                  "loss_ce: {loss_ce:.3f}, loss_ce_b: {loss_ce_b:.3f}".format(**avg))
            if writer is not None:
                it = idx + epoch * n_iter
                writer.add_scalar("train/class_error", avg["class_error"], it)
                writer.add_scalar("train/totall_loss", avg["loss"], it)          # (sic) the reference's tag, :216
                writer.add_scalar("train/loss_bbox", avg["loss_bbox"], it)
                writer.add_scalar("train/loss_giou", avg["loss_giou"], it)
                writer.add_scalar("train/loss_ce", avg["loss_ce"], it)
                writer.add_scalar("train/loss_ce_b", avg["loss_ce_b"], it)
        end = time.time()
    if loss is not None:
        if monitor is None:
            _check_tracker(tracker, store, loss_dict, epoch, n_iter - 1, rank, world, _dist)
        else:
            _check_tracker_monitored(monitor, tracker, store, loss_dict, epoch, n_iter - 1, rank, world, _dist)
            _read_monitor(monitor, None, 0, monitor_t, epoch, n_iter - 1)
    return loss


def _read_monitor(monitor, writer, it, seen, epoch, idx):
    """The step monitor at an iteration that has just synchronised (one device-to-host read).  Non-finite PARAMETERS -- in the newest recorded
    row, or in the table of the first skipped step -- stop training: a NaN weight that the loss does not see (a box head whose NaN boxes
    merely stay unmatched) would otherwise skip or poison every step from here on.  Every rank holds the same parameters and records the
    same tables, so all ranks stop at this iteration.  With a ``writer`` a row newer than step ``seen`` goes out as ``monitor/*`` scalars.
    Returns the step count of the newest row seen so far."""
    rows, bad = monitor.read()
    new = bool(rows) and rows[0][0] > seen
    for where, table in ((("the first skipped step, after optimizer step %d (%d skipped since)" % bad[:2], bad[2]),) if bad else ()) + \
                        ((("optimizer step %d" % rows[0][0], rows[0][3]),) if new else ()):
        params = monitor.nonfinite_names(table, "param")
        if params:
            raise FloatingPointError("step monitor: %d tensor(s) with a non-finite parameter in %s (seen at epoch %d, iteration %d), first %s; "
                                     "tensors with a non-finite gradient there: %d, first %s"
                                     % (len(params), where, epoch, idx, params[:20], len(monitor.nonfinite_names(table, "grad")),
                                        monitor.nonfinite_names(table, "grad")[:20]))
    if not new:
        return seen
    if writer is not None:
        for name, s in monitor.summary(rows[0]).items():
            if name == "all":
                writer.add_scalar("monitor/zero_grad_fraction", s["zero_grad_fraction"], it)
            else:
                for k in ("grad_norm", "param_norm", "update_ratio"):
                    writer.add_scalar("monitor/%s/%s" % (k, name), s[k], it)
    return rows[0][0]


def _check_tracker_monitored(monitor, *args):
    """``_check_tracker`` whose FloatingPointError also says WHERE the first skipped step was non-finite (monitor.StepMonitor.bad)"""
    try:
        switched = _check_tracker(*args)
        if switched:
            monitor.clear_bad()              # the steps a timed-out cooperative launch poisoned are explained: re-arm the bad slot
        return switched
    except FloatingPointError as e:
        bad = monitor.bad()
        if bad is None:
            raise
        step, count, table = bad
        grads, params = monitor.nonfinite_names(table, "grad"), monitor.nonfinite_names(table, "param")
        raise FloatingPointError("%s; step monitor: the first skipped step followed optimizer step %d (bad_step), %d step(s) skipped since "
                                 "(bad_count); %d tensor(s) with a non-finite gradient, first %s; %d tensor(s) with a non-finite parameter, "
                                 "first %s" % (e, step, count, len(grads), grads[:20], len(params), params[:20])) from e


class _StepTracker:
    """Device-side record of what went wrong since the last check: [a non-finite loss was seen, -(first such iteration + 1), the cooperative
    decoder launch's error word].  The iteration is stored NEGATED (initially -inf) so that the MAX all-reduce over the ranks yields the
    FIRST offending iteration of any rank; the counter lives on the device (no per-step host-to-device copy)."""

    def __init__(self, device):
        self.device = device
        self.reset()

    def reset(self):
        self.state = torch.tensor([0.0, float("-inf"), 0.0], dtype=torch.float32, device=self.device)
        self.it = torch.zeros((), dtype=torch.float32, device=self.device)

    def update(self, loss, coop_sync):
        bad = (~torch.isfinite(loss.detach())).reshape(()).to(torch.float32)
        self.it = self.it + 1.0
        first = torch.where((self.state[0] == 0) & (bad > 0), -self.it, self.state[1])
        self.state = torch.stack([torch.maximum(self.state[0], bad), first, torch.maximum(self.state[2], coop_sync[2].to(torch.float32))])


def _check_tracker(tracker, store, loss_dict, epoch, idx, rank, world, _dist):
    """MAX-reduce the tracker over the ranks (the only host sync of the loop).  A timed-out cooperative decoder launch on any rank: every
    rank clears its words, switches to the launch chain and goes on (returns True; the poisoned steps were skipped by the optimizer on
    every rank -- the NaN gradients reached the others through the all-reduce).  Otherwise a non-finite loss stops every rank together."""
    state = tracker.state
    if world > 1:
        _dist.all_reduce(state, op=_dist.ReduceOp.MAX)
    flag, negfirst, coop = state.tolist()
    if coop:
        if not store.coop_failed():          # another rank's launch failed: same switch here, so that all ranks run the same launch sequence
            store.coop_sync.zero_()
            store.coop_off = True
        tracker.reset()
        return True
    if flag:
        losses = {k: float(v.detach()) if torch.is_tensor(v) else v for k, v in loss_dict.items()}
        print("Loss is non-finite on some rank, stopping training")
        print(losses)
        raise FloatingPointError("non-finite loss first seen at epoch %d, iteration %d (checked at iteration %d, rank %d of %d; this rank's "
                                 "last loss terms: %s); steps with a non-finite gradient norm were skipped by the optimizer, the weights hold "
                                 "the last finite update" % (epoch, int(-negfirst) - 1, idx, rank, world, losses))
    return False
