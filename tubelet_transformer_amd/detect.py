"""Inference surface: a captured eval forward (``GraphedEval``) and ranked detections decoded on the device (``Detector``).

``PostProcessAVA.decode`` / ``PostProcess.decode`` (criterion.py) return the dense ``[B, Q, C]`` score tables a frame-mAP evaluator wants.
A user who wants boxes, labels and scores of a clip wants the few rows above a threshold, best first.  ``decode_topk_host`` below is the
DEFINITION of that result, in numpy; ``csrc/detect.hip`` computes it in one launch per batch from the raw head outputs.

AVA rule (``mode="ava"``): ``pb = softmax(logits_b)[1]``; a query passes the gate when ``pb > actor_thr`` (strictly, the reference's
``> 0.8``); ``score(q, c) = sigmoid(logit) * pb``; a candidate is a (q, c) of a gated query whose score is not NaN and ``>= score_thr``.
The best K are kept by score descending, then q ascending, then c ascending; ``aux`` is ``pb``.

JHMDB / UCF101-24 rule (any other mode; ``PostProcess.decode`` plus the counted-once rule of ``evaluation.FrameMAPUCF``): logits carry the
no-object column last.  A query's label is the first maximum of its fp32 LOGIT row, a NaN counting as a maximum (``np.argmax``).  That
equals the arg-max over ``decode()``'s probabilities whenever those have no duplicated maximum: softmax is monotone, so the probabilities'
maxima sit where the logits' do, and only rounding can merge two distinct logits into one duplicated probability, which moves neither
first maximum unless it creates a new tie in front.  The score is that column's softmax probability; a row is a candidate unless its label
is the no-object column, its score is NaN or ``< score_thr``.  Order: score descending, then q ascending; ``aux`` is the visibility
probability ``softmax(logits_b)[1]`` (one per clip in the model's outputs).

Tie rule: equal scores keep (q, c) ascending, and K cuts by that order -- ``fmap_key(score, q * C + c)`` of csrc/map_common.h.
``queries`` index the clip's slice of ``Qs`` queries starting at ``q_begin`` (the key frame's queries of a tubelet model).  Rows at and
after ``count[b]`` are box 0, score 0, aux 0, label -1, query -1, so whole buffers compare equal.

Fail-safe: a timed-out cooperative decoder launch poisons the forward's outputs with NaN; NaN scores are never candidates, so such a batch
has ``count == 0`` until ``Detections.to_host()`` -- the only place that synchronises -- reads the error word and runs the batch again on
the launch chain.
"""
import os
import numpy as np
import torch

from . import ab, lib
from .misc import NestedTensor, nested_tensor_from_tensor_list

FIELDS = ("boxes", "scores", "labels", "queries", "aux", "count", "total")
ACTOR_FIELDS = ("boxes", "actor", "queries", "actions", "count", "total")


# ---------------------------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------------------------
def _softmax64(x):
    x = x.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(x - np.max(x, axis=-1, keepdims=True))
        return e / e.sum(axis=-1, keepdims=True)


def boxes_xyxy_f32(boxes, sizes):
    """box_ops.box_cxcywh_to_xyxy and the multiply by (w, h, w, h) of decode(), in fp32 numpy: one rounding per operation, as torch's"""
    bx = np.asarray(boxes, dtype=np.float32)
    sz = np.asarray(sizes, dtype=np.float32)
    cx, cy, w, h = bx[..., 0], bx[..., 1], bx[..., 2], bx[..., 3]
    half = np.float32(0.5)
    xyxy = np.stack([cx - half * w, cy - half * h, cx + half * w, cy + half * h], axis=-1)
    H, W = sz[:, 0], sz[:, 1]
    return (xyxy * np.stack([W, H, W, H], axis=1)[:, None, :]).astype(np.float32)


def decode_topk_host(logits, logits_b, boxes, sizes, mode, actor_thr, score_thr, K, q_begin=None, Qs=None):
    """The ranked detections of a batch (module docstring), in numpy: probabilities in fp64 from the fp32 inputs, boxes in fp32.
    logits [B, Qtot, C] (ava) or [B, Qtot, C + 1]; logits_b [B, Qtot, NB] or [B, NB]; boxes [B, Qtot, 4] cxcywh; sizes [B, 2] (h, w).
    Returns a dict of the ``FIELDS`` arrays: boxes [B, K, 4] f32, scores / aux [B, K] f32, labels / queries [B, K] i32, count / total [B] i32."""
    lg = np.asarray(logits, dtype=np.float32)
    lb = np.asarray(logits_b, dtype=np.float32)
    B, Qtot = lg.shape[0], lg.shape[1]
    Qs = Qtot if Qs is None else int(Qs)
    K = int(K)
    qb = np.zeros(B, dtype=np.int64) if q_begin is None else np.asarray(q_begin, dtype=np.int64).reshape(B)
    pix = boxes_xyxy_f32(boxes, sizes)
    ava = mode == "ava"
    C = lg.shape[2] if ava else lg.shape[2] - 1
    pb_all = _softmax64(lb)[..., 1]                                    # [B, Qtot] or [B]
    out = dict(boxes=np.zeros((B, K, 4), np.float32), scores=np.zeros((B, K), np.float32), labels=np.full((B, K), -1, np.int32),
               queries=np.full((B, K), -1, np.int32), aux=np.zeros((B, K), np.float32), count=np.zeros(B, np.int32), total=np.zeros(B, np.int32))
    for b in range(B):
        q0 = int(qb[b])
        if q0 < 0 or q0 + Qs > Qtot:                                   # a slice outside the clip's queries: an empty result
            continue
        rows = lg[b, q0:q0 + Qs]
        pb = pb_all[b, q0:q0 + Qs] if pb_all.ndim == 2 else np.full(Qs, pb_all[b])
        if ava:
            with np.errstate(over="ignore"):
                s = (1.0 / (1.0 + np.exp(-rows.astype(np.float64)))) * pb[:, None]
            ok = (pb[:, None] > actor_thr) & ~np.isnan(s) & (s >= score_thr)
            qq, cc = np.nonzero(ok)                                    # (q, c) ascending
            sc = s[qq, cc]
        else:
            lab = np.argmax(rows, axis=1)                              # the first maximum, a NaN counting as one
            p = _softmax64(rows)[np.arange(Qs), lab]
            ok = (lab != C) & ~np.isnan(p) & (p >= score_thr)
            qq = np.nonzero(ok)[0]
            cc, sc = lab[qq], p[qq]
        order = np.argsort(-sc, kind="stable")[:K]                     # score descending, equal scores in (q, c) order
        n = len(order)
        out["total"][b], out["count"][b] = len(sc), n
        qq, cc = qq[order], cc[order]
        out["boxes"][b, :n] = pix[b, q0 + qq]
        out["scores"][b, :n] = sc[order].astype(np.float32)
        out["labels"][b, :n], out["queries"][b, :n] = cc, qq
        out["aux"][b, :n] = pb[qq].astype(np.float32)
    return out


def _decode_topk_torch(logits, logits_b, boxes, sizes, mode, actor_thr, score_thr, K, q_begin, Qs):
    """``decode_topk_host`` restated in torch on the inputs' device (fp64 probabilities, a stable sort): the path of shapes beyond the
    kernel's bounds.  No host synchronisation."""
    from . import box_ops
    dev = logits.device
    B, Qtot = logits.shape[0], logits.shape[1]
    lg, lb, bx = logits.float(), logits_b.float(), boxes.float()
    h, w = sizes.to(dev, torch.float32).unbind(1)
    pix = box_ops.box_cxcywh_to_xyxy(bx) * torch.stack([w, h, w, h], dim=1)[:, None, :]
    qb = torch.zeros(B, dtype=torch.int64, device=dev) if q_begin is None else q_begin.to(dev, torch.int64)
    valid = (qb >= 0) & (qb + Qs <= Qtot)
    rows = (torch.where(valid, qb, torch.zeros_like(qb))[:, None] + torch.arange(Qs, device=dev)[None, :])          # [B, Qs]
    lg = torch.gather(lg, 1, rows[:, :, None].expand(B, Qs, lg.shape[2]))
    pix = torch.gather(pix, 1, rows[:, :, None].expand(B, Qs, 4))
    pb = lb.double().softmax(-1)[..., 1]
    pb = torch.gather(pb, 1, rows) if pb.dim() == 2 else pb[:, None].expand(B, Qs)
    if mode == "ava":
        C = lg.shape[2]
        s = lg.double().sigmoid() * pb[:, :, None]
        ok = (pb[:, :, None] > actor_thr) & ~torch.isnan(s) & (s >= score_thr)
        s, ok = s.reshape(B, Qs * C), ok.reshape(B, Qs * C)
        lab = None
    else:
        C = lg.shape[2] - 1
        # the first maximum of the logit row; a row with a NaN has a NaN probability and is no candidate, whatever its label
        lab = (lg == lg.max(-1, keepdim=True).values).to(torch.int8).argmax(-1)
        s = torch.gather(lg.double().softmax(-1), 2, lab[:, :, None])[:, :, 0]
        ok = (lab != C) & ~torch.isnan(s) & (s >= score_thr)
    ok = ok & valid[:, None]
    N = s.shape[1]
    key = torch.where(ok, s, torch.full_like(s, float("-inf")))
    idx = torch.sort(key, dim=1, descending=True, stable=True).indices
    if N < K:
        idx = torch.cat([idx, torch.zeros(B, K - N, dtype=idx.dtype, device=dev)], dim=1)
    idx = idx[:, :K]
    total = ok.sum(1).to(torch.int32)
    count = total.clamp(max=K)
    live = torch.arange(K, device=dev)[None, :] < count[:, None]
    q = idx // C if mode == "ava" else idx
    c = idx % C if mode == "ava" else torch.gather(lab, 1, idx)
    zero = lambda t: torch.where(live, t, torch.zeros_like(t))
    minus = lambda t: torch.where(live, t, torch.full_like(t, -1)).to(torch.int32)
    return (torch.where(live[:, :, None], torch.gather(pix, 1, q[:, :, None].expand(B, K, 4)), torch.zeros((), device=dev)),
            zero(torch.gather(s, 1, idx).float()), minus(c), minus(q), zero(torch.gather(pb, 1, q).float()), count, total)


def decode_actors_host(logits, logits_b, boxes, sizes, actor_thr, A, q_begin=None, Qs=None):
    """The ACTORS of a batch under the AVA rule, in numpy: the DEFINITION of ``tuber_detect_actors``.  ``decode_topk_host``
    ranks (query, class) pairs, so a person doing three things is three rows; here a row is a person.  A query of the clip's slice is an actor
    when ``pb = softmax(logits_b)[1]`` is not NaN and ``pb > actor_thr`` (the gate of ``decode_topk_host``); actors are ranked by ``pb`` descending,
    then query ascending (``fmap_key(pb, q)``), and the best ``A`` kept, each with its WHOLE action row ``sigmoid(logit) * pb`` -- the number
    ``decode_topk_host`` calls the score of (q, c) -- unthresholded, a NaN logit staying NaN.  Probabilities in fp64 from the fp32 inputs, boxes in
    fp32.  logits [B, Qtot, C]; logits_b [B, Qtot, NB] or [B, NB]; boxes [B, Qtot, 4] cxcywh; sizes [B, 2] (h, w).  Returns a dict of the
    ``ACTOR_FIELDS`` arrays: boxes [B, A, 4] f32, actor [B, A] f32, queries [B, A] i32, actions [B, A, C] f32, count / total [B] i32; rows at and
    after ``count[b]``: box 0, actor 0, query -1, actions 0."""
    lg = np.asarray(logits, dtype=np.float32)
    lb = np.asarray(logits_b, dtype=np.float32)
    B, Qtot, C = lg.shape
    Qs = Qtot if Qs is None else int(Qs)
    A = int(A)
    qb = np.zeros(B, dtype=np.int64) if q_begin is None else np.asarray(q_begin, dtype=np.int64).reshape(B)
    pix = boxes_xyxy_f32(boxes, sizes)
    pb_all = _softmax64(lb)[..., 1]                                    # [B, Qtot] or [B]
    out = dict(boxes=np.zeros((B, A, 4), np.float32), actor=np.zeros((B, A), np.float32), queries=np.full((B, A), -1, np.int32),
               actions=np.zeros((B, A, C), np.float32), count=np.zeros(B, np.int32), total=np.zeros(B, np.int32))
    for b in range(B):
        q0 = int(qb[b])
        if q0 < 0 or q0 + Qs > Qtot:                                   # a slice outside the clip's queries: an empty result
            continue
        rows = lg[b, q0:q0 + Qs]
        pb = pb_all[b, q0:q0 + Qs] if pb_all.ndim == 2 else np.full(Qs, pb_all[b])
        with np.errstate(invalid="ignore"):
            qq = np.nonzero(~np.isnan(pb) & (pb > actor_thr))[0]       # query ascending
        order = np.argsort(-pb[qq], kind="stable")[:A]                 # pb descending, equal pb in query order
        n = len(order)
        out["total"][b], out["count"][b] = len(qq), n
        qq = qq[order]
        with np.errstate(over="ignore"):
            s = (1.0 / (1.0 + np.exp(-rows[qq].astype(np.float64)))) * pb[qq][:, None]
        out["boxes"][b, :n] = pix[b, q0 + qq]
        out["actor"][b, :n] = pb[qq].astype(np.float32)
        out["queries"][b, :n] = qq
        out["actions"][b, :n] = s.astype(np.float32)
    return out


def _decode_actors_torch(logits, logits_b, boxes, sizes, actor_thr, A, q_begin, Qs):
    """``decode_actors_host`` restated in torch on the inputs' device (fp64 probabilities, a stable sort): the path of shapes beyond
    ``tuber_detect_actors_limits``.  No host synchronisation.  Returns the ``ACTOR_FIELDS`` tensors."""
    from . import box_ops
    dev = logits.device
    B, Qtot, C = logits.shape
    lg, lb, bx = logits.float(), logits_b.float(), boxes.float()
    h, w = sizes.to(dev, torch.float32).unbind(1)
    pix = box_ops.box_cxcywh_to_xyxy(bx) * torch.stack([w, h, w, h], dim=1)[:, None, :]
    qb = torch.zeros(B, dtype=torch.int64, device=dev) if q_begin is None else q_begin.to(dev, torch.int64)
    valid = (qb >= 0) & (qb + Qs <= Qtot)
    rows = (torch.where(valid, qb, torch.zeros_like(qb))[:, None] + torch.arange(Qs, device=dev)[None, :])          # [B, Qs]
    lg = torch.gather(lg, 1, rows[:, :, None].expand(B, Qs, C))
    pix = torch.gather(pix, 1, rows[:, :, None].expand(B, Qs, 4))
    pb = lb.double().softmax(-1)[..., 1]
    pb = torch.gather(pb, 1, rows) if pb.dim() == 2 else pb[:, None].expand(B, Qs)
    ok = ~torch.isnan(pb) & (pb > actor_thr) & valid[:, None]
    key = torch.where(ok, pb, torch.full_like(pb, float("-inf")))
    idx = torch.sort(key, dim=1, descending=True, stable=True).indices
    if Qs < A:
        idx = torch.cat([idx, torch.zeros(B, A - Qs, dtype=idx.dtype, device=dev)], dim=1)
    q = idx[:, :A]
    total = ok.sum(1).to(torch.int32)
    count = total.clamp(max=A)
    live = torch.arange(A, device=dev)[None, :] < count[:, None]
    pa = torch.gather(pb, 1, q)                                                                                      # [B, A] fp64
    act = torch.gather(lg, 1, q[:, :, None].expand(B, A, C)).double().sigmoid() * pa[:, :, None]
    zero = torch.zeros((), device=dev)
    return (torch.where(live[:, :, None], torch.gather(pix, 1, q[:, :, None].expand(B, A, 4)), zero), torch.where(live, pa.float(), zero),
            torch.where(live, q, torch.full_like(q, -1)).to(torch.int32), torch.where(live[:, :, None], act.float(), zero), count, total)


# ---------------------------------------------------------------------------------------------------------------------
# captured eval forward
# ---------------------------------------------------------------------------------------------------------------------
def graph_key(clip_shape, mask_shape, dtype, store_id, flat_ptr, coop_off, switches, precision):
    """what a captured eval forward is valid for: the shapes and dtype of its static inputs, the parameter store it reads (weights change
    in place at fixed addresses: an optimizer step or ``WeightAverage.applied`` keeps a capture valid), and everything that selects kernels"""
    return (tuple(int(n) for n in clip_shape), tuple(int(n) for n in mask_shape), str(dtype), int(store_id), int(flat_ptr), bool(coop_off),
            tuple(sorted(switches)), str(precision))


class _Capture:
    __slots__ = ("graph", "clips", "mask", "outputs", "statics", "extra")


class GraphedEval:
    """``model(samples)`` in eval mode as a hipGraph replay.  ``__call__(samples)`` returns the dict ``model(samples)`` returns (``pred_*``,
    ``_stacked``, ``aux_outputs`` when the model has them); the tensors are views of the capture's static outputs and stay valid until the
    next call.  A new key (``graph_key``) is captured on first sight: copy in, one eager warm-up, capture, replay.  Once ``max_shapes``
    captures exist further keys run eagerly and are counted in ``eager_calls`` -- there is no eviction, so a ragged loader cannot thrash;
    ``max_shapes=0`` never captures.  Each capture keeps its activations in a private pool.

    ``epilogue`` (used by ``Detector``): an object with ``statics(outputs)`` -> a dict of tensors allocated once per capture, outside it, and
    ``launch(outputs, statics)`` -> anything, run behind the forward inside the capture; ``run(samples, feed)`` calls ``feed(statics)`` to
    fill them before the replay and returns ``(outputs, launch's result)``."""

    def __init__(self, model, max_shapes=4, epilogue=None):
        self.model = model
        self.max_shapes = int(max_shapes)
        self.epilogue = epilogue
        self.captures = 0
        self.eager_calls = 0
        self._graphs = {}
        self._eager_statics = {}

    def key_of(self, samples):
        st, _ = self.model.engine()
        return graph_key(samples.tensors.shape, samples.mask.shape, samples.tensors.dtype, id(st), st.flat.data_ptr(), st.coop_off, ab.active(),
                         os.environ.get("TUBER_EVAL_PRECISION", ""))

    def __call__(self, samples):
        return self.run(samples)[0]

    def _eager(self, samples, feed):
        outputs = self.model(samples)
        extra = None
        if self.epilogue is not None:
            lg = outputs["pred_logits"]
            statics = self._eager_statics.get((lg.shape[0], lg.device))       # one set of buffers per batch size: the eager path allocates and
            if statics is None:                                                # fills nothing per call, it is the forward plus the epilogue
                statics = self._eager_statics[lg.shape[0], lg.device] = self.epilogue.statics(outputs)
            if feed is not None:
                feed(statics)
            extra = self.epilogue.launch(outputs, statics)
        return outputs, extra

    @torch.no_grad()
    def run(self, samples, feed=None):
        if self.model.training:
            raise RuntimeError("GraphedEval captures an eval forward: call model.eval() first")
        if not isinstance(samples, NestedTensor):
            samples = nested_tensor_from_tensor_list(samples)
        st, _ = self.model.engine()
        samples = samples.to(st.device)
        key = self.key_of(samples)
        cap = self._graphs.get(key)
        if cap is None:
            if len(self._graphs) >= self.max_shapes:
                self.eager_calls += self.max_shapes > 0                # (max_shapes = 0 asks for the eager path: nothing overflowed)
                return self._eager(samples, feed)
            cap = self._capture(samples, feed)
            self._graphs[key] = cap
            self.captures += 1
        else:
            cap.clips.copy_(samples.tensors)
            cap.mask.copy_(samples.mask)
            if feed is not None:
                feed(cap.statics)
        cap.graph.replay()
        return cap.outputs, cap.extra

    def _capture(self, samples, feed):
        cap = _Capture()
        cap.clips, cap.mask = samples.tensors.clone(), samples.mask.clone()
        static = NestedTensor(cap.clips, cap.mask)
        outputs = self.model(static)                                   # eager warm-up: every lazy buffer of the engine exists afterwards
        cap.statics = self.epilogue.statics(outputs) if self.epilogue is not None else None
        if feed is not None:
            feed(cap.statics)
        if self.epilogue is not None:
            self.epilogue.launch(outputs, cap.statics)
        del outputs
        torch.cuda.synchronize()
        cap.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cap.graph):
            cap.outputs = self.model(static)
            cap.extra = self.epilogue.launch(cap.outputs, cap.statics) if self.epilogue is not None else None
        return cap


# ---------------------------------------------------------------------------------------------------------------------
# detections
# ---------------------------------------------------------------------------------------------------------------------
def host_parts(parts):
    """the tensors ``parts`` as typed, shaped numpy arrays, in ONE device-to-host copy (it synchronises with the producing stream); tensors that
    are on the CPU already pass through without the concatenation.  All of ``parts`` are on one device.  The one packed copy of the package."""
    parts = [t.contiguous() for t in parts]
    if not any(t.is_cuda for t in parts):
        return [t.numpy() for t in parts]
    blob = torch.cat([t.reshape(-1).view(torch.uint8) for t in parts]).cpu().numpy()
    host, o = [], 0
    for t in parts:
        n = t.numel() * t.element_size()
        host.append(blob[o:o + n].view(np.dtype(str(t.dtype).replace("torch.", ""))).reshape(tuple(t.shape)))
        o += n
    return host


# dtype, shape behind the leading [clips] (n: the rows per clip, K or A; C: the classes) and the value in an empty result, per field name
FIELD_SPEC = {"boxes": (torch.float32, ("n", 4), 0), "scores": (torch.float32, ("n",), 0), "labels": (torch.int32, ("n",), -1),
              "queries": (torch.int32, ("n",), -1), "aux": (torch.float32, ("n",), 0), "actor": (torch.float32, ("n",), 0),
              "actions": (torch.float32, ("n", "C"), 0), "count": (torch.int32, (), 0), "total": (torch.int32, (), 0)}


def field_tensors(fields, B, n, device, C=None, filled=True):
    """the tensors of ``fields`` for B clips of n rows each: an empty result (zero, -1 in labels / queries), or uninitialised (``filled=False``)"""
    out = []
    for k in fields:
        dtype, tail, fill = FIELD_SPEC[k]
        shape = (B,) + tuple({"n": n, "C": C}.get(d, d) for d in tail)
        out.append(torch.full(shape, fill, dtype=dtype, device=device) if filled else torch.empty(shape, dtype=dtype, device=device))
    return out


class Record:
    """What the four result classes share.  ``FIELDS`` names the tensors of a result, ``ROW_FIELDS`` those with a row per detection, which
    ``to_host`` trims to ``count``.  What a failed cooperative decoder launch means differs -- a detector's result runs its batch again, a
    video's raises -- and stays in the ``to_host`` of either family."""
    __slots__ = ()
    FIELDS = ROW_FIELDS = ()

    def __init__(self, *tensors):
        for k, t in zip(self.FIELDS, tensors):
            setattr(self, k, t)

    def tensors(self):
        return tuple(getattr(self, k) for k in self.FIELDS)

    def _fetch(self, extra=()):
        """(every field as a dict of numpy arrays, the ``extra`` tensors -- the cooperative decoder's error word, link records -- as a list), in
        ONE device-to-host copy"""
        host = host_parts(list(self.tensors()) + list(extra))
        return dict(zip(self.FIELDS, host)), host[len(self.FIELDS):]

    def _trimmed(self, host, i, **first):
        """row ``i`` of the fetched fields as a dict trimmed to its ``count``"""
        n = int(host["count"][i])
        return dict({k: host[k][i, :n].copy() for k in self.ROW_FIELDS}, **first, count=n, total=int(host["total"][i]))


class _BatchRecord(Record):
    """a ``Detector``'s result: the view of its buffers and the way to run the batch again"""
    __slots__ = ("_retry",)

    def __init__(self, *tensors):
        super().__init__(*tensors)
        self._retry = None           # (ParamStore, callable -> the same record of the same batch): set by Detector, consumed by to_host

    def to_host(self):
        """a list, per clip, of dicts of numpy arrays trimmed to ``count``: one copy.  The only place that synchronises; it reads the cooperative
        decoder's error word there and, on a failure, runs the batch once more on the launch chain (a new key, hence a new capture).  A
        poisoned forward has NaN scores and NaN actor probabilities, hence neither a detection nor an actor."""
        retry, self._retry = self._retry, None
        store, again = retry if retry is not None else (None, None)
        host, word = self._fetch([store.coop_sync] if store is not None else [])
        if word and word[0][2] and not store.coop_off and store.coop_failed():
            host, _ = again()._fetch()
        return [self._trimmed(host, b) for b in range(len(host["count"]))]


class Detections(_BatchRecord):
    """Ranked detections of a batch as device tensors: boxes [B, K, 4] f32 xyxy pixels, scores / aux [B, K] f32, labels / queries [B, K]
    i32 (-1 in empty rows), count [B] = min(total, K), total [B].  A detector's result is a view of its buffers: valid until its next call."""
    __slots__ = FIELDS + ("actors",)
    FIELDS, ROW_FIELDS = FIELDS, FIELDS[:5]

    def __init__(self, boxes, scores, labels, queries, aux, count, total):
        super().__init__(boxes, scores, labels, queries, aux, count, total)
        self.actors = None           # the ``Actors`` of the same batch: ``Detector(..., actors=A)``


class Actors(_BatchRecord):
    """The actors of a batch as device tensors (``decode_actors_host``): boxes [B, A, 4] f32 xyxy pixels, actor [B, A] f32 (the actor probability),
    queries [B, A] i32 (-1 in empty rows), actions [B, A, C] f32 (every class's score ``sigmoid(logit) * actor``), count [B] = min(total, A),
    total [B].  A detector's result is a view of its buffers: valid until its next call.  ``to_host()``: ``boxes``, ``actor``, ``queries``,
    ``actions`` [count, C], ``count``, ``total`` per clip."""
    __slots__ = ACTOR_FIELDS
    FIELDS, ROW_FIELDS = ACTOR_FIELDS, ACTOR_FIELDS[:4]

    def __init__(self, boxes, actor, queries, actions, count, total):
        super().__init__(boxes, actor, queries, actions, count, total)


def empty_detections(B, K, device):
    return Detections(*field_tensors(FIELDS, B, K, device))


def empty_actors(B, A, C, device):
    return Actors(*field_tensors(ACTOR_FIELDS, B, A, device, C))


def actors_launch(logits, logits_b, boxes, sizes, q_begin, Qs, actor_thr, A, out=None):
    """one ``tuber_detect_actors`` launch on the current stream over AVA head outputs as the forward produced them (fp32 or bf16, contiguous);
    arguments as ``detect_launch``.  ``out``: the ``Actors`` to write (allocated when None).  Beyond the kernel's bounds
    (``tuber_detect_actors_limits``) the torch restatement of ``decode_actors_host`` answers."""
    dev = logits.device
    B, Qtot, C = logits.shape
    NB = logits_b.shape[-1]
    lb_rows = Qtot if logits_b.dim() == 3 else 1
    if out is None:
        out = empty_actors(B, A, C, dev)
    lim = [lib.query("tuber_detect_actors_limits", w) for w in (0, 1, 2)]
    if Qs > lim[0] or A > lim[1] or NB > lim[2] or A * C > 0x7FFFFFFF:
        res = _decode_actors_torch(logits, logits_b, boxes, sizes, actor_thr, A, q_begin, Qs)
        for dst, src in zip(out.tensors(), res):
            dst.copy_(src)
        return out
    dtypes = 0
    for t, bit in ((logits, 1), (logits_b, 2), (boxes, 4)):
        if t.dtype == torch.bfloat16:
            dtypes |= bit
        elif t.dtype != torch.float32:
            raise TypeError("actors_launch: head outputs are fp32 or bf16, got %s" % t.dtype)
        if not t.is_contiguous():
            raise ValueError("actors_launch: head outputs must be contiguous")
    if sizes.dtype != torch.float32 or (q_begin is not None and q_begin.dtype != torch.int32):
        raise TypeError("actors_launch: sizes is fp32 [B, 2], q_begin int32 [B]")
    lib.call("tuber_detect_actors", logits, logits_b, boxes, sizes, q_begin, B, Qtot, Qs, C, NB, lb_rows, dtypes, float(actor_thr), int(A),
             *out.tensors())
    return out


def detect_launch(mode, logits, logits_b, boxes, sizes, q_begin, Qs, actor_thr, score_thr, K, out=None):
    """one ``tuber_detect_ava`` / ``tuber_detect_top1`` launch on the current stream over head outputs as the forward produced them (fp32 or
    bf16, contiguous); sizes [B, 2] fp32 (h, w) and q_begin [B] int32 (or None) on the device.  ``out``: the ``Detections`` to write
    (allocated when None).  Beyond the kernel's bounds (``tuber_detect_limits``) the torch restatement of ``decode_topk_host`` answers."""
    dev = logits.device
    B, Qtot, CW = logits.shape
    C = CW if mode == "ava" else CW - 1
    NB = logits_b.shape[-1]
    lb_rows = Qtot if logits_b.dim() == 3 else 1
    if out is None:
        out = empty_detections(B, K, dev)
    if Qs * C > lib.query("tuber_detect_limits", 0) or K > lib.query("tuber_detect_limits", 1) or NB > lib.query("tuber_detect_limits", 2):
        res = _decode_topk_torch(logits, logits_b, boxes, sizes, mode, actor_thr, score_thr, K, q_begin, Qs)
        for dst, src in zip(out.tensors(), res):
            dst.copy_(src)
        return out
    dtypes = 0
    for t, bit in ((logits, 1), (logits_b, 2), (boxes, 4)):
        if t.dtype == torch.bfloat16:
            dtypes |= bit
        elif t.dtype != torch.float32:
            raise TypeError("detect_launch: head outputs are fp32 or bf16, got %s" % t.dtype)
        if not t.is_contiguous():
            raise ValueError("detect_launch: head outputs must be contiguous")
    if sizes.dtype != torch.float32 or (q_begin is not None and q_begin.dtype != torch.int32):
        raise TypeError("detect_launch: sizes is fp32 [B, 2], q_begin int32 [B]")
    lib.call("tuber_detect_ava" if mode == "ava" else "tuber_detect_top1", logits, logits_b, boxes, sizes, q_begin, B, Qtot, Qs, C, NB, lb_rows,
             dtypes, float(actor_thr), float(score_thr), int(K), *out.tensors())
    return out


class Detector:
    """``Detector(cfg, model)(samples, sizes, key_pos=None)`` -> ``Detections`` on the device; nothing is copied to the host.
    ``graphed=True``: the forward and the decode launch replay as one hipGraph per input shape (``GraphedEval``), ``sizes`` / the key-frame
    slice being static inputs; ``graphed=False``: the eager forward plus the one launch.  The rule comes from ``model.dataset_mode``, the
    defaults from ``CONFIG.VAL.DETECT``.  ``key_pos`` [B]: the key frame of each clip, needed when the model carries QUERY_NUM queries per
    frame (``SINGLE_FRAME: False``, JHMDB / UCF101-24): the detections are those of that frame's queries.

    ``actors=A`` (AVA models; default None: off): a second launch behind the first one, ``tuber_detect_actors`` over the same head outputs, and the
    result carries ``.actors``, the ``Actors`` of the batch: the best A queries by actor probability, each with its whole action row.  The
    JHMDB / UCF101-24 models carry one label per query -- their ranked detections already are per actor -- so ``actors`` raises there."""

    def __init__(self, cfg, model, score_thr=None, topk=None, actor_thr=None, graphed=True, max_shapes=4, actors=None):
        from .config import detect_settings
        d = detect_settings(cfg)
        self.cfg, self.model = cfg, model
        self.score_thr = float(d["score_thr"] if score_thr is None else score_thr)
        self.topk = int(d["topk"] if topk is None else topk)
        self.actor_thr = float(d["actor_thr"] if actor_thr is None else actor_thr)
        if self.topk < 1:
            raise ValueError("Detector: topk = %r must be >= 1" % (topk,))
        self.mode = model.dataset_mode
        if actors is not None:
            if self.mode != "ava":
                raise ValueError("Detector: actors = %r needs an AVA model; a %s model carries one label per query: use tubes()" % (actors, self.mode))
            if isinstance(actors, bool) or int(actors) != actors or actors < 1:
                raise ValueError("Detector: actors = %r must be an integer >= 1" % (actors,))
        self.actors = None if actors is None else int(actors)
        self.graphed = bool(graphed)
        self.Q = int(cfg.CONFIG.MODEL.QUERY_NUM)
        self.sliced = model.query_embed.num_embeddings != self.Q       # QUERY_NUM queries per frame: a call names its key frames
        self.eval = GraphedEval(model, max_shapes=max_shapes if self.graphed else 0, epilogue=self)

    # -- GraphedEval's epilogue protocol ----------------------------------------------------------------------------
    def statics(self, outputs):
        lg = outputs["pred_logits"]
        B, dev = lg.shape[0], lg.device
        statics = {"sizes": torch.zeros(B, 2, dtype=torch.float32, device=dev), "q_begin": torch.zeros(B, dtype=torch.int32, device=dev),
                   "out": empty_detections(B, self.topk, dev)}
        if self.actors is not None:
            statics["out"].actors = empty_actors(B, self.actors, lg.shape[2], dev)
        return statics

    def launch(self, outputs, statics):
        lg = outputs["pred_logits"]
        qb, Qs = statics["q_begin"] if self.sliced else None, self.Q if self.sliced else lg.shape[1]
        det = detect_launch(self.mode, lg, outputs["pred_logits_b"], outputs["pred_boxes"], statics["sizes"], qb, Qs, self.actor_thr, self.score_thr,
                            self.topk, out=statics["out"])
        if self.actors is not None:
            actors_launch(lg, outputs["pred_logits_b"], outputs["pred_boxes"], statics["sizes"], qb, Qs, self.actor_thr, self.actors, out=det.actors)
        return det

    def _q_begin(self, key_pos):
        """first query of the key frame's slice: evaluation.py's ``key_pos // DS_RATE * Q`` (AVA, SINGLE_FRAME: False) / ``key_pos * Q``"""
        kp = torch.as_tensor(key_pos).to(torch.int64).reshape(-1)
        if self.mode == "ava":
            kp = kp // int(self.cfg.CONFIG.MODEL.DS_RATE)
        return (kp * self.Q).to(torch.int32)

    @torch.no_grad()
    def __call__(self, samples, sizes, key_pos=None):
        if self.model.training:
            raise RuntimeError("Detector runs an eval forward: call model.eval() first")
        if self.sliced and key_pos is None:
            raise ValueError("Detector: the model carries %d queries per clip, QUERY_NUM = %d per frame: pass key_pos" %
                             (self.model.query_embed.num_embeddings, self.Q))
        sizes = torch.as_tensor(sizes)
        qb = self._q_begin(key_pos) if self.sliced else None

        def feed(statics):
            statics["sizes"].copy_(sizes)
            if qb is not None:
                statics["q_begin"].copy_(qb)

        def run():
            return self.eval.run(samples, feed)[1]
        det = run()
        det._retry = (self.model.engine()[0], run)
        if det.actors is not None:
            det.actors._retry = (det._retry[0], lambda: run().actors)
        return det
