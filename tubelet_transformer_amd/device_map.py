"""Validation frame-mAP on the device (csrc/frame_map.hip): an opt-in replacement for the result files + ``evaluation.FrameMAP`` at the end
of ``validate_tuber_detection`` (``CONFIG.VAL.DEVICE_MAP``).

``DeviceFrameMAP`` keeps the decoded detections of the loop in growing device buffers (the host knows every count, so nothing is read back
while the loop runs), the few ground-truth boxes on the host, and computes at the end what ``FrameMAP`` computes from the files: per
(frame, class) the greedy score-ordered matching (``tuber_frame_match``), per class the ranking (``torch.sort``, plumbing) and the VOC average
precision (``tuber_ranked_ap``), then the mean by the host code both evaluators share (``evaluation.mean_ap``).

Equal scores: the reference orders by numpy's default sort, whose permutation of equal keys is an artefact of introsort.  Here the rule is
DEFINED: equal scores keep store order -- frame id ascending (ids in order of first appearance among the detections), then row order --
inside a frame and in the per-class ranking.  That is ``FrameMAP(stable=True)``, always; it is the unmodified ``FrameMAP()`` whenever no
class has two equal scores.  ``evaluate()`` leaves the number of rows per class that share their score with another row in ``ties``.

A store on the CPU, and a store with a frame beyond the kernel's bounds (``tuber_frame_match_max_dets`` detections,
``tuber_frame_match_max_gt`` ground-truth boxes), is evaluated by ``to_host_evaluator().evaluate()``: no frame is ever dropped or cut.

``DeviceFrameMAPUCF`` is the same store under the JHMDB / UCF101-24 counting rule of ``evaluation.FrameMAPUCF`` (``validate_tuber_ucf_detection``):
a row of C + 1 probabilities is one detection, of its arg-max class; the matching step is ``tuber_frame_match_top1``, the rest is shared.

``DeviceVideoMAP`` is that store again with the tube id of every ground-truth line: besides frame-mAP it links the rows into action tubes
(``tuber_tube_link``), matches them against the ground-truth tubes by spatio-temporal IoU (``tuber_tube_match``, csrc/tube_map.hip) and gives
video-mAP at several thresholds -- ``evaluation.VideoMAP`` on the device.  With ``tube_nms`` set, duplicate tubes are removed between the two
steps (``tuber_tube_nms``; ``evaluation.tube_nms`` is the definition).
"""
import logging
import time

import numpy as np
import torch

from . import lib
from .evaluation import FrameMAP, FrameMAPUCF, mean_ap
from . import evaluation as _ev

log = logging.getLogger(__name__)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the host side of the tube kernels (csrc/tube_map.hip), shared with video.py
# ---------------------------------------------------------------------------------------------------------------------------------------
LINK_NAMES = ("row_cls", "row_head", "tube_score", "tube_len", "tube_last")


def link_records(N, dev):
    """the five link-record tensors of N rows as the linkers want them: ``row_cls`` / ``row_head`` are written for every row, ``tube_score`` /
    ``tube_len`` / ``tube_last`` at head rows only, hence their fill"""
    i32 = torch.int32
    return dict(row_cls=torch.empty(N, dtype=i32, device=dev), row_head=torch.empty(N, dtype=i32, device=dev),
                tube_score=torch.zeros(N, dtype=torch.float64, device=dev), tube_len=torch.zeros(N, dtype=i32, device=dev),
                tube_last=torch.full((N,), -1, dtype=i32, device=dev))


def link_limits():
    """(the most rows per slot, the most active tubes) the linkers take"""
    return lib.query("tuber_frame_match_max_dets"), lib.query("tuber_tube_link_max_active")


def link_beyond(what, rows, max_gap):
    """why the linker cannot take ``rows`` rows per slot with ``max_gap`` (``what`` names them), or None"""
    most, active = link_limits()
    return "%s: beyond %d rows or %d active tubes" % (what, most, active) if rows > most or rows * (max_gap + 1) > active else None


def link_ranked(boxes, labels, scores, C, link_iou, max_gap):
    """``tuber_tube_link_ranked`` over the padded store [S][K] of one video as it is -> (link records, slot_off, video_off) on the device"""
    S, K = scores.shape
    dev = boxes.device
    slot_off = torch.arange(S + 1, dtype=torch.int32, device=dev) * K                   # rows behind a key's count carry label -1: not counted
    video_off = torch.tensor([0, S], dtype=torch.int32).to(dev)
    link = link_records(S * K, dev)
    lib.call("tuber_tube_link_ranked", boxes.contiguous(), labels.contiguous(), scores.contiguous(), slot_off, video_off, 1, S, S * K, int(C), K,
             float(link_iou), int(max_gap), *(link[k] for k in LINK_NAMES))
    return link, slot_off, video_off


def tube_nms_launch(boxes, slot_off, video_off, link, V, S, N, C, max_rows, min_len, iou):
    """``tuber_tube_nms`` over a device link record -> tube_keep [N] uint8 on the device (1 kept head, 0 suppressed head, 2 not a head or
    shorter than ``min_len``, 3 a (video, class) beyond the kernel's bound)"""
    keep = torch.full((N,), 2, dtype=torch.uint8, device=boxes.device)
    work = torch.empty(max(lib.query("tuber_tube_nms_work_bytes", N), 16), dtype=torch.uint8, device=boxes.device)
    lib.call("tuber_tube_nms", boxes, slot_off, video_off, *(link[k] for k in LINK_NAMES), int(V), int(S), N, int(C), int(max_rows), int(min_len),
             float(iou), work, keep)
    return keep


DENSE_NAMES = ("dense_box", "dense_score", "row_span", "row_next")


def dense_beyond(S, K, G):
    """why ``tuber_tube_dense`` cannot take a [S][K] store with ``G`` frames per row, or None"""
    return "%d key frames of %d rows with up to %d frames per row: beyond 32 bits" % (S, K, G) if S * K * G > 0x7FFFFFFF else None


def tube_dense_launch(boxes, scores, row_head, keys, max_gap, G):
    """``tuber_tube_dense`` over the padded store [S][K] of one video behind its link step -> dict(dense_box [S * K, G, 4] fp32, dense_score
    [S * K, G] fp32, row_span / row_next [S * K] int32) on the device; the entries behind a row's span are not written"""
    S, K = scores.shape
    dev, i32 = boxes.device, torch.int32
    slot_frame = torch.tensor([int(k) for k in keys], dtype=i32).to(dev)
    out = dict(dense_box=torch.empty(S * K, G, 4, dtype=torch.float32, device=dev), dense_score=torch.empty(S * K, G, dtype=torch.float32, device=dev),
               row_span=torch.empty(S * K, dtype=i32, device=dev), row_next=torch.empty(S * K, dtype=i32, device=dev))
    lib.call("tuber_tube_dense", boxes.contiguous(), scores.contiguous(), row_head, slot_frame, S, K, int(max_gap), int(G), *(out[k] for k in DENSE_NAMES))
    return out


# the ranking step of the UCF and the video evaluators (plain torch: CPU tensors as well) and the stage timer of every evaluate*()
def _nan_last(s):
    """torch.sort ranks NaN first, np.argsort(-score) last: a NaN score (a broken model) ranks below every number"""
    return s.masked_fill(s != s, float("-inf"))


def rank_by_class(score, cls, counted, C):
    """Every class's ranking over its counted rows: one stable sort by score (descending, NaN last, equal scores in input order), one by class
    bucket; a row that is not counted goes to bucket ``C`` (row C of a [C + 1][N] layout, which ``tuber_ranked_ap`` does not read or reads
    with n_gt 0).  ``score`` [N] float, ``cls`` [N] long, ``counted`` [N] bool -> (ranked scores [N] with -inf for NaN, bucket [N] ascending,
    perm [N]: the input row at every rank, pos [N]: the rank inside its bucket, from 0)."""
    bucket = torch.where(counted, cls.clamp(0, C), torch.full_like(cls, C))
    ranked, by_score = torch.sort(_nan_last(score), descending=True, stable=True)
    bucket, by_class = torch.sort(bucket[by_score], stable=True)
    count = torch.zeros(C + 1, dtype=torch.long, device=score.device).scatter_add_(0, bucket, torch.ones_like(bucket))
    pos = torch.arange(score.shape[0], device=score.device) - (count.cumsum(0) - count)[bucket]
    return ranked[by_class], bucket, by_score[by_class], pos


def bucket_tie_counts(ranked, bucket, C):
    """rows per bucket [C + 1] that share their score with a neighbour of their bucket in the ranking of ``rank_by_class``"""
    ties = torch.zeros(C + 1, dtype=torch.long, device=ranked.device)
    if ranked.shape[0] > 1:
        eq = (ranked[1:] == ranked[:-1]) & (bucket[1:] == bucket[:-1])
        member = torch.zeros(ranked.shape[0], dtype=torch.bool, device=ranked.device)
        member[1:] |= eq
        member[:-1] |= eq
        ties.scatter_add_(0, bucket, member.long())
    return ties


class _Stages:
    """the stage timer of an ``evaluate*(timings=)``: with a dict, ``mark(name)`` records a HIP event at the end of stage ``name`` and
    ``read_back`` leaves ``<name>_ms`` per stage (device time) and ``read_back_ms`` (host time) in it; with None both only do the work"""

    def __init__(self, timings):
        self.timings, self.marks = timings, []
        self.mark("start")

    def mark(self, name):
        if self.timings is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.marks.append((name, e))

    def read_back(self, *tensors):
        """the tensors as numpy arrays"""
        if self.timings is not None:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        out = [t.cpu().numpy() for t in tensors]
        if self.timings is not None:
            self.timings["read_back_ms"] = (time.perf_counter() - t0) * 1e3
            for (_, e0), (name, e1) in zip(self.marks[:-1], self.marks[1:]):
                self.timings[name + "_ms"] = e0.elapsed_time(e1)
        return out


class DeviceFrameMAP:
    """Arguments as ``evaluation.FrameMAP``; ``device``: where the detection buffers live (a CPU store runs the host evaluator)."""

    def __init__(self, class_num, class_whitelist=None, exclude_keys=(), iou_threshold=0.5, gt_min_score=1e-2, device="cuda", widths=None):
        self.class_num, self.iou = int(class_num), float(iou_threshold)
        self.whitelist = set(class_whitelist) if class_whitelist is not None else None
        self.exclude = set(exclude_keys)
        self.gt_min_score = gt_min_score
        self.device = torch.device(device)
        self._init_store(*(widths or (self.class_num, self.class_num)))

    def _init_store(self, score_width, label_width):
        """the empty store: ``score_width`` columns per detection row, ``label_width`` per ground-truth line"""
        self.score_width, self.label_width = score_width, label_width
        self.frame_ids, self.frame_keys = {}, []          # frames with detections: key -> id, in order of first appearance
        self.det_count = []                               # rows per frame id
        self.row_fid = []                                 # frame id per stored row (host)
        self.n = 0                                        # rows stored (the cursor: a host integer)
        self._box = torch.empty((0, 4), dtype=torch.float32, device=self.device)
        self._score = torch.empty((0, self.score_width), dtype=torch.float32, device=self.device)
        self.gt_keys, self._gt_box, self._gt_lab = [], [], []
        self.ties = None                                  # after evaluate(): {class_id: rows that share their score with another row}
        self.path = None                                  # after evaluate(): "device" or "host"

    # ------------------------------------------------------------------------------------------------------------------
    # the store
    # ------------------------------------------------------------------------------------------------------------------
    def _wanted(self, cls):
        return self.whitelist is None or cls in self.whitelist

    def _settings(self):
        return dict(class_num=self.class_num, class_whitelist=self.whitelist, exclude_keys=self.exclude, iou_threshold=self.iou,
                    gt_min_score=self.gt_min_score)

    def _reserve(self, extra):
        need = self.n + extra
        if need <= self._box.shape[0]:
            return
        cap = max(need, 2 * self._box.shape[0], 1024)
        box = torch.empty((cap, 4), dtype=torch.float32, device=self.device)
        score = torch.empty((cap, self.score_width), dtype=torch.float32, device=self.device)
        box[:self.n] = self._box[:self.n]
        score[:self.n] = self._score[:self.n]
        self._box, self._score = box, score

    @property
    def boxes(self):
        return self._box[:self.n]

    @property
    def scores(self):
        return self._score[:self.n]

    def add_detections(self, keys, boxes, scores):
        """``keys``: one frame key per row; ``boxes`` [n, 4] fp32 xyxy, ``scores`` [n, C] fp32 on the store's device.  Rows of an excluded
        key are dropped (``FrameMAP.load_detections`` skips their lines).  No device read."""
        keys = list(keys)
        assert boxes.shape == (len(keys), 4) and scores.shape == (len(keys), self.score_width), (boxes.shape, scores.shape, len(keys))
        assert boxes.dtype == torch.float32 and scores.dtype == torch.float32
        keep = [i for i, k in enumerate(keys) if k not in self.exclude]
        if len(keep) != len(keys):
            if not keep:
                return
            sel = torch.tensor(keep, dtype=torch.long).to(self.device)
            boxes, scores, keys = boxes.index_select(0, sel), scores.index_select(0, sel), [keys[i] for i in keep]
        for k in keys:
            fid = self.frame_ids.get(k)
            if fid is None:
                fid = self.frame_ids[k] = len(self.frame_keys)
                self.frame_keys.append(k)
                self.det_count.append(0)
            self.det_count[fid] += 1
            self.row_fid.append(fid)
        self._reserve(len(keys))
        self._box[self.n:self.n + len(keys)] = boxes
        self._score[self.n:self.n + len(keys)] = scores
        self.n += len(keys)

    def add_ground_truth(self, keys, boxes, labels):
        """``keys``: one frame key per box; ``boxes`` [m, 4] xyxy (kept fp64), ``labels`` [m, C] (a class is set where its value exceeds
        ``gt_min_score``).  Host data: take them from the loader's CPU tensors."""
        keys = list(keys)
        boxes = np.asarray(boxes.detach().cpu().numpy() if torch.is_tensor(boxes) else boxes, dtype=np.float64).reshape(-1, 4)
        labels = np.asarray(labels.detach().cpu().numpy() if torch.is_tensor(labels) else labels, dtype=np.float64).reshape(-1, self.label_width)
        assert len(boxes) == len(keys) == len(labels), (len(boxes), len(keys), len(labels))
        for i, k in enumerate(keys):
            if k in self.exclude:
                continue
            self.gt_keys.append(k)
            self._gt_box.append(boxes[i])
            self._gt_lab.append(labels[i])

    def _gt_extra(self):
        """further per-line ground truth a subclass stores, as keyword arguments of its ``add_ground_truth`` (``merge`` carries them)"""
        return {}

    def gt_arrays(self):
        """(boxes [m, 4] fp64, labels [m, C] fp64) in store order"""
        if not self.gt_keys:
            return np.zeros((0, 4)), np.zeros((0, self.label_width))
        return np.stack(self._gt_box), np.stack(self._gt_lab)

    @classmethod
    def merge(cls, stores):
        """One store holding the rows of ``stores`` in the order given (rank order: the order in which rank 0 loads the result files);
        a key seen in several of them maps to one frame id."""
        first = stores[0]
        out = cls(device=first.device, **first._settings())
        for s in stores:
            out.add_detections([s.frame_keys[f] for f in s.row_fid], s.boxes.to(out.device), s.scores.to(out.device))
            gb, gl = s.gt_arrays()
            out.add_ground_truth(s.gt_keys, gb, gl, **s._gt_extra())
        return out

    def all_gather_merge(self):
        """Under torch.distributed: every rank's store merged in rank order (a collective; every rank gets the merged store).  The tensors
        are padded to the largest row count and gathered, the keys and the ground truth travel as objects."""
        import torch.distributed as dist
        world = dist.get_world_size()
        gb, gl = self.gt_arrays()
        meta = [None] * world
        dist.all_gather_object(meta, dict(n=self.n, frame_keys=self.frame_keys, row_fid=self.row_fid, gt_keys=self.gt_keys, gt_box=gb, gt_lab=gl,
                                          gt_extra=self._gt_extra()))
        nmax = max(m["n"] for m in meta)
        box = torch.zeros((nmax, 4), dtype=torch.float32, device=self.device)
        score = torch.zeros((nmax, self.score_width), dtype=torch.float32, device=self.device)
        box[:self.n], score[:self.n] = self.boxes, self.scores
        boxes, scores = [torch.empty_like(box) for _ in range(world)], [torch.empty_like(score) for _ in range(world)]
        dist.all_gather(boxes, box)
        dist.all_gather(scores, score)
        parts = []
        for m, b, s in zip(meta, boxes, scores):
            part = type(self)(device=self.device, **self._settings())
            part.add_detections([m["frame_keys"][f] for f in m["row_fid"]], b[:m["n"]], s[:m["n"]])
            part.add_ground_truth(m["gt_keys"], m["gt_box"], m["gt_lab"], **m["gt_extra"])
            parts.append(part)
        return type(self).merge(parts)

    # ------------------------------------------------------------------------------------------------------------------
    # evaluation
    # ------------------------------------------------------------------------------------------------------------------
    def to_host_evaluator(self, stable=True):
        """A ``FrameMAP`` whose gt / det dictionaries hold the store, in store order: what ``load_gt`` / ``load_detections`` build from
        result files with the same lines."""
        ev = FrameMAP(self.class_num, class_whitelist=self.whitelist, exclude_keys=self.exclude, iou_threshold=self.iou,
                      gt_min_score=self.gt_min_score, stable=stable)
        gb, gl = self.gt_arrays()
        for k, box, lab in zip(self.gt_keys, gb, gl):
            for x in np.nonzero(lab > self.gt_min_score)[0]:
                if self._wanted(int(x) + 1):
                    ev.gt.setdefault(k, []).append((int(x) + 1, np.asarray(box, dtype=float)))
        boxes = self.boxes.cpu().numpy().astype(np.float64)
        scores = self.scores.cpu().numpy().astype(np.float64)
        wanted = [x for x in range(self.class_num) if self._wanted(x + 1)]
        for r, fid in enumerate(self.row_fid):
            items = ev.det.setdefault(self.frame_keys[fid], [])
            box, row = boxes[r], scores[r].tolist()
            items.extend((x + 1, box, row[x]) for x in wanted)
        return ev

    @staticmethod
    def _tie_counts(ranked):
        """rows per class that share their score with a neighbour of the descending ranking [C, N]"""
        if ranked.shape[1] < 2:
            return torch.zeros(ranked.shape[0], dtype=torch.int64, device=ranked.device)
        eq = ranked[:, 1:] == ranked[:, :-1]
        member = torch.zeros(ranked.shape, dtype=torch.bool, device=ranked.device)
        member[:, 1:] |= eq
        member[:, :-1] |= eq
        return member.sum(dim=1)

    def _finish(self, ap, ties):
        per_class = {c + 1: float(ap[c]) for c in range(self.class_num) if self._wanted(c + 1) and not np.isnan(ap[c])}
        self.ties = {c + 1: int(ties[c]) for c in range(self.class_num) if self._wanted(c + 1)}
        ncat = getattr(self, "num_categories", None) or (max(self.whitelist) if self.whitelist else self.class_num)
        return mean_ap(per_class, ncat), per_class

    def _evaluate_host(self):
        self.path = "host"
        ev = self.to_host_evaluator(stable=True)
        mAP, per_class = ev.evaluate()
        s = self.scores.cpu().t().contiguous()
        ranked = torch.sort(_nan_last(s), dim=1, descending=True, stable=True).values if s.numel() else s
        ties = self._tie_counts(ranked).numpy()
        self.ties = {c + 1: int(ties[c]) for c in range(self.class_num) if self._wanted(c + 1)}
        return mAP, per_class

    def _frame_layout(self, gt_keys):
        """The frame-major layout both matching kernels read: frame ids over the detections' keys and then ``gt_keys`` (frames that only
        have ground truth come last), the rows stable-sorted by frame id, per-frame counts and CSR offsets, the ground truth's frame ids and
        their stable order."""
        dev = self.device
        ids = dict(self.frame_ids)
        gfid = np.asarray([ids.setdefault(k, len(ids)) for k in gt_keys], dtype=np.int64)
        F = len(ids)
        fid = torch.tensor(self.row_fid, dtype=torch.int32).to(dev)
        order = torch.sort(fid, stable=True).indices if self.n else torch.zeros(0, dtype=torch.long, device=dev)
        box, score = self.boxes.index_select(0, order).contiguous(), self.scores.index_select(0, order).contiguous()
        det_n = np.zeros(F, dtype=np.int64)
        det_n[:len(self.det_count)] = self.det_count
        gt_n = np.bincount(gfid, minlength=F) if F else np.zeros(0, dtype=np.int64)
        det_off = np.concatenate([[0], np.cumsum(det_n)]).astype(np.int32)
        gt_off = np.concatenate([[0], np.cumsum(gt_n)]).astype(np.int32)
        gorder = np.argsort(gfid, kind="stable")
        return ids, F, order, box, score, det_n, gt_n, det_off, gt_off, gfid, gorder

    def device_arrays(self):
        """The operands of ``tuber_frame_match`` on the store's device: rows stable-sorted by frame id, the two CSR offset arrays over all
        frames (frames that only have ground truth come after those with detections), label bytes, class mask, boxes per class."""
        C, dev = self.class_num, self.device
        gb, gl = self.gt_arrays()
        ids, F, order, box, score, det_n, gt_n, det_off, gt_off, gfid, gorder = self._frame_layout(self.gt_keys)
        mask = np.asarray([1 if self._wanted(c + 1) else 0 for c in range(C)], dtype=np.uint8)
        lab = ((gl[gorder] > self.gt_min_score) & (mask[None, :] != 0)).astype(np.uint8)
        n_gt = lab.sum(axis=0).astype(np.int32)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return dict(F=F, N=self.n, G=len(gfid), C=C, order=order, det_box=box, det_score=score, det_off=up(det_off), gt_box=up(gb[gorder]),
                    gt_lab=up(lab), gt_off=up(gt_off), class_mask=up(mask), n_gt=up(n_gt), max_dets=int(det_n.max()) if F else 0,
                    max_gt=int(gt_n.max()) if F else 0)

    def match_flags(self, a=None):
        """``tuber_frame_match`` over the store: flags [N, C] uint8 for the rows in frame order (``device_arrays()['order']``)"""
        a = a or self.device_arrays()
        flags = torch.empty((a["N"], a["C"]), dtype=torch.uint8, device=self.device)
        lib.call("tuber_frame_match", a["det_box"], a["det_score"], a["det_off"], a["gt_box"], a["gt_lab"], a["gt_off"], a["class_mask"],
                 a["F"], a["N"], a["G"], a["C"], self.iou, flags)
        return flags

    def evaluate(self, timings=None):
        """-> (mAP, {class_id: AP}); ``ties`` and ``path`` are set.  Bitwise reproducible run to run.  ``timings``: a dict that receives
        the device time of every stage in ms (HIP events) and the host time of the read-back (scripts/device_map_bench.py)."""
        if self.device.type != "cuda":
            return self._evaluate_host()
        stages = _Stages(timings)
        a = self.device_arrays()
        if self._beyond_bounds(a):
            return self._evaluate_host()
        self.path = "device"
        stages.mark("frame_sort_and_uploads")
        return self._finish(*stages.read_back(*self._evaluate_device(a, stages.mark)))

    def _beyond_bounds(self, a):
        """a frame the matching kernels do not take: logged once, the store is evaluated on the host"""
        if a["max_dets"] > lib.query("tuber_frame_match_max_dets") or a["max_gt"] > lib.query("tuber_frame_match_max_gt"):
            log.warning("DeviceFrameMAP: a frame has %d detections / %d ground-truth boxes, beyond the kernel's %d / %d: evaluating on the host",
                        a["max_dets"], a["max_gt"], lib.query("tuber_frame_match_max_dets"), lib.query("tuber_frame_match_max_gt"))
            return True
        return False

    def _evaluate_device(self, a, mark):
        """the device stages behind the layout -> (ap [C] fp64, ties [C]) on the device"""
        C, N = a["C"], a["N"]
        flags = self.match_flags(a)
        mark("tuber_frame_match")
        # every class's ranking: scores descending over all rows, equal scores in store order (NaN last, as np.argsort(-score) has it)
        ranked, idx = torch.sort(_nan_last(a["det_score"].t().contiguous()), dim=1, descending=True, stable=True)
        flags_ranked = flags.t().contiguous().gather(1, idx) if N else torch.empty((C, 0), dtype=torch.uint8, device=self.device)
        mark("rank_sort_and_gather")
        ap = torch.empty(C, dtype=torch.float64, device=self.device)
        n_tp = torch.empty(C, dtype=torch.int32, device=self.device)
        lib.call("tuber_ranked_ap", flags_ranked, a["n_gt"], C, N, ap, n_tp)
        mark("tuber_ranked_ap")
        ties = self._tie_counts(ranked)
        mark("tie_count")
        return ap, ties


class DeviceFrameMAPUCF(DeviceFrameMAP):
    """``evaluation.FrameMAPUCF`` on the store of ``DeviceFrameMAP``: a detection row is ``[C + 1]`` probabilities (the classes, then
    no-object) and counts once, as its arg-max class with that probability, unless no-object is the arg-max; a ground-truth line is a box and
    the one-hot row the loop writes to ``GT_*.txt``; a ground-truth box under 10 px^2 is dropped and puts its key on the exclude list -- decided
    in ``evaluate()`` over everything stored, as the reference loads every ground-truth file before any detection file.  The mean runs over 24
    categories whatever ``class_num`` is.

    Equal scores keep store order: frames in order of first appearance in the store, then row order.  That is ``FrameMAPUCF(stable=True)`` on
    files with the same lines whenever the first stored row of every frame is not behind a counted row of a later frame (always, when a
    frame's rows arrive together), and the unmodified ``FrameMAPUCF()`` when no class has two equal scores."""

    TINY = 10                                             # evaluate_ucf.py:60-62

    def __init__(self, class_num=24, iou_threshold=0.5, label_width=None, device="cuda"):
        super().__init__(class_num, iou_threshold=iou_threshold, device=device,
                         widths=(int(class_num) + 1, int(label_width) if label_width else max(21, int(class_num))))
        self.num_categories = 24                          # evaluate_ucf.py:15-20

    def _settings(self):
        return dict(class_num=self.class_num, iou_threshold=self.iou, label_width=self.label_width)

    def ucf_ground_truth(self):
        """-> (excluded keys, [(key, class 0-based, box)] in store order): ``FrameMAPUCF.load_gt`` over the stored lines"""
        gb, gl = self.gt_arrays()
        tiny = (gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1]) < self.TINY
        excluded = {k for k, t in zip(self.gt_keys, tiny) if t}
        rows = [(k, int(x), gb[i]) for i, k in enumerate(self.gt_keys) if not tiny[i] for x in np.nonzero(~(gl[i] <= 1e-2))[0]]
        return excluded, rows

    def to_host_evaluator(self, stable=True):
        """A ``FrameMAPUCF`` whose gt / det dictionaries hold the store in store order: what ``load_gt`` / ``load_detections`` build from
        result files with the same lines."""
        ev = FrameMAPUCF(self.class_num, iou_threshold=self.iou, stable=stable)
        ev.exclude, rows = self.ucf_ground_truth()
        for k, x, box in rows:
            ev.gt.setdefault(k, []).append((x + 1, np.asarray(box, dtype=float)))
        boxes = self.boxes.cpu().numpy().astype(np.float64)
        probs = self.scores.cpu().numpy().astype(np.float64)
        for k in self.frame_keys:
            ev.det[k] = []
        for r, fid in enumerate(self.row_fid):
            k = self.frame_keys[fid]
            if k in ev.exclude or int(np.argmax(probs[r])) == self.class_num:
                continue
            x = int(np.argmax(probs[r, :self.class_num]))
            ev.det[k].append((x + 1, boxes[r], float(probs[r, x])))
        ev.det = {k: d for k, d in ev.det.items() if d}
        return ev

    def _evaluate_host(self):
        self.path = "host"
        ev = self.to_host_evaluator(stable=True)
        mAP, per_class = ev.evaluate()
        _, scores, _ = ev.match()
        self.ties = {}
        for c in range(1, self.class_num + 1):
            s = np.concatenate(scores[c]) if c in scores else np.zeros(0)
            _, counts = np.unique(np.where(np.isnan(s), -np.inf, s), return_counts=True)
            self.ties[c] = int(counts[counts > 1].sum())
        return mAP, per_class

    def device_arrays(self):
        """The operands of ``tuber_frame_match_top1`` on the store's device: rows stable-sorted by frame id, the CSR offsets over all
        frames, one ground-truth row per (kept line, class set in it), the exclude list as a byte per frame, boxes per class."""
        C, dev = self.class_num, self.device
        excluded, rows = self.ucf_ground_truth()
        ids, F, order, box, prob, det_n, gt_n, det_off, gt_off, gfid, gorder = self._frame_layout([k for k, _, _ in rows])
        gcls = np.asarray([x for _, x, _ in rows], dtype=np.int32)[gorder]
        gbox = np.asarray([b for _, _, b in rows], dtype=np.float64).reshape(-1, 4)[gorder]
        skip = np.zeros(F, dtype=np.uint8)
        skip[np.asarray([ids[k] for k in excluded if k in ids], dtype=np.int64)] = 1
        n_gt = np.bincount(gcls[(gcls >= 0) & (gcls < C)], minlength=C).astype(np.int32)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return dict(F=F, N=self.n, G=len(gfid), C=C, order=order, det_box=box, det_prob=prob, det_off=up(det_off), gt_box=up(gbox),
                    gt_cls=up(gcls), gt_off=up(gt_off), frame_skip=up(skip), n_gt=up(n_gt), max_dets=int(det_n.max()) if F else 0,
                    max_gt=int(gt_n.max()) if F else 0)

    def match_flags(self, a=None):
        """``tuber_frame_match_top1`` over the store: (det_cls [N] int32, det_flag [N] uint8) for the rows in frame order"""
        a = a or self.device_arrays()
        cls = torch.empty(a["N"], dtype=torch.int32, device=self.device)
        flag = torch.empty(a["N"], dtype=torch.uint8, device=self.device)
        lib.call("tuber_frame_match_top1", a["det_box"], a["det_prob"], a["det_off"], a["gt_box"], a["gt_cls"], a["gt_off"], a["frame_skip"],
                 a["F"], a["N"], a["G"], a["C"], self.iou, cls, flag)
        return cls, flag

    def _evaluate_device(self, a, mark):
        C, N, dev = a["C"], a["N"], self.device
        cls, flag = self.match_flags(a)
        mark("tuber_frame_match_top1")
        cls = cls.long()
        score = a["det_prob"].gather(1, cls.clamp(0, C)[:, None])[:, 0] if N else torch.zeros(0, device=dev)
        ranked, bucket, perm, pos = rank_by_class(score, cls, flag != 2, C)
        flags_ranked = torch.full((C + 1, N), 2, dtype=torch.uint8, device=dev)
        flags_ranked[bucket, pos] = flag[perm]
        mark("rank_sort_and_scatter")
        ap = torch.empty(C, dtype=torch.float64, device=dev)
        n_tp = torch.empty(C, dtype=torch.int32, device=dev)
        lib.call("tuber_ranked_ap", flags_ranked, a["n_gt"], C, N, ap, n_tp)
        mark("tuber_ranked_ap")
        ties = bucket_tie_counts(ranked, bucket, C)
        mark("tie_count")
        return ap, ties[:C]


class DeviceVideoMAP(DeviceFrameMAPUCF):
    """``DeviceFrameMAPUCF`` that also links its rows into action tubes and computes video-mAP (``evaluation.VideoMAP``: the definition).
    ``evaluate()`` is unchanged (frame-mAP); ``link()`` / ``tubes()`` give the tubes, ``evaluate_video()`` the video-mAPs.  Keys are
    ``"<video>-<frame number>"``.  ``add_ground_truth(..., tubes=)`` takes one integer tube id per line; without it the id is the ordinal of
    the line among its frame's lines of the same class.  A CPU store, a store beyond a kernel bound and a key that does not parse are evaluated
    by ``to_video_host_evaluator()``: no row is ever dropped.  ``tube_nms`` (default None: off): the spatio-temporal IoU above which a tube
    is a duplicate of a higher-scored kept tube of its (video, class) and is neither matched nor ranked (``tuber_tube_nms``,
    ``evaluation.tube_nms``: the definition); ``tubes()`` drops such tubes."""

    def __init__(self, class_num=24, iou_threshold=0.5, label_width=None, device="cuda", link_iou=0.2, max_gap=2, min_len=1,
                 thresholds=(0.2, 0.5, 0.75, "0.5:0.95"), tube_nms=None):
        super().__init__(class_num, iou_threshold, label_width, device)
        self.link_iou, self.max_gap, self.min_len, self.thresholds = float(link_iou), int(max_gap), int(min_len), tuple(thresholds)
        self.tube_nms = None if tube_nms is None else float(tube_nms)
        self.video_path = None                            # after evaluate_video(): "device" or "host"

    def _init_store(self, score_width, label_width):
        super()._init_store(score_width, label_width)
        self._gt_tube = []                                # per ground-truth line: its tube id or None

    def _settings(self):
        return dict(super()._settings(), link_iou=self.link_iou, max_gap=self.max_gap, min_len=self.min_len, thresholds=self.thresholds,
                    tube_nms=self.tube_nms)

    def _gt_extra(self):
        return dict(tubes=list(self._gt_tube))

    def add_ground_truth(self, keys, boxes, labels, tubes=None):
        keys = list(keys)
        tubes = [None] * len(keys) if tubes is None else [None if t is None else int(t) for t in tubes]
        assert len(tubes) == len(keys), (len(tubes), len(keys))
        super().add_ground_truth(keys, boxes, labels)
        self._gt_tube.extend(tubes)
        assert len(self._gt_tube) == len(self.gt_keys)

    def video_ground_truth(self):
        """-> (keys, [(class 0-based, box, tube id or None)]): one row per (line, class set in it), in store order; tiny boxes are kept"""
        gb, gl = self.gt_arrays()
        keys, rows = [], []
        for i, k in enumerate(self.gt_keys):
            for x in np.nonzero(~(gl[i] <= 1e-2))[0]:
                keys.append(k)
                rows.append((int(x), gb[i], self._gt_tube[i]))
        return keys, rows

    def to_video_host_evaluator(self):
        """an ``evaluation.VideoMAP`` holding the store, in store order"""
        ev = _ev.VideoMAP(self.class_num, self.link_iou, self.max_gap, self.min_len, self.thresholds, tube_nms=self.tube_nms)
        ev.add_detections([self.frame_keys[f] for f in self.row_fid], self.boxes.cpu().numpy(), self.scores.cpu().numpy())
        keys, rows = self.video_ground_truth()
        ev.add_ground_truth(keys, [r[1] for r in rows], [r[0] for r in rows], [r[2] for r in rows])
        return ev

    def video_arrays(self):
        """The operands of ``tuber_tube_link`` / ``tuber_tube_match`` on the store's device: the rows in layout order (video, slot, store
        order), the CSR offsets of the slots and videos, one ground-truth row per (slot, class, tube) in slot order with the tube's rank among
        the ids of its (video, class), tubes per class; ``beyond``: why the kernels cannot take the store, or None."""
        C, dev = self.class_num, self.device
        gkeys, grows = self.video_ground_truth()
        frame_slot_keys = list(self.frame_keys)
        lay = _ev.tube_layout(frame_slot_keys, gkeys)     # one detection "row" per frame id: rows of a frame share their slot
        S, V = lay["S"], lay["V"]
        fslot = torch.from_numpy(lay["det_slot"]).to(dev)
        slot = fslot[torch.tensor(self.row_fid, dtype=torch.long).to(dev)] if self.n else torch.zeros(0, dtype=torch.long, device=dev)
        order = torch.sort(slot, stable=True).indices
        rows_per = np.zeros(S, dtype=np.int64)
        np.add.at(rows_per, lay["det_slot"], np.asarray(self.det_count, dtype=np.int64))
        gt = _ev.ground_truth_tubes(lay, grows)
        rank, per_vc = {}, {}
        for key in sorted(gt):
            rank[key] = per_vc[key[:2]] = per_vc.get(key[:2], 0)
            per_vc[key[:2]] += 1
        flat = sorted((s, key[1], rank[key], key) for key, g in gt.items() if 0 <= key[1] < C for s in g)
        gslot = np.asarray([f[0] for f in flat], dtype=np.int64)
        gt_per = np.bincount(gslot, minlength=S) if S else np.zeros(0, dtype=np.int64)
        n_gt = np.bincount(np.asarray([k[1] for k in gt if 0 <= k[1] < C], dtype=np.int64), minlength=C).astype(np.int32)
        thr = _ev.expand_thresholds(self.thresholds)
        a = dict(V=V, S=S, N=self.n, G=len(flat), C=C, T=len(thr), thr=thr, layout=lay, max_rows=int(rows_per.max()) if S else 0,
                 max_gt_rows=int(gt_per.max()) if S else 0, max_gt_tubes=max(per_vc.values()) if per_vc else 0)
        a["beyond"] = self._video_beyond(a)
        if a["beyond"]:
            return a
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        a.update(order=order, row_slot=slot.index_select(0, order), det_box=self.boxes.index_select(0, order).contiguous(),
                 det_prob=self.scores.index_select(0, order).contiguous(),
                 slot_off=up(np.concatenate([[0], np.cumsum(rows_per)]).astype(np.int32)), video_off=up(lay["video_off"].astype(np.int32)),
                 gt_box=up(np.asarray([gt[f[3]][f[0]] for f in flat], dtype=np.float64).reshape(-1, 4)),
                 gt_cls=up(np.asarray([f[1] for f in flat], dtype=np.int32)), gt_tube=up(np.asarray([f[2] for f in flat], dtype=np.int32)),
                 gt_off=up(np.concatenate([[0], np.cumsum(gt_per)]).astype(np.int32)), thresholds=up(np.asarray(thr, dtype=np.float64)),
                 n_gt=up(n_gt))
        return a

    def _video_beyond(self, a):
        if not a["layout"]["parsed"]:
            return "a key is not of the form <video>-<frame number>"
        why = link_beyond("%d rows in a frame with MAX_GAP %d" % (a["max_rows"], self.max_gap), a["max_rows"], self.max_gap)
        if why:
            return why
        if a["max_gt_rows"] > lib.query("tuber_frame_match_max_gt") or a["max_gt_tubes"] > lib.query("tuber_tube_match_max_gt"):
            return "%d ground-truth boxes in a frame / %d ground-truth tubes in a (video, class): beyond %d / %d" % (
                a["max_gt_rows"], a["max_gt_tubes"], lib.query("tuber_frame_match_max_gt"), lib.query("tuber_tube_match_max_gt"))
        if a["T"] > lib.query("tuber_tube_match_max_thresholds"):
            return "%d thresholds: beyond %d" % (a["T"], lib.query("tuber_tube_match_max_thresholds"))
        if max(a["S"], a["V"] * a["C"], a["T"] * a["N"]) >= 2 ** 31:
            return "sizes beyond 32-bit indices"
        return None

    def link(self, a=None):
        """``tuber_tube_link`` over the store -> device tensors in layout order: ``order`` (layout row -> store row), ``det_box``, ``det_prob``,
        ``row_slot``, ``row_cls``, ``row_head`` (-1: not counted), and at head rows ``tube_score`` (fp64), ``tube_len``, ``tube_last``; ``layout``.
        A store the kernel cannot take gives the host's arrays (``evaluation.VideoMAP.link``) as CPU tensors."""
        if self.device.type == "cuda":
            a = a or self.video_arrays()
        if self.device.type != "cuda" or a["beyond"]:
            host = self.to_video_host_evaluator().link()
            return {k: (torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v) for k, v in host.items() if k != "tubes"}
        N, dev = a["N"], self.device
        out = dict(link_records(N, dev), order=a["order"], det_box=a["det_box"], det_prob=a["det_prob"], row_slot=a["row_slot"], layout=a["layout"])
        lib.call("tuber_tube_link", a["det_box"], a["det_prob"], a["slot_off"], a["video_off"], a["V"], a["S"], N, a["C"], a["max_rows"],
                 self.link_iou, self.max_gap, *(out[k] for k in LINK_NAMES))
        return out

    def nms(self, a, link):
        """``tube_nms_launch`` over the store's device link record -> tube_keep [N] uint8 on the device"""
        return tube_nms_launch(a["det_box"], a["slot_off"], a["video_off"], link, a["V"], a["S"], a["N"], a["C"], a["max_rows"], self.min_len, self.tube_nms)

    def tubes(self):
        """the linked tubes read back: a list of dict(video, cls (1-based), score, frames, boxes, head, rows) in head order; with ``tube_nms``
        set, without the suppressed ones"""
        a = self.video_arrays() if self.device.type == "cuda" else None
        link = self.link(a)
        keep = None
        if self.tube_nms is not None and link["row_head"].device.type == "cuda":
            keep = self.nms(a, link).cpu().numpy()
        link = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in link.items()}
        if self.tube_nms is not None and (keep is None or (keep == 3).any()):
            keep = _ev.tube_nms(link, self.tube_nms, self.min_len)
        return [t for t in _ev.tubes_from_link(link) if keep is None or keep[t["head"]] != 0]

    def match_video(self, a, link):
        """``tuber_tube_match`` -> tube_flag [T, N] uint8 on the device (1 true positive, 0 false positive, 2 not counted)"""
        N, dev = a["N"], self.device
        flags = torch.empty((a["T"], N), dtype=torch.uint8, device=dev)
        work = torch.empty(N * max(a["max_gt_tubes"], 1), dtype=torch.float64, device=dev)
        lib.call("tuber_tube_match", a["det_box"], a["slot_off"], a["video_off"], link["row_cls"], link["row_head"], link["tube_score"],
                 link["tube_len"], link["tube_last"], a["gt_box"], a["gt_cls"], a["gt_tube"], a["gt_off"], a["thresholds"], a["V"], a["S"], N,
                 a["G"], a["C"], a["T"], a["max_rows"], a["max_gt_rows"], a["max_gt_tubes"], self.min_len, work, flags)
        return flags

    def evaluate_video(self, timings=None):
        """-> {threshold: (video-mAP, {class_id: AP})} as ``VideoMAP.evaluate()``; ``video_path`` is set.  Bitwise reproducible run to run.
        ``timings``: a dict that receives the device time of every stage in ms (HIP events) and the host time of the read-back."""
        if self.device.type != "cuda":
            return self._evaluate_video_host("the store is on the CPU")
        stages = _Stages(timings)
        mark = stages.mark
        a = self.video_arrays()
        if a["beyond"]:
            return self._evaluate_video_host(a["beyond"])
        self.video_path = "device"
        C, N, T, dev = a["C"], a["N"], a["T"], self.device
        mark("layout_and_uploads")
        link = self.link(a)
        mark("tuber_tube_link")
        keep = None
        if self.tube_nms is not None:
            # the match kernel sees a suppressed tube as one of no detections: with min_len >= 1 its phase 2 skips the head (flag 2, no
            # ground-truth tube taken, its work row never read); phase 1 reads tube_len only into a divisor of that row
            keep = self.nms(a, link)
            link = dict(link, tube_len=link["tube_len"].masked_fill(keep == 0, 0))
            mark("tuber_tube_nms")
        flags = self.match_video(a, link)
        mark("tuber_tube_match")
        # every class's ranking over its counted tubes (rows that are no counted head: bucket C), the same for every threshold
        _, bucket, perm, pos = rank_by_class(link["tube_score"], link["row_cls"].long(), flags[0] != 2, C)
        flags_ranked = torch.full((T, C + 1, N), 2, dtype=torch.uint8, device=dev)
        if N:
            flags_ranked[:, bucket, pos] = flags[:, perm]
        mark("rank_sort_and_scatter")
        n_gt = torch.cat([a["n_gt"], torch.zeros(1, dtype=torch.int32, device=dev)]).repeat(T).contiguous()
        ap = torch.empty(T * (C + 1) + (0 if keep is None else 1), dtype=torch.float64, device=dev)
        lib.call("tuber_ranked_ap", flags_ranked, n_gt, T * (C + 1), N, ap, None)
        if keep is not None:
            ap[-1] = (keep == 3).any()                    # the kernel's escape travels with the APs: no read-back of its own
        mark("tuber_ranked_ap")
        ap, = stages.read_back(ap)
        if keep is not None:
            if ap[-1] != 0.0:
                return self._evaluate_video_host("more than %d tubes of a (video, class) live at one frame" % lib.query("tuber_tube_link_max_active"))
            ap = ap[:-1]
        ap = ap.reshape(T, C + 1)
        at = {}
        for i, thr in enumerate(a["thr"]):
            per_class = {c + 1: float(ap[i, c]) for c in range(C) if not np.isnan(ap[i, c])}
            at[thr] = (mean_ap(per_class, self.num_categories), per_class)
        return _ev.collect_thresholds(self.thresholds, at)

    def _evaluate_video_host(self, why):
        log.warning("DeviceVideoMAP: %s: evaluating video-mAP on the host", why)
        self.video_path = "host"
        return self.to_video_host_evaluator().evaluate()
