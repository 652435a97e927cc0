"""Evaluation loop, result files and frame-mAP.

Mirrors ``utils/video_action_recognition.py:222-454`` (``validate_tuber_detection``): eval-mode forward on the HIP path,
``postprocessors['bbox']``, the per-rank text files ``{BASE_PATH}/{RES_DIR}/{rank}.txt`` / ``GT_{rank}.txt`` in the reference's
exact format (``"{image_id} [x1, y1, x2, y2, <C scores>, <actor probs>]"`` and ``"{image_id} [<6 raw-box numbers>, <C labels>]"``),
so the reference's own evaluator can be pointed at them unchanged, and a compact numpy restatement of the metric it computes
(``evaluates/evaluate_ava.py:17-171`` driving the vendored PASCAL evaluator ``evaluates/utils/object_detection_evaluation.py:309``:
per-class VOC average precision at IoU >= 0.5, greedy score-ordered matching, one detection per ground-truth box, classes without
ground truth excluded from the mean).  ``tests/golden/frame_map_case.json`` pins it against the reference evaluator run in the
build container (``oracle/gen_eval_golden.py``).  Host-side code: runs once per epoch on rank 0 -- nothing on the golden case, minutes at
AVA's size, which is what ``CONFIG.VAL.DEVICE_MAP`` (device_map.py: the same metric on the device, no files needed) is for.
"""
import glob
import math
import os
import time

import numpy as np
import torch


# ---------------------------------------------------------------------------------------------------------------------
# result files
# ---------------------------------------------------------------------------------------------------------------------
def write_result_files(base_path, res_dir, rank, det_ids, det_boxes, det_scores, det_binary, gt_ids, gt_boxes, gt_labels):
    """video_action_recognition.py:397-407: one line per (frame, query) / per ground-truth box."""
    d = os.path.join(base_path, res_dir)
    os.makedirs(d, exist_ok=True)
    det_path = os.path.join(d, "%d.txt" % rank)
    gt_path = os.path.join(d, "GT_%d.txt" % rank)
    with open(det_path, "w") as f:
        for x in range(len(det_ids)):
            data = np.concatenate([det_boxes[x], det_scores[x], det_binary[x]])
            f.write("{} {}\n".format(det_ids[x], data.tolist()))
    with open(gt_path, "w") as f:
        for x in range(len(gt_ids)):
            data = np.concatenate([gt_boxes[x], gt_labels[x]])
            f.write("{} {}\n".format(gt_ids[x], data.tolist()))
    return det_path, gt_path


def _parse(line):
    key = line.split(" [")[0]
    vals = [float(v) for v in line.split(" [")[1].split("]")[0].split(",")]
    return key, vals


# ---------------------------------------------------------------------------------------------------------------------
# frame-mAP
# ---------------------------------------------------------------------------------------------------------------------
def _iou_one_to_many(box, boxes):
    x1 = np.maximum(box[0], boxes[:, 0]); y1 = np.maximum(box[1], boxes[:, 1])
    x2 = np.minimum(box[2], boxes[:, 2]); y2 = np.minimum(box[3], boxes[:, 3])
    inter = np.maximum(x2 - x1, 0.0) * np.maximum(y2 - y1, 0.0)
    a = (box[2] - box[0]) * (box[3] - box[1])
    b = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    return inter / (a + b - inter)


def _average_precision(precision, recall):
    """area under the monotone precision envelope (VOC 2010+; object_detection/utils/metrics.py:compute_average_precision)"""
    if precision is None or len(precision) == 0:
        return float("nan")
    r = np.concatenate([[0.0], recall, [1.0]])
    p = np.concatenate([[0.0], precision, [0.0]])
    for i in range(len(p) - 2, -1, -1):
        p[i] = max(p[i], p[i + 1])
    idx = np.where(r[1:] != r[:-1])[0] + 1
    return float(np.sum((r[idx] - r[idx - 1]) * p[idx]))


def mean_ap(per_class, ncat):
    """the reference's mean: np.nanmean over an array indexed by class id up to the largest category id, NaN where a class has no
    ground truth (object_detection_evaluation.py: average_precision_per_class) -- same summation order, same bits.  Shared by
    FrameMAP and device_map.DeviceFrameMAP."""
    arr = np.full(max(ncat, max(per_class) if per_class else 0), np.nan)
    for cls, ap in per_class.items():
        arr[cls - 1] = ap
    return float(np.nanmean(arr)) if per_class else float("nan")


class FrameMAP:
    """Frame-level mean average precision from the result files (STDetectionEvaluater semantics, evaluate_ava.py:17-171).
    ``stable=False`` orders equal scores as the reference does (numpy's default sort: an artefact of introsort); ``stable=True`` keeps
    them in file order, inside a frame and in the per-class ranking -- the rule device_map.DeviceFrameMAP computes by.  Without equal
    scores the two are the same evaluator."""

    def __init__(self, class_num, class_whitelist=None, exclude_keys=(), iou_threshold=0.5, gt_min_score=1e-2, stable=False):
        self.class_num, self.iou = class_num, iou_threshold
        self.stable = stable
        self.whitelist = set(class_whitelist) if class_whitelist is not None else None
        self.exclude = set(exclude_keys)
        self.gt_min_score = gt_min_score
        self.gt, self.det = {}, {}

    def _wanted(self, cls):
        return self.whitelist is None or cls in self.whitelist

    def load_gt(self, paths):
        for path in paths:
            for line in open(path):
                key, v = _parse(line)
                if key in self.exclude:
                    continue
                labels = np.asarray(v[6:])
                for x in np.nonzero(labels > self.gt_min_score)[0]:
                    if self._wanted(int(x) + 1):
                        self.gt.setdefault(key, []).append((int(x) + 1, np.asarray(v[2:6], dtype=float)))

    def load_detections(self, paths):
        for path in paths:
            for line in open(path):
                key, v = _parse(line)
                if key in self.exclude:
                    continue
                box = np.asarray(v[0:4], dtype=float)
                scores = v[4:self.class_num + 4]
                for x, s in enumerate(scores):
                    if self._wanted(x + 1):
                        self.det.setdefault(key, []).append((x + 1, box, float(s)))

    def num_categories_(self):
        return getattr(self, "num_categories", None) or (max(self.whitelist) if self.whitelist else self.class_num)

    def match(self):
        """-> (n_gt, scores, tps): ground-truth boxes per class, and per class the lists (one entry per image, in image order) of the
        valid detections' scores in matching order and of their true-positive flags.  Detections of images without ground truth count as
        false positives (the PASCAL evaluator scores them against an empty ground-truth list, object_detection_evaluation.py:601-620)."""
        # The data flow (and therefore the resolution of score ties) follows the reference exactly: per image all (box, class)
        # entries in file order are ordered by np.argsort(-score) (evaluate_ava.py:150), matched greedily per class in that
        # order (per_image_evaluation.py:354-366), concatenated per class in image order, and ranked by np.argsort(score)[::-1]
        # (metrics.py:56-57).  numpy's default sort is deterministic, so equal inputs give the reference's permutation.
        n_gt = {}
        for key, items in self.gt.items():
            for cls, _ in items:
                n_gt[cls] = n_gt.get(cls, 0) + 1
        scores, tps = {}, {}
        for key, dets in self.det.items():
            gts = self.gt.get(key, [])
            cls_a = np.asarray([d[0] for d in dets], dtype=int)
            box_a = np.vstack([d[1] for d in dets])
            sc_a = np.asarray([d[2] for d in dets], dtype=float)
            index = np.argsort(-sc_a, kind="stable") if self.stable else np.argsort(-sc_a)
            cls_a, box_a, sc_a = cls_a[index], box_a[index], sc_a[index]
            valid = (box_a[:, 0] < box_a[:, 2]) & (box_a[:, 1] < box_a[:, 3])      # per_image_evaluation.py:445-449
            cls_a, box_a, sc_a = cls_a[valid], box_a[valid], sc_a[valid]
            for cls in range(1, self.class_num + 1):
                sel = cls_a == cls
                if not sel.any():
                    continue
                gboxes = np.asarray([b for c, b in gts if c == cls], dtype=float).reshape(-1, 4)
                taken = np.zeros(len(gboxes), dtype=bool)
                tp = np.zeros(int(sel.sum()), dtype=bool)
                if len(gboxes):
                    for i, box in enumerate(box_a[sel]):
                        iou = _iou_one_to_many(box, gboxes)
                        j = int(np.argmax(iou))
                        if iou[j] >= self.iou and not taken[j]:
                            taken[j] = True
                            tp[i] = True
                scores.setdefault(cls, []).append(sc_a[sel])
                tps.setdefault(cls, []).append(tp)
        return n_gt, scores, tps

    def evaluate(self):
        """-> (mAP, {class_id: AP})"""
        n_gt, scores, tps = self.match()
        per_class = {}
        for cls in range(1, self.class_num + 1):
            if not self._wanted(cls) or n_gt.get(cls, 0) == 0:
                continue
            if cls not in scores:
                per_class[cls] = 0.0
                continue
            s = np.concatenate(scores[cls]); t = np.concatenate(tps[cls])
            order = np.argsort(-s, kind="stable") if self.stable else np.argsort(s)[::-1]
            t = t[order]
            ctp = np.cumsum(t).astype(float); cfp = np.cumsum(~t).astype(float)
            per_class[cls] = _average_precision(ctp / np.maximum(ctp + cfp, np.finfo(np.float64).eps), ctp / n_gt[cls])
        return mean_ap(per_class, self.num_categories_()), per_class


def read_labelmap(path):
    """utils/utils.py:10-25: pbtxt label map -> ([{id, name}], {ids})."""
    labelmap, ids, name = [], set(), ""
    with open(path) as f:
        for line in f:
            if line.startswith("  name:"):
                name = line.split('"')[1]
            elif line.startswith("  id:") or line.startswith("  label_id:"):
                cid = int(line.strip().split(" ")[-1])
                labelmap.append({"id": cid, "name": name})
                ids.add(cid)
    return labelmap, ids


# ---------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------
def _forward_checked(model, samples, graphed=None):
    """model(samples) of a validation iteration.  The cooperative decoder launch (csrc/decoder_coop.hip) fails safe -- a timed-out
    barrier leaves NaN outputs and an error word -- and the loop copies the outputs to the host right after this anyway, so the word is
    read here (16 bytes) every iteration: on a failure the engine switches to the launch chain and the batch is run again (ADVICE r05:
    the evaluation path never looked at the word).  ``graphed``: the loop's detect.GraphedEval under CONFIG.VAL.GRAPHED -- the same
    outputs from a hipGraph replay; the repeat after a failure is a new key there (``coop_off``), hence a new capture."""
    forward = model if graphed is None else graphed
    outputs = forward(samples)
    store = model.engine()[0]
    if not store.coop_off and store.coop_failed():
        outputs = forward(samples)
    return outputs


def _graphed_eval(cfg, model):
    """CONFIG.VAL.GRAPHED: the loop's captured eval forward (built at the top of a validation loop, dropped with it), or None"""
    graphed = getattr(cfg.CONFIG.VAL, "GRAPHED", False)
    if graphed is False:                     # the default, or a config node built without the key: exactly the plain loop
        return None
    from .config import detect_settings
    from .detect import GraphedEval
    detect_settings(cfg)                     # anything but True / False raises, naming the key
    return GraphedEval(model)


def _with_averaged_weights(fn):
    """CONFIG.TRAIN.EMA.ENABLE and .EVAL with a weight averager on the model (weight_avg.py): the loop runs on the averaged weights
    (``WeightAverage.applied``: the live weights and buffers are back afterwards); otherwise exactly the plain loop"""
    import functools

    @functools.wraps(fn)
    def run(cfg, model, *args, **kwargs):
        from .weight_avg import eval_context
        with eval_context(cfg, model):
            return fn(cfg, model, *args, **kwargs)
    return run


def _whitelist_and_excluded(C, excluded_timestamps):
    """(class whitelist from DATA.LABEL_PATH for the 80-class label space or None, excluded frame keys from the csv) of the AVA metric"""
    white = None
    if getattr(C.DATA, "LABEL_PATH", None) and os.path.isfile(C.DATA.LABEL_PATH):
        _, white = read_labelmap(C.DATA.LABEL_PATH)
    excl = []
    if excluded_timestamps and os.path.isfile(excluded_timestamps):
        excl = [l.strip().replace(",", "_") for l in open(excluded_timestamps) if l.strip()]
    return (white if C.DATA.NUM_CLASSES == 80 else None), excl


@_with_averaged_weights
@torch.no_grad()
def validate_tuber_detection(cfg, model, criterion, postprocessors, data_loader, epoch, writer=None, excluded_timestamps=None,
                             verbose=True):
    """video_action_recognition.py:222-454.  Differences: no 30 s sleep, no hard-coded /xxx/ path (``excluded_timestamps`` = csv path
    or None), the distributed barriers are only issued when torch.distributed is initialised, the metric is FrameMAP."""
    import torch.distributed as dist
    C = cfg.CONFIG
    ddp = dist.is_available() and dist.is_initialized()
    rank = dist.get_rank() if ddp else 0                   # the reference reads cfg.DDP_CONFIG.GPU_WORLD_RANK / _SIZE, which its
    world = dist.get_world_size() if ddp else 1            # launcher fills from the same process group
    model.eval()
    criterion.eval()
    dev = next(model.parameters()).device
    res = os.path.join(C.LOG.BASE_PATH, C.LOG.RES_DIR)
    if rank == 0:
        os.makedirs(res, exist_ok=True)
        for p in glob.glob(os.path.join(res, "*.txt")):
            os.remove(p)
    det_scores, det_boxes, det_binary, det_ids, gt_labels, gt_boxes, gt_ids = [], [], [], [], [], [], []
    # CONFIG.VAL.DEVICE_MAP (device_map.py): the detections stay on the device and the metric is computed there; the files are optional then
    dm = getattr(C.VAL, "DEVICE_MAP", None)
    store, files = None, True
    if dm is not None and dm.ENABLE:
        from .device_map import DeviceFrameMAP
        white, excl = _whitelist_and_excluded(C, excluded_timestamps)
        store = DeviceFrameMAP(C.DATA.NUM_CLASSES, class_whitelist=white, exclude_keys=excl, device=dev)
        files = bool(dm.FILES)
    meters = {k: [0.0, 0] for k in ("loss", "loss_bbox", "loss_giou", "loss_ce", "loss_ce_b", "class_error")}
    graphed = _graphed_eval(cfg, model)
    end = time.time()
    for idx, data in enumerate(data_loader):
        samples, targets = data[0], data[1]
        samples = samples.to(dev)            # reference :280 / :513; runs the HIP clip pre-pass when the loader yields ClipBatch
        batch_id = [t["image_id"] for t in targets]
        host_targets = targets               # the loader's own tensors: the device evaluator takes its ground truth from them, without a sync
        targets = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in t.items() if k != "image_id"} for t in targets]
        outputs = _forward_checked(model, samples, graphed)
        loss_dict = criterion(outputs, targets)
        sizes = torch.stack([t["size"] for t in targets], dim=0)
        Q = C.MODEL.QUERY_NUM
        if store is None:
            scores, boxes, output_b = postprocessors["bbox"](outputs, sizes)
        else:
            d_scores, d_boxes, d_binary = postprocessors["bbox"].decode(outputs, sizes)
            if files:                        # what PostProcessAVA.forward returns, bit for bit
                scores, boxes, output_b = d_scores.cpu().numpy(), d_boxes.cpu().numpy(), d_binary.cpu().numpy()
            for b in range(len(targets)):
                frame_id, key_pos = batch_id[b][0], batch_id[b][1]
                sl = slice(None) if C.MODEL.SINGLE_FRAME else slice(key_pos // C.MODEL.DS_RATE * Q, (key_pos // C.MODEL.DS_RATE + 1) * Q)
                store.add_detections([frame_id] * Q, d_boxes[b, sl], d_scores[b, sl])
                raw = host_targets[b]["raw_boxes"]
                sel = (raw[:, 1] == key_pos).nonzero().reshape(-1)
                rb = raw[sel].reshape(len(sel), -1)
                first = float(host_targets[0]["raw_boxes"][0, 0])
                store.add_ground_truth([batch_id[int(float(rb[x, 0]) - first)][0] for x in range(len(rb))], rb[:, 2:6].double(),
                                       host_targets[b]["labels"][sel].reshape(len(sel), -1))
        for b in range(len(targets) if files else 0):
            frame_id, key_pos = batch_id[b][0], batch_id[b][1]
            if not C.MODEL.SINGLE_FRAME:
                k = key_pos // C.MODEL.DS_RATE
                sl = slice(k * Q, (k + 1) * Q)
                det_scores.append(scores[b, sl]); det_boxes.append(boxes[b, sl]); det_binary.append(output_b[b, sl])
            else:
                det_scores.append(scores[b]); det_boxes.append(boxes[b]); det_binary.append(output_b[b])
            det_ids.extend([frame_id] * Q)
            raw = targets[b]["raw_boxes"]
            sel = (raw[:, 1] == key_pos).nonzero().reshape(-1)
            lab = targets[b]["labels"][sel].reshape(len(sel), -1)
            rb = raw[sel].reshape(len(sel), -1)
            gt_labels.append(lab.cpu().numpy()); gt_boxes.append(rb.cpu().numpy())
            first = float(targets[0]["raw_boxes"][0, 0])
            gt_ids.extend(batch_id[int(float(rb[x, 0]) - first)][0] for x in range(len(rb)))
        wd = criterion.weight_dict
        total = float(sum(loss_dict[k] * wd[k] for k in loss_dict if k in wd))
        if not math.isfinite(total):
            raise FloatingPointError("loss is %r in evaluation: %r" % (total, {k: float(v) for k, v in loss_dict.items()}))
        n = len(targets)
        for k, v in (("loss", total), ("loss_bbox", loss_dict["loss_bbox"]), ("loss_giou", loss_dict["loss_giou"]),
                     ("loss_ce", loss_dict["loss_ce"]), ("loss_ce_b", loss_dict.get("loss_ce_b", 0.0)),
                     ("class_error", loss_dict["class_error"])):
            meters[k][0] += float(v) * n; meters[k][1] += n
        if verbose and rank == 0:
            print("Epoch: [%d][%d/%d]  batch time %.3f  " % (epoch, idx + 1, len(data_loader), time.time() - end) +
                  ", ".join("%s: %.3f" % (k, s / max(c, 1)) for k, (s, c) in meters.items()))
        end = time.time()
    graphed = None                           # the captures and their private pools go with it
    cat = lambda xs, w: np.concatenate(xs, axis=0) if xs else np.zeros((0, w))
    nc = C.DATA.NUM_CLASSES
    if files:
        write_result_files(C.LOG.BASE_PATH, C.LOG.RES_DIR, rank, det_ids, cat(det_boxes, 4), cat(det_scores, nc), cat(det_binary, 1),
                           gt_ids, cat(gt_boxes, 6), cat(gt_labels, nc))
    if writer is not None and rank == 0:
        for k, (s, c) in meters.items():
            writer.add_scalar("val/" + k, s / max(c, 1), epoch)
    if dist.is_available() and dist.is_initialized():
        dist.barrier()
    if store is not None and ddp:
        store = store.all_gather_merge()     # every rank's rows in rank order: the order in which rank 0 loads the files
    mAP = 0.0
    if rank == 0:
        if store is not None:
            mAP, per_class = store.evaluate()
        else:
            white, excl = _whitelist_and_excluded(C, excluded_timestamps)
            ev = FrameMAP(nc, class_whitelist=white, exclude_keys=excl)
            ev.load_gt([os.path.join(res, "GT_%d.txt" % r) for r in range(world)])
            ev.load_detections([os.path.join(res, "%d.txt" % r) for r in range(world)])
            mAP, per_class = ev.evaluate()
        if verbose:
            print("mAP: %.5f" % mAP)
        if writer is not None:
            writer.add_scalar("val/val_mAP_epoch", mAP, epoch)
    if dist.is_available() and dist.is_initialized():
        dist.barrier()
    return mAP


# ---------------------------------------------------------------------------------------------------------------------
# JHMDB / UCF101-24 (utils/video_action_recognition.py:456-689, evaluates/evaluate_ucf.py)
# ---------------------------------------------------------------------------------------------------------------------
class FrameMAPUCF(FrameMAP):
    """``STDetectionEvaluaterUCF`` semantics (evaluates/evaluate_ucf.py:22-166) on top of the same PASCAL matching:
    ground-truth lines whose box is smaller than 10 px^2 put their image on an exclude list (:60-62); a detection line is
    ``[x1,y1,x2,y2, <C class probabilities>, <no-object probability>]`` and counts ONCE, as its arg-max class with that score,
    unless the no-object column is the overall arg-max (:109-126).  Pinned against the reference evaluator by
    ``oracle/gen_eval_golden.py`` -> ``tests/golden/frame_map_ucf_case.json``.  ``stable``: as ``FrameMAP``; the rule
    device_map.DeviceFrameMAPUCF computes by."""

    def __init__(self, class_num=24, iou_threshold=0.5, stable=False):
        super().__init__(class_num, None, (), iou_threshold, stable=stable)
        self.num_categories = 24          # evaluate_ucf.py:15-20: the category list is the 24 UCF101-24 names whatever class_num is

    def load_gt(self, paths):
        for path in paths:
            for line in open(path):
                key, v = _parse(line)
                if (v[4] - v[2]) * (v[5] - v[3]) < 10:
                    self.exclude.add(key)
                    continue
                labels = np.asarray(v[6:])
                self.gt.setdefault(key, [])
                for x in np.nonzero(~(labels <= 1e-2))[0]:
                    self.gt[key].append((int(x) + 1, np.asarray(v[2:6], dtype=float)))
        self.gt = {k: g for k, g in self.gt.items() if g}

    def load_detections(self, paths):
        for path in paths:
            for line in open(path):
                key, v = _parse(line)
                if key in self.exclude:
                    continue
                rest = np.asarray(v[4:])
                if int(np.argmax(rest)) == len(rest) - 1:
                    continue
                scores = np.asarray(v[4:self.class_num + 4])
                x = int(np.argmax(scores))
                self.det.setdefault(key, []).append((x + 1, np.asarray(v[0:4], dtype=float), float(scores[x])))


# ---------------------------------------------------------------------------------------------------------------------
# video-mAP over linked action tubes (the definition; the reference ships the frame-level evaluator only)
# ---------------------------------------------------------------------------------------------------------------------
VIDEO_MAP_RANGE = tuple(round(0.5 + 0.05 * i, 2) for i in range(10))          # the members of "0.5:0.95"


def expand_thresholds(thresholds):
    """the numeric thresholds a list of settings needs, ascending: its numbers and, for "0.5:0.95", 0.50, 0.55, ..., 0.95"""
    out = set()
    for t in thresholds:
        out.update(VIDEO_MAP_RANGE if t == "0.5:0.95" else (float(t),))
    return sorted(out)


def split_key(key):
    """"<video>-<frame number>" -> (video, frame), split at the last "-"; None when the key is not of that form"""
    video, sep, frame = str(key).rpartition("-")
    if not sep or not video or not (frame.isascii() and frame.isdigit()):
        return None
    return video, int(frame)


def tube_layout(det_keys, gt_keys):
    """The slot layout of a store: videos in order of first appearance (detections first, then ground truth); a video's slots are the
    consecutive frame numbers from its smallest to its largest; ``det_slot`` / ``gt_slot``: the global slot of every row.  A key that does
    not parse is a one-slot video of its own name (``parsed`` is False then)."""
    ids, lo, hi, parsed = {}, [], [], True
    rows = []
    for k in list(det_keys) + list(gt_keys):
        p = split_key(k)
        if p is None:
            parsed, p = False, (str(k), 0)
        v = ids.get(p[0])
        if v is None:
            v = ids[p[0]] = len(lo)
            lo.append(p[1]); hi.append(p[1])
        else:
            lo[v] = min(lo[v], p[1]); hi[v] = max(hi[v], p[1])
        rows.append((v, p[1]))
    lo_a, hi_a = np.asarray(lo, dtype=np.int64).reshape(-1), np.asarray(hi, dtype=np.int64).reshape(-1)
    video_off = np.concatenate([[0], np.cumsum(hi_a - lo_a + 1)]).astype(np.int64)
    slot = np.asarray([video_off[v] + f - lo[v] for v, f in rows], dtype=np.int64)
    nd = len(det_keys)
    return dict(videos=list(ids), V=len(lo), S=int(video_off[-1]), video_off=video_off, first_frame=lo_a, det_slot=slot[:nd], gt_slot=slot[nd:],
                parsed=parsed)


def ground_truth_tubes(lay, gt_rows):
    """``gt_rows``: [(class 0-based, box fp64, tube id or None)] aligned with ``lay['gt_slot']`` -> {(video, class, id): {slot: box}}.  A missing
    id is the ordinal of the line among its slot's lines of the same class; a second line with the same (slot, class, id) is ignored."""
    ordinal, tubes = {}, {}
    for slot, (c, box, tid) in zip(lay["gt_slot"].tolist(), gt_rows):
        o = ordinal.get((slot, c), 0)
        ordinal[(slot, c)] = o + 1
        tid = o if tid is None else int(tid)
        v = int(np.searchsorted(lay["video_off"], slot, side="right")) - 1
        tubes.setdefault((v, int(c), tid), {}).setdefault(slot, np.asarray(box, dtype=np.float64))
    return tubes


def tubes_from_link(link):
    """the linked tubes of ``VideoMAP.link()`` (or of the device arrays read back) as a list of dict(video, cls (1-based), score, frames, boxes,
    head, rows: the layout rows), in head order"""
    lay, head, slot = link["layout"], np.asarray(link["row_head"]), np.asarray(link["row_slot"])
    rows = {}
    for r in np.nonzero(head >= 0)[0].tolist():
        rows.setdefault(int(head[r]), []).append(r)
    out = []
    for h in sorted(rows):
        v = int(np.searchsorted(lay["video_off"], slot[h], side="right")) - 1
        frames = [int(lay["first_frame"][v] + slot[r] - lay["video_off"][v]) for r in rows[h]]
        out.append(dict(video=lay["videos"][v], cls=int(link["row_cls"][h]) + 1, score=float(link["tube_score"][h]), frames=frames,
                        boxes=np.asarray(link["det_box"])[rows[h]], head=h, rows=rows[h]))
    return out


def link_slot(tubes, s, cur, score, box64, link_iou, max_gap, base=0):
    """One slot of the greedy linking of ONE (video, class): the step ``link_rows`` and ``TubeLinker.push`` share, ``tube_link_kernel`` on the
    host.  ``tubes``: [[head, fp64 score sum, count, last slot, last box fp64], ...]; ``s``: the slot's ordinal; ``cur``: its counted rows of the
    class, indices into ``score`` (fp32) and ``box64``, ascending.  The tubes whose last detection is at most ``max_gap`` + 1 slots back are
    visited by descending mean score (fp64 sum of the fp32 scores / count), equal means by ascending head; each takes, among the slot's
    unclaimed rows whose fp64 IoU with its last box is >= ``link_iou``, the highest score (equal scores: the first row); rows left over start
    tubes with the head ``base`` + row.  -> (the tubes that survive the slot, {row: the tube that took or began with it}); the records of
    ``tubes`` are updated in place."""
    active = [t for t in tubes if s - t[3] <= max_gap + 1]
    active.sort(key=lambda t: (-(t[1] / t[2]), t[0]))
    takes = {}
    for t in active:
        cand = [r for r in cur if r not in takes]
        if not cand:
            break
        with np.errstate(all="ignore"):
            iou = _iou_one_to_many(t[4], box64[cand])
        best = None
        for r, u in zip(cand, iou):
            if u >= link_iou and (best is None or score[r] > score[best]):
                best = r
        if best is not None:
            takes[best] = t
            t[1] += float(score[best]); t[2] += 1; t[3] = s; t[4] = box64[best].copy()
    for r in cur:
        if r not in takes:
            takes[r] = [base + r, float(score[r]), 1, s, box64[r].copy()]
            active.append(takes[r])
    return active, takes


def _counted_rows(box, cls, score, class_num):
    """the rows the linkers count: a class inside [0, class_num), a box with x1 < x2 and y1 < y2, a score that is no NaN"""
    return (cls >= 0) & (cls < class_num) & (box[:, 0] < box[:, 2]) & (box[:, 1] < box[:, 3]) & ~np.isnan(score)


def link_rows(box, cls, score, slot, video_off, class_num, link_iou, max_gap):
    """The greedy linking of per-frame detections into tubes, over rows in layout order (video, slot, store order): ``box`` [N, 4] fp32 xyxy,
    ``cls`` [N] the 0-based class of a row, ``score`` [N] fp32, ``slot`` [N] the global slot, ``video_off`` [V + 1] the slots of every video.  A
    row is counted unless its class is outside [0, class_num), its box has x1 >= x2 or y1 >= y2, or its score is NaN.  Per (video, class), slots
    ascending, ``link_slot`` links the slot's rows.  -> dict: ``row_head`` (layout row of the tube's first detection, -1 for a row that is not
    counted) and, at head rows, ``tube_score`` (fp64 mean), ``tube_len``, ``tube_last`` (last slot).
    The body of ``VideoMAP.link``, the definition of ``tuber_tube_link_ranked`` and the fallback of ``video.VideoDetections.tubes``."""
    box = np.asarray(box, dtype=np.float32).reshape(-1, 4)
    cls, score, slot = np.asarray(cls).reshape(-1), np.asarray(score).reshape(-1), np.asarray(slot).reshape(-1)
    N = len(box)
    box64 = box.astype(np.float64)
    video = np.searchsorted(np.asarray(video_off), slot, side="right") - 1
    head = np.full(N, -1, dtype=np.int64)
    tscore, tlen, tlast = np.zeros(N), np.zeros(N, dtype=np.int64), np.full(N, -1, dtype=np.int64)
    groups = {}
    for r in np.nonzero(_counted_rows(box, cls, score, int(class_num)))[0].tolist():
        groups.setdefault((int(video[r]), int(cls[r])), []).append(r)
    for rows in groups.values():
        tubes, i = [], 0
        while i < len(rows):
            s, j = slot[rows[i]], i
            while j < len(rows) and slot[rows[j]] == s:
                j += 1
            tubes, takes = link_slot(tubes, s, rows[i:j], score, box64, link_iou, max_gap)
            i = j
            for r, t in takes.items():                # a tube's record at its head is that of its last take
                head[r] = t[0]
                tscore[t[0]], tlen[t[0]], tlast[t[0]] = t[1] / t[2], t[2], t[3]
    return dict(row_head=head, tube_score=tscore, tube_len=tlen, tube_last=tlast)


def tube_nms(link, nms_iou, min_len=1):
    """Spatio-temporal NMS over linked tubes: the definition of ``tuber_tube_nms``.  ``link``: a link record as
    ``VideoMAP.link()`` or ``link_rows`` leave it (``det_box``, ``row_slot``, ``row_cls``, ``row_head``, ``tube_score``, ``layout``).  A tube is
    the rows of its head's class that carry its head, one per slot (the first one); it is a candidate with at least ``min_len`` rows.
    ``stIoU(d, e)`` of two tubes of one (video, class): the fp64 sum, over the slots both have a row in, ascending, of ``_iou_one_to_many`` on the
    two fp32 boxes promoted to fp64, divided by the number of slots either has a row in; 0 without a shared slot (gap slots belong to neither).
    Per (video, class) the candidates are visited in ``VideoMAP.match``'s order -- descending score, NaN last, equal scores by ascending head
    -- and one is suppressed iff its stIoU with a tube KEPT before it is strictly greater than ``nms_iou``; a suppressed tube suppresses
    nothing.  -> ``tube_keep`` uint8 [N] in layout order: 1 kept head, 0 suppressed head, 2 not a head or shorter than ``min_len``."""
    nms_iou, min_len = float(nms_iou), int(min_len)
    if not 0.0 <= nms_iou <= 1.0 or min_len < 1:
        raise ValueError("tube_nms: nms_iou = %r must lie in [0, 1] and min_len = %r be >= 1" % (nms_iou, min_len))
    head, slot, cls = np.asarray(link["row_head"]).reshape(-1), np.asarray(link["row_slot"]).reshape(-1), np.asarray(link["row_cls"]).reshape(-1)
    score = np.asarray(link["tube_score"], dtype=np.float64).reshape(-1)
    box64 = np.asarray(link["det_box"], dtype=np.float32).reshape(-1, 4).astype(np.float64)
    video_off = np.asarray(link["layout"]["video_off"])
    N = len(head)
    keep = np.full(N, 2, dtype=np.uint8)
    video = np.searchsorted(video_off, slot, side="right") - 1
    rows = {}                                                  # head -> {slot: row}
    for r in np.nonzero(head >= 0)[0].tolist():
        h = int(head[r])
        if h <= r and head[h] == h and cls[h] == cls[r] and video[h] == video[r]:
            rows.setdefault(h, {}).setdefault(int(slot[r]), r)
    groups = {}
    for h in sorted(rows):
        if len(rows[h]) >= min_len:
            groups.setdefault((int(video[h]), int(cls[h])), []).append(h)

    def st_iou(d, e):
        shared = sorted(set(d) & set(e))
        total = 0.0
        for s in shared:
            with np.errstate(all="ignore"):
                total += float(_iou_one_to_many(box64[d[s]], box64[e[s]][None, :])[0])
        return total / (len(d) + len(e) - len(shared)) if shared else 0.0

    for heads in groups.values():
        kept = []
        for h in sorted(heads, key=lambda h: (-score[h] if score[h] == score[h] else np.inf, h)):
            suppressed = any(st_iou(rows[h], rows[k]) > nms_iou for k in kept)
            keep[h] = 0 if suppressed else 1
            if not suppressed:
                kept.append(h)
    return keep


# ---------------------------------------------------------------------------------------------------------------------------------------
# dense tubes: a box on every frame of a tube's extent
# ---------------------------------------------------------------------------------------------------------------------------------------
def _dense_keys(who, keys):
    """the frame numbers of the key ordinals as int64; they must ascend strictly"""
    keys = np.asarray([int(k) for k in keys], dtype=np.int64)
    if len(keys) > 1 and not (np.diff(keys) > 0).all():
        raise ValueError("%s: the key frames must be strictly ascending, got %s" % (who, keys.tolist()[:16]))
    return keys


def dense_extent(keys, max_gap):
    """G, the most frames one row can own: ``max(1, max over s of keys[min(s + max_gap + 1, S - 1)] - keys[s])`` -- a host integer, known from
    the keys alone"""
    keys, gap = _dense_keys("dense_extent", keys), int(max_gap)
    S = len(keys)
    return max([1] + [int(keys[min(s + gap + 1, S - 1)] - keys[s]) for s in range(S)])


def _dense_fill(box_a, score_a, box_b, score_b, g, out_box, out_score):
    """The arithmetic of ``dense_rows`` / ``dense_tube`` / ``tuber_tube_dense``: the ``g`` frames a key row owns into ``out_box[:g]`` /
    ``out_score[:g]``.  ``j = 0``: the row's own bytes.  ``j >= 1``: ``float32(float64(a) + (float64(b) - float64(a)) * (float64(j) /
    float64(g)))`` per coordinate and for the score, every operation rounded on its own; a NaN result is the one quiet NaN 0x7FC00000."""
    out_box[0], out_score[0] = box_a, score_a
    if g > 1:
        a = np.concatenate([box_a, [score_a]]).astype(np.float64)
        b = np.concatenate([box_b, [score_b]]).astype(np.float64)
        with np.errstate(all="ignore"):
            w = np.arange(1, g, dtype=np.float64) / np.float64(g)
            d = b - a
            v = (a[None, :] + d[None, :] * w[:, None]).astype(np.float32)
        v[np.isnan(v)] = np.float32(np.nan)
        out_box[1:g], out_score[1:g] = v[:, :4], v[:, 4]


def dense_rows(box, score, row_head, keys, K, max_gap, G=None, dense_box=None, dense_score=None):
    """Per-frame boxes between linked key detections: the definition of ``tuber_tube_dense`` and the host path of
    ``tubes(dense=True)`` / ``tracks(dense=True)``.  A padded [S][K] store of ONE video: ``box`` [S * K, 4] fp32, ``score`` [S * K] fp32,
    ``row_head`` [S * K] as ``link_rows`` / ``tuber_tube_link_ranked`` wrote it, ``keys`` [S] the frame number of every key ordinal, strictly
    ascending.  The SUCCESSOR of a counted row r of slot s is the first row with r's head in the slots ``s + 1 .. s + max_gap + 1`` (the
    linker bridges no more; one row per slot); ``span(r) = keys[s'] - keys[s]`` with a successor, 1 without, 0 for a row with head < 0.  Row
    r owns the frames ``keys[s] + j``, ``j < span(r)``: at j = 0 its own bytes, behind that the fp64 interpolation towards the successor
    (``_dense_fill``).  -> ``dense_box`` [S * K, G, 4] fp32, ``dense_score`` [S * K, G] fp32 (given, or zeros; entries at ``j >= span(r)``
    are left as they were), ``row_span`` [S * K], ``row_next`` [S * K] (the successor row, -1 without one).  ``G``: ``dense_extent`` by
    default; a row whose span exceeds a smaller one gets ``row_span`` -1 and nothing else, as in the kernel."""
    keys, K, gap = _dense_keys("dense_rows", keys), int(K), int(max_gap)
    S = len(keys)
    N = S * K
    box = np.asarray(box, dtype=np.float32).reshape(N, 4)
    score = np.asarray(score, dtype=np.float32).reshape(N)
    head = np.asarray(row_head).reshape(N)
    G = dense_extent(keys, gap) if G is None else int(G)
    if G < 1 or gap < 0 or K < 1:
        raise ValueError("dense_rows: G = %d and K = %d must be >= 1, max_gap = %d >= 0" % (G, K, gap))
    dense_box = np.zeros((N, G, 4), dtype=np.float32) if dense_box is None else dense_box
    dense_score = np.zeros((N, G), dtype=np.float32) if dense_score is None else dense_score
    span, nxt = np.zeros(N, dtype=np.int64), np.full(N, -1, dtype=np.int64)
    for r in np.nonzero(head >= 0)[0].tolist():
        s, n = r // K, -1
        for t in range(s + 1, min(s + gap + 1, S - 1) + 1):
            m = np.nonzero(head[t * K:(t + 1) * K] == head[r])[0]
            if len(m):
                n = t * K + int(m[0])
                break
        g = int(keys[n // K] - keys[s]) if n >= 0 else 1
        if g > G:
            span[r] = -1
            continue
        span[r], nxt[r] = g, n
        _dense_fill(box[r], score[r], box[n], score[n], g, dense_box[r], dense_score[r])
    return dict(dense_box=dense_box, dense_score=dense_score, row_span=span, row_next=nxt)


def dense_tube(frames, boxes, scores):
    """``dense_rows`` for one assembled tube on the host (``video.VideoStream.tubes(dense=True)``): its key frames (strictly ascending), [L, 4]
    fp32 boxes and [L] fp32 scores -> dict(``frames``: every frame from the first key to the last, ``boxes`` [F, 4] fp32, ``frame_scores``
    [F] fp32, ``key_index`` [F]: the index of the key that owns the frame).  The arithmetic is ``dense_rows``' (``_dense_fill``)."""
    keys = _dense_keys("dense_tube", frames)
    L = len(keys)
    boxes = np.asarray(boxes, dtype=np.float32).reshape(L, 4)
    scores = np.asarray(scores, dtype=np.float32).reshape(L)
    spans = [int(keys[i + 1] - keys[i]) for i in range(L - 1)] + [1] * min(L, 1)
    F = sum(spans)
    out_box, out_score, at = np.zeros((F, 4), dtype=np.float32), np.zeros(F, dtype=np.float32), 0
    for i, g in enumerate(spans):
        n = min(i + 1, L - 1)
        _dense_fill(boxes[i], scores[i], boxes[n], scores[n], g, out_box[at:at + g], out_score[at:at + g])
        at += g
    return dict(frames=list(range(int(keys[0]), int(keys[0]) + F)) if L else [], boxes=out_box, frame_scores=out_score,
                key_index=np.repeat(np.arange(L, dtype=np.int64), spans))


def dense_from_rows(rows, keys, K, dense):
    """one tube's dense fields from the per-row record ``dense_rows`` / ``tuber_tube_dense`` leave: ``rows`` the tube's rows in slot order ->
    ``dense_tube``'s dict"""
    rows = np.asarray(rows, dtype=np.int64)
    span = np.asarray(dense["row_span"])[rows].astype(np.int64)
    first = int(keys[int(rows[0]) // K])
    owned = np.arange(dense["dense_score"].shape[1])[None, :] < span[:, None]           # row-major: the rows in order, each one's frames in order
    return dict(frames=list(range(first, first + int(span.sum()))), boxes=dense["dense_box"][rows][owned], frame_scores=dense["dense_score"][rows][owned],
                key_index=np.repeat(np.arange(len(rows), dtype=np.int64), span))


def actor_tracks(box, actor, queries, actions, S, A, link_iou, max_gap, window):
    """Actor tracks of ONE video: the definition of ``tuber_track_actions`` and the fallback of ``video.VideoActors.tracks``.
    The rows are a padded [S][A] actor store (``detect.decode_actors_host`` per key frame): ``box`` [S * A, 4] fp32 xyxy, ``actor`` [S * A] fp32,
    ``queries`` [S * A] (-1: a row behind its key's count), ``actions`` [S * A, C] fp32; row r = slot * A + a, the slots being key ordinals.

    1. Link, class-agnostic: ``link_rows`` with ``class_num = 1``, the class 0 for an actor row and -1 for a row behind the count, the score the
       actor probability -> ``row_head``, ``tube_score`` (the track's mean actor probability), ``tube_len``, ``tube_last``, unchanged.
    2. Aggregate.  A track has the rows r_0 < ... < r_{L-1} at the slots s_i.  Per class: ``track_mean`` [S * A, C] fp64 at the head row, the fp64
       sum of ``float64(actions[r_i])`` in slot order divided by L; ``track_peak`` [S * A, C] fp32 at the head row, the maximum; ``row_smooth``
       [S * A, C] fp64 at every row of a track, the fp64 sum in slot order over the rows j of the track with ``|s_j - s_i| <= window`` divided by
       their number (``window`` counts key frames, like ``max_gap``).  A NaN propagates as in numpy's sum and max.  Rows with ``row_head`` -1
       hold zeros, and so do the track fields at rows that are no head."""
    S, A, window = int(S), int(A), int(window)
    N = S * A
    box = np.asarray(box, dtype=np.float32).reshape(N, 4)
    actor = np.asarray(actor, dtype=np.float32).reshape(N)
    queries = np.asarray(queries).reshape(N)
    actions = np.asarray(actions, dtype=np.float32).reshape(N, -1)
    C = actions.shape[1]
    slot = np.repeat(np.arange(S, dtype=np.int64), A)
    out = link_rows(box, np.where(queries >= 0, 0, -1), actor, slot, [0, S], 1, link_iou, max_gap)
    smooth, mean, peak = np.zeros((N, C)), np.zeros((N, C)), np.zeros((N, C), dtype=np.float32)
    members = {}
    for r in np.nonzero(out["row_head"] >= 0)[0].tolist():
        members.setdefault(int(out["row_head"][r]), []).append(r)          # ascending rows: slot order, one row per slot
    for h, rows in members.items():
        acc = np.zeros(C)
        for r in rows:
            acc = acc + actions[r].astype(np.float64)
        mean[h] = acc / len(rows)
        peak[h] = np.max(actions[rows], axis=0)
        for r in rows:
            near = [j for j in rows if abs(int(slot[j]) - int(slot[r])) <= window]
            acc = np.zeros(C)
            for j in near:
                acc = acc + actions[j].astype(np.float64)
            smooth[r] = acc / len(near)
    out.update(row_smooth=smooth, track_mean=mean, track_peak=peak)
    return out


class TubeLinker:
    """``link_rows`` for ONE video whose slots arrive in pieces: ``push(box, cls, score, K)`` links the next ``len(cls) // K`` slots of ``K`` rows
    each (rows behind a slot's count: class -1) and returns, per new row, ``row_head`` (the GLOBAL row ``ordinal * K + position`` of the tube's
    first detection, -1 for a row that is not counted), ``row_score`` (the tube's fp64 mean after taking the row) and ``row_len`` (its count
    after taking the row); a tube's score and length are those of its last row.  Between pushes a class keeps what ``link_rows`` keeps between
    slots: per tube the head, the fp64 score sum, the count, the last slot and the last box.  Pushing everything at once gives ``link_rows``'
    ``row_head`` and, at a tube's last row, its ``tube_score`` (bit for bit) and ``tube_len``.  ``K`` is the same for every push of a video.
    The definition of ``tuber_tube_link_stream`` and the fallback of ``video.VideoStream`` beyond the linker's bounds."""

    def __init__(self, class_num, link_iou, max_gap):
        self.class_num, self.link_iou, self.max_gap = int(class_num), float(link_iou), int(max_gap)
        self.reset()

    def reset(self):
        """the next push is slot 0 of a new video"""
        self.slots, self.K = 0, None
        self._tubes = {}                              # class -> [[head, fp64 score sum, count, last slot, last box fp64], ...]

    def push(self, box, cls, score, K):
        box = np.asarray(box, dtype=np.float32).reshape(-1, 4)
        cls, score, K = np.asarray(cls).reshape(-1), np.asarray(score).reshape(-1), int(K)
        N, C = len(box), self.class_num
        if K < 1 or N % K or len(cls) != N or len(score) != N:
            raise ValueError("TubeLinker.push: %d boxes, %d classes, %d scores in slots of %d rows" % (N, len(cls), len(score), K))
        if self.K not in (None, K):
            raise ValueError("TubeLinker.push: %d rows per slot after %d" % (K, self.K))
        self.K = K
        base = self.slots * K                         # the global row of this push's row 0
        box64 = box.astype(np.float64)
        head = np.full(N, -1, dtype=np.int64)
        rscore, rlen = np.zeros(N), np.zeros(N, dtype=np.int64)
        groups = {}
        for r in np.nonzero(_counted_rows(box, cls, score, C))[0].tolist():
            groups.setdefault(int(cls[r]), []).append(r)
        for c, rows in groups.items():
            tubes, i = self._tubes.get(c, []), 0
            while i < len(rows):
                s, j = self.slots + rows[i] // K, i
                while j < len(rows) and self.slots + rows[j] // K == s:
                    j += 1
                tubes, takes = link_slot(tubes, s, rows[i:j], score, box64, self.link_iou, self.max_gap, base)
                i = j
                for r, t in takes.items():
                    head[r], rscore[r], rlen[r] = t[0], t[1] / t[2], t[2]
            self._tubes[c] = tubes
        self.slots += N // K
        return dict(row_head=head, row_score=rscore, row_len=rlen)


def smooth_range(base, n, window, flush=False):
    """``[lo, hi)``: the key-frame slots whose smoothed rows a push of the slots ``[base, base + n)`` emits.  A smoothed
    row looks ``window`` slots ahead, so it is emitted ``window`` slots late: ``lo = max(base - window, 0)``; ``hi = base + n`` when ``flush``
    (the end of the video: what is there is all there will be), else ``max(base + n - window, lo)``.  Over the pushes of a video the ranges
    partition ``[0, S)`` in order.  Host integer arithmetic: ``video.VideoStream`` sizes its buffers with it and synchronises nowhere."""
    base, n, window = int(base), int(n), int(window)
    if base < 0 or n < 0 or window < 0:
        raise ValueError("smooth_range: base = %d, n = %d, window = %d must be >= 0" % (base, n, window))
    lo = max(base - window, 0)
    return lo, (base + n if flush else max(base + n - window, lo))


def track_ring_slots(max_gap, window):
    """H, the key-frame slots an ``ActorTracker`` (and ``tuber_track_actions_stream``) keeps between pushes: ``max(2 * window, max_gap + 1) + 1``.
    A new row looks for its predecessor at most ``max_gap + 1`` slots back; the smoothed slot ``t`` is emitted when slot ``t + window`` has
    arrived and reads back to ``t - window``: 2 * window + 1 slots, the newest one included."""
    return max(2 * int(window), int(max_gap) + 1) + 1


class ActorTracker:
    """``actor_tracks`` for ONE video whose key frames arrive in pieces: the definition of ``tuber_track_actions_stream``
    and the fallback of ``video.VideoStream(..., actors=A)`` beyond its bounds.

    ``push(box, actor, queries, actions, A, flush=False)`` takes the next ``n = len(queries) // A`` slots of a padded [n][A] actor store
    (``actor_tracks``' layout) and returns, per new row, ``row_head`` / ``row_score`` / ``row_len`` -- exactly
    ``TubeLinker(1, link_iou, max_gap).push(box, where(queries >= 0, 0, -1), actor, A)``, heads being global rows ``ordinal * A + position``
    -- and ``row_mean`` [n * A, C] fp64 / ``row_peak`` [n * A, C] fp32: the track's running mean (the fp64 sum of ``float64(actions)`` over the
    track's rows so far, in slot order, divided by their count) and running maximum (``np.max``: a NaN stays) after taking the row; zeros at
    rows with head -1.  At a track's last row they are ``actor_tracks``' ``track_mean`` / ``track_peak`` bit for bit.

    ``smooth`` [(hi - lo) * A, C] fp64 with ``smooth_lo`` / ``smooth_hi`` = ``smooth_range(base, n, window, flush)``: ``actor_tracks``'
    ``row_smooth`` of the slots ``[lo, hi)``, emitted ``window`` slots late because it is centred -- per row the fp64 sum, in slot order, over
    the members of its track at the slots ``[t - window, min(t + window, newest)]`` divided by their number.  ``flush=True`` marks the end of
    the video (a push without rows is legal then); ``reset()`` starts a new video.

    Between pushes the tracker keeps the last H = ``track_ring_slots(max_gap, window)`` slots in a ring, entry ``ordinal % H``: per row the head,
    the count, the running fp64 sum, the fp32 peak and the fp32 action row.  Every pushed slot, an empty one included, writes its entry, so an
    entry of an ordinal below 0 or not yet pushed is never consulted."""

    def __init__(self, link_iou, max_gap, window):
        self.link_iou, self.max_gap, self.window = float(link_iou), int(max_gap), int(window)
        if self.max_gap < 0 or self.window < 0:
            raise ValueError("ActorTracker: max_gap = %d and window = %d must be >= 0" % (self.max_gap, self.window))
        self.H = track_ring_slots(self.max_gap, self.window)
        self.linker = TubeLinker(1, self.link_iou, self.max_gap)
        self.reset()

    def reset(self):
        """the next push is slot 0 of a new video"""
        self.linker.reset()
        self.slots, self.A, self.C = 0, None, None
        self._head = self._cnt = self._sum = self._peak = self._act = None

    def _member(self, t, h):
        """the position in slot t of the row whose head is h, -1 when the slot has none"""
        hit = np.nonzero(self._head[t % self.H] == h)[0]
        return int(hit[0]) if len(hit) else -1

    def _smooth_slot(self, t, newest, out):
        """the smoothed rows of slot t into ``out`` [A, C], the newest slot pushed being ``newest``"""
        w, H = self.window, self.H
        for a in range(self.A):
            h = int(self._head[t % H, a])
            if h < 0:
                continue
            acc, n = np.zeros(self.C), 0
            for u in range(max(t - w, 0), min(t + w, newest) + 1):
                j = self._member(u, h)
                if j >= 0:
                    acc = acc + self._act[u % H, j].astype(np.float64)
                    n += 1
            out[a] = acc / n

    def push(self, box, actor, queries, actions, A, flush=False):
        A = int(A)
        queries = np.asarray(queries).reshape(-1)
        N = len(queries)
        if A < 1 or N % A:
            raise ValueError("ActorTracker.push: %d rows in slots of %d" % (N, A))
        actions = np.asarray(actions, dtype=np.float32)
        actions = actions.reshape(N, -1) if N else actions.reshape(0, self.C or 0)
        C = actions.shape[1] if N else (self.C or 0)
        if self.A is None and N:
            self.A, self.C, H = A, C, self.H
            self._head = np.full((H, A), -1, dtype=np.int64)
            self._cnt = np.zeros((H, A), dtype=np.int64)
            self._sum, self._peak, self._act = np.zeros((H, A, C)), np.zeros((H, A, C), dtype=np.float32), np.zeros((H, A, C), dtype=np.float32)
        elif N and (A, C) != (self.A, self.C):
            raise ValueError("ActorTracker.push: slots of %d rows with %d classes after %d with %d" % (A, C, self.A, self.C))
        n, base, w, H = N // A, self.slots, self.window, self.H
        link = self.linker.push(box, np.where(queries >= 0, 0, -1), np.asarray(actor, dtype=np.float32).reshape(-1), A) if N else dict(
            row_head=np.zeros(0, dtype=np.int64), row_score=np.zeros(0), row_len=np.zeros(0, dtype=np.int64))
        lo, hi = smooth_range(base, n, w, flush)
        mean, peak = np.zeros((N, C)), np.zeros((N, C), dtype=np.float32)
        smooth = np.zeros(((hi - lo) * A, C))
        for i in range(n):
            s, e = base + i, (base + i) % H
            self._head[e] = link["row_head"][i * A:(i + 1) * A]      # the entry of slot s - H goes: nothing looks that far back
            self._cnt[e] = 0
            for a in range(A):
                h, r = int(self._head[e, a]), i * A + a
                if h < 0:
                    self._sum[e, a], self._peak[e, a], self._act[e, a] = 0.0, 0.0, 0.0
                    continue
                v = actions[r]
                cnt, acc, top = 1, np.zeros(C) + v.astype(np.float64), v.copy()
                for t in range(s - 1, max(s - self.max_gap - 1, 0) - 1, -1):      # the predecessor: the same head at most max_gap + 1 slots back
                    j = self._member(t, h)
                    if j >= 0:
                        cnt = int(self._cnt[t % H, j]) + 1
                        acc = self._sum[t % H, j] + v.astype(np.float64)
                        with np.errstate(invalid="ignore"):
                            top = np.max(np.stack([self._peak[t % H, j], v]), axis=0)
                        break
                self._cnt[e, a], self._sum[e, a], self._peak[e, a], self._act[e, a] = cnt, acc, top, v
                mean[r], peak[r] = acc / cnt, top
            if s - w >= 0:                                            # slot s - window has its whole window now
                self._smooth_slot(s - w, s, smooth[(s - w - lo) * A:(s - w - lo + 1) * A])
        self.slots = base + n
        if flush:                                                     # the end: the last slots take what is there
            for t in range(max(self.slots - w, lo), self.slots):
                self._smooth_slot(t, self.slots - 1, smooth[(t - lo) * A:(t - lo + 1) * A])
        return dict(row_head=link["row_head"], row_score=link["row_score"], row_len=link["row_len"], row_mean=mean, row_peak=peak, smooth=smooth,
                    smooth_lo=lo, smooth_hi=hi)


class VideoMAP:
    """Video-level mean average precision over action tubes: per (video, class) the per-frame detections are linked greedily into tubes
    (``link``), the tubes are matched against the ground-truth tubes by spatio-temporal IoU (``match``), and the ranked flags give VOC AP per
    class (``evaluate``).  Counting rule of ``FrameMAPUCF`` (a row of C + 1 probabilities is one detection of its arg-max class; not counted
    when no-object is the arg-max, the box is not a box, or the arg-max probability is NaN); no exclude list.  Plain numpy / Python: the
    definition ``device_map.DeviceVideoMAP`` reproduces, and its fallback."""

    def __init__(self, class_num=24, link_iou=0.2, max_gap=2, min_len=1, thresholds=(0.2, 0.5, 0.75, "0.5:0.95"), tube_nms=None):
        self.class_num, self.link_iou, self.max_gap, self.min_len = int(class_num), float(link_iou), int(max_gap), int(min_len)
        self.thresholds = tuple(thresholds)
        self.tube_nms = None if tube_nms is None else float(tube_nms)     # the stIoU above which a lower-ranked tube is a duplicate (``tube_nms``)
        self.num_categories = 24
        self.det_keys, self._box, self._prob = [], [], []
        self.gt_keys, self.gt_rows = [], []

    def add_detections(self, keys, boxes, probs):
        """``keys``: one "<video>-<frame>" key per row; ``boxes`` [n, 4] fp32 xyxy, ``probs`` [n, C + 1] fp32"""
        keys = list(keys)
        boxes, probs = np.asarray(boxes, dtype=np.float32).reshape(-1, 4), np.asarray(probs, dtype=np.float32).reshape(-1, self.class_num + 1)
        assert len(boxes) == len(keys) == len(probs), (len(boxes), len(keys), len(probs))
        self.det_keys.extend(keys); self._box.append(boxes); self._prob.append(probs)

    def add_ground_truth(self, keys, boxes, classes, tubes=None):
        """one line per box: its key, box (fp64 xyxy), 0-based class and, with ``tubes``, the integer id of its tube"""
        keys = list(keys)
        boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
        tubes = [None] * len(keys) if tubes is None else [None if t is None else int(t) for t in tubes]
        assert len(boxes) == len(keys) == len(classes) == len(tubes)
        self.gt_keys.extend(keys)
        self.gt_rows.extend((int(c), boxes[i], tubes[i]) for i, c in enumerate(classes))

    def link(self):
        """-> dict: ``order`` (layout row -> store row), ``det_box``, ``det_prob``, ``row_slot`` in layout order, ``row_cls`` (arg-max column),
        ``row_head`` (layout row of the tube's first detection, -1 for a row that is not counted), at head rows ``tube_score`` (fp64 mean of
        the fp32 scores), ``tube_len``, ``tube_last`` (last slot); ``layout``; ``tubes`` (``tubes_from_link``); with ``tube_nms`` set,
        ``tube_keep`` (``tube_nms``)."""
        C, N = self.class_num, len(self.det_keys)
        lay = tube_layout(self.det_keys, self.gt_keys)
        box = np.concatenate(self._box) if self._box else np.zeros((0, 4), np.float32)
        prob = np.concatenate(self._prob) if self._prob else np.zeros((0, C + 1), np.float32)
        order = np.argsort(lay["det_slot"], kind="stable")
        box, prob, slot = box[order], prob[order], lay["det_slot"][order]
        cls = prob.argmax(axis=1) if N else np.zeros(0, dtype=np.int64)
        score = prob[np.arange(N), cls]
        rows = link_rows(box, cls, score, slot, lay["video_off"], C, self.link_iou, self.max_gap)
        head, tscore, tlen, tlast = rows["row_head"], rows["tube_score"], rows["tube_len"], rows["tube_last"]
        link = dict(order=order, det_box=box, det_prob=prob, row_slot=slot, row_cls=cls, row_head=head, tube_score=tscore, tube_len=tlen,
                    tube_last=tlast, layout=lay)
        link["tubes"] = tubes_from_link(link)
        if self.tube_nms is not None:
            link["tube_keep"] = tube_nms(link, self.tube_nms, self.min_len)
        return link

    def st_iou(self, link=None):
        """-> (gt, overlaps): the ground-truth tubes {(video, class, id): {slot: box}} and {head: {(video, class, id): stIoU}} over the
        ground-truth tubes of the tube's (video, class)"""
        link = link or self.link()
        gt = ground_truth_tubes(link["layout"], self.gt_rows)
        by_vc = {}
        for key in sorted(gt):
            by_vc.setdefault(key[:2], []).append(key)
        box64, slot = link["det_box"].astype(np.float64), link["row_slot"]
        videos = {name: v for v, name in enumerate(link["layout"]["videos"])}
        overlaps = {}
        for t in link["tubes"]:
            mine = {int(slot[r]): r for r in t["rows"]}
            row = overlaps[t["head"]] = {}
            for key in by_vc.get((videos[t["video"]], t["cls"] - 1), []):
                g = gt[key]
                shared = sorted(set(mine) & set(g))
                total = 0.0
                for s in shared:
                    with np.errstate(all="ignore"):
                        total += float(_iou_one_to_many(box64[mine[s]], g[s][None, :])[0])
                row[key] = total / (len(mine) + len(g) - len(shared)) if shared else 0.0
        return gt, overlaps

    def match(self, link=None):
        """-> (n_gt {class 1-based: ground-truth tubes}, flags {threshold: uint8 [N] in layout order: 1 true positive, 0 false positive, 2 not
        counted}, link) over ``expand_thresholds(self.thresholds)``.  With ``tube_nms`` set, a suppressed tube is treated exactly like one shorter
        than ``min_len``: flag 2, it takes no ground-truth tube and is not ranked."""
        link = link or self.link()
        gt, overlaps = self.st_iou(link)
        n_gt = {}
        for (_, c, _) in gt:
            if 0 <= c < self.class_num:
                n_gt[c + 1] = n_gt.get(c + 1, 0) + 1
        N = len(link["row_head"])
        groups = {}
        keep = None
        if self.tube_nms is not None:
            keep = link["tube_keep"] if "tube_keep" in link else tube_nms(link, self.tube_nms, self.min_len)
        for t in link["tubes"]:
            if len(t["frames"]) >= self.min_len and (keep is None or keep[t["head"]] == 1):
                groups.setdefault((t["video"], t["cls"]), []).append(t)
        flags = {}
        for thr in expand_thresholds(self.thresholds):
            fl = flags[thr] = np.full(N, 2, dtype=np.uint8)
            for tubes in groups.values():
                taken = set()
                for t in sorted(tubes, key=lambda t: (-t["score"] if t["score"] == t["score"] else np.inf, t["head"])):
                    bk, bv = None, 0.0
                    for key, x in overlaps[t["head"]].items():             # ascending tube id
                        if key not in taken and (bk is None or x > bv):
                            bk, bv = key, x
                    tp = bk is not None and bv >= thr
                    if tp:
                        taken.add(bk)
                    fl[t["head"]] = 1 if tp else 0
        return n_gt, flags, link

    def evaluate(self):
        """-> {threshold: (video-mAP, {class_id: AP})} for the configured thresholds; "0.5:0.95" is the mean over its ten members"""
        n_gt, flags, link = self.match()
        N = len(link["row_head"])
        is_head = link["row_head"] == np.arange(N)
        at = {}
        for thr, fl in flags.items():
            per_class = {}
            for cls in range(1, self.class_num + 1):
                if n_gt.get(cls, 0) == 0:
                    continue
                heads = np.nonzero(is_head & (link["row_cls"] == cls - 1) & (fl != 2))[0]
                if len(heads) == 0:
                    per_class[cls] = 0.0
                    continue
                t = (fl[heads] == 1)[np.argsort(-link["tube_score"][heads], kind="stable")]
                ctp = np.cumsum(t).astype(float); cfp = np.cumsum(~t).astype(float)
                per_class[cls] = _average_precision(ctp / np.maximum(ctp + cfp, np.finfo(np.float64).eps), ctp / n_gt[cls])
            at[thr] = (mean_ap(per_class, self.num_categories), per_class)
        return collect_thresholds(self.thresholds, at)


def collect_thresholds(thresholds, at):
    """{numeric threshold: (mAP, per_class)} -> the same for the configured ``thresholds``, "0.5:0.95" as the mean over its members"""
    out = {}
    for t in thresholds:
        if t == "0.5:0.95":
            members = [at[m] for m in VIDEO_MAP_RANGE]
            per_class = {c: float(np.mean([m[1][c] for m in members])) for c in members[0][1]}
            out[t] = (float(np.mean([m[0] for m in members])), per_class)
        else:
            out[t] = at[float(t)]
    return out


@_with_averaged_weights
@torch.no_grad()
def validate_tuber_ucf_detection(cfg, model, criterion, postprocessors, data_loader, epoch, writer=None, verbose=True, results=None):
    """utils/video_action_recognition.py:456-689 (called by train_tuber_jhmdb.py:83 / eval_tuber_jhmdb.py:77): eval-mode forward on
    the HIP path, ``PostProcess``, the key frame's QUERY_NUM tubelet queries of every clip written to ``{rank}.txt`` (box + C+1
    class probabilities), ``binary_{rank}.txt`` (visibility probabilities) and ``GT_{rank}.txt`` (raw box + one-hot label), then
    frame-mAP@0.5 by ``FrameMAPUCF`` on rank 0.  Differences from the reference: barriers only when torch.distributed is
    initialised; the one-hot width is max(21, NUM_CLASSES) (the reference hard-codes 21, :564, which UCF101-24 would overflow).
    With ``CONFIG.VAL.DEVICE_MAP.ENABLE`` the same rows go from ``PostProcess.decode`` into a ``device_map.DeviceFrameMAPUCF`` and the
    metric is computed on the device; the three files are written only with ``FILES``.  With ``CONFIG.VAL.VIDEO_MAP.ENABLE`` the rows go
    into a ``device_map.DeviceVideoMAP`` (``FILES`` keeps its meaning), the return value is still frame-mAP, and the video-mAPs over linked
    tubes are printed, written to the writer as ``val/video_mAP@<thr>`` and left in ``results`` (a dict: ``results["video_mAP"][thr]``,
    ``results["video_AP"][thr]``); with ``CONFIG.VAL.TUBE_NMS.IOU`` the tubes of a (video, class) go through ``tube_nms`` before they are
    matched.  A DistributedSampler's padded repeat frames are not de-duplicated."""
    import torch.distributed as dist
    C = cfg.CONFIG
    ddp = dist.is_available() and dist.is_initialized()
    rank = dist.get_rank() if ddp else 0
    world = dist.get_world_size() if ddp else 1
    model.eval()
    criterion.eval()
    dev = next(model.parameters()).device
    res = os.path.join(C.LOG.BASE_PATH, C.LOG.RES_DIR)
    if rank == 0:
        os.makedirs(res, exist_ok=True)
        for p in glob.glob(os.path.join(res, "*.txt")):
            os.remove(p)
    Q, nc = C.MODEL.QUERY_NUM, C.DATA.NUM_CLASSES
    width = max(21, nc)
    buff_output, buff_anno, buff_id, buff_binary, gt_label, gt_anno, gt_id = [], [], [], [], [], [], []
    dm = getattr(C.VAL, "DEVICE_MAP", None)
    store, files, frame_on_device = None, True, True
    vm = getattr(C.VAL, "VIDEO_MAP", None)
    video = vm is not None and vm.ENABLE
    if video:
        from .config import tube_nms_settings, video_map_settings
        from .device_map import DeviceVideoMAP
        store = DeviceVideoMAP(class_num=nc, label_width=width, device=dev, tube_nms=tube_nms_settings(cfg)["iou"], **video_map_settings(cfg))
        frame_on_device = dm is not None and bool(dm.ENABLE)      # without DEVICE_MAP frame-mAP still comes from the result files
        files = bool(dm.FILES) if frame_on_device else True
    elif dm is not None and dm.ENABLE:
        from .device_map import DeviceFrameMAPUCF
        store = DeviceFrameMAPUCF(class_num=nc, label_width=width, device=dev)
        files = bool(dm.FILES)

    def onehot_of(lab):
        onehot = np.zeros((len(lab), width), dtype=np.int64)
        for i in range(len(lab)):
            onehot[i, int(lab[i])] = 1
        return onehot
    meters = {k: [0.0, 0] for k in ("loss", "loss_bbox", "loss_giou", "loss_ce", "class_error")}
    graphed = _graphed_eval(cfg, model)
    end = time.time()
    for idx, data in enumerate(data_loader):
        samples, targets = data[0], data[1]
        samples = samples.to(dev)
        batch_id = [t["image_id"] for t in targets]
        host_targets = targets               # the loader's own tensors: the device evaluator takes its ground truth from them, without a sync
        targets = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in t.items() if k != "image_id"} for t in targets]
        outputs = _forward_checked(model, samples, graphed)
        loss_dict = criterion(outputs, targets)
        sizes = torch.stack([t["size"] for t in targets], dim=0)
        if store is None:
            scores, boxes, output_b = postprocessors["bbox"](outputs, sizes)
        else:
            d_scores, d_boxes, d_binary = postprocessors["bbox"].decode(outputs, sizes)
            if files:                        # what PostProcess.forward returns, bit for bit
                scores, boxes, output_b = d_scores.cpu().numpy(), d_boxes.cpu().numpy(), d_binary.cpu().numpy()
            first = None
            for b in range(len(host_targets)):
                raw = host_targets[b]["raw_boxes"]
                if len(raw) == 0:
                    continue
                frame_id, key_pos = batch_id[b][0], int(batch_id[b][1])
                store.add_detections([frame_id] * Q, d_boxes[b, key_pos * Q:(key_pos + 1) * Q, :], d_scores[b, key_pos * Q:(key_pos + 1) * Q, :])
                raw = raw.reshape(-1, raw.shape[-1])
                if first is None:
                    first = float(host_targets[0]["raw_boxes"].reshape(-1, raw.shape[-1])[0, 0])
                store.add_ground_truth([batch_id[int(float(raw[x, 0]) - first)][0] for x in range(len(raw))], raw[:, 2:6].double(),
                                       onehot_of(host_targets[b]["labels"]))
        for b in range(len(targets) if files else 0):
            raw = targets[b]["raw_boxes"]
            if len(raw) == 0:
                continue
            frame_id, key_pos = batch_id[b][0], int(batch_id[b][1])
            buff_output.append(scores[b, key_pos * Q:(key_pos + 1) * Q, :])
            buff_anno.append(boxes[b, key_pos * Q:(key_pos + 1) * Q, :])
            for _ in range(Q):
                buff_id.append(frame_id)
                buff_binary.append(output_b[..., 0])
            raw = raw.reshape(-1, raw.shape[-1])
            gt_label.append(onehot_of(targets[b]["labels"]))
            gt_anno.append(raw.detach().cpu().numpy())
            first = float(targets[0]["raw_boxes"].reshape(-1, raw.shape[-1])[0, 0])
            gt_id.extend(batch_id[int(float(raw[x, 0]) - first)][0] for x in range(len(raw)))
        wd = criterion.weight_dict
        total = float(sum(loss_dict[k] * wd[k] for k in loss_dict if k in wd))
        if not math.isfinite(total):
            raise FloatingPointError("loss is %r in evaluation: %r" % (total, {k: float(v) for k, v in loss_dict.items()}))
        n = len(targets)
        for k, v in (("loss", total), ("loss_bbox", loss_dict["loss_bbox"]), ("loss_giou", loss_dict["loss_giou"]),
                     ("loss_ce", loss_dict["loss_ce"]), ("class_error", loss_dict["class_error"])):
            meters[k][0] += float(v) * n; meters[k][1] += n
        if verbose and rank == 0:
            print("Epoch: [%d][%d/%d]  batch time %.3f  " % (epoch, idx + 1, len(data_loader), time.time() - end) +
                  ", ".join("%s: %.3f" % (k, s / max(c, 1)) for k, (s, c) in meters.items()))
        end = time.time()
    graphed = None                           # the captures and their private pools go with it
    if writer is not None and rank == 0:
        for k, name in (("class_error", "class_error"), ("loss", "totall_loss"), ("loss_bbox", "loss_bbox"), ("loss_giou", "loss_giou"), ("loss_ce", "loss_ce")):
            writer.add_scalar("val/" + name, meters[k][0] / max(meters[k][1], 1), epoch)
    cat = lambda xs, w: np.concatenate(xs, axis=0) if xs else np.zeros((0, w))
    out_a, anno_a = cat(buff_output, nc + 1), cat(buff_anno, 4)
    gl, ga = cat(gt_label, width), cat(gt_anno, 6)
    if files:
        with open(os.path.join(res, "%d.txt" % rank), "w") as f:
            for x in range(len(buff_id)):
                f.write("{} {}\n".format(buff_id[x], np.concatenate([anno_a[x], out_a[x]]).tolist()))
        with open(os.path.join(res, "binary_%d.txt" % rank), "w") as f:
            for x in range(len(buff_id)):
                f.write("{} {}\n".format(buff_id[x], np.asarray(buff_binary[x]).tolist()))
        with open(os.path.join(res, "GT_%d.txt" % rank), "w") as f:
            for x in range(len(gt_id)):
                f.write("{} {}\n".format(gt_id[x], np.concatenate([ga[x], gl[x]]).tolist()))
    if ddp:
        dist.barrier()
    if store is not None and ddp:
        store = store.all_gather_merge()     # every rank's rows in rank order: the order in which rank 0 loads the files
    mAP = 0
    if rank == 0:
        if store is not None and frame_on_device:
            mAP, per_class = store.evaluate()
        else:
            ev = FrameMAPUCF(class_num=nc)
            ev.load_gt([os.path.join(res, "GT_%d.txt" % r) for r in range(world)])
            ev.load_detections([os.path.join(res, "%d.txt" % r) for r in range(world)])
            mAP, per_class = ev.evaluate()
        if verbose:
            print("mAP: %.5f" % mAP)
        if writer is not None:
            writer.add_scalar("val/val_mAP_epoch", mAP, epoch)
        if video:
            vres = store.evaluate_video()
            if results is not None:
                results["video_mAP"] = {t: m for t, (m, _) in vres.items()}
                results["video_AP"] = {t: ap for t, (_, ap) in vres.items()}
            if verbose:
                print("video-mAP: " + ", ".join("@%s %.5f" % (t, m) for t, (m, _) in vres.items()))
            if writer is not None:
                for t, (m, _) in vres.items():
                    writer.add_scalar("val/video_mAP@%s" % t, m, epoch)
    if ddp:
        dist.barrier()
    return mAP
