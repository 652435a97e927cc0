"""Whole-video inference: frames in, detections per key frame and action tubes out.

The reference reaches its model through a dataset loader that cuts one clip per annotated key frame on CPU workers
(``datasets/ava_frame.py:37-74,133-152``, ``datasets/jhmdb_frame.py:194-223``); it has no path from a video to detections.  Here a video is
resident ONCE on the device at working resolution (``tuber_frames_resize``, every frame resized once), the overlapping clips of a batch of key
frames are gathered from it by one launch (``tuber_video_clips``, csrc/video_clips.hip) reading a frame-index table (``clip_indices``), the
captured ``detect.Detector`` runs over them, and the ranked detections of all key frames are linked into tubes by the wave-per-(video, class)
linker in its ranked form (``tuber_tube_link_ranked``, csrc/tube_map.hip; ``evaluation.link_rows`` is its definition and its fallback).

``VideoStream`` is the same computation for a video that arrives in pieces: a ring of the last R frames instead of the
resident video (``tuber_video_clips_ring`` evaluates the index rule itself), the same batches of key frames as soon as their clips can no longer
change, and the linker resumed push by push (``tuber_tube_link_stream``; ``evaluation.TubeLinker`` is its definition and its fallback).
``VideoDetector`` is the definition the stream is held to.  With ``actors=A`` the stream carries the actor tracks of section 6i as well
(DESIGN.md section 6j): per-track action sums resumed push by push (``tuber_track_actions_stream``; ``evaluation.ActorTracker`` is its
definition and its fallback) and ``VideoStream.tracks()``.

``tubes(dense=True)`` / ``tracks(dense=True)`` put a box on every frame of a tube's extent, interpolated between the linked
key detections: ``tuber_tube_dense`` behind the link step over a whole video (``evaluation.dense_rows`` is its definition and its fallback),
``evaluation.dense_tube`` on the host for the closed tubes of a stream.

``VideoDetector(..., keep_video=True)`` leaves the resident video with its result, whose ``crops(tubes)`` cuts the boxes
of tubes and tracks out of it on the device (``crops.tube_crops`` / ``tuber_tube_crops``; ``crops.crop_rows`` is its definition and its fallback).
"""
import functools
import sys

import numpy as np
import torch

from . import input_pipeline as ip
from . import lib
from .detect import ACTOR_FIELDS, FIELDS, Detector, Record, field_tensors, host_parts
from .device_map import DENSE_NAMES, dense_beyond, link_beyond, link_limits, link_ranked, tube_dense_launch, tube_nms_launch
from .misc import NestedTensor

RULES = ("ava", "jhmdb", "edge")


def clip_indices(n_frames, keys, T, rate=1, rule="ava"):
    """The frames of the clip around every key frame: int32 [len(keys), T] of 0-based frame numbers in [0, n_frames).

    ``rule="ava"`` (datasets/ava_frame.py:43,143-145): ``start = max(key - T//2 * rate, 0)``, then
    ``clip(range(start, start + T * rate, rate), 0, n - 1)`` -- a clip at the front of a video starts at frame 0, so its key frame sits before
    position T//2.  ``rule="jhmdb"`` (datasets/jhmdb_frame.py:201-208, ids 0-based; ``rate`` is not used): ``start = max(key - T//2, 0)``,
    ``end = min(key + T - T//2, n - 1)``, ``range(start, end)``; a short clip gets ``(T - len) // 2`` copies of frame 0 in front -- the
    reference's pad, whatever ``start`` is -- and copies of ``end`` behind.  ``rule="edge"`` is not a reference rule: it keeps the key frame
    at position T//2, ``clamp(key + (i - T//2) * rate, 0, n - 1)``."""
    n, T, rate = int(n_frames), int(T), int(rate)
    if n < 1 or T < 1 or rate < 1:
        raise ValueError("clip_indices: n_frames = %d, T = %d, rate = %d must be >= 1" % (n, T, rate))
    if rule not in RULES:
        raise ValueError("clip_indices: rule %r is not one of %s" % (rule, ", ".join(RULES)))
    keys = [int(k) for k in keys]
    out = np.zeros((len(keys), T), dtype=np.int32)
    for i, key in enumerate(keys):
        if not 0 <= key < n:
            raise ValueError("clip_indices: key frame %d outside the video's %d frames" % (key, n))
        if rule == "ava":
            start = max(key - T // 2 * rate, 0)
            out[i] = np.clip(np.arange(start, start + T * rate, rate), 0, n - 1)
        elif rule == "jhmdb":
            start = max(key - T // 2, 0)
            end = min(key + T - T // 2, n - 1)
            ids = list(range(start, end))
            if len(ids) < T:
                front = (T - len(ids)) // 2
                ids = [0] * front + ids + [end] * (T - len(ids) - front)
            out[i] = ids[:T]
        else:
            out[i] = np.clip(key + (np.arange(T) - T // 2) * rate, 0, n - 1)
    return out


def working_geometry(H0, W0, size):
    """(nh, nw, y1, x1, h, w) of the reference's val pipeline for a H0 x W0 video: the short side resized to ``size``
    (datasets/ava_frame.py:86-91,127,149: ``int`` of the float sizes), then the window of ``Resize_Custom(size)``
    (datasets/video_transforms.py:210-227) in the resized frame"""
    oh, ow, size = int(H0), int(W0), int(size)
    if oh <= ow:
        nh, nw = size, size * (ow / oh)
    else:
        nw, nh = size, size * (oh / ow)
    H, W = int(nh), int(nw)
    if W < H:
        w, h = size, int(size * (H / W))
    else:
        h, w = size, int(size * (W / H))
    h, w = min(h, H), min(w, W)
    return H, W, int(round((H - h) / 2.0)), int(round((W - w) / 2.0)), h, w


def _nms_value(who, nms):
    """None, or the NMS threshold as a float in [0, 1]"""
    if nms is None:
        return None
    nms = float(nms)
    if not 0.0 <= nms <= 1.0:
        raise ValueError("%s: nms = %r must be None or a number in [0, 1]" % (who, nms))
    return nms


def _track_labels(mean, label_thr):
    """the 0-based classes with ``mean >= label_thr`` by mean descending, then class"""
    with np.errstate(invalid="ignore"):
        return sorted(np.nonzero(mean >= label_thr)[0].tolist(), key=lambda c: (-mean[c], c))


def _densified(t, dense):
    """the dict of a tube or track with a box on every frame (``dense``: ``evaluation.dense_tube``'s dict): ``frames`` / ``boxes`` per frame, the
    key frames and their boxes under ``keys`` / ``key_boxes``, and ``frame_scores`` / ``key_index`` beside them"""
    return dict(t, keys=t["frames"], key_boxes=t["boxes"], **dense)


class _VideoRecord(Record):
    """What ``VideoDetections`` and ``VideoActors`` share: a row per key frame, the defaults of ``tubes()`` / ``tracks()``, and ``to_host``."""

    def __init__(self, keys, tensors, settings, store, nms_iou, dense=False):
        super().__init__(*tensors)
        self.keys = [int(k) for k in keys]
        self.nms_iou = None if nms_iou is None else float(nms_iou)                      # the default of tubes(nms=) / tracks(nms=): CONFIG.VAL.TUBE_NMS
        self.dense = bool(dense)                                                       # the default of tubes(dense=) / tracks(dense=): CONFIG.VAL.VIDEO_MAP.DENSE
        self.settings = dict(settings)
        self._store = store                                                            # the engine's ParamStore: to_host reads its error word
        self.row_head = self.row_score = self.row_len = None                           # the link records of a VideoStream push
        if not all(len(self.keys) == t.shape[0] for t in tensors):
            raise ValueError("%s: %d keys, %d rows" % (type(self).__name__, len(self.keys), self.boxes.shape[0]))

    def to_host(self):
        """a list, per key frame, of dicts of numpy arrays trimmed to ``count`` (``key``, the per-row fields, ``count``, ``total``): one copy, the
        place that synchronises.  A cooperative decoder launch that timed out during the video leaves empty key frames (detect.py,
        "Fail-safe"); its error word travels in the same copy and raises here, the engine having switched to the launch chain: run the video
        again."""
        word = [self._store.coop_sync] if self._store is not None and self.boxes.device.type == "cuda" else []
        host, word = self._fetch(word)
        if word and word[0][2] and not self._store.coop_off:
            self._store.check_coop()
        return [self._trimmed(host, i, key=key) for i, key in enumerate(self.keys)]

    def _keep(self, host, link, nms, min_len):
        """None without ``nms``; else the kernel's ``tube_keep``, or ``evaluation.tube_nms`` over the host record ``link`` on the host path and at
        the kernel's escape"""
        from .evaluation import tube_nms
        if nms is None:
            return None
        keep = host.get("tube_keep")
        return tube_nms(link, nms, max(min_len, 1)) if keep is None or (keep == 3).any() else keep      # the host path, or the kernel's escape

    def _extent(self, dense, max_gap):
        """None without ``dense`` (None: the record's default); else G, the most frames a row can own (``evaluation.dense_extent``) -- host
        integers only, and keys that do not ascend strictly raise here, before anything is launched"""
        from .evaluation import dense_extent
        return dense_extent(self.keys, max_gap) if (self.dense if dense is None else bool(dense)) else None

    def _dense(self, host, score, max_gap, G, linked_on_host):
        """(None, None) without ``G``; else (the per-row dense record, why it was made on the host behind a device link or None): the
        kernel's four arrays as they were fetched, or ``evaluation.dense_rows`` on the host path, beyond 32 bits and at the kernel's escape"""
        from .evaluation import dense_rows
        if G is None:
            return None, None
        S, K = self.boxes.shape[:2]
        span = host.get("row_span")
        if span is not None and not (span == -1).any():
            return host, None
        why = None if linked_on_host else (dense_beyond(S, K, G) or "tuber_tube_dense left a row to the host (more than %d frames)" % G)
        return dense_rows(host["boxes"].reshape(-1, 4), score.reshape(-1), host["row_head"], self.keys, K, max_gap), why

    def _linked(self, link, slot_off, video_off, names, C, nms, min_len, dense=None):
        """the fields and the link records ``names`` (with ``nms``, ``tube_keep`` of ``tuber_tube_nms`` as well; with ``dense`` = (scores,
        max_gap, G), the four outputs of ``tuber_tube_dense``) as one dict, in one copy"""
        S, n = self.boxes.shape[:2]
        if nms is not None:
            link["tube_keep"] = tube_nms_launch(self.boxes.contiguous(), slot_off, video_off, link, 1, S, S * n, C, n, max(int(min_len), 1), nms)
            names += ("tube_keep",)
        if dense is not None and dense[2] is not None and not dense_beyond(S, n, dense[2]):
            link.update(tube_dense_launch(self.boxes, dense[0], link["row_head"], self.keys, dense[1], dense[2]))
            names += DENSE_NAMES
        host, records = self._fetch([link[k] for k in names])
        return dict(host, **dict(zip(names, records)))


class VideoDetections(_VideoRecord):
    """The ranked detections of a video's key frames: ``keys`` (frame numbers) and, as tensors on one device, ``boxes`` [n, K, 4] fp32 xyxy in
    source-video pixels, ``scores`` / ``aux`` [n, K] fp32, ``labels`` / ``queries`` [n, K] int32 (-1 in the rows behind ``count``), ``count`` /
    ``total`` [n] int32 -- the fields of ``detect.Detections``, a row per key frame."""
    FIELDS, ROW_FIELDS = FIELDS, FIELDS[:5]

    def __init__(self, keys, boxes, scores, labels, queries, aux, count, total, class_num, settings=None, store=None, nms_iou=None, dense=False):
        # the defaults of tubes(): CONFIG.VAL.VIDEO_MAP, CONFIG.VAL.TUBE_NMS.IOU
        super().__init__(keys, (boxes, scores, labels, queries, aux, count, total), settings or dict(link_iou=0.2, max_gap=2, min_len=1), store, nms_iou,
                         dense)
        self.class_num = int(class_num)
        self.tubes_path = None                                                         # "device" or "host" after tubes()
        self.actors = None                                                             # the ``VideoActors`` of ``VideoDetector(..., actors=A)``
        # ``VideoDetector(..., keep_video=True)``: the resident video uint8 [N, nh, nw, 3], the size (H0, W0) the boxes refer to, CONFIG.VAL.CROPS
        self.video, self.source_size, self.crop_settings = None, None, None

    # -- tubes ------------------------------------------------------------------------------------------------------------
    def _link_device(self, link_iou, max_gap, nms=None, min_len=1, G=None):
        """``tuber_tube_link_ranked`` (and, with ``nms``, ``tuber_tube_nms``, with ``G``, ``tuber_tube_dense`` behind it) over the padded store
        as it is, or None where the linker's bounds refuse it"""
        K = self.scores.shape[1]
        if self.boxes.device.type != "cuda":
            return None, "the store is on the CPU"
        why = link_beyond("%d rows per key frame with max_gap %d" % (K, max_gap), K, max_gap)
        if why:
            return None, why
        link, slot_off, video_off = link_ranked(self.boxes, self.labels, self.scores, self.class_num, link_iou, max_gap)
        return self._linked(link, slot_off, video_off, ("row_head", "tube_score", "tube_len", "tube_last"), self.class_num, nms, min_len,
                            (self.scores, max_gap, G)), None

    def tubes(self, link_iou=None, max_gap=None, min_len=None, nms=None, dense=None):
        """The action tubes of the video: a list of ``dict(cls, score, frames, boxes, length)`` in head order (the order of the tubes' first
        detections) -- ``cls`` 1-based as in ``evaluation.tubes_from_link``, ``score`` the fp64 mean of the linked fp32 scores, ``frames`` the key
        frame numbers, ``boxes`` [length, 4] in source pixels; tubes shorter than ``min_len`` are dropped.  The slots of the linker are key
        ORDINALS, so ``max_gap`` counts key frames.  Defaults: ``CONFIG.VAL.VIDEO_MAP``.  Linked on the device by ``tuber_tube_link_ranked``;
        beyond its bounds (K > 64 rows per key frame or K * (max_gap + 1) > ``tuber_tube_link_max_active()`` = 64) or on a CPU store
        ``evaluation.link_rows`` answers, one line says so, and ``tubes_path`` is "host" instead of "device".  ``VideoDetector``'s default
        ``topk`` is 21 = 64 // (MAX_GAP + 1) with the shipped MAX_GAP of 2, so that the default path is the device's.  ``nms`` (default:
        ``CONFIG.VAL.TUBE_NMS.IOU``; None: off): per class a tube whose spatio-temporal IoU with a higher-scored kept tube exceeds it is
        dropped -- one more launch, ``tuber_tube_nms``, whose bytes travel in the same copy; on the host path
        ``evaluation.tube_nms``.  ``dense`` (default: ``CONFIG.VAL.VIDEO_MAP.DENSE``, False): a box on EVERY frame from the tube's first key
        to its last -- ``frames`` becomes that range and ``boxes`` [F, 4]: a key frame carries its detection's bytes,
        a frame between two linked keys the fp64 interpolation of the two boxes (``evaluation.dense_rows``: the definition), a key the linker
        bridged over is filled like any other gap; the key frames and their boxes move to ``keys`` / ``key_boxes``, ``frame_scores`` [F] fp32
        is the score interpolated alike and ``key_index`` [F] the index into ``keys`` of the key that owns the frame.  One more launch,
        ``tuber_tube_dense``, behind the link (and the NMS, which decides on the key rows as before), its four outputs in the same copy;
        on the host path, beyond 32 bits or at the kernel's escape ``evaluation.dense_rows``.  The keys must ascend strictly."""
        from .evaluation import dense_from_rows, link_rows, tubes_from_link
        nms = _nms_value("VideoDetections.tubes", self.nms_iou if nms is None else nms)
        link_iou = float(self.settings["link_iou"] if link_iou is None else link_iou)
        max_gap = int(self.settings["max_gap"] if max_gap is None else max_gap)
        min_len = int(self.settings["min_len"] if min_len is None else min_len)
        S, K = self.scores.shape
        G = self._extent(dense, max_gap)
        slot = np.repeat(np.arange(S, dtype=np.int64), K)
        host, why = self._link_device(link_iou, max_gap, nms, min_len, G)
        if host is None:
            print("[tuber] VideoDetections.tubes: %s; linking on the host" % why, file=sys.stderr, flush=True)
            host = self._fetch()[0]
            host.update(link_rows(host["boxes"].reshape(-1, 4), host["labels"].reshape(-1), host["scores"].reshape(-1), slot, [0, S], self.class_num,
                                  link_iou, max_gap))
        rows, dense_why = self._dense(host, host["scores"], max_gap, G, why is not None)
        if dense_why:
            print("[tuber] VideoDetections.tubes: %s; per-frame boxes on the host" % dense_why, file=sys.stderr, flush=True)
        self.tubes_path = "host" if why or dense_why else "device"
        layout = dict(videos=["video"], video_off=np.asarray([0, S]), first_frame=np.asarray([0]))
        link = dict(layout=layout, row_head=host["row_head"], row_slot=slot, row_cls=host["labels"].reshape(-1), tube_score=host["tube_score"],
                    det_box=host["boxes"].reshape(-1, 4))
        keep = self._keep(host, link, nms, min_len)
        out = []
        for t in tubes_from_link(link):
            if len(t["frames"]) >= min_len and (keep is None or keep[t["head"]] != 0):
                d = dict(cls=t["cls"], score=t["score"], frames=[self.keys[s] for s in t["frames"]], boxes=t["boxes"], length=len(t["frames"]))
                out.append(d if rows is None else _densified(d, dense_from_rows(t["rows"], self.keys, K, rows)))
        return out

    # -- crops ------------------------------------------------------------------------------------------------------------
    def crops(self, tubes, size=None, scale=None, samples=None, normalize=False):
        """The pixels of ``tubes`` -- the dicts of ``tubes()`` or of ``actors.tracks()``, dense or not -- cut out of the resident video and
        resampled to ``size``: ``crops.tube_crops(self.video, tubes, ..., source_size=self.source_size)``, a
        ``crops.TubeCrops`` whose ``[i]`` is tube i's rows, uint8 [F, h, w, 3] on the device (``normalize=True``: fp32 [F, 3, h, w] through the
        clips' mean/std table).  One upload of the crop table, one ``tuber_tube_crops`` launch, no synchronisation.  The boxes are in
        source-video pixels and the video is held at working resolution: ``source_size`` carries the ratio.  Defaults: ``CONFIG.VAL.CROPS``
        (SIZE 112 x 112, SCALE 1.0, SAMPLES 1).  Needs ``VideoDetector(..., keep_video=True)``."""
        from .crops import tube_crops
        if self.video is None:
            raise RuntimeError("VideoDetections.crops: the video was not kept: construct VideoDetector(..., keep_video=True)")
        st = self.crop_settings or dict(size=(112, 112), scale=1.0, samples=1)
        return tube_crops(self.video, tubes, st["size"] if size is None else size, source_size=self.source_size,
                          scale=st["scale"] if scale is None else scale, samples=st["samples"] if samples is None else samples, normalize=normalize)


class VideoActors(_VideoRecord):
    """The actors of a video's key frames (``VideoDetector(..., actors=A)``): ``keys`` (frame numbers) and, as tensors on one
    device, ``boxes`` [n, A, 4] fp32 xyxy in source-video pixels, ``actor`` [n, A] fp32 (the actor probability), ``queries`` [n, A] int32 (-1 in
    the rows behind ``count``), ``actions`` [n, A, C] fp32 (every class's score), ``count`` / ``total`` [n] int32 -- the fields of
    ``detect.Actors``, a row per key frame."""
    FIELDS, ROW_FIELDS = ACTOR_FIELDS, ACTOR_FIELDS[:4]

    def __init__(self, keys, boxes, actor, queries, actions, count, total, settings=None, store=None, nms_iou=None, dense=False):
        # the defaults of tracks(): CONFIG.VAL.ACTORS, CONFIG.VAL.TUBE_NMS.ACTORS_IOU
        super().__init__(keys, (boxes, actor, queries, actions, count, total),
                         settings or dict(link_iou=0.2, max_gap=2, min_len=1, window=1, label_thr=0.05), store, nms_iou, dense)
        self.class_num = int(actions.shape[2])
        self.tracks_path = None                                                        # "device" or "host" after tracks()
        # the track records of a VideoStream(actors=A) push: row_head / row_score / row_len [n, A], row_mean / row_peak [n, A, C], smooth [m, A, C]
        self.row_mean = self.row_peak = self.smooth = None
        self.smooth_first = None                                                       # the key ordinal of smooth's first slot (a host int)

    # -- tracks -----------------------------------------------------------------------------------------------------------
    NAMES = ("row_head", "tube_score", "tube_len", "tube_last", "row_smooth", "track_mean", "track_peak")

    def _tracks_device(self, link_iou, max_gap, window, nms=None, min_len=1, G=None):
        """``tuber_tube_link_ranked`` with one class and ``tuber_track_actions`` (and, with ``nms``, ``tuber_tube_nms``, with ``G``,
        ``tuber_tube_dense``) over the padded store as it is, everything read back in one copy; or None where the kernels' bounds refuse it"""
        S, A, C = self.actions.shape
        if self.boxes.device.type != "cuda":
            return None, "the store is on the CPU"
        (rows, active), max_a, max_c = link_limits(), lib.query("tuber_track_actions_limits", 0), lib.query("tuber_track_actions_limits", 1)
        if A > min(rows, max_a) or A * (max_gap + 1) > active or C > max_c:
            return None, "%d actors per key frame with max_gap %d and %d classes: beyond %d rows, %d active tracks or %d classes" % (
                A, max_gap, C, min(rows, max_a), active, max_c)
        label = torch.where(self.queries >= 0, 0, -1).to(torch.int32)                   # one class; a row behind its key's count is not counted
        link, slot_off, video_off = link_ranked(self.boxes, label, self.actor, 1, link_iou, max_gap)
        f64 = torch.float64
        link.update(row_smooth=torch.empty(S * A, C, dtype=f64, device=label.device), track_mean=torch.empty(S * A, C, dtype=f64, device=label.device),
                    track_peak=torch.empty(S * A, C, dtype=torch.float32, device=label.device))
        lib.call("tuber_track_actions", self.actions.contiguous(), link["row_head"], link["tube_last"], S, A, C, int(window), link["row_smooth"],
                 link["track_mean"], link["track_peak"])
        return self._linked(link, slot_off, video_off, self.NAMES, 1, nms, min_len, (self.actor, max_gap, G)), None

    def tracks(self, link_iou=None, max_gap=None, min_len=None, window=None, label_thr=None, nms=None, dense=None):
        """The actor tracks of the video -- who is there, from when to when, doing what: a list, in head order (the order of the tracks' first
        rows), of ``dict(score, frames, boxes, actor, queries, actions, smooth, mean, peak, labels, length)``: ``score`` the fp64 mean actor
        probability, ``frames`` the key frame numbers, ``boxes`` [L, 4] in source pixels, ``actor`` / ``queries`` [L], ``actions`` [L, C] fp32 the
        action scores per key, ``smooth`` [L, C] fp64 those scores averaged over the track's keys at most ``window`` key frames away, ``mean``
        [C] fp64 / ``peak`` [C] fp32 over the track, ``labels`` the 0-based classes with ``mean >= label_thr`` by mean descending, then class;
        tracks shorter than ``min_len`` are dropped.  ``evaluation.actor_tracks`` is the definition.  Defaults: ``CONFIG.VAL.ACTORS``.  On the
        device: ``tuber_tube_link_ranked`` with one class, ``tuber_track_actions``, one copy back.  Beyond their bounds (A > 64,
        A * (max_gap + 1) > 64, C > 4096) or on a CPU store the definition answers on the host, one line says so, and ``tracks_path`` is "host"
        instead of "device".  ``nms`` (default: ``CONFIG.VAL.TUBE_NMS.ACTORS_IOU``; None: off): a track whose spatio-temporal IoU with a
        kept track of higher mean actor probability exceeds it is dropped, class-agnostically: ``tuber_tube_nms`` on
        the device, ``evaluation.tube_nms`` on the host path.  The aggregates of the kept tracks are unchanged.  ``dense`` (default:
        ``CONFIG.VAL.VIDEO_MAP.DENSE``): as in ``VideoDetections.tubes`` -- ``frames`` / ``boxes`` per frame, ``keys`` / ``key_boxes`` /
        ``frame_scores`` (the interpolated actor probability) / ``key_index`` added; the per-key fields (``actor``, ``actions``, ``smooth``,
        ...) stay per key and are addressed per frame through ``key_index``."""
        from .evaluation import actor_tracks, dense_from_rows
        nms = _nms_value("VideoActors.tracks", self.nms_iou if nms is None else nms)
        st = self.settings
        link_iou = float(st["link_iou"] if link_iou is None else link_iou)
        max_gap = int(st["max_gap"] if max_gap is None else max_gap)
        min_len = int(st["min_len"] if min_len is None else min_len)
        window = int(st["window"] if window is None else window)
        label_thr = float(st["label_thr"] if label_thr is None else label_thr)
        if max_gap < 0 or window < 0:
            raise ValueError("VideoActors.tracks: max_gap = %d and window = %d must be >= 0" % (max_gap, window))
        S, A, C = self.actions.shape
        G = self._extent(dense, max_gap)
        host, why = self._tracks_device(link_iou, max_gap, window, nms, min_len, G)
        if host is None:
            print("[tuber] VideoActors.tracks: %s; tracks on the host" % why, file=sys.stderr, flush=True)
            host = self._fetch()[0]
            host.update(actor_tracks(host["boxes"], host["actor"], host["queries"], host["actions"], S, A, link_iou, max_gap, window))
        dense_rec, dense_why = self._dense(host, host["actor"], max_gap, G, why is not None)
        if dense_why:
            print("[tuber] VideoActors.tracks: %s; per-frame boxes on the host" % dense_why, file=sys.stderr, flush=True)
        self.tracks_path = "host" if why or dense_why else "device"
        head = np.asarray(host["row_head"]).reshape(-1)
        box, actor, query, act = host["boxes"].reshape(-1, 4), host["actor"].reshape(-1), host["queries"].reshape(-1), host["actions"].reshape(-1, C)
        members = {}
        for r in np.nonzero(head >= 0)[0].tolist():
            members.setdefault(int(head[r]), []).append(r)
        keep = self._keep(host, dict(layout=dict(video_off=np.asarray([0, S])), row_head=head, row_slot=np.repeat(np.arange(S, dtype=np.int64), A),
                                     row_cls=np.where(query >= 0, 0, -1), tube_score=host["tube_score"], det_box=box), nms, min_len)
        out = []
        for h in sorted(members):
            rows = members[h]
            if len(rows) < min_len or (keep is not None and keep[h] == 0):
                continue
            mean = np.array(host["track_mean"][h], dtype=np.float64)
            d = dict(score=float(host["tube_score"][h]), frames=[self.keys[r // A] for r in rows], boxes=box[rows].copy(), actor=actor[rows].copy(),
                     queries=query[rows].copy(), actions=act[rows].copy(), smooth=np.array(host["row_smooth"][rows], dtype=np.float64), mean=mean,
                     peak=np.array(host["track_peak"][h], dtype=np.float32), labels=_track_labels(mean, label_thr), length=len(rows))
            out.append(d if dense_rec is None else _densified(d, dense_from_rows(rows, self.keys, A, dense_rec)))
        return out


class _VideoRunner:
    """What ``VideoDetector`` and ``VideoStream`` share: the settings, the checks of a call, the buffers of a video size, the resize launch and the
    ``Detector`` run over the clip buffer.  Where the frames come from (the resident video and its index table, or the ring and its rule) and
    what becomes of the rows is the subclass's."""

    def __init__(self, cfg, model, batch, score_thr, topk, actor_thr, graphed, rule, actors):
        from .config import actor_settings, dense_setting, detect_settings, video_map_settings
        self.cfg, self.model, self.batch = cfg, model, int(batch)
        vm = video_map_settings(cfg)
        self.dense = dense_setting(cfg)    # the default of tubes(dense=) / tracks(dense=): kept out of ``settings``
        self.settings = dict(link_iou=float(vm["link_iou"]), max_gap=int(vm["max_gap"]), min_len=int(vm["min_len"]))
        if topk is None:
            topk = max(1, min(detect_settings(cfg)["topk"], lib.query("tuber_tube_link_max_active") // (self.settings["max_gap"] + 1)))
        self.detector = Detector(cfg, model, score_thr=score_thr, topk=topk, actor_thr=actor_thr, graphed=graphed, actors=actors)
        self.actor_settings = None
        if actors is not None:
            st = actor_settings(cfg)
            self.actor_settings = {k: st[k] for k in ("link_iou", "max_gap", "min_len", "window", "label_thr")}
        self.mode = model.dataset_mode
        self.rule = rule if rule is not None else ("ava" if self.mode == "ava" else "jhmdb")
        if self.rule not in RULES:
            raise ValueError("%s: rule %r is not one of %s" % (type(self).__name__, rule, ", ".join(RULES)))
        D = cfg.CONFIG.DATA
        self.T, self.rate, self.size, self.class_num = int(D.TEMP_LEN), int(D.FRAME_RATE), int(D.IMG_SIZE), int(D.NUM_CLASSES)
        self._bufs = {}                    # (device, H0, W0) -> the buffers of a video size

    def _stride(self, stride):
        """one second's worth for AVA (30 frames: the reference's ``timef * 30``, datasets/ava_frame.py:43) and 1 for JHMDB / UCF101-24"""
        stride = int(stride) if stride is not None else (30 if self.mode == "ava" else 1)
        if stride < 1:
            raise ValueError("%s: stride = %r must be >= 1" % (type(self).__name__, stride))
        return stride

    def _check_eval(self):
        if self.model.training:
            raise RuntimeError("%s runs an eval forward: call model.eval() first" % type(self).__name__)

    def _frames(self, frames, n, least):
        """the frames of a call as a uint8 tensor [n, H, W, 3] of at least ``least`` frames (``n``: the letter the message calls their number)"""
        self._check_eval()
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < least:
            raise ValueError("%s wants uint8 frames [%s, H, W, 3], got %s %s" % (type(self).__name__, n, frames.dtype, tuple(frames.shape)))
        return frames

    def _buffers(self, dev, H0, W0):
        """the buffers of a video size: one clip buffer, one zero mask (every frame of a video has one size), the per-batch constants and the
        resize coefficients"""
        key = (str(dev), H0, W0)
        b = self._bufs.get(key)
        if b is None:
            nh, nw, y1, x1, h, w = working_geometry(H0, W0, self.size)
            B, T = self.batch, self.T
            b = self._bufs[key] = dict(H0=H0, W0=W0, nh=nh, nw=nw, window=(y1, x1, h, w), same=(nh, nw) == (H0, W0),
                                       clips=torch.empty(B, 3, T, h, w, dtype=torch.float32, device=dev),
                                       mask=torch.zeros(B, h, w, dtype=torch.bool, device=dev),
                                       key_pos=torch.full((B,), T // 2, dtype=torch.int64, device=dev),
                                       sizes=torch.tensor([[H0, W0]] * B, dtype=torch.float32).to(dev, non_blocking=True),
                                       lut=ip._device_tables(dev, (ip.MEAN, ip.STD))[0])
            if not b["same"]:
                b["coeffs"] = ip._device_coeffs(dev, H0, W0, nh, nw)
        return b

    @staticmethod
    def _scratch(b, chunk, dev):
        """the scratch ``tuber_frames_resize`` wants for up to ``chunk`` frames: only a resize in both directions runs in two passes"""
        two_pass = not b["same"] and b["nw"] != b["W0"] and b["nh"] != b["H0"]
        return torch.empty(chunk * b["coeffs"][4] * b["nw"] * 3, dtype=torch.uint8, device=dev) if two_pass else None

    def _resize(self, b, src, dst, tmp):
        """the frames ``src`` [m, H0, W0, 3] at working resolution into ``dst[:m]``: ``tuber_frames_resize``, or a copy where the sizes agree"""
        if b["same"]:
            dst[:src.shape[0]].copy_(src)
        else:
            (bh, kh, bv, kv), ksh, ksv, y0, rows = b["coeffs"]
            lib.call("tuber_frames_resize", src, tmp, dst, src.shape[0], b["H0"], b["W0"], b["nh"], b["nw"], bh, kh, ksh, bv, kv, ksv, y0, rows)

    def _stores(self, rows, dev):
        """the uninitialised stores of ``rows`` key frames: the seven detection fields and, with ``actors``, the six actor fields (else None)"""
        A = self.detector.actors
        return (field_tensors(FIELDS, rows, self.detector.topk, dev, filled=False),
                None if A is None else field_tensors(ACTOR_FIELDS, rows, A, dev, self.class_num, filled=False))

    def _detect(self, b, stores, row):
        """the ``Detector`` over the clip buffer, its fields copied device-to-device into the rows ``row .. row + batch - 1`` of the stores"""
        det = self.detector(NestedTensor(b["clips"], b["mask"]), b["sizes"], b["key_pos"])
        for full, rec in zip(stores, (det, det.actors)):
            if full is not None:
                for dst, src in zip(full, rec.tensors()):
                    dst[row:row + self.batch].copy_(src)


class VideoDetector(_VideoRunner):
    """``VideoDetector(cfg, model)(frames)`` -> ``VideoDetections``: every key frame of a video through the captured ``detect.Detector``.

    ``frames``: uint8 [N, H0, W0, 3] (numpy, a host tensor or a device tensor).  They are uploaded ``chunk`` frames at a time and each frame is
    resized ONCE (``tuber_frames_resize``) to the reference's val size (``working_geometry``); the raw frames never need to be resident.
    ``keys``: frame numbers, by default ``range(0, N, stride)``; ``stride`` defaults to one second's worth for AVA (30 frames: the reference's
    ``timef * 30``, datasets/ava_frame.py:43) and 1 for JHMDB / UCF101-24.  Per batch of ``batch`` keys: one ``tuber_video_clips`` launch over a
    slice of the one index table (``clip_indices``, uploaded up front), the one ``Detector`` with ``key_pos = T // 2`` and ``sizes = (H0, W0)``,
    and the seven fields copied device-to-device into the video's store.  The last batch is padded by repeating its last key -- one graph
    shape -- and its surplus rows are dropped.  Once the first call has captured its graph, a call synchronises nowhere.

    ``rule``: ``clip_indices``' rule, by default the model's ``dataset_mode`` ("ava", otherwise "jhmdb").  ``topk``: by default
    ``min(CONFIG.VAL.DETECT.TOPK, tuber_tube_link_max_active() // (CONFIG.VAL.VIDEO_MAP.MAX_GAP + 1))`` -- 21 with the shipped settings (TOPK 100,
    64 active tubes, MAX_GAP 2) -- so that ``tubes()`` with its defaults links on the device.  ``score_thr`` / ``actor_thr`` / ``graphed``: as
    ``Detector``.  ``actors=A`` (AVA models; default None: off): the ``Detector``'s actor decode as well, its six tensors copied device-to-device
    into the video's store beside the seven; the result carries ``.actors``, a ``VideoActors``, whose ``tracks()`` answers "who is there, from
    when to when, doing what" (DESIGN.md section 6i).  ``keep_video=True`` (default False: off, nothing about a call changes): the result
    carries ``video``, the resident uint8 [N, nh, nw, 3] tensor the call builds anyway, and ``source_size = (H0, W0)``, and its
    ``crops(tubes)`` cuts tubes and actor tracks out of it on the device.  The cost: the resident video -- 134 MB for
    512 frames of 256 x 340 -- stays allocated for as long as the result is alive instead of being freed when the call returns."""

    def __init__(self, cfg, model, batch=2, score_thr=None, topk=None, actor_thr=None, graphed=True, rule=None, actors=None, keep_video=False):
        from .config import crop_settings, tube_nms_settings
        self.nms = tube_nms_settings(cfg)                  # the defaults of tubes(nms=) / tracks(nms=): kept out of ``settings``
        self.keep_video = bool(keep_video)
        self.crop_settings = crop_settings(cfg)            # the defaults of VideoDetections.crops()
        if int(batch) < 1:
            raise ValueError("VideoDetector: batch = %r must be >= 1" % (batch,))
        super().__init__(cfg, model, batch, score_thr, topk, actor_thr, graphed, rule, actors)

    @torch.no_grad()
    def __call__(self, frames, keys=None, stride=None, chunk=256):
        frames = self._frames(frames, "N", 1)
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError("VideoDetector: chunk = %r must be >= 1" % (chunk,))
        store, _ = self.model.engine()
        dev = store.device
        N, H0, W0 = (int(v) for v in frames.shape[:3])
        keys = [int(k) for k in (range(0, N, self._stride(stride)) if keys is None else keys)]
        if not keys:
            raise ValueError("VideoDetector: no key frames")
        n, B, T = len(keys), self.batch, self.T
        nb = (n + B - 1) // B
        table = clip_indices(N, keys + [keys[-1]] * (nb * B - n), T, self.rate, self.rule)      # the padded last batch repeats its last key
        table = torch.from_numpy(table).to(dev, non_blocking=True)
        b = self._buffers(dev, H0, W0)
        tmp = self._scratch(b, chunk, dev)
        # the video at working resolution on the device, uploaded and resized ``chunk`` frames at a time
        resident = torch.empty(N, b["nh"], b["nw"], 3, dtype=torch.uint8, device=dev)
        for i in range(0, N, chunk):
            self._resize(b, frames[i:i + chunk].to(dev, non_blocking=True).contiguous(), resident[i:], tmp)
        stores = self._stores(nb * B, dev)
        for i in range(nb):
            lib.call("tuber_video_clips", resident, N, b["nh"], b["nw"], table[i * B:], B, T, *b["window"], b["lut"], b["clips"])
            self._detect(b, stores, i * B)
        vd = VideoDetections(keys, *[t[:n] for t in stores[0]], class_num=self.class_num, settings=self.settings, store=store, nms_iou=self.nms["iou"],
                             dense=self.dense)
        if stores[1] is not None:
            vd.actors = VideoActors(keys, *[t[:n] for t in stores[1]], settings=self.actor_settings, store=store, nms_iou=self.nms["actors_iou"],
                                    dense=self.dense)
        if self.keep_video:
            vd.video, vd.source_size, vd.crop_settings = resident, (H0, W0), self.crop_settings
        return vd


# ---------------------------------------------------------------------------------------------------------------------------------------
# a video that arrives in pieces
# ---------------------------------------------------------------------------------------------------------------------------------------
def clip_span(T, rate=1, rule="ava"):
    """the largest number of consecutive frame numbers between the first and the last frame one key's clip may read, both included: the rule's
    look-back + look-ahead + 1.  ava / edge: T frames ``rate`` apart, ``(T - 1) * rate + 1``; jhmdb: ``key - T//2 .. key + T - T//2``, the
    last one being the pad behind a clip whose start was clamped: ``T + 1``.  Frame 0 as jhmdb's front pad does not count: the ring keeps it in
    a slot of its own."""
    if rule not in RULES:
        raise ValueError("clip_span: rule %r is not one of %s" % (rule, ", ".join(RULES)))
    T, rate = int(T), int(rate)
    return T + 1 if rule == "jhmdb" else (T - 1) * rate + 1


@functools.lru_cache(maxsize=4096)
def frames_needed(key, T, rate=1, rule="ava"):
    """the smallest frame count n > key from which on ``clip_indices(n, [key], ...)`` no longer changes: a stream of n frames can run this key
    frame.  ava / edge: the clip's last frame has arrived.  jhmdb: ``key + T - T//2`` frames always do (``end`` is no longer clamped); one
    fewer do as well when the clip is not clamped at the front, the missing frame being the pad that repeats ``end``."""
    key, T, rate = int(key), int(T), int(rate)
    if rule == "ava":
        return max(key - T // 2 * rate, 0) + (T - 1) * rate + 1
    if rule == "edge":
        return key + max(T - 1 - T // 2, 0) * rate + 1
    n = key + T - T // 2 + 1
    final = clip_indices(n, [key], T, rate, rule)
    while n - 1 > key and np.array_equal(clip_indices(n - 1, [key], T, rate, rule), final):
        n -= 1
    return n


def ring_frames(T, rate, rule, batch, stride, max_chunk):
    """R, the frames the ring of a ``VideoStream`` holds: ``clip_span`` (the rule's look-back + look-ahead) + ``(batch - 1) * stride`` +
    ``max_chunk``.  Why that is enough: key frames run in full batches, so the oldest frame still needed is the first frame of the clip of the
    first key of the batch that waits, and the batch waits only while its LAST key, ``(batch - 1) * stride`` frames on, lacks a frame of its
    clip; the frames pushed so far therefore end inside that clip, at most ``clip_span - 1 + (batch - 1) * stride`` frames after the oldest
    one needed.  A piece adds at most ``max_chunk`` frames before the batches that became ready are run."""
    return clip_span(T, rate, rule) + (int(batch) - 1) * int(stride) + int(max_chunk)


class StreamSchedule:
    """The host integers of a ``VideoStream``: which ring slots the next frames go to and which batches of key frames run after them.
    ``push(m)`` -> ``[(offset, length, [first key ordinal of a batch, ...]), ...]``: the pieces of at most ``max_chunk`` frames a push of m
    frames is cut into and the full batches that are ready after each; ``finish()`` -> ``(n_total, [(first key ordinal, keys), ...])``: the
    batches that remain once the frame count is known, the last one possibly short, and the schedule is reset for the next video."""

    def __init__(self, T, rate, rule, batch, stride, max_chunk):
        self.T, self.rate, self.rule, self.batch, self.stride, self.max_chunk = int(T), int(rate), rule, int(batch), int(stride), int(max_chunk)
        self.R = ring_frames(self.T, self.rate, rule, self.batch, self.stride, self.max_chunk)
        self.frames = self.decided = self._scan = 0      # frames pushed; key frames run (the next key ordinal); key frames known to be ready

    def ready(self, n):
        """key frames of a stream of n frames whose clips can no longer change: a prefix of the keys, ``frames_needed`` growing with the key"""
        k = self._scan
        while k * self.stride < n and frames_needed(k * self.stride, self.T, self.rate, self.rule) <= n:
            k += 1
        self._scan = k
        return k

    def push(self, m):
        plan = []
        for i in range(0, int(m), self.max_chunk):
            length = min(self.max_chunk, int(m) - i)
            self.frames += length
            batches = []
            while self.ready(self.frames) - self.decided >= self.batch:
                batches.append(self.decided)
                self.decided += self.batch
            plan.append((i, length, batches))
        return plan

    def finish(self):
        n_total = self.frames
        keys = (n_total - 1) // self.stride + 1 if n_total else 0          # len(range(0, n_total, stride))
        batches = [(k, min(self.batch, keys - k)) for k in range(self.decided, keys, self.batch)]
        self.frames = self.decided = self._scan = 0
        return n_total, batches


class VideoStream(_VideoRunner):
    """``VideoDetector`` for a video that arrives in pieces: ``push(frames)`` as they come, ``finish()`` at the end, ``tubes()`` whenever wanted.
    The rows of every ``push`` and of ``finish``, concatenated, are ``VideoDetector(cfg, model, batch, ...)(video, stride=stride)``'s, bit for
    bit, and so are the tubes.

    ``push(frames)``: uint8 [n, H0, W0, 3] (numpy, a host tensor or a device tensor), H0 x W0 fixed by the first push of a video.  The frames
    are resized (``tuber_frames_resize``) into the slots ``f % R`` of a ring of R = ``ring_frames(...)`` frames at working resolution, at most
    ``max_chunk`` at a time; frame 0 is kept in a slot of its own as well.  After each piece every key frame (``range(0, inf, stride)``) whose
    clip can no longer change (``frames_needed``) is decided, and the decided keys run in the batches ``VideoDetector`` forms -- keys
    ``i * batch .. i * batch + batch - 1``, full batches only, a remainder waits -- each one ``tuber_video_clips_ring`` launch and the captured
    ``Detector``.  Returns the ``VideoDetections`` of the keys this push decided, or None.  With ``link=True`` it also carries, as device
    tensors, ``row_head`` [n, K] int32 (the tube's first detection as key ordinal * K + position, -1: not counted), ``row_score`` [n, K] fp64
    and ``row_len`` [n, K] int32 (the tube's mean score and length after taking the row): one ``tuber_tube_link_stream`` launch per push, or
    ``evaluation.TubeLinker`` on the host beyond the linker's bounds (one line says so).  Readiness and ring arithmetic are host integers:
    once the first push has captured its graph, ``push`` synchronises nowhere.

    ``finish()``: the end of the video.  The remaining keys run with the frame count known (the end clamps, jhmdb's end pad), the last batch
    padded by repeating its last key; returns their ``VideoDetections`` or None, then resets the frame counter, the key ordinal and the link
    state (a memset) for the next video, which allocates and captures nothing new when it has the same size.

    ``tubes()``: the tubes that CLOSED since the last call -- no key frame still to come can extend them: the next key ordinal is more than
    ``max_gap`` + 1 past their last one -- and after ``finish()`` all that remain; ``dict(cls, score, frames, boxes, length, head)`` in head
    order, as ``VideoDetections.tubes`` (``head``: key ordinal * K + position of the first detection).  It runs on the host and makes one
    device-to-host copy per call; the rows of open tubes are kept on the host in between.

    Device memory does not grow with the video: the ring, (R + 1) * nh * nw * 3 bytes; the link state, ``tuber_tube_link_state_bytes(C)`` =
    2560 * C bytes; one batch of clips; and the ``VideoDetections`` of the pushes since the last ``tubes()`` call (``link=False``: none are
    kept).  ``rule`` / ``topk`` / ``score_thr`` / ``actor_thr`` / ``graphed`` / ``stride``: as ``VideoDetector``.

    ``actors=A`` (AVA models, ``link=True``; default None: off): ``VideoDetector(..., actors=A)`` for the stream.  The
    ``VideoDetections`` of a push carries ``.actors``, the ``VideoActors`` of the decided keys -- ``VideoDetector``'s rows bit for bit -- and on
    it, as device tensors, ``row_head`` / ``row_score`` / ``row_len`` [n, A] (the actors' own ``tuber_tube_link_stream`` call with one class),
    ``row_mean`` [n, A, C] fp64 / ``row_peak`` [n, A, C] fp32 (what the row's track has been doing SO FAR: its running mean and maximum) and
    ``smooth`` [m, A, C] fp64 with ``smooth_first``, the key ordinal of its first slot: ``actor_tracks``' ``row_smooth``, which looks
    ``window`` keys ahead and therefore comes ``window`` keys late (``evaluation.smooth_range``; ``finish()`` flushes, and returns a
    ``VideoDetections`` without keys when only smoothed rows were left) -- one ``tuber_track_actions_stream`` call per push.  ``tracks()``
    returns the actor tracks that closed since the last call.  The stream then also holds the actors' link state (2560 bytes) and the track
    ring (``tuber_track_stream_state_bytes``); beyond the kernel's bounds ``evaluation.ActorTracker`` answers on the host, one line says so,
    and ``tracks_path`` is "host" instead of "device".

    Tube NMS (``CONFIG.VAL.TUBE_NMS``) is not part of the stream: when a tube closes, a tube that would suppress it may
    still be open with its final score unknown, so no streaming rule equals the whole-video one.  A config that sets it is ignored here, with
    one line on stderr at construction; ``tubes()`` / ``tracks()`` return every closed tube.

    Dense tubes (``tubes(dense=True)`` / ``tracks(dense=True)``, default ``CONFIG.VAL.VIDEO_MAP.DENSE``) ARE part of the
    stream: a closed tube never changes, so a box on every frame of its extent is filled in on the host where the tube is assembled
    (``evaluation.dense_tube``) and equals ``VideoDetector``'s, bit for bit.

    Crops (``VideoDetector(..., keep_video=True)``) are not part of the stream and it takes no ``keep_video``: the ring
    holds only the recent frames, so the pixels of a tube are gone by the time it closes.  ``crops.tube_crops`` over frames the caller kept
    does the same work."""

    def __init__(self, cfg, model, batch=2, stride=None, rule=None, max_chunk=64, score_thr=None, topk=None, actor_thr=None, graphed=True,
                 link=True, actors=None):
        from .config import tube_nms_settings
        from .evaluation import ActorTracker, TubeLinker
        if any(v is not None for v in tube_nms_settings(cfg).values()):
            print("[tuber] VideoStream: CONFIG.VAL.TUBE_NMS is ignored: a closed tube's suppressor may still be open, so tube NMS is defined over "
                  "whole videos only (VideoDetector)", file=sys.stderr, flush=True)
        self.max_chunk, self.link = int(max_chunk), bool(link)
        if int(batch) < 1 or self.max_chunk < 1:
            raise ValueError("VideoStream: batch = %r and max_chunk = %r must be >= 1" % (batch, max_chunk))
        if actors is not None and not self.link:
            raise ValueError("VideoStream: actors = %r needs link=True: the actor tracks are link records" % (actors,))
        super().__init__(cfg, model, batch, score_thr, topk, actor_thr, graphed, rule, actors)
        self.stride = self._stride(stride)
        self.schedule = StreamSchedule(self.T, self.rate, self.rule, self.batch, self.stride, self.max_chunk)
        self.R = self.schedule.R
        K, gap = self.detector.topk, self.settings["max_gap"]
        self._why_host = link_beyond("%d rows per key frame with max_gap %d" % (K, gap), K, gap)
        self._host_linker = _HostDefinition(lambda: TubeLinker(self.class_num, self.settings["link_iou"], gap))
        self._cur = None                   # the current video's buffers
        self.wrapped = False               # whether a ring slot has been overwritten in the current video
        self._pending = []                 # link records since the last tubes() call; None marks the end of a video
        self._tubes = TubeAssembler(gap, self.settings["min_len"])                      # the rows of open tubes, on the host
        # actor tracks (actors=A): their own pending list and their own open rows; tubes() and tracks() consume neither the other's
        self.tracks_path = None            # "device" or "host" once a push has decided keys
        self._why_host_tracks, self._host_tracker = None, None
        self._pending_tracks, self._assembler = [], None
        self._video_keys = 0               # keys decided in the current video
        if actors is not None:
            A, st = self.detector.actors, self.actor_settings
            self._host_tracker = _HostDefinition(lambda: ActorTracker(st["link_iou"], st["max_gap"], st["window"]))
            self._assembler = TrackAssembler(A, st["max_gap"], st["window"], st["min_len"], st["label_thr"])
            self._track_bytes = lib.query("tuber_track_stream_state_bytes", A, self.class_num, st["max_gap"], st["window"])
            if A > lib.query("tuber_frame_match_max_dets") or not self._track_bytes:
                self._why_host_tracks = "%d actors per key frame with max_gap %d, window %d and %d classes: beyond %d rows, %d active tracks, window %d or %d classes" % (
                    A, st["max_gap"], st["window"], self.class_num, min(lib.query("tuber_frame_match_max_dets"), lib.query("tuber_track_stream_limits", 0)),
                    lib.query("tuber_tube_link_max_active"), lib.query("tuber_track_stream_limits", 2), lib.query("tuber_track_stream_limits", 1))

    # -- buffers ----------------------------------------------------------------------------------------------------------
    def _buffers(self, dev, H0, W0):
        """the shared buffers of a video size plus the stream's own: the ring, the resize scratch, the link state and, with actors, theirs"""
        b = super()._buffers(dev, H0, W0)
        if "ring" not in b:
            b["tmp"] = self._scratch(b, self.max_chunk, dev)
            b["ring"] = torch.empty(self.R + 1, b["nh"], b["nw"], 3, dtype=torch.uint8, device=dev)
            b["state"] = torch.zeros(lib.query("tuber_tube_link_state_bytes", self.class_num), dtype=torch.uint8, device=dev)
            if self.detector.actors is not None and self._why_host_tracks is None:      # the actors' own link state (one class) and the track ring
                b["actor_state"] = torch.zeros(lib.query("tuber_tube_link_state_bytes", 1), dtype=torch.uint8, device=dev)
                b["track_state"] = torch.zeros(self._track_bytes, dtype=torch.uint8, device=dev)
        return b

    def device_bytes(self):
        """bytes of the current video size's ring and link state -- with ``actors``, of the actors' link state and the track ring as well: what the
        stream holds instead of the resident video"""
        b = self._cur
        return 0 if b is None else b["ring"].numel() + b["state"].numel() + sum(b[k].numel() for k in ("actor_state", "track_state") if k in b)

    def _store_frames(self, b, src, first):
        """frames ``first .. first + len(src) - 1`` into their ring slots: a run that crosses the ring's end is two calls"""
        R, m = self.R, int(src.shape[0])
        s0 = first % R
        for lo, hi, slot in ((0, min(m, R - s0), s0), (min(m, R - s0), m, 0)):
            if hi > lo:
                self._resize(b, src[lo:hi], b["ring"][slot:], b["tmp"])
        if first == 0:
            b["ring"][R].copy_(b["ring"][0])                   # frame 0 in its fixed slot as well
        self.wrapped = self.wrapped or first + m > R

    # -- key frames -------------------------------------------------------------------------------------------------------
    def _run(self, b, stores, row, first_ord, n_keys, n_total):
        """one batch: the keys ``first_ord .. first_ord + n_keys - 1`` (the last one repeated up to ``batch``) into rows ``row ..`` of the stores"""
        lib.call("tuber_video_clips_ring", b["ring"], self.R, b["nh"], b["nw"], first_ord * self.stride, self.stride, n_keys, self.batch, self.T,
                 self.rate, RULES.index(self.rule), n_total, *b["window"], b["lut"], b["clips"])
        self._detect(b, stores, row)

    def _result(self, b, stores, first_ord, n, store, flush=False):
        """the ``VideoDetections`` of the keys ``first_ord .. first_ord + n - 1`` in the first n rows of the stores, linked; with actors its
        ``.actors`` as well, tracked (``flush``: these are the video's last keys)"""
        full, full_a = stores
        if n == 0 and not (full_a is not None and flush and self._video_keys and self.actor_settings["window"]):
            return None                    # (with actors, a finish() that runs no key still emits the smoothed rows that waited for it)
        vd = VideoDetections([(first_ord + i) * self.stride for i in range(n)], *[t[:n] for t in full], class_num=self.class_num,
                             settings=self.settings, store=store)
        if self.link and n:
            self._link(b, vd, first_ord)
            self._pending.append((first_ord, vd))
        if full_a is not None:
            vd.actors = VideoActors(vd.keys, *[t[:n] for t in full_a], settings=self.actor_settings, store=store)
            self._track(b, vd.actors, first_ord, flush)
            self._pending_tracks.append((first_ord, vd.actors))
            self._video_keys += n
        return vd

    def _track(self, b, va, first_ord, flush):
        """the track records of the keys ``first_ord ..`` onto ``va``: ``tuber_tube_link_stream`` with one class, the label derived from
        ``queries`` on the device, then ``tuber_track_actions_stream``; ``evaluation.ActorTracker`` on the host beyond their bounds"""
        from .evaluation import smooth_range
        n, A, C = va.actions.shape
        st, dev = self.actor_settings, va.actions.device
        if (first_ord + n) * A > 0x7FFFFFFF:
            raise RuntimeError("VideoStream: key ordinal %d with %d actors per key frame: row numbers beyond 32 bits" % (first_ord + n, A))
        lo, hi = smooth_range(first_ord, n, st["window"], flush)
        va.smooth_first = lo
        f64, i32 = torch.float64, torch.int32
        if self._why_host_tracks is None:
            self.tracks_path = "device"
            va.row_head, va.row_score, va.row_len = torch.empty(n, A, dtype=i32, device=dev), torch.empty(n, A, dtype=f64, device=dev), torch.empty(n, A, dtype=i32, device=dev)
            va.row_mean, va.row_peak = torch.empty(n, A, C, dtype=f64, device=dev), torch.empty(n, A, C, dtype=torch.float32, device=dev)
            va.smooth = torch.empty(hi - lo, A, C, dtype=f64, device=dev)
            if n:
                label = torch.where(va.queries >= 0, 0, -1).to(i32).contiguous()         # one class; a row behind its key's count is not counted
                lib.call("tuber_tube_link_stream", va.boxes.contiguous(), label, va.actor.contiguous(), n, A, first_ord, 1, st["link_iou"], st["max_gap"],
                         b["actor_state"], va.row_head, va.row_score, va.row_len)
            lib.call("tuber_track_actions_stream", va.actions.contiguous(), va.row_head, n, A, C, first_ord, st["max_gap"], st["window"], 1 if flush else 0,
                     b["track_state"], va.row_mean, va.row_peak, va.smooth)
            return
        tracker = self._host_tracker("[tuber] VideoStream: %s; tracks on the host" % self._why_host_tracks)
        self.tracks_path = "host"
        host = va._fetch()[0]
        got = tracker.push(host["boxes"].reshape(-1, 4), host["actor"].reshape(-1), host["queries"].reshape(-1), host["actions"].reshape(n * A, C), A,
                           flush=flush)
        up = lambda a, dtype, *shape: torch.from_numpy(np.ascontiguousarray(a.astype(dtype))).reshape(*shape).to(dev)
        va.row_head, va.row_score, va.row_len = up(got["row_head"], np.int32, n, A), up(got["row_score"], np.float64, n, A), up(got["row_len"], np.int32, n, A)
        va.row_mean, va.row_peak = up(got["row_mean"], np.float64, n, A, C), up(got["row_peak"], np.float32, n, A, C)
        va.smooth = up(got["smooth"], np.float64, hi - lo, A, C)

    def _link(self, b, vd, first_ord):
        n, K = vd.scores.shape
        dev = vd.scores.device
        why = self._why_host
        if why is None and (first_ord + n) * K > 0x7FFFFFFF:
            why = "key ordinal %d with %d rows per key frame: row numbers beyond 32 bits" % (first_ord + n, K)
        if why is None:
            vd.row_head = torch.empty(n, K, dtype=torch.int32, device=dev)
            vd.row_score = torch.empty(n, K, dtype=torch.float64, device=dev)
            vd.row_len = torch.empty(n, K, dtype=torch.int32, device=dev)
            lib.call("tuber_tube_link_stream", vd.boxes.contiguous(), vd.labels.contiguous(), vd.scores.contiguous(), n, K, first_ord, self.class_num,
                     self.settings["link_iou"], self.settings["max_gap"], b["state"], vd.row_head, vd.row_score, vd.row_len)
            return
        linker = self._host_linker("[tuber] VideoStream: %s; linking on the host" % why)
        host = vd._fetch()[0]
        got = linker.push(host["boxes"].reshape(-1, 4), host["labels"].reshape(-1), host["scores"].reshape(-1), K)
        vd.row_head = torch.from_numpy(got["row_head"].reshape(n, K).astype(np.int32)).to(dev)
        vd.row_score = torch.from_numpy(got["row_score"].reshape(n, K)).to(dev)
        vd.row_len = torch.from_numpy(got["row_len"].reshape(n, K).astype(np.int32)).to(dev)

    @torch.no_grad()
    def push(self, frames):
        frames = self._frames(frames, "n", 0)
        m, H0, W0 = (int(v) for v in frames.shape[:3])
        sch = self.schedule
        if sch.frames and (H0, W0) != (self._cur["H0"], self._cur["W0"]):
            raise ValueError("VideoStream: frames of %d x %d in a video of %d x %d" % (H0, W0, self._cur["H0"], self._cur["W0"]))
        if m == 0:
            return None
        store, _ = self.model.engine()
        dev = store.device
        if not sch.frames:
            self._cur = self._buffers(dev, H0, W0)
        b, B = self._cur, self.batch
        first_frame, first_ord = sch.frames, sch.decided
        plan = sch.push(m)                                      # host integers first: the pieces, and the batches ready after each
        total = sum(len(batches) for _, _, batches in plan)
        stores = self._stores(total * B, dev) if total else None
        row = 0
        for i, length, batches in plan:
            src = frames[i:i + length].to(dev, non_blocking=True).contiguous()
            self._store_frames(b, src, first_frame + i)
            for k in batches:
                self._run(b, stores, row, k, B, -1)
                row += B
        return self._result(b, stores, first_ord, row, store) if row else None

    @torch.no_grad()
    def finish(self):
        self._check_eval()
        decided = self.schedule.decided
        n_total, batches = self.schedule.finish()
        self.wrapped = False
        if not n_total:
            return None
        b, B = self._cur, self.batch
        store, _ = self.model.engine()
        out = None
        if batches:
            stores = self._stores(len(batches) * B, store.device)
            for i, (k, n_keys) in enumerate(batches):
                self._run(b, stores, i * B, k, n_keys, n_total)
            out = self._result(b, stores, batches[0][0], batches[-1][0] + batches[-1][1] - batches[0][0], store, flush=True)
        elif self.detector.actors is not None:                  # no key left to run: the smoothed rows that waited for the end (S = 0, flush)
            out = self._result(b, self._stores(0, store.device), decided, 0, store, flush=True)
        b["state"].zero_()
        for k in ("actor_state", "track_state"):
            if k in b:
                b[k].zero_()
        self._host_linker.reset()
        if self.link:
            self._pending.append(None)
        if self.detector.actors is not None:
            self._host_tracker.reset()
            self._pending_tracks.append(None)
            self._video_keys = 0
        return out

    # -- tubes and actor tracks -------------------------------------------------------------------------------------------
    TUBE_NAMES = ("boxes", "labels", "row_head", "row_score", "row_len", "scores")
    TRACK_NAMES = ("boxes", "actor", "queries", "actions", "row_head", "row_score", "row_len", "row_mean", "row_peak", "smooth")

    @staticmethod
    def _drain(pending, assembler, names, last=(), dense=False):
        """the records of ``pending`` through ``assembler`` -> what closed (``dense``: with a box on every frame): ONE device-to-host copy for
        every record, ``end()`` at the markers of a video's end"""
        host = host_parts([getattr(p[1], k) for p in pending if p is not None for k in names])
        out, i, m = [], 0, len(names)
        for p in pending:
            if p is None:                                       # the end of a video: whatever is open closes
                assembler.end()
                out += assembler.take(dense)
                continue
            first_ord, rec = p
            assembler.add(first_ord, rec.keys, *host[m * i:m * i + m], *(getattr(rec, k) for k in last))
            i += 1
        return out + assembler.take(dense)

    def tubes(self, dense=None):
        """The tubes that closed since the last call (the class docstring).  ``dense`` (default: ``CONFIG.VAL.VIDEO_MAP.DENSE``): every closed
        tube through ``evaluation.dense_tube`` on the host, where it was assembled anyway -- ``VideoDetections.tubes(dense=True)``'s dicts
        (plus ``head``), bit for bit; no device state is added and ``push`` is as it was."""
        if not self.link:
            raise RuntimeError("VideoStream(link=False) keeps no link records: no tubes")
        pending, self._pending = self._pending, []
        return self._drain(pending, self._tubes, self.TUBE_NAMES, dense=self.dense if dense is None else bool(dense))

    def tracks(self, dense=None):
        """The actor tracks (``actors=A``) that CLOSED since the last call: the next key ordinal is more than ``max(max_gap + 1, window)`` past
        their last one -- no key frame still to come can extend them, and the smoothed row of their last key has been emitted -- and after
        ``finish()`` all that remain.  ``VideoActors.tracks``' dicts plus ``head`` (key ordinal * A + position of the first row), in head
        order; ``score`` / ``mean`` / ``peak`` are the records of the track's last row.  One device-to-host copy per call; the rows of open
        tracks are kept on the host in between (``TrackAssembler``; ``TubeAssembler`` for ``tubes()``).  ``tubes()`` keeps its own records:
        neither consumes the other's.  ``dense`` (default: ``CONFIG.VAL.VIDEO_MAP.DENSE``): as in ``tubes``, the interpolated score being
        the actor probability -- ``VideoActors.tracks(dense=True)``'s dicts."""
        if self._assembler is None:
            raise RuntimeError("VideoStream without actors=A keeps no actor records: no tracks")
        pending, self._pending_tracks = self._pending_tracks, []
        return self._drain(pending, self._assembler, self.TRACK_NAMES, ("smooth_first",), dense=self.dense if dense is None else bool(dense))


class _HostDefinition:
    """Say it once, then use the host definition: ``self(line)`` prints ``line`` on stderr the first time only and returns the object ``make()``
    built on first use; ``reset()`` resets it for the next video if it was ever built."""

    def __init__(self, make):
        self.make, self.made = make, None

    def __call__(self, line):
        if self.made is None:
            print(line, file=sys.stderr, flush=True)
            self.made = self.make()
        return self.made

    def reset(self):
        if self.made is not None:
            self.made.reset()


class _Assembler:
    """What ``TubeAssembler`` and ``TrackAssembler`` share: open records by head, a record closing once the next key ordinal is more than
    ``stale`` past its last one or the video ends, closed records shorter than ``min_len`` dropped, ``take()`` in head order."""

    SCORE, SCORE_IS_PUBLIC = None, True                # the per-key field ``take(dense=True)`` interpolates, and whether the plain dict shows it

    def __init__(self, stale, min_len):
        self.stale, self.min_len = int(stale), int(min_len)
        self._open, self._closed, self._next = {}, [], 0

    def _rows(self, first_ord, keys, row_head, row_score, row_len):
        """every counted row (s, q) of a push with the open record it extends -- a new one for a new head -- its frame, score, length and last
        ordinal already noted"""
        head = np.asarray(row_head)
        for s, q in zip(*np.nonzero(head >= 0)):
            h = int(head[s, q])
            t = self._open.setdefault(h, dict(head=h, frames=[]))
            t["frames"].append(int(keys[s]))
            t["score"], t["length"], t["last"] = float(row_score[s, q]), int(row_len[s, q]), int(first_ord) + int(s)
            yield s, q, t

    def _advance(self, next_ord):
        self._next = int(next_ord)
        self._close(False)

    def end(self):
        self._close(True)
        self._next = 0

    def _close(self, everything):
        for h in sorted(self._open):
            t = self._open[h]
            if everything or self._next - t["last"] > self.stale:
                del self._open[h]
                if t["length"] >= self.min_len:
                    self._closed.append(self._finished(t))

    def take(self, dense=False):
        out, self._closed = sorted(self._closed, key=lambda t: t["head"]), []
        return [self._emit(t, dense) for t in out]

    def _emit(self, t, dense):
        """a closed record as its public dict: without ``dense`` as ``_finished`` left it; with it through ``evaluation.dense_tube``, the
        interpolated score being the record's ``SCORE`` field (per key)"""
        from .evaluation import dense_tube
        t = dict(t)
        score = t.get(self.SCORE) if self.SCORE_IS_PUBLIC else t.pop(self.SCORE, None)
        if not dense:
            return t
        if score is None:
            raise RuntimeError("%s: dense tubes need the per-key %s, which add() was not given" % (type(self).__name__, self.SCORE))
        return _densified(t, dense_tube(t["frames"], t["boxes"], score))


class TubeAssembler(_Assembler):
    """The host side of ``VideoStream.tubes()``: the per-push link records of a stream (host arrays) in, closed tubes out.
    ``add(first_ord, keys, boxes, labels, row_head, row_score, row_len)`` takes the records of the keys ``first_ord ..`` ([n, K, ...] arrays);
    ``end()`` marks the end of the video; ``take()`` returns the tubes closed since the last call, in head order: after ``end()`` all of them,
    before it those whose last key lies more than ``max_gap + 1`` ordinals behind the next one.  A tube is ``VideoDetections.tubes``' dict plus
    ``head``; tubes shorter than ``min_len`` are dropped.  ``take(dense=True)``: ``VideoDetections.tubes(dense=True)``'s dicts instead
    (``evaluation.dense_tube`` per closed tube); it needs ``add(..., scores)``, the [n, K] fp32 scores of the rows."""
    SCORE, SCORE_IS_PUBLIC = "scores", False

    def __init__(self, max_gap, min_len=1):
        super().__init__(int(max_gap) + 1, min_len)

    def add(self, first_ord, keys, boxes, labels, row_head, row_score, row_len, scores=None):
        for s, q, t in self._rows(first_ord, keys, row_head, row_score, row_len):
            t.setdefault("cls", int(labels[s, q]) + 1)
            t.setdefault("boxes", []).append(boxes[s, q].copy())
            if scores is not None:
                t.setdefault("scores", []).append(np.float32(scores[s, q]))
        self._advance(first_ord + len(keys))

    def _finished(self, t):
        out = dict(cls=t["cls"], score=t["score"], frames=t["frames"], boxes=np.stack(t["boxes"]), length=t["length"], head=t["head"])
        if len(t.get("scores", ())) == len(t["frames"]):
            out["scores"] = np.asarray(t["scores"], dtype=np.float32)
        return out


class TrackAssembler(_Assembler):
    """The host side of ``VideoStream.tracks()``: the per-push records of a stream's actors (host arrays) in, closed actor tracks out.
    ``add(first_ord, keys, boxes, actor, queries, actions, row_head, row_score, row_len, row_mean, row_peak, smooth, smooth_first)`` takes the
    records of the keys ``first_ord ..`` ([n, A, ...] arrays; ``smooth`` [m, A, C] belongs to the slots ``smooth_first ..``, which lag
    ``window`` keys behind); ``end()`` marks the end of the video; ``take()`` returns the tracks closed since the last call, in head order: after
    ``end()`` all of them, before it those whose last key lies more than ``max(max_gap + 1, window)`` ordinals behind the next one.  A track
    is ``VideoActors.tracks``' dict plus ``head``; tracks shorter than ``min_len`` are dropped.  ``take(dense=True)``:
    ``VideoActors.tracks(dense=True)``'s dicts instead (``evaluation.dense_tube`` per closed track over its ``actor`` probabilities)."""
    SCORE, SCORE_IS_PUBLIC = "actor", True

    def __init__(self, A, max_gap, window, min_len=1, label_thr=0.05):
        super().__init__(max(int(max_gap) + 1, int(window)), min_len)
        self.A, self.max_gap, self.window, self.label_thr = int(A), int(max_gap), int(window), float(label_thr)
        self._waiting = {}

    def add(self, first_ord, keys, boxes, actor, queries, actions, row_head, row_score, row_len, row_mean, row_peak, smooth, smooth_first):
        for s, a, t in self._rows(first_ord, keys, row_head, row_score, row_len):
            for k, src in (("boxes", boxes), ("actor", actor), ("queries", queries), ("actions", actions)):
                t.setdefault(k, []).append(np.array(src[s, a]))
            t["mean"], t["peak"] = np.array(row_mean[s, a], dtype=np.float64), np.array(row_peak[s, a], dtype=np.float32)
            t.setdefault("smooth", [])
            self._waiting.setdefault(t["last"], []).append((int(a), t["head"]))     # the row's smoothed scores come `window` keys later
        for j in range(len(smooth)):                                      # slots in order: a track's smoothed rows arrive in slot order
            for a, h in self._waiting.pop(int(smooth_first) + j, []):
                self._open[h]["smooth"].append(np.array(smooth[j, a], dtype=np.float64))
        self._advance(int(first_ord) + len(keys))

    def end(self):
        super().end()
        self._waiting = {}

    def _finished(self, t):
        if len(t["smooth"]) != len(t["frames"]):
            raise RuntimeError("TrackAssembler: track %d closes with %d of its %d smoothed rows" % (t["head"], len(t["smooth"]), len(t["frames"])))
        return dict(score=t["score"], frames=t["frames"], boxes=np.stack(t["boxes"]), actor=np.stack(t["actor"]), queries=np.stack(t["queries"]),
                    actions=np.stack(t["actions"]), smooth=np.stack(t["smooth"]), mean=t["mean"], peak=t["peak"],
                    labels=_track_labels(t["mean"], self.label_thr), length=t["length"], head=t["head"])
