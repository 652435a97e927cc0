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
"""
import functools
import sys

import numpy as np
import torch

from . import input_pipeline as ip
from . import lib
from .detect import ACTOR_FIELDS, FIELDS, Detector
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


def _nms_device(boxes, slot_off, video_off, link, S, N, C, K, min_len, nms):
    """``tuber_tube_nms`` behind ``tuber_tube_link_ranked`` over a padded [S][K] store -> tube_keep [N] uint8 on the device"""
    keep = torch.full((N,), 2, dtype=torch.uint8, device=boxes.device)
    work = torch.empty(max(lib.query("tuber_tube_nms_work_bytes", N), 16), dtype=torch.uint8, device=boxes.device)
    lib.call("tuber_tube_nms", boxes, slot_off, video_off, link["row_cls"], link["row_head"], link["tube_score"], link["tube_len"], link["tube_last"], 1,
             S, N, int(C), K, max(int(min_len), 1), float(nms), work, keep)
    return keep


class VideoDetections:
    """The ranked detections of a video's key frames: ``keys`` (frame numbers) and, as tensors on one device, ``boxes`` [n, K, 4] fp32 xyxy in
    source-video pixels, ``scores`` / ``aux`` [n, K] fp32, ``labels`` / ``queries`` [n, K] int32 (-1 in the rows behind ``count``), ``count`` /
    ``total`` [n] int32 -- the fields of ``detect.Detections``, a row per key frame."""

    def __init__(self, keys, boxes, scores, labels, queries, aux, count, total, class_num, settings=None, store=None, nms_iou=None):
        self.keys = [int(k) for k in keys]
        self.nms_iou = None if nms_iou is None else float(nms_iou)                      # the default of tubes(nms=): CONFIG.VAL.TUBE_NMS.IOU
        self.boxes, self.scores, self.labels, self.queries, self.aux, self.count, self.total = boxes, scores, labels, queries, aux, count, total
        self.class_num = int(class_num)
        self.settings = dict(settings or dict(link_iou=0.2, max_gap=2, min_len=1))      # the defaults of tubes(): CONFIG.VAL.VIDEO_MAP
        self.tubes_path = None                                                         # "device" or "host" after tubes()
        self._store = store                                                            # the engine's ParamStore: to_host reads its error word
        self.row_head = self.row_score = self.row_len = None                           # the link records of a VideoStream push (link=True)
        self.actors = None                                                             # the ``VideoActors`` of ``VideoDetector(..., actors=A)``
        if not (len(self.keys) == boxes.shape[0] == scores.shape[0] == count.shape[0]):
            raise ValueError("VideoDetections: %d keys, %d rows" % (len(self.keys), boxes.shape[0]))

    def tensors(self):
        return tuple(getattr(self, k) for k in FIELDS)

    def _fetch(self, extra=()):
        """every field (and ``extra`` tensors) as numpy arrays, in ONE device-to-host copy"""
        parts = [t.contiguous() for t in list(self.tensors()) + list(extra)]
        if self.boxes.device.type != "cuda":
            return [t.numpy() for t in parts]
        blob = torch.cat([t.reshape(-1).view(torch.uint8) for t in parts]).cpu().numpy()
        host, o = [], 0
        for t in parts:
            n = t.numel() * t.element_size()
            host.append(blob[o:o + n].view(np.dtype(str(t.dtype).replace("torch.", ""))).reshape(tuple(t.shape)))
            o += n
        return host

    def to_host(self):
        """a list, per key frame, of dicts of numpy arrays trimmed to ``count`` (``key``, ``boxes``, ``scores``, ``labels``, ``queries``, ``aux``,
        ``count``, ``total``): one copy, the place that synchronises.  A cooperative decoder launch that timed out during the video leaves empty
        key frames (detect.py, "Fail-safe"); its error word travels in the same copy and raises here, the engine having switched to the launch
        chain: run the video again."""
        word = [self._store.coop_sync] if self._store is not None and self.boxes.device.type == "cuda" else []
        host = self._fetch(word)
        if word and host[-1][2] and not self._store.coop_off:
            self._store.check_coop()
        host = dict(zip(FIELDS, host))
        out = []
        for i, key in enumerate(self.keys):
            n = int(host["count"][i])
            d = {k: host[k][i, :n].copy() for k in ("boxes", "scores", "labels", "queries", "aux")}
            d["key"], d["count"], d["total"] = key, n, int(host["total"][i])
            out.append(d)
        return out

    # -- tubes ------------------------------------------------------------------------------------------------------------
    def _link_device(self, link_iou, max_gap, nms=None, min_len=1):
        """``tuber_tube_link_ranked`` (and, with ``nms``, ``tuber_tube_nms`` behind it) over the padded store as it is, or None where the
        linker's bounds refuse it"""
        S, K = self.scores.shape
        if self.boxes.device.type != "cuda":
            return None, "the store is on the CPU"
        if K > lib.query("tuber_frame_match_max_dets") or K * (max_gap + 1) > lib.query("tuber_tube_link_max_active"):
            return None, "%d rows per key frame with max_gap %d: beyond %d rows or %d active tubes" % (
                K, max_gap, lib.query("tuber_frame_match_max_dets"), lib.query("tuber_tube_link_max_active"))
        dev, N = self.boxes.device, S * K
        slot_off = torch.arange(S + 1, dtype=torch.int32, device=dev) * K               # rows behind a key's count carry label -1: not counted
        video_off = torch.tensor([0, S], dtype=torch.int32).to(dev)
        out = dict(row_cls=torch.empty(N, dtype=torch.int32, device=dev), row_head=torch.empty(N, dtype=torch.int32, device=dev),
                   tube_score=torch.zeros(N, dtype=torch.float64, device=dev), tube_len=torch.zeros(N, dtype=torch.int32, device=dev),
                   tube_last=torch.full((N,), -1, dtype=torch.int32, device=dev))
        lib.call("tuber_tube_link_ranked", self.boxes.contiguous(), self.labels.contiguous(), self.scores.contiguous(), slot_off, video_off, 1, S, N,
                 self.class_num, K, float(link_iou), int(max_gap), out["row_cls"], out["row_head"], out["tube_score"], out["tube_len"], out["tube_last"])
        names = ("row_head", "tube_score", "tube_len", "tube_last")
        if nms is not None:
            out["tube_keep"] = _nms_device(self.boxes.contiguous(), slot_off, video_off, out, S, N, self.class_num, K, min_len, nms)
            names += ("tube_keep",)
        host = self._fetch([out[k] for k in names])
        return dict(zip(FIELDS + names, host)), None

    def tubes(self, link_iou=None, max_gap=None, min_len=None, nms=None):
        """The action tubes of the video: a list of ``dict(cls, score, frames, boxes, length)`` in head order (the order of the tubes' first
        detections) -- ``cls`` 1-based as in ``evaluation.tubes_from_link``, ``score`` the fp64 mean of the linked fp32 scores, ``frames`` the key
        frame numbers, ``boxes`` [length, 4] in source pixels; tubes shorter than ``min_len`` are dropped.  The slots of the linker are key
        ORDINALS, so ``max_gap`` counts key frames.  Defaults: ``CONFIG.VAL.VIDEO_MAP``.  Linked on the device by ``tuber_tube_link_ranked``;
        beyond its bounds (K > 64 rows per key frame or K * (max_gap + 1) > ``tuber_tube_link_max_active()`` = 64) or on a CPU store
        ``evaluation.link_rows`` answers, one line says so, and ``tubes_path`` is "host" instead of "device".  ``VideoDetector``'s default
        ``topk`` is 21 = 64 // (MAX_GAP + 1) with the shipped MAX_GAP of 2, so that the default path is the device's.  ``nms`` (default:
        ``CONFIG.VAL.TUBE_NMS.IOU``; None: off): per class a tube whose spatio-temporal IoU with a higher-scored kept tube exceeds it is
        dropped -- one more launch, ``tuber_tube_nms``, whose bytes travel in the same copy; on the host path
        ``evaluation.tube_nms``."""
        from .evaluation import link_rows, tube_nms, tubes_from_link
        nms = _nms_value("VideoDetections.tubes", self.nms_iou if nms is None else nms)
        link_iou = float(self.settings["link_iou"] if link_iou is None else link_iou)
        max_gap = int(self.settings["max_gap"] if max_gap is None else max_gap)
        min_len = int(self.settings["min_len"] if min_len is None else min_len)
        S, K = self.scores.shape
        slot = np.repeat(np.arange(S, dtype=np.int64), K)
        host, why = self._link_device(link_iou, max_gap, nms, min_len)
        if host is None:
            print("[tuber] VideoDetections.tubes: %s; linking on the host" % why, file=sys.stderr, flush=True)
            host = dict(zip(FIELDS, self._fetch()))
            host.update(link_rows(host["boxes"].reshape(-1, 4), host["labels"].reshape(-1), host["scores"].reshape(-1), slot, [0, S], self.class_num,
                                  link_iou, max_gap))
        self.tubes_path = "host" if why else "device"
        layout = dict(videos=["video"], video_off=np.asarray([0, S]), first_frame=np.asarray([0]))
        link = dict(layout=layout, row_head=host["row_head"], row_slot=slot, row_cls=host["labels"].reshape(-1), tube_score=host["tube_score"],
                    det_box=host["boxes"].reshape(-1, 4))
        keep = None
        if nms is not None:
            keep = host.get("tube_keep")
            if keep is None or (keep == 3).any():                                      # the host path, or the kernel's escape
                keep = tube_nms(link, nms, max(min_len, 1))
        out = []
        for t in tubes_from_link(link):
            if len(t["frames"]) >= min_len and (keep is None or keep[t["head"]] != 0):
                out.append(dict(cls=t["cls"], score=t["score"], frames=[self.keys[s] for s in t["frames"]], boxes=t["boxes"], length=len(t["frames"])))
        return out


class VideoActors:
    """The actors of a video's key frames (``VideoDetector(..., actors=A)``): ``keys`` (frame numbers) and, as tensors on one
    device, ``boxes`` [n, A, 4] fp32 xyxy in source-video pixels, ``actor`` [n, A] fp32 (the actor probability), ``queries`` [n, A] int32 (-1 in
    the rows behind ``count``), ``actions`` [n, A, C] fp32 (every class's score), ``count`` / ``total`` [n] int32 -- the fields of
    ``detect.Actors``, a row per key frame."""

    def __init__(self, keys, boxes, actor, queries, actions, count, total, settings=None, store=None, nms_iou=None):
        self.keys = [int(k) for k in keys]
        self.nms_iou = None if nms_iou is None else float(nms_iou)                      # the default of tracks(nms=): CONFIG.VAL.TUBE_NMS.ACTORS_IOU
        self.boxes, self.actor, self.queries, self.actions, self.count, self.total = boxes, actor, queries, actions, count, total
        self.class_num = int(actions.shape[2])
        # the defaults of tracks(): CONFIG.VAL.ACTORS
        self.settings = dict(settings or dict(link_iou=0.2, max_gap=2, min_len=1, window=1, label_thr=0.05))
        self.tracks_path = None                                                        # "device" or "host" after tracks()
        self._store = store
        # the track records of a VideoStream(actors=A) push: row_head / row_score / row_len [n, A], row_mean / row_peak [n, A, C], smooth [m, A, C]
        self.row_head = self.row_score = self.row_len = self.row_mean = self.row_peak = self.smooth = None
        self.smooth_first = None                                                       # the key ordinal of smooth's first slot (a host int)
        if not (len(self.keys) == boxes.shape[0] == actor.shape[0] == actions.shape[0] == count.shape[0]):
            raise ValueError("VideoActors: %d keys, %d rows" % (len(self.keys), boxes.shape[0]))

    def tensors(self):
        return tuple(getattr(self, k) for k in ACTOR_FIELDS)

    def _fetch(self, extra=()):
        """every field (and ``extra`` tensors) as numpy arrays, in ONE device-to-host copy"""
        parts = [t.contiguous() for t in list(self.tensors()) + list(extra)]
        if self.boxes.device.type != "cuda":
            return [t.numpy() for t in parts]
        blob = torch.cat([t.reshape(-1).view(torch.uint8) for t in parts]).cpu().numpy()
        host, o = [], 0
        for t in parts:
            n = t.numel() * t.element_size()
            host.append(blob[o:o + n].view(np.dtype(str(t.dtype).replace("torch.", ""))).reshape(tuple(t.shape)))
            o += n
        return host

    def to_host(self):
        """a list, per key frame, of dicts of numpy arrays trimmed to ``count`` (``key``, ``boxes``, ``actor``, ``queries``, ``actions``,
        ``count``, ``total``): one copy, the place that synchronises; the cooperative decoder's error word travels in it and raises here, as in
        ``VideoDetections.to_host``."""
        word = [self._store.coop_sync] if self._store is not None and self.boxes.device.type == "cuda" else []
        host = self._fetch(word)
        if word and host[-1][2] and not self._store.coop_off:
            self._store.check_coop()
        host = dict(zip(ACTOR_FIELDS, host))
        out = []
        for i, key in enumerate(self.keys):
            n = int(host["count"][i])
            d = {k: host[k][i, :n].copy() for k in ("boxes", "actor", "queries", "actions")}
            d["key"], d["count"], d["total"] = key, n, int(host["total"][i])
            out.append(d)
        return out

    # -- tracks -----------------------------------------------------------------------------------------------------------
    NAMES = ("row_head", "tube_score", "tube_len", "tube_last", "row_smooth", "track_mean", "track_peak")

    def _tracks_device(self, link_iou, max_gap, window, nms=None, min_len=1):
        """``tuber_tube_link_ranked`` with one class and ``tuber_track_actions`` (and, with ``nms``, ``tuber_tube_nms``) over the padded store as
        it is, everything read back in one copy; or None where the kernels' bounds refuse it"""
        S, A, C = self.actions.shape
        if self.boxes.device.type != "cuda":
            return None, "the store is on the CPU"
        rows, active = lib.query("tuber_frame_match_max_dets"), lib.query("tuber_tube_link_max_active")
        max_a, max_c = lib.query("tuber_track_actions_limits", 0), lib.query("tuber_track_actions_limits", 1)
        if A > min(rows, max_a) or A * (max_gap + 1) > active or C > max_c:
            return None, "%d actors per key frame with max_gap %d and %d classes: beyond %d rows, %d active tracks or %d classes" % (
                A, max_gap, C, min(rows, max_a), active, max_c)
        dev, N = self.boxes.device, S * A
        f64, i32 = torch.float64, torch.int32
        slot_off = torch.arange(S + 1, dtype=i32, device=dev) * A
        video_off = torch.tensor([0, S], dtype=i32).to(dev)
        label = torch.where(self.queries >= 0, 0, -1).to(i32).contiguous()               # one class; a row behind its key's count is not counted
        out = dict(row_cls=torch.empty(N, dtype=i32, device=dev), row_head=torch.empty(N, dtype=i32, device=dev),
                   tube_score=torch.zeros(N, dtype=f64, device=dev), tube_len=torch.zeros(N, dtype=i32, device=dev),
                   tube_last=torch.full((N,), -1, dtype=i32, device=dev), row_smooth=torch.empty(N, C, dtype=f64, device=dev),
                   track_mean=torch.empty(N, C, dtype=f64, device=dev), track_peak=torch.empty(N, C, dtype=torch.float32, device=dev))
        lib.call("tuber_tube_link_ranked", self.boxes.contiguous(), label, self.actor.contiguous(), slot_off, video_off, 1, S, N, 1, A, float(link_iou),
                 int(max_gap), out["row_cls"], out["row_head"], out["tube_score"], out["tube_len"], out["tube_last"])
        lib.call("tuber_track_actions", self.actions.contiguous(), out["row_head"], out["tube_last"], S, A, C, int(window), out["row_smooth"],
                 out["track_mean"], out["track_peak"])
        names = self.NAMES
        if nms is not None:
            out["tube_keep"] = _nms_device(self.boxes.contiguous(), slot_off, video_off, out, S, N, 1, A, min_len, nms)
            names += ("tube_keep",)
        host = self._fetch([out[k] for k in names])
        return dict(zip(ACTOR_FIELDS + names, host)), None

    def tracks(self, link_iou=None, max_gap=None, min_len=None, window=None, label_thr=None, nms=None):
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
        the device, ``evaluation.tube_nms`` on the host path.  The aggregates of the kept tracks are unchanged."""
        from .evaluation import actor_tracks, tube_nms
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
        host, why = self._tracks_device(link_iou, max_gap, window, nms, min_len)
        if host is None:
            print("[tuber] VideoActors.tracks: %s; tracks on the host" % why, file=sys.stderr, flush=True)
            host = dict(zip(ACTOR_FIELDS, self._fetch()))
            host.update(actor_tracks(host["boxes"], host["actor"], host["queries"], host["actions"], S, A, link_iou, max_gap, window))
        self.tracks_path = "host" if why else "device"
        head = np.asarray(host["row_head"]).reshape(-1)
        box, actor, query, act = host["boxes"].reshape(-1, 4), host["actor"].reshape(-1), host["queries"].reshape(-1), host["actions"].reshape(-1, C)
        members = {}
        for r in np.nonzero(head >= 0)[0].tolist():
            members.setdefault(int(head[r]), []).append(r)
        keep = None
        if nms is not None:
            keep = host.get("tube_keep")
            if keep is None or (keep == 3).any():                                      # the host path, or the kernel's escape
                keep = tube_nms(dict(layout=dict(video_off=np.asarray([0, S])), row_head=head, row_slot=np.repeat(np.arange(S, dtype=np.int64), A),
                                     row_cls=np.where(query >= 0, 0, -1), tube_score=host["tube_score"], det_box=box), nms, max(min_len, 1))
        out = []
        for h in sorted(members):
            rows = members[h]
            if len(rows) < min_len or (keep is not None and keep[h] == 0):
                continue
            mean = np.array(host["track_mean"][h], dtype=np.float64)
            with np.errstate(invalid="ignore"):
                labels = sorted(np.nonzero(mean >= label_thr)[0].tolist(), key=lambda c: (-mean[c], c))
            out.append(dict(score=float(host["tube_score"][h]), frames=[self.keys[r // A] for r in rows], boxes=box[rows].copy(), actor=actor[rows].copy(),
                            queries=query[rows].copy(), actions=act[rows].copy(), smooth=np.array(host["row_smooth"][rows], dtype=np.float64), mean=mean,
                            peak=np.array(host["track_peak"][h], dtype=np.float32), labels=labels, length=len(rows)))
        return out


class VideoDetector:
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
    when to when, doing what" (DESIGN.md section 6i)."""

    def __init__(self, cfg, model, batch=2, score_thr=None, topk=None, actor_thr=None, graphed=True, rule=None, actors=None):
        from .config import actor_settings, detect_settings, tube_nms_settings, video_map_settings
        self.cfg, self.model = cfg, model
        self.nms = tube_nms_settings(cfg)                  # the defaults of tubes(nms=) / tracks(nms=): kept out of ``settings``
        self.batch = int(batch)
        if self.batch < 1:
            raise ValueError("VideoDetector: batch = %r must be >= 1" % (batch,))
        vm = video_map_settings(cfg)
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
            raise ValueError("VideoDetector: rule %r is not one of %s" % (rule, ", ".join(RULES)))
        D = cfg.CONFIG.DATA
        self.T, self.rate, self.size, self.class_num = int(D.TEMP_LEN), int(D.FRAME_RATE), int(D.IMG_SIZE), int(D.NUM_CLASSES)
        self._bufs = {}

    def _resident(self, frames, dev, chunk):
        """the video at working resolution on the device, uint8 [N, nh, nw, 3]: uploaded and resized ``chunk`` frames at a time"""
        N, H0, W0 = (int(v) for v in frames.shape[:3])
        nh, nw = working_geometry(H0, W0, self.size)[:2]
        out = torch.empty(N, nh, nw, 3, dtype=torch.uint8, device=dev)
        same = (nh, nw) == (H0, W0)
        if not same:
            (bh, kh, bv, kv), ksh, ksv, y0, rows = ip._device_coeffs(dev, H0, W0, nh, nw)
            tmp = torch.empty(chunk * rows * nw * 3, dtype=torch.uint8, device=dev) if (nw != W0 and nh != H0) else None
        for i in range(0, N, chunk):
            src = frames[i:i + chunk].to(dev, non_blocking=True).contiguous()
            if same:
                out[i:i + chunk].copy_(src)
            else:
                lib.call("tuber_frames_resize", src, tmp, out[i:], src.shape[0], H0, W0, nh, nw, bh, kh, ksh, bv, kv, ksv, y0, rows)
        return out

    @torch.no_grad()
    def __call__(self, frames, keys=None, stride=None, chunk=256):
        if self.model.training:
            raise RuntimeError("VideoDetector runs an eval forward: call model.eval() first")
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
            raise ValueError("VideoDetector wants uint8 frames [N, H, W, 3], got %s %s" % (frames.dtype, tuple(frames.shape)))
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError("VideoDetector: chunk = %r must be >= 1" % (chunk,))
        store, _ = self.model.engine()
        dev = store.device
        N, H0, W0 = (int(v) for v in frames.shape[:3])
        if keys is None:
            stride = int(stride) if stride is not None else (30 if self.mode == "ava" else 1)
            if stride < 1:
                raise ValueError("VideoDetector: stride = %r must be >= 1" % (stride,))
            keys = range(0, N, stride)
        keys = [int(k) for k in keys]
        if not keys:
            raise ValueError("VideoDetector: no key frames")
        n, B, T = len(keys), self.batch, self.T
        nb = (n + B - 1) // B
        table = clip_indices(N, keys + [keys[-1]] * (nb * B - n), T, self.rate, self.rule)      # the padded last batch repeats its last key
        table = torch.from_numpy(table).to(dev, non_blocking=True)
        resident = self._resident(frames, dev, chunk)
        nh, nw, y1, x1, h, w = working_geometry(H0, W0, self.size)
        lut = ip._device_tables(dev, (ip.MEAN, ip.STD))[0]
        bufs = self._bufs.get((str(dev), h, w))
        if bufs is None:                       # one clip buffer, one zero mask (every frame of a video has one size), the per-batch constants
            bufs = self._bufs[str(dev), h, w] = (torch.empty(B, 3, T, h, w, dtype=torch.float32, device=dev),
                                                 torch.zeros(B, h, w, dtype=torch.bool, device=dev),
                                                 torch.full((B,), T // 2, dtype=torch.int64, device=dev))
        clips, mask, key_pos = bufs
        sizes = torch.tensor([[H0, W0]] * B, dtype=torch.float32).to(dev, non_blocking=True)
        K = self.detector.topk
        f32, i32 = torch.float32, torch.int32
        full = [torch.empty(nb * B, K, 4, dtype=f32, device=dev), torch.empty(nb * B, K, dtype=f32, device=dev), torch.empty(nb * B, K, dtype=i32, device=dev),
                torch.empty(nb * B, K, dtype=i32, device=dev), torch.empty(nb * B, K, dtype=f32, device=dev), torch.empty(nb * B, dtype=i32, device=dev),
                torch.empty(nb * B, dtype=i32, device=dev)]
        A, full_a = self.detector.actors, None
        if A is not None:
            full_a = [torch.empty(nb * B, A, 4, dtype=f32, device=dev), torch.empty(nb * B, A, dtype=f32, device=dev),
                      torch.empty(nb * B, A, dtype=i32, device=dev), torch.empty(nb * B, A, self.class_num, dtype=f32, device=dev),
                      torch.empty(nb * B, dtype=i32, device=dev), torch.empty(nb * B, dtype=i32, device=dev)]
        samples = NestedTensor(clips, mask)
        for b in range(nb):
            lib.call("tuber_video_clips", resident, N, nh, nw, table[b * B:], B, T, y1, x1, h, w, lut, clips)
            det = self.detector(samples, sizes, key_pos)
            for dst, src in zip(full, det.tensors()):
                dst[b * B:(b + 1) * B].copy_(src)
            if full_a is not None:
                for dst, src in zip(full_a, det.actors.tensors()):
                    dst[b * B:(b + 1) * B].copy_(src)
        vd = VideoDetections(keys, *[t[:n] for t in full], class_num=self.class_num, settings=self.settings, store=store, nms_iou=self.nms["iou"])
        if full_a is not None:
            vd.actors = VideoActors(keys, *[t[:n] for t in full_a], settings=self.actor_settings, store=store, nms_iou=self.nms["actors_iou"])
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


class VideoStream:
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
    one line on stderr at construction; ``tubes()`` / ``tracks()`` return every closed tube."""

    def __init__(self, cfg, model, batch=2, stride=None, rule=None, max_chunk=64, score_thr=None, topk=None, actor_thr=None, graphed=True,
                 link=True, actors=None):
        from .config import actor_settings, detect_settings, tube_nms_settings, video_map_settings
        self.cfg, self.model = cfg, model
        if any(v is not None for v in tube_nms_settings(cfg).values()):
            print("[tuber] VideoStream: CONFIG.VAL.TUBE_NMS is ignored: a closed tube's suppressor may still be open, so tube NMS is defined over "
                  "whole videos only (VideoDetector)", file=sys.stderr, flush=True)
        self.batch, self.max_chunk, self.link = int(batch), int(max_chunk), bool(link)
        if self.batch < 1 or self.max_chunk < 1:
            raise ValueError("VideoStream: batch = %r and max_chunk = %r must be >= 1" % (batch, max_chunk))
        if actors is not None and not self.link:
            raise ValueError("VideoStream: actors = %r needs link=True: the actor tracks are link records" % (actors,))
        vm = video_map_settings(cfg)
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
            raise ValueError("VideoStream: rule %r is not one of %s" % (rule, ", ".join(RULES)))
        self.stride = int(stride) if stride is not None else (30 if self.mode == "ava" else 1)
        if self.stride < 1:
            raise ValueError("VideoStream: stride = %r must be >= 1" % (stride,))
        D = cfg.CONFIG.DATA
        self.T, self.rate, self.size, self.class_num = int(D.TEMP_LEN), int(D.FRAME_RATE), int(D.IMG_SIZE), int(D.NUM_CLASSES)
        self.schedule = StreamSchedule(self.T, self.rate, self.rule, self.batch, self.stride, self.max_chunk)
        self.R = self.schedule.R
        K, gap = self.detector.topk, self.settings["max_gap"]
        self._why_host = None
        if K > lib.query("tuber_frame_match_max_dets") or K * (gap + 1) > lib.query("tuber_tube_link_max_active"):
            self._why_host = "%d rows per key frame with max_gap %d: beyond %d rows or %d active tubes" % (
                K, gap, lib.query("tuber_frame_match_max_dets"), lib.query("tuber_tube_link_max_active"))
        self._host_linker, self._said = None, False
        self._bufs = {}                    # (device, H0, W0) -> the buffers of a video size
        self._cur = None                   # the current video's buffers
        self.wrapped = False               # whether a ring slot has been overwritten in the current video
        self._pending = []                 # link records since the last tubes() call; None marks the end of a video
        self._open = {}                    # head -> the rows of an open tube, on the host
        # actor tracks (actors=A): their own pending list and their own open rows; tubes() and tracks() consume neither the other's
        self.tracks_path = None            # "device" or "host" once a push has decided keys
        self._why_host_tracks, self._host_tracker, self._said_tracks = None, None, False
        self._pending_tracks, self._assembler = [], None
        self._video_keys = 0               # keys decided in the current video
        if actors is not None:
            A, st = self.detector.actors, self.actor_settings
            self._assembler = TrackAssembler(A, st["max_gap"], st["window"], st["min_len"], st["label_thr"])
            self._track_bytes = lib.query("tuber_track_stream_state_bytes", A, self.class_num, st["max_gap"], st["window"])
            if A > lib.query("tuber_frame_match_max_dets") or not self._track_bytes:
                self._why_host_tracks = "%d actors per key frame with max_gap %d, window %d and %d classes: beyond %d rows, %d active tracks, window %d or %d classes" % (
                    A, st["max_gap"], st["window"], self.class_num, min(lib.query("tuber_frame_match_max_dets"), lib.query("tuber_track_stream_limits", 0)),
                    lib.query("tuber_tube_link_max_active"), lib.query("tuber_track_stream_limits", 2), lib.query("tuber_track_stream_limits", 1))

    # -- buffers ----------------------------------------------------------------------------------------------------------
    def _buffers(self, dev, H0, W0):
        key = (str(dev), H0, W0)
        b = self._bufs.get(key)
        if b is None:
            nh, nw, y1, x1, h, w = working_geometry(H0, W0, self.size)
            B, T, R = self.batch, self.T, self.R
            b = dict(H0=H0, W0=W0, nh=nh, nw=nw, window=(y1, x1, h, w), same=(nh, nw) == (H0, W0),
                     ring=torch.empty(R + 1, nh, nw, 3, dtype=torch.uint8, device=dev),
                     clips=torch.empty(B, 3, T, h, w, dtype=torch.float32, device=dev), mask=torch.zeros(B, h, w, dtype=torch.bool, device=dev),
                     key_pos=torch.full((B,), T // 2, dtype=torch.int64, device=dev),
                     sizes=torch.tensor([[H0, W0]] * B, dtype=torch.float32).to(dev, non_blocking=True),
                     lut=ip._device_tables(dev, (ip.MEAN, ip.STD))[0],
                     state=torch.zeros(lib.query("tuber_tube_link_state_bytes", self.class_num), dtype=torch.uint8, device=dev))
            if not b["same"]:
                b["coeffs"] = ip._device_coeffs(dev, H0, W0, nh, nw)
                rows = b["coeffs"][4]
                b["tmp"] = torch.empty(self.max_chunk * rows * nw * 3, dtype=torch.uint8, device=dev) if (nw != W0 and nh != H0) else None
            if self.detector.actors is not None and self._why_host_tracks is None:      # the actors' own link state (one class) and the track ring
                b["actor_state"] = torch.zeros(lib.query("tuber_tube_link_state_bytes", 1), dtype=torch.uint8, device=dev)
                b["track_state"] = torch.zeros(self._track_bytes, dtype=torch.uint8, device=dev)
            self._bufs[key] = b
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
            if hi <= lo:
                continue
            if b["same"]:
                b["ring"][slot:slot + hi - lo].copy_(src[lo:hi])
            else:
                (bh, kh, bv, kv), ksh, ksv, y0, rows = b["coeffs"]
                lib.call("tuber_frames_resize", src[lo:hi], b["tmp"], b["ring"][slot:], hi - lo, b["H0"], b["W0"], b["nh"], b["nw"], bh, kh, ksh, bv, kv,
                         ksv, y0, rows)
        if first == 0:
            b["ring"][R].copy_(b["ring"][0])                   # frame 0 in its fixed slot as well
        self.wrapped = self.wrapped or first + m > R

    # -- key frames -------------------------------------------------------------------------------------------------------
    def _run(self, b, full, row, first_ord, n_keys, n_total, full_a=None):
        """one batch: the keys ``first_ord .. first_ord + n_keys - 1`` (the last one repeated up to ``batch``) into rows ``row ..`` of ``full``
        (and of ``full_a``: the six actor fields)"""
        B = self.batch
        lib.call("tuber_video_clips_ring", b["ring"], self.R, b["nh"], b["nw"], first_ord * self.stride, self.stride, n_keys, B, self.T, self.rate,
                 RULES.index(self.rule), n_total, *b["window"], b["lut"], b["clips"])
        det = self.detector(NestedTensor(b["clips"], b["mask"]), b["sizes"], b["key_pos"])
        for dst, src in zip(full, det.tensors()):
            dst[row:row + B].copy_(src)
        if full_a is not None:
            for dst, src in zip(full_a, det.actors.tensors()):
                dst[row:row + B].copy_(src)

    def _result(self, b, full, first_ord, n, store, full_a=None, flush=False):
        """the ``VideoDetections`` of the keys ``first_ord .. first_ord + n - 1`` in the first n rows of ``full``, linked; with ``full_a`` its
        ``.actors`` as well, tracked (``flush``: these are the video's last keys)"""
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
        from .evaluation import ActorTracker, smooth_range
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
        if not self._said_tracks:
            print("[tuber] VideoStream: %s; tracks on the host" % self._why_host_tracks, file=sys.stderr, flush=True)
            self._said_tracks = True
        self.tracks_path = "host"
        if self._host_tracker is None:
            self._host_tracker = ActorTracker(st["link_iou"], st["max_gap"], st["window"])
        host = dict(zip(ACTOR_FIELDS, va._fetch()))
        got = self._host_tracker.push(host["boxes"].reshape(-1, 4), host["actor"].reshape(-1), host["queries"].reshape(-1), host["actions"].reshape(n * A, C), A,
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
        from .evaluation import TubeLinker
        if not self._said:
            print("[tuber] VideoStream: %s; linking on the host" % why, file=sys.stderr, flush=True)
            self._said = True
        if self._host_linker is None:
            self._host_linker = TubeLinker(self.class_num, self.settings["link_iou"], self.settings["max_gap"])
        host = dict(zip(FIELDS, vd._fetch()))
        got = self._host_linker.push(host["boxes"].reshape(-1, 4), host["labels"].reshape(-1), host["scores"].reshape(-1), K)
        vd.row_head = torch.from_numpy(got["row_head"].reshape(n, K).astype(np.int32)).to(dev)
        vd.row_score = torch.from_numpy(got["row_score"].reshape(n, K)).to(dev)
        vd.row_len = torch.from_numpy(got["row_len"].reshape(n, K).astype(np.int32)).to(dev)

    def _empty(self, rows, dev):
        K, f32, i32 = self.detector.topk, torch.float32, torch.int32
        return [torch.empty(rows, K, 4, dtype=f32, device=dev), torch.empty(rows, K, dtype=f32, device=dev), torch.empty(rows, K, dtype=i32, device=dev),
                torch.empty(rows, K, dtype=i32, device=dev), torch.empty(rows, K, dtype=f32, device=dev), torch.empty(rows, dtype=i32, device=dev),
                torch.empty(rows, dtype=i32, device=dev)]

    def _empty_actors(self, rows, dev):
        A = self.detector.actors
        if A is None:
            return None
        f32, i32 = torch.float32, torch.int32
        return [torch.empty(rows, A, 4, dtype=f32, device=dev), torch.empty(rows, A, dtype=f32, device=dev), torch.empty(rows, A, dtype=i32, device=dev),
                torch.empty(rows, A, self.class_num, dtype=f32, device=dev), torch.empty(rows, dtype=i32, device=dev), torch.empty(rows, dtype=i32, device=dev)]

    @torch.no_grad()
    def push(self, frames):
        if self.model.training:
            raise RuntimeError("VideoStream runs an eval forward: call model.eval() first")
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError("VideoStream wants uint8 frames [n, H, W, 3], got %s %s" % (frames.dtype, tuple(frames.shape)))
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
        full = self._empty(total * B, dev) if total else None
        full_a = self._empty_actors(total * B, dev) if total else None
        row = 0
        for i, length, batches in plan:
            src = frames[i:i + length].to(dev, non_blocking=True).contiguous()
            self._store_frames(b, src, first_frame + i)
            for k in batches:
                self._run(b, full, row, k, B, -1, full_a)
                row += B
        return self._result(b, full, first_ord, row, store, full_a) if row else None

    @torch.no_grad()
    def finish(self):
        if self.model.training:
            raise RuntimeError("VideoStream runs an eval forward: call model.eval() first")
        decided = self.schedule.decided
        n_total, batches = self.schedule.finish()
        self.wrapped = False
        if not n_total:
            return None
        b, B = self._cur, self.batch
        store, _ = self.model.engine()
        out = None
        if batches:
            full, full_a = self._empty(len(batches) * B, store.device), self._empty_actors(len(batches) * B, store.device)
            for i, (k, n_keys) in enumerate(batches):
                self._run(b, full, i * B, k, n_keys, n_total, full_a)
            out = self._result(b, full, batches[0][0], batches[-1][0] + batches[-1][1] - batches[0][0], store, full_a, flush=True)
        elif self.detector.actors is not None:                  # no key left to run: the smoothed rows that waited for the end (S = 0, flush)
            out = self._result(b, self._empty(0, store.device), decided, 0, store, self._empty_actors(0, store.device), flush=True)
        b["state"].zero_()
        for k in ("actor_state", "track_state"):
            if k in b:
                b[k].zero_()
        if self._host_linker is not None:
            self._host_linker.reset()
        if self._host_tracker is not None:
            self._host_tracker.reset()
        if self.link:
            self._pending.append(None)
        if self.detector.actors is not None:
            self._pending_tracks.append(None)
            self._video_keys = 0
        return out

    # -- tubes ------------------------------------------------------------------------------------------------------------
    def tubes(self):
        if not self.link:
            raise RuntimeError("VideoStream(link=False) keeps no link records: no tubes")
        pending, self._pending = self._pending, []
        recs = [p for p in pending if p is not None]
        names = ("boxes", "labels", "row_head", "row_score", "row_len")
        parts = [getattr(vd, k).contiguous() for _, vd in recs for k in names]
        host, o = [], 0
        if parts:                                               # one copy for every record
            blob = torch.cat([t.reshape(-1).view(torch.uint8) for t in parts]).cpu().numpy()
            for t in parts:
                nbytes = t.numel() * t.element_size()
                host.append(blob[o:o + nbytes].view(np.dtype(str(t.dtype).replace("torch.", ""))).reshape(tuple(t.shape)))
                o += nbytes
        gap, min_len, out, i = self.settings["max_gap"], self.settings["min_len"], [], 0
        next_ord = None

        def close(everything):
            for h in sorted(self._open):
                t = self._open[h]
                if everything or next_ord - t["last"] > gap + 1:
                    del self._open[h]
                    if t["length"] >= min_len:
                        out.append(dict(cls=t["cls"], score=t["score"], frames=t["frames"], boxes=np.stack(t["boxes"]), length=t["length"], head=h))
        for p in pending:
            if p is None:                                       # the end of a video: whatever is open closes
                close(True)
                next_ord = None
                continue
            first_ord, vd = p
            boxes, labels, head, score, length = host[5 * i:5 * i + 5]
            i += 1
            for s, q in zip(*np.nonzero(head >= 0)):
                h = int(head[s, q])
                t = self._open.get(h)
                if t is None:
                    t = self._open[h] = dict(cls=int(labels[s, q]) + 1, frames=[], boxes=[])
                t["frames"].append(vd.keys[s])
                t["boxes"].append(boxes[s, q].copy())
                t["score"], t["length"], t["last"] = float(score[s, q]), int(length[s, q]), first_ord + int(s)
            next_ord = first_ord + len(vd.keys)
        if next_ord is not None:
            close(False)
        return out

    # -- actor tracks -----------------------------------------------------------------------------------------------------
    TRACK_NAMES = ("boxes", "actor", "queries", "actions", "row_head", "row_score", "row_len", "row_mean", "row_peak", "smooth")

    def tracks(self):
        """The actor tracks (``actors=A``) that CLOSED since the last call: the next key ordinal is more than ``max(max_gap + 1, window)`` past
        their last one -- no key frame still to come can extend them, and the smoothed row of their last key has been emitted -- and after
        ``finish()`` all that remain.  ``VideoActors.tracks``' dicts plus ``head`` (key ordinal * A + position of the first row), in head
        order; ``score`` / ``mean`` / ``peak`` are the records of the track's last row.  One device-to-host copy per call; the rows of open
        tracks are kept on the host in between (``TrackAssembler``).  ``tubes()`` keeps its own records: neither consumes the other's."""
        if self._assembler is None:
            raise RuntimeError("VideoStream without actors=A keeps no actor records: no tracks")
        pending, self._pending_tracks = self._pending_tracks, []
        recs = [p for p in pending if p is not None]
        parts = [getattr(va, k).contiguous() for _, va in recs for k in self.TRACK_NAMES]
        host, o = [], 0
        if parts:                                               # one copy for every record
            blob = torch.cat([t.reshape(-1).view(torch.uint8) for t in parts]).cpu().numpy()
            for t in parts:
                nbytes = t.numel() * t.element_size()
                host.append(blob[o:o + nbytes].view(np.dtype(str(t.dtype).replace("torch.", ""))).reshape(tuple(t.shape)))
                o += nbytes
        out, i, m = [], 0, len(self.TRACK_NAMES)
        for p in pending:
            if p is None:                                       # the end of a video: whatever is open closes
                self._assembler.end()
                out += self._assembler.take()
                continue
            first_ord, va = p
            self._assembler.add(first_ord, va.keys, *host[m * i:m * i + m], va.smooth_first)
            i += 1
        return out + self._assembler.take()


class TrackAssembler:
    """The host side of ``VideoStream.tracks()``: the per-push records of a stream's actors (host arrays) in, closed actor tracks out.
    ``add(first_ord, keys, boxes, actor, queries, actions, row_head, row_score, row_len, row_mean, row_peak, smooth, smooth_first)`` takes the
    records of the keys ``first_ord ..`` ([n, A, ...] arrays; ``smooth`` [m, A, C] belongs to the slots ``smooth_first ..``, which lag
    ``window`` keys behind); ``end()`` marks the end of the video; ``take()`` returns the tracks closed since the last call, in head order: after
    ``end()`` all of them, before it those whose last key lies more than ``max(max_gap + 1, window)`` ordinals behind the next one.  A track
    is ``VideoActors.tracks``' dict plus ``head``; tracks shorter than ``min_len`` are dropped."""

    def __init__(self, A, max_gap, window, min_len=1, label_thr=0.05):
        self.A, self.max_gap, self.window, self.min_len, self.label_thr = int(A), int(max_gap), int(window), int(min_len), float(label_thr)
        self._open, self._waiting, self._closed, self._next = {}, {}, [], 0

    def add(self, first_ord, keys, boxes, actor, queries, actions, row_head, row_score, row_len, row_mean, row_peak, smooth, smooth_first):
        head = np.asarray(row_head)
        for s, a in zip(*np.nonzero(head >= 0)):
            h, o = int(head[s, a]), int(first_ord) + int(s)
            t = self._open.get(h)
            if t is None:
                t = self._open[h] = dict(frames=[], boxes=[], actor=[], queries=[], actions=[], smooth=[])
            t["frames"].append(int(keys[s]))
            for k, src in (("boxes", boxes), ("actor", actor), ("queries", queries), ("actions", actions)):
                t[k].append(np.array(src[s, a]))
            t["score"], t["length"], t["last"] = float(row_score[s, a]), int(row_len[s, a]), o
            t["mean"], t["peak"] = np.array(row_mean[s, a], dtype=np.float64), np.array(row_peak[s, a], dtype=np.float32)
            self._waiting.setdefault(o, []).append((int(a), h))           # the row's smoothed scores come `window` keys later
        for j in range(len(smooth)):                                      # slots in order: a track's smoothed rows arrive in slot order
            for a, h in self._waiting.pop(int(smooth_first) + j, []):
                self._open[h]["smooth"].append(np.array(smooth[j, a], dtype=np.float64))
        self._next = int(first_ord) + len(keys)
        self._close(False)

    def end(self):
        self._close(True)
        self._waiting, self._next = {}, 0

    def _close(self, everything):
        for h in sorted(self._open):
            t = self._open[h]
            if not (everything or self._next - t["last"] > max(self.max_gap + 1, self.window)):
                continue
            del self._open[h]
            if t["length"] < self.min_len:
                continue
            if len(t["smooth"]) != len(t["frames"]):
                raise RuntimeError("TrackAssembler: track %d closes with %d of its %d smoothed rows" % (h, len(t["smooth"]), len(t["frames"])))
            mean = t["mean"]
            with np.errstate(invalid="ignore"):
                labels = sorted(np.nonzero(mean >= self.label_thr)[0].tolist(), key=lambda c: (-mean[c], c))
            self._closed.append(dict(score=t["score"], frames=t["frames"], boxes=np.stack(t["boxes"]), actor=np.stack(t["actor"]),
                                     queries=np.stack(t["queries"]), actions=np.stack(t["actions"]), smooth=np.stack(t["smooth"]), mean=mean,
                                     peak=t["peak"], labels=labels, length=t["length"], head=h))

    def take(self):
        out, self._closed = sorted(self._closed, key=lambda t: t["head"]), []
        return out
