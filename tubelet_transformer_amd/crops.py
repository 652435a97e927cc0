"""Crops of action tubes and actor tracks out of the video.

``tubes(dense=True)`` / ``tracks(dense=True)`` put a box on every frame of a tube; this module cuts those boxes out of the frames and resamples
them to one size, so that a second network (re-identification, pose, a per-actor classifier) can consume "person 3, frames 120-410" without the
video leaving the device.  ``crop_values`` / ``crop_rows`` (plain numpy, fp64) are the definition and the host path; ``tuber_tube_crops``
(csrc/tube_crops.hip) restates it on the device and is held to its bytes; ``tube_crops`` is the entry both ``VideoDetections.crops`` and a
caller with frames of their own go through.

The resampling is RoIAlign's: the box, enlarged by ``scale`` about its centre, is divided into ``h x w`` bins, every bin is the mean of an
``s x s`` regular grid of bilinear samples (``samples``, RoIAlign's ``sampling_ratio``), and a sample position outside the frame is clamped to
it (edge replication: ``grid_sample(padding_mode="border", align_corners=False)``).  Coordinates are continuous, pixel ``j`` covers
``[j, j + 1)``."""
import sys

import numpy as np
import torch

from . import lib

MAX_SAMPLES = 4


def _checked(frames, frame_index, boxes, size, source_size, scale, samples):
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3 or frames.shape[1] < 1 or frames.shape[2] < 1:
        raise ValueError("crops: frames must be uint8 [N, H, W, 3] with H, W >= 1, got %s %s" % (frames.dtype, frames.shape))
    frame_index = np.asarray(frame_index).reshape(-1).astype(np.int64)
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    if len(frame_index) != len(boxes):
        raise ValueError("crops: %d frame indices, %d boxes" % (len(frame_index), len(boxes)))
    h, w = (int(v) for v in size)
    H, W = frames.shape[1:3]
    H0, W0 = (H, W) if source_size is None else (int(v) for v in source_size)
    scale = float(scale)
    if h < 1 or w < 1 or H0 < 1 or W0 < 1:
        raise ValueError("crops: size = %r and source_size = %r must be >= 1" % (tuple(size), source_size))
    if not (scale > 0.0 and np.isfinite(scale)):
        raise ValueError("crops: scale = %r must be a finite number > 0" % (scale,))
    if isinstance(samples, bool) or int(samples) != samples or not 1 <= int(samples) <= MAX_SAMPLES:
        raise ValueError("crops: samples = %r must be an integer in 1 .. %d" % (samples, MAX_SAMPLES))
    return frames, frame_index, boxes, (h, w), (H0, W0), scale, int(samples)


def _axis(lo, hi, size, size0, n, s, scale):
    """the ``n * s`` sample positions of one axis: (first pixel, second pixel, weight of the second), every fp64 operation rounded on its own"""
    f = np.float64(size) / np.float64(size0)
    c = (np.float64(lo) + np.float64(hi)) * 0.5
    b = (np.float64(hi) - np.float64(lo)) * np.float64(scale)
    origin = (c - b * 0.5) * f
    step = (b * f) / np.float64(n * s)
    with np.errstate(invalid="ignore"):
        u = origin + (np.arange(n * s, dtype=np.float64) + 0.5) * step - 0.5
        u = np.where(u > 0.0, u, 0.0)                                     # max(u, 0); a NaN (an overflowing scale) is 0 as well
        u = np.where(u < np.float64(size - 1), u, np.float64(size - 1))
    i0 = np.floor(u).astype(np.int64)
    return i0, np.minimum(i0 + 1, size - 1), u - i0


def _row_values(frame, box, size, source_size, scale, s):
    """one valid row of ``crop_values``: float64 [h, w, 3]"""
    h, w = size
    H, W = frame.shape[:2]
    with np.errstate(over="ignore"):
        j0, j1, a = _axis(box[0], box[2], W, source_size[1], w, s, scale)
        i0, i1, b = _axis(box[1], box[3], H, source_size[0], h, s, scale)
    a, b = a[None, :, None], b[:, None, None]
    p0, p1 = frame[i0].astype(np.float64), frame[i1].astype(np.float64)   # the source lines of every sample line
    top = p0[:, j0] + (p0[:, j1] - p0[:, j0]) * a
    bot = p1[:, j0] + (p1[:, j1] - p1[:, j0]) * a
    val = (top + (bot - top) * b).reshape(h, s, w, s, 3)
    acc = np.zeros((h, w, 3), dtype=np.float64)
    for dy in range(s):
        for dx in range(s):
            acc = acc + val[:, dy, :, dx]
    return acc / np.float64(s * s)


def _valid(frame_index, boxes, N):
    return ((frame_index >= 0) & (frame_index < N) & np.isfinite(boxes).all(axis=1)).astype(np.uint8)


def crop_values(frames, frame_index, boxes, size, source_size=None, scale=1.0, samples=1):
    """The definition of a crop (and of ``tuber_tube_crops``): ``(values float64 [R, h, w, 3], valid uint8 [R])``.

    ``frames`` uint8 [N, H, W, 3]; row r cuts ``boxes[r]`` (fp32 xyxy in source-video pixels, pixel j covering [j, j + 1)) out of frame
    ``frame_index[r]`` and resamples it to ``size = (h, w)``.  ``source_size = (H0, W0)``: the resolution the boxes refer to, by default the
    frames' own; it differs when ``frames`` is a video held at working resolution.  ``scale`` > 0 enlarges the box about its centre;
    ``samples = s`` in 1 .. 4: every output pixel is the mean of an s x s regular grid of bilinear samples (1: plain bilinear).  Per axis, all
    in fp64, every operation rounded on its own (x shown; y alike with H, H0, h, y1, y2)::

        fx = float64(W) / float64(W0)
        cx = (x1 + x2) * 0.5          bw = (x2 - x1) * scale
        X1 = (cx - bw * 0.5) * fx     sx = (bw * fx) / float64(w * s)
        sample column c in [0, w*s):   u = X1 + (c + 0.5) * sx - 0.5;  u = min(max(u, 0), W - 1)
                                       j0 = floor(u); j1 = min(j0 + 1, W - 1); a = u - j0
        per channel:  top = p[i0,j0] + (p[i0,j1] - p[i0,j0]) * a;  bot likewise on line i1;  val = top + (bot - top) * b
        output (i, j): acc = 0; for dy: for dx: acc = acc + val(i*s + dy, j*s + dx);  value = acc / float64(s * s)

    The clamp is edge replication.  A box with x2 < x1 gives a mirrored crop and one without area a constant: the formula decides.  A row whose
    ``frame_index`` lies outside [0, N) or whose box has a coordinate that is not finite is all zeros with ``valid`` 0."""
    frames, frame_index, boxes, size, source_size, scale, s = _checked(frames, frame_index, boxes, size, source_size, scale, samples)
    valid = _valid(frame_index, boxes, len(frames))
    out = np.zeros((len(boxes),) + size + (3,), dtype=np.float64)
    for r in np.nonzero(valid)[0].tolist():
        out[r] = _row_values(frames[frame_index[r]], boxes[r], size, source_size, scale, s)
    return out, valid


def crop_rows(frames, frame_index, boxes, size, source_size=None, scale=1.0, samples=1):
    """``crop_values`` as pixels: ``(uint8 [R, h, w, 3], valid uint8 [R])`` with ``byte = floor(value + 0.5)`` -- what ``tuber_tube_crops``
    writes, byte for byte.  Rows are rounded one at a time, so the fp64 values of a long table are never all resident."""
    frames, frame_index, boxes, size, source_size, scale, s = _checked(frames, frame_index, boxes, size, source_size, scale, samples)
    valid = _valid(frame_index, boxes, len(frames))
    out = np.zeros((len(boxes),) + size + (3,), dtype=np.uint8)
    for r in np.nonzero(valid)[0].tolist():
        out[r] = np.floor(_row_values(frames[frame_index[r]], boxes[r], size, source_size, scale, s) + 0.5).astype(np.uint8)
    return out, valid


def crop_table(tubes):
    """The crop table of a list of tubes or tracks -- the dicts ``tubes()`` / ``tracks()`` return, dense or not: ``(frame_index int32 [R], boxes
    fp32 [R, 4], offsets int64 [len(tubes) + 1])``, a row per entry of a tube's ``frames`` / ``boxes`` in order; tube i owns the rows
    ``offsets[i] .. offsets[i + 1] - 1``."""
    index, boxes, offsets = [], [], [0]
    for i, t in enumerate(tubes):
        f = np.asarray(t["frames"], dtype=np.int64).reshape(-1)
        b = np.asarray(t["boxes"], dtype=np.float32).reshape(-1, 4)
        if len(f) != len(b):
            raise ValueError("crop_table: tube %d has %d frames and %d boxes" % (i, len(f), len(b)))
        if len(f) and (f.min() < -2 ** 31 or f.max() >= 2 ** 31):
            raise ValueError("crop_table: tube %d has a frame number beyond 32 bits" % i)
        index.append(f.astype(np.int32))
        boxes.append(b)
        offsets.append(offsets[-1] + len(f))
    return (np.concatenate(index) if index else np.zeros(0, dtype=np.int32), np.concatenate(boxes) if boxes else np.zeros((0, 4), dtype=np.float32),
            np.asarray(offsets, dtype=np.int64))


def normalized(pixels, lut):
    """uint8 [R, h, w, 3] through the mean/std table ``lut`` fp32 [3, 256] (``input_pipeline.normalize_lut``) -> fp32 [R, 3, h, w]: what
    ``tuber_tube_crops`` writes when it is given the table"""
    return np.stack([lut[c][pixels[..., c]] for c in range(3)], axis=1).astype(np.float32)


class TubeCrops:
    """The crops of a list of tubes: ``pixels`` uint8 [R, h, w, 3] (``normalize=True``: fp32 [R, 3, h, w]) and ``valid`` uint8 [R] -- tensors on
    the device of the frames -- ``offsets`` int64 [len + 1] (host) and ``path``, "device" or "host".  ``crops[i]`` is the view of tube i's
    rows, one per entry of its ``frames``; ``len(crops)`` the number of tubes."""

    def __init__(self, pixels, valid, offsets, path):
        self.pixels, self.valid, self.offsets, self.path = pixels, valid, np.asarray(offsets, dtype=np.int64), path

    def __len__(self):
        return len(self.offsets) - 1

    def __getitem__(self, i):
        i = range(len(self))[i]                                           # negative indices; an IndexError beyond the tubes
        return self.pixels[int(self.offsets[i]):int(self.offsets[i + 1])]

    def to_host(self):
        """``(pixels, valid)`` as numpy arrays, in ONE device-to-host copy: the place that synchronises"""
        from .detect import host_parts
        pixels, valid = host_parts([self.pixels, self.valid])
        return pixels, valid


def crops_beyond(H, W, size, samples):
    """why ``tuber_tube_crops`` cannot take frames of width W resampled to ``size`` with ``samples``, or None"""
    max_w, max_out, max_s = (lib.query("tuber_tube_crops_limits", k) for k in range(3))
    if W > max_w or max(size) > max_out or samples > max_s:
        return "frames %d wide resampled to %d x %d with %d samples: beyond a width of %d, a crop side of %d or %d samples" % (
            W, size[0], size[1], samples, max_w, max_out, max_s)
    return None


def tube_crops(frames, tubes, size, source_size=None, scale=1.0, samples=1, normalize=False):
    """The crops of ``tubes`` (the dicts of ``tubes()`` / ``tracks()``, dense or not) out of ``frames`` -> ``TubeCrops``.

    ``frames``: uint8 [N, H, W, 3], a tensor or numpy.  ``size`` / ``source_size`` / ``scale`` / ``samples``: as ``crop_values``.
    ``normalize``: fp32 [R, 3, h, w] through the mean/std table of the clips (``input_pipeline.normalize_lut``) instead of uint8
    [R, h, w, 3] -- a crop pixel is then what a clip pixel of the same byte is, ready for a second network.  Frames on the device:
    ``crop_table`` on the host, ONE upload of the table, ONE ``tuber_tube_crops`` launch, no synchronisation.  Frames on the CPU, or sizes
    beyond ``tuber_tube_crops_limits``: ``crop_rows`` on the host, one line on stderr says why, and ``path`` is "host" instead of "device"."""
    from . import input_pipeline as ip
    if isinstance(frames, np.ndarray):
        frames = torch.from_numpy(np.ascontiguousarray(frames))
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[1] < 1 or frames.shape[2] < 1:
        raise ValueError("tube_crops wants uint8 frames [N, H, W, 3], got %s %s" % (frames.dtype, tuple(frames.shape)))
    index, boxes, offsets = crop_table(tubes)
    N, H, W = (int(v) for v in frames.shape[:3])
    _, _, _, size, source_size, scale, samples = _checked(np.zeros((0, H, W, 3), np.uint8), index, boxes, size, source_size, scale, samples)
    R, (h, w) = len(index), size
    why = "the frames are on the CPU" if frames.device.type != "cuda" else crops_beyond(H, W, size, samples)
    if why:
        print("[tuber] tube_crops: %s; crops on the host" % why, file=sys.stderr, flush=True)
        pixels, valid = crop_rows(frames.cpu().numpy(), index, boxes, size, source_size, scale, samples)
        if normalize:
            pixels = normalized(pixels, ip.normalize_lut())
        return TubeCrops(torch.from_numpy(pixels).to(frames.device), torch.from_numpy(valid).to(frames.device), offsets, "host")
    dev = frames.device
    pixels = torch.empty((R, 3, h, w) if normalize else (R, h, w, 3), dtype=torch.float32 if normalize else torch.uint8, device=dev)
    valid = torch.empty(R, dtype=torch.uint8, device=dev)
    if R:
        table = np.empty(R * 20, dtype=np.uint8)                          # the boxes (16-byte aligned) and, behind them, the frame numbers
        table[:R * 16] = boxes.reshape(-1).view(np.uint8)
        table[R * 16:] = index.view(np.uint8)
        table = torch.from_numpy(table).to(dev, non_blocking=True)
        lut = ip._device_tables(dev, (ip.MEAN, ip.STD))[0] if normalize else None
        lib.call("tuber_tube_crops", frames.contiguous(), N, H, W, table[R * 16:], table, R, h, w, float(np.float64(W) / np.float64(source_size[1])),
                 float(np.float64(H) / np.float64(source_size[0])), scale, samples, lut, pixels, valid)
    return TubeCrops(pixels, valid, offsets, "device")
