"""Whole-video inference on the GPU (tubelet_transformer_amd/video.py): ``tuber_video_clips`` (csrc/video_clips.hip) against the
numpy gather it is defined by, ``tuber_tube_link_ranked`` (csrc/tube_map.hip) against ``evaluation.link_rows`` -- its definition -- and against
``tuber_tube_link`` on rows derived by arg-max, the linker's bounds and the host fallback of ``VideoDetections.tubes``, and ``VideoDetector`` end
to end on the name-hashed models of tests/test_detect_gpu.py against the same batches assembled in numpy.  Everything compared here is exact:
the gather moves table entries, the linker's sums are sequential fp64 in slot order, and a replayed forward on identical input bits is
deterministic."""
import os

import numpy as np
import pytest
import torch

from tubelet_transformer_amd import input_pipeline as ip
from tubelet_transformer_amd import lib, synth
from tubelet_transformer_amd.config import load_cfg
from tubelet_transformer_amd.detect import FIELDS, Detector
from tubelet_transformer_amd.evaluation import _iou_one_to_many, link_rows
from tubelet_transformer_amd.misc import NestedTensor
from tubelet_transformer_amd.tuber import build_model
from tubelet_transformer_amd.video import VideoDetections, VideoDetector, clip_indices, working_geometry

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


# ------------------------------------------------------------------------------------------------------------------------------
# tuber_video_clips
# ------------------------------------------------------------------------------------------------------------------------------
def _gather(frames, index, window, lut):
    """out[b][c][t][y][x] = lut[c][frames[clamp(index[b][t])][y1 + y][x1 + x][c]], in numpy"""
    y1, x1, h, w = window
    f = frames[np.clip(index, 0, len(frames) - 1)][:, :, y1:y1 + h, x1:x1 + w, :]           # [B, T, h, w, 3]
    return np.stack([lut[c][f[..., c]] for c in range(3)], axis=1).astype(np.float32)       # [B, 3, T, h, w]


CLIP_SHAPES = {
    "scalar_5x7_full": dict(n=7, H=5, W=7, window=(0, 0, 5, 7)),            # frames of 105 B: every second frame and every row misaligned
    "vector_6x12_crop": dict(n=7, H=6, W=12, window=(1, 2, 4, 8)),          # w % 4 == 0: dword loads, 16-byte stores, a crop
}


@pytest.mark.parametrize("offset", (0, 1, 3))
@pytest.mark.parametrize("shape", sorted(CLIP_SHAPES))
def test_video_clips_equals_the_numpy_gather(dev, shape, offset):
    s = CLIP_SHAPES[shape]
    n, H, W, window = s["n"], s["H"], s["W"], s["window"]
    B, T = 3, 4
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    index = np.array([[2, 2, 3, 3], [6, 5, 4, 3], [-1, 0, n - 1, n]], dtype=np.int32)        # repeats, a descending run, -1 and n (clamped)
    lut = ip.normalize_lut()
    want = _gather(frames, index, window, lut)
    buf = torch.zeros(offset + frames.size, dtype=torch.uint8, device=dev)                   # the video at any byte alignment
    buf[offset:].copy_(torch.from_numpy(frames).reshape(-1))
    out = torch.full((B, 3, T) + window[2:], 7.0, dtype=torch.float32, device=dev)
    lib.call("tuber_video_clips", buf[offset:], n, H, W, torch.from_numpy(index).to(dev), B, T, *window, torch.from_numpy(lut).to(dev), out)
    assert np.array_equal(out.cpu().numpy(), want)


def test_video_clips_refuses_bad_arguments_and_writes_nothing(dev):
    n, H, W, B, T = 7, 6, 12, 3, 4
    frames = torch.zeros(n, H, W, 3, dtype=torch.uint8, device=dev)
    index = torch.zeros(B, T, dtype=torch.int32, device=dev)
    lut = torch.from_numpy(ip.normalize_lut()).to(dev)
    out = torch.full((B, 3, T, H, W), 7.0, dtype=torch.float32, device=dev)
    ok = dict(frames=frames, nframes=n, H=H, W=W, index=index, B=B, T=T, y1=0, x1=0, h=H, w=W, lut=lut, out=out)
    rc = lambda **kw: lib.call_rc("tuber_video_clips", *{**ok, **kw}.values())
    for name in ("frames", "index", "lut", "out"):
        assert rc(**{name: None}) == EINVAL, name
    for name in ("nframes", "H", "W", "B", "T", "h", "w"):
        assert rc(**{name: 0}) == EINVAL and rc(**{name: -1}) == EINVAL, name
    for kw in (dict(y1=-1), dict(x1=-1), dict(y1=1), dict(x1=1), dict(y1=3, h=4), dict(x1=8, w=8), dict(h=H + 1), dict(w=W + 1)):
        assert rc(**kw) == EINVAL, kw                                   # a window outside H x W
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                     # untouched
    assert rc() == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())


# ------------------------------------------------------------------------------------------------------------------------------
# tuber_tube_link_ranked
# ------------------------------------------------------------------------------------------------------------------------------
LINK_IOU = 0.25
A = (0, 0, 10, 10)
PAD = ((0, 0, 0, 0), -1, 0.0)


def ranked_fixture():
    """S = 6 slots of K = 4 rows, C = 3, two videos (slots 0-3 and 4-5), max_gap = 1: (box, label, score) per row, PAD = a row behind a key's count"""
    nan = float("nan")
    slots = [
        [(A, 0, 0.8), ((100, 0, 110, 10), 0, 0.8), (A, 1, 0.7), PAD],                   # two tubes of class 0 with equal means (0.8)
        [PAD, PAD, PAD, PAD],                                                           # an empty slot, inside the gap of both
        [((6, 0, 16, 10), 0, 0.6),                                                      # IoU with A exactly 0.25 = LINK_IOU: linked
         ((101, 0, 111, 10), 0, 0.5), ((99, 0, 109, 10), 0, 0.5),                       # two equal scores for one tube: it takes the first
         ((2, 0, 12, 10), 0, nan)],                                                     # a NaN score: not counted
        [(A, 1, 0.9),                                                                   # class 1 again after two slots without it: beyond the gap
         ((5, 0, 5, 10), 0, 0.9),                                                       # x1 >= x2: not counted
         ((7, 0, 17, 10), 0, 0.7), PAD],
        [(A, 2, 0.6), ((2, 0, 12, 10), 2, 0.9), PAD, PAD],
        [((1, 0, 11, 10), 2, 0.7), ((3, 0, 13, 10), 2, 0.7), (A, 5, 0.9), PAD],         # equal scores again; a label >= C
    ]
    box = np.array([r[0] for s in slots for r in s], dtype=np.float32)
    label = np.array([r[1] for s in slots for r in s], dtype=np.int32)
    score = np.array([r[2] for s in slots for r in s], dtype=np.float32)
    return dict(box=box, label=label, score=score, S=6, K=4, C=3, max_gap=1, video_off=np.array([0, 4, 6], dtype=np.int32))


def _link_outputs(N, dev, fill=None):
    out = dict(row_cls=torch.empty(N, dtype=torch.int32, device=dev), row_head=torch.empty(N, dtype=torch.int32, device=dev),
               tube_score=torch.zeros(N, dtype=torch.float64, device=dev), tube_len=torch.zeros(N, dtype=torch.int32, device=dev),
               tube_last=torch.full((N,), -1, dtype=torch.int32, device=dev))
    if fill is not None:
        for t in out.values():
            t.fill_(fill)
    return out


def _ranked(fx, dev, max_gap=None, out=None, K=None):
    K = fx["K"] if K is None else K
    N = len(fx["label"])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = _link_outputs(N, dev) if out is None else out
    slot_off = up((np.arange(fx["S"] + 1) * K).astype(np.int32))
    code = lib.call_rc("tuber_tube_link_ranked", up(fx["box"]), up(fx["label"]), up(fx["score"]), slot_off, up(fx["video_off"]), len(fx["video_off"]) - 1,
                       fx["S"], N, fx["C"], K, LINK_IOU, fx["max_gap"] if max_gap is None else max_gap, out["row_cls"], out["row_head"],
                       out["tube_score"], out["tube_len"], out["tube_last"])
    torch.cuda.synchronize()
    return code, {k: v.cpu().numpy() for k, v in out.items()}


def test_tube_link_ranked_equals_the_host_definition(dev):
    fx = ranked_fixture()
    box, label, score, K, C = fx["box"], fx["label"], fx["score"], fx["K"], fx["C"]
    slot = np.repeat(np.arange(fx["S"]), K)
    want = link_rows(box, label, score, slot, fx["video_off"], C, LINK_IOU, fx["max_gap"])
    # before the launch: the fixture holds what it is there for
    head = want["row_head"]
    assert label[0] == label[1] and score[0] == score[1] and head[0] == 0 and head[1] == 1 and slot[0] == slot[1]       # equal scores in a slot ...
    assert want["tube_len"][0] >= 2 and want["tube_len"][1] >= 2                    # ... of two tubes whose means were equal when slot 2 was linked
    assert score[9] == score[10] and head[9] == 1 and head[10] == 10                # equal scores for one tube: the first row, the other starts a tube
    assert (label[4:8] == -1).all() and head[8] == 0 and slot[8] - slot[0] == 2      # an empty slot inside the gap: bridged
    assert label[2] == label[12] == 1 and not (label[4:12] == 1).any() and slot[12] - slot[2] == 3 and head[12] == 12      # ... and beyond it: a new tube
    assert (label == -1).sum() == 9 and (head[label == -1] == -1).all() and head[22] == -1 and label[22] >= C
    assert np.isnan(score[11]) and head[11] == -1
    assert box[13, 0] >= box[13, 2] and head[13] == -1
    assert _iou_one_to_many(box[0].astype(np.float64), box[8:9].astype(np.float64))[0] == LINK_IOU      # exactly the threshold: linked
    assert head[14] == 0 and want["tube_len"][0] == 3 and want["tube_last"][0] == 3
    assert head[20] == 17 and head[21] == 16                                         # the better tube picks first, and the first of the equal scores
    code, got = _ranked(fx, dev)
    assert code == 0
    for k in ("row_head", "tube_len", "tube_last"):
        assert np.array_equal(got[k].astype(np.int64), want[k]), k
    assert np.array_equal(got["tube_score"].view(np.int64), want["tube_score"].view(np.int64))
    assert got["row_cls"].tolist() == [l if 0 <= l < C else C for l in label.tolist()]


def test_tube_link_ranked_equals_tube_link_on_arg_max_rows(dev):
    rng = np.random.default_rng(5)
    C, S, max_gap = 4, 9, 2
    rows_per = rng.integers(0, 7, S)
    rows_per[3] = 0
    N = int(rows_per.sum())
    anchors = np.array([[10, 10, 50, 60], [30, 15, 70, 65], [100, 20, 140, 80]], dtype=np.float32)
    box = anchors[rng.integers(3, size=N)] + rng.integers(-6, 7, (N, 4)).astype(np.float32)
    prob = (rng.integers(1, 10, (N, C + 1)) / 10.0).astype(np.float32)                      # a lattice: ties between columns and rows
    prob[2, 1] = np.nan
    prob[5] = [0.1, 0.1, 0.1, 0.1, 0.9]                                                     # no-object on top
    label = prob.argmax(axis=1)
    score = prob[np.arange(N), label]
    assert np.isnan(score).any() and (label == C).any() and len(set(score[~np.isnan(score)].tolist())) < N - 1
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    slot_off, video_off = up(np.concatenate([[0], np.cumsum(rows_per)]).astype(np.int32)), up(np.array([0, 5, S], dtype=np.int32))
    a, b = _link_outputs(N, dev), _link_outputs(N, dev)
    lib.call("tuber_tube_link", up(box), up(prob), slot_off, video_off, 2, S, N, C, int(rows_per.max()), 0.2, max_gap, a["row_cls"], a["row_head"],
             a["tube_score"], a["tube_len"], a["tube_last"])
    lib.call("tuber_tube_link_ranked", up(box), up(label.astype(np.int32)), up(score), slot_off, video_off, 2, S, N, C, int(rows_per.max()), 0.2, max_gap,
             b["row_cls"], b["row_head"], b["tube_score"], b["tube_len"], b["tube_last"])
    torch.cuda.synchronize()
    assert int((a["row_head"] >= 0).sum()) > 10 and int(a["tube_len"].max()) >= 3
    for k in a:
        assert torch.equal(a[k].view(torch.int64) if k == "tube_score" else a[k], b[k].view(torch.int64) if k == "tube_score" else b[k]), k


def _store(fx, dev, K=None):
    K = fx["K"] if K is None else K
    S = fx["S"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    label = fx["label"].reshape(S, K)
    count = t((label >= 0).sum(1).astype(np.int32))
    return VideoDetections([10 * s for s in range(S)], t(fx["box"].reshape(S, K, 4)), t(fx["score"].reshape(S, K)), t(label),
                           t(np.where(label >= 0, 0, -1).astype(np.int32)), t(np.zeros((S, K), np.float32)), count, count.clone(), class_num=fx["C"])


def _same_tubes(a, b):
    assert [(t["cls"], t["frames"], t["length"]) for t in a] == [(t["cls"], t["frames"], t["length"]) for t in b]
    assert [np.float64(t["score"]).view(np.int64) for t in a] == [np.float64(t["score"]).view(np.int64) for t in b]
    assert all(np.array_equal(x["boxes"], y["boxes"]) for x, y in zip(a, b))


def test_beyond_the_linkers_bounds_the_entry_refuses_and_tubes_answers_on_the_host(dev, capsys):
    assert lib.query("tuber_tube_link_max_active") == 64
    fx = ranked_fixture()
    # the same rows as S = 1 slot-pairs of K = 33: 33 * (1 + 1) = 66 active tubes
    wide = dict(fx, S=1, K=33, video_off=np.array([0, 1], dtype=np.int32), box=np.resize(fx["box"], (33, 4)), label=np.resize(fx["label"], 33),
                score=np.resize(fx["score"], 33))
    out = _link_outputs(33, dev, fill=7)
    code, got = _ranked(wide, dev, out=out)
    assert code == EINVAL and all((v == 7).all() for v in got.values())            # refused, nothing written
    assert _ranked(wide, dev, max_gap=0)[0] == 0                                    # 33 rows alone are within the bounds
    assert _ranked(fx, dev, max_gap=16)[0] == EINVAL                                # 4 * 17 = 68
    # VideoDetections: within the bounds on the device, beyond them on the host, the same tubes as a CPU copy of the store gives
    vd = _store(fx, dev)
    on_device = vd.tubes(link_iou=LINK_IOU, max_gap=1)
    assert vd.tubes_path == "device" and capsys.readouterr().err == ""
    cpu = _store(fx, torch.device("cpu"))
    _same_tubes(on_device, cpu.tubes(link_iou=LINK_IOU, max_gap=1))
    assert [(t["cls"], t["frames"]) for t in on_device][:3] == [(1, [0, 20, 30]), (1, [0, 20]), (2, [0])]
    capsys.readouterr()
    beyond = vd.tubes(link_iou=LINK_IOU, max_gap=16)
    assert vd.tubes_path == "host" and "linking on the host" in capsys.readouterr().err
    _same_tubes(beyond, cpu.tubes(link_iou=LINK_IOU, max_gap=16))


# ------------------------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------------------------
H0, W0, NFRAMES, SIZE = 96, 160, 40, 48                                  # working resolution 48 x 80
KEYS = [0, 9, 20, 31, 39]                                               # both ends; batch = 2: three batches, the last one padded
# The name-hashed weights are no detector (tests/test_detect_gpu.py): the AVA model's actor probabilities sit near 0.125 and the JHMDB model puts
# no-object on top of every row.  Everything compared here is bit for bit, so no decision has to be separated: the AVA gate and both score
# thresholds are 0 (every (query, class) of every key frame is a candidate, the best K kept), and the JHMDB test lowers the no-object bias by 2 for
# its duration, as test_detect_gpu does.
SETTINGS = {"ava": dict(actor_thr=0.0, score_thr=0.0, topk=8), "jhmdb": dict(actor_thr=0.0, score_thr=0.0, topk=4)}
CONFIGS = {"ava": "TubeR_CSN50_AVA21.yaml", "jhmdb": "Tuber_CSN152_JHMDB.yaml"}


def _model(name):
    cfg = load_cfg(os.path.join(ROOT, "configuration", name))
    cfg.CONFIG.DATA.IMG_SIZE = SIZE
    model, _, _ = build_model(cfg)
    synth.load_name_hashed(model)
    model.to(torch.device("cuda:0")).eval()
    return cfg, model


def _count_syncs(monkeypatch, fn):
    """``fn()`` with every host read or wait counted: Tensor.cpu / .item / .tolist / .numpy, torch.cuda.synchronize, stream and event waits"""
    seen = []

    def counted(owner, name):
        real = getattr(owner, name)

        def wrapper(*args, **kwargs):
            seen.append(name)
            return real(*args, **kwargs)
        monkeypatch.setattr(owner, name, wrapper)
    for name in ("cpu", "item", "tolist", "numpy"):
        counted(torch.Tensor, name)
    counted(torch.cuda, "synchronize")
    counted(torch.cuda.Stream, "synchronize")
    counted(torch.cuda.Event, "synchronize")
    try:
        return fn(), seen
    finally:
        monkeypatch.undo()


def _launches(fn):
    seen = []
    lib.set_launch_hook(lambda name, args, launch: (seen.append(name), launch(name, *args))[1])
    try:
        return fn(), seen
    finally:
        lib.set_launch_hook(None)


@pytest.mark.parametrize("which", ("ava", "jhmdb"))
def test_video_detector_equals_the_batches_assembled_in_numpy(dev, which, monkeypatch):
    cfg, model = _model(CONFIGS[which])
    model.engine()
    bias = model.class_fc.bias.data
    saved = bias.clone()
    if which == "jhmdb":
        bias[-1] -= 2.0
    try:
        _end_to_end(dev, which, cfg, model, monkeypatch)
    finally:
        bias.copy_(saved)


def _end_to_end(dev, which, cfg, model, monkeypatch):
    kw = SETTINGS[which]
    T, rate = cfg.CONFIG.DATA.TEMP_LEN, cfg.CONFIG.DATA.FRAME_RATE
    frames = np.random.default_rng(11).integers(0, 256, (NFRAMES, H0, W0, 3), dtype=np.uint8)
    nh, nw, y1, x1, h, w = working_geometry(H0, W0, SIZE)
    assert (nh, nw, y1, x1, h, w) == (48, 80, 0, 0, 48, 80)
    # the expected result: every frame resized once, the batches (the padded last one included) gathered in numpy, the same Detector settings
    src = torch.from_numpy(frames).to(dev)
    (bh, kh, bv, kv), ksh, ksv, y0, rows = ip._device_coeffs(dev, H0, W0, nh, nw)
    small = torch.empty(NFRAMES, nh, nw, 3, dtype=torch.uint8, device=dev)
    tmp = torch.empty(NFRAMES * rows * nw * 3, dtype=torch.uint8, device=dev)
    lib.call("tuber_frames_resize", src, tmp, small, NFRAMES, H0, W0, nh, nw, bh, kh, ksh, bv, kv, ksv, y0, rows)
    small = small.cpu().numpy()
    rule = "ava" if which == "ava" else "jhmdb"
    index = clip_indices(NFRAMES, KEYS + [KEYS[-1]], T, rate, rule)
    assert index.shape == (6, T) and index.min() == 0 and index.max() == NFRAMES - 1
    clips = _gather(small, index, (y1, x1, h, w), ip.normalize_lut())
    det = Detector(cfg, model, **kw)
    want = {k: [] for k in FIELDS}
    mask = torch.zeros(2, h, w, dtype=torch.bool, device=dev)
    for b in range(3):
        d = det(NestedTensor(torch.from_numpy(clips[2 * b:2 * b + 2]).to(dev), mask), [[H0, W0]] * 2, [T // 2] * 2)
        for k, t in zip(FIELDS, d.tensors()):
            want[k].append(t.clone())
    want = {k: torch.cat(v)[:len(KEYS)] for k, v in want.items()}
    print("%s: candidates per key %s, kept %s" % (which, want["total"].tolist(), want["count"].tolist()))
    assert int(want["count"].max()) >= 1                                # at least one key frame with detections
    # the video path
    vdet = VideoDetector(cfg, model, batch=2, **kw)
    assert vdet.rule == rule and vdet.T == T and vdet.detector.topk == kw["topk"]
    first = vdet(frames, keys=KEYS)                                     # captures the graph
    first = {k: t.clone() for k, t in zip(FIELDS, first.tensors())}
    (vd, seen), syncs = _count_syncs(monkeypatch, lambda: _launches(lambda: vdet(torch.from_numpy(frames), keys=KEYS, chunk=16)))
    assert syncs == [], syncs                                           # a replaying call reads nothing back and waits for nothing
    assert seen.count("tuber_video_clips") == 3 and seen.count("tuber_frames_resize") == 3          # a launch per batch; 40 frames in chunks of 16
    assert vdet.detector.eval.captures == 1 and vdet.detector.eval.eager_calls == 0
    assert vd.keys == KEYS and vd.class_num == cfg.CONFIG.DATA.NUM_CLASSES
    for k, t in zip(FIELDS, vd.tensors()):
        assert t.shape == want[k].shape and torch.equal(t, want[k]), k
        assert torch.equal(first[k], want[k]), k
    # tubes: on the device, and what the host definition gives on the store read back
    tubes = vd.tubes()
    assert vd.tubes_path == "device"
    cpu = VideoDetections(vd.keys, *[t.cpu() for t in vd.tensors()], class_num=vd.class_num, settings=vd.settings)
    _same_tubes(tubes, cpu.tubes())
    assert cpu.tubes_path == "host" and len(tubes) >= 1
    print("%s: %d tubes, lengths %s" % (which, len(tubes), sorted((t["length"] for t in tubes), reverse=True)[:8]))
    host = vd.to_host()
    assert [hh["key"] for hh in host] == KEYS and [hh["count"] for hh in host] == want["count"].tolist()
    # default keys: range(0, N, stride); the first key frame's clip is the same clip, so its row is the same bits
    strided = vdet(frames, stride=13)
    assert strided.keys == [0, 13, 26, 39] and strided.scores.shape == (4, kw["topk"])
    for k, t in zip(FIELDS, strided.tensors()):
        assert torch.equal(t[0], want[k][0]), k
    # the defaults: the rule of the model, and a topk that keeps tubes() on the device
    dflt = VideoDetector(cfg, model, graphed=False)
    assert dflt.detector.topk == 21 and dflt.settings == dict(link_iou=0.2, max_gap=2, min_len=1)
