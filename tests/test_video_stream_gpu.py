"""Streaming video inference on the GPU (tubelet_transformer_amd/video.py ``VideoStream``): ``tuber_video_clips_ring``
(csrc/video_clips.hip) against ``clip_indices`` + the numpy gather on the linear video, ``tuber_tube_link_stream`` and its size query
``tuber_tube_link_state_bytes`` (csrc/tube_map.hip) against ``evaluation.TubeLinker`` -- its definition -- and the one-shot
``tuber_tube_link_ranked``, and ``VideoStream`` end to end against ``VideoDetector`` on the name-hashed models of tests/test_video_gpu.py.
Everything compared here is exact: the gather moves table entries, the linker's sums are sequential fp64 in slot order, and a replayed forward
on identical input bits is deterministic."""
import itertools

import numpy as np
import pytest
import torch

from test_video_gpu import CONFIGS, SETTINGS, _count_syncs, _gather, _launches, _model, _same_tubes
from test_video_stream_cpu import FIXTURES, one_shot, pushed, same_records, video_rows
from tubelet_transformer_amd import input_pipeline as ip
from tubelet_transformer_amd import lib
from tubelet_transformer_amd.detect import FIELDS
from tubelet_transformer_amd.evaluation import TubeLinker
from tubelet_transformer_amd.video import RULES, VideoDetector, VideoStream, clip_indices

pytestmark = pytest.mark.gpu
EINVAL = -1

# ------------------------------------------------------------------------------------------------------------------------------
# tuber_video_clips_ring
# ------------------------------------------------------------------------------------------------------------------------------
NVIDEO, R, B, T = 13, 6, 3, 4
RING_SHAPES = {
    "scalar_5x7_full": dict(H=5, W=7, window=(0, 0, 5, 7)),              # frames of 105 B: every second slot and every row misaligned
    "vector_6x12_crop": dict(H=6, W=12, window=(1, 2, 4, 8)),            # w % 4 == 0: dword loads, 16-byte stores, a crop
}
# (frames pushed, first_key, key_step, n_keys, n_total): n_total < 0 mid-stream, 13 at the end of the video.  With R = 6 and T = 4 a clip of rate 2
# spans 7 frames: it fits the ring where its first frame is frame 0 (the fixed slot) or its last one is clamped at the video's end.
START = (6, 0, 2, 2, -1)                  # keys 0, 2 and the repeat (n_keys = 2 < B): clips that start at frame 0
WRAP = (9, 5, 1, 3, -1)                   # the ring holds frames 3 .. 8, slots 3 4 5 0 1 2: the clips of keys 5, 6, 7 straddle its wrap
END = (13, 10, 1, 3, 13)                  # keys 10, 11, 12: the end clamps; jhmdb pads key 12 in FRONT with frame 0, whose slot 0 % R holds frame 12
RING_CASES = {
    ("ava", 1): (START, WRAP, END), ("ava", 2): ((7, 0, 1, 2, -1), (13, 11, 1, 2, 13)),
    ("jhmdb", 1): (START, WRAP, END), ("jhmdb", 2): (START, WRAP, END),
    ("edge", 1): (START, WRAP, END), ("edge", 2): ((7, 2, 2, 2, -1), (13, 11, 1, 2, 13)),
}


def _ring_of(frames, pushed_frames, rng):
    """the ring after ``pushed_frames`` frames: frame f in slot f % R, frame 0 in slot R; slots never written hold noise"""
    ring = rng.integers(0, 256, (R + 1,) + frames.shape[1:], dtype=np.uint8)
    holds = {}
    for f in range(pushed_frames):
        ring[f % R] = frames[f]
        holds[f % R] = f
    ring[R] = frames[0]
    return ring, holds


@pytest.mark.parametrize("offset", (0, 1, 3))
@pytest.mark.parametrize("shape", sorted(RING_SHAPES))
def test_video_clips_ring_equals_clip_indices_and_the_numpy_gather(dev, shape, offset):
    s = RING_SHAPES[shape]
    H, W, window = s["H"], s["W"], s["window"]
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (NVIDEO, H, W, 3), dtype=np.uint8)
    lut = ip.normalize_lut()
    lut_d = torch.from_numpy(lut).to(dev)
    seen = set()
    for (rule, rate), cases in sorted(RING_CASES.items()):
        for pushed_frames, first_key, key_step, n_keys, n_total in cases:
            ring, holds = _ring_of(frames, pushed_frames, rng)
            keys = [first_key + min(i, n_keys - 1) * key_step for i in range(B)]
            index = clip_indices(n_total if n_total > 0 else 1000, keys, T, rate, rule)
            # before the launch: the case is what it is there for, and the ring holds every frame it needs
            assert all(f == 0 or holds.get(f % R) == f for f in index.reshape(-1).tolist()), (rule, rate, first_key)
            if n_total < 0:
                assert np.array_equal(index, clip_indices(pushed_frames, keys, T, rate, rule))       # a decided key: no later frame changes it
            slots = [[f % R for f in row if f] for row in index.tolist()]
            if any(row != sorted(row) for row in slots):                # a clip whose later frames sit in earlier slots
                seen.add("wrap")
            if any(row[0] == 0 for row in index.tolist()):
                seen.add("starts at frame 0")
            if n_keys < B:
                seen.add("repeat")
            if rule == "jhmdb" and n_total > 0 and index[-1].tolist() == [0, 10, 11, 12]:
                assert holds[0 % R] == 12                               # frame 0 has left the ring: the pad comes from the fixed slot
                seen.add("front pad at the end")
            if n_total > 0 and (index == n_total - 1).sum() >= 2:
                seen.add("end clamp")
            want = _gather(frames, index, window, lut)
            buf = torch.zeros(offset + ring.size, dtype=torch.uint8, device=dev)                    # the ring at any byte alignment
            buf[offset:].copy_(torch.from_numpy(ring).reshape(-1))
            out = torch.full((B, 3, T) + window[2:], 7.0, dtype=torch.float32, device=dev)
            lib.call("tuber_video_clips_ring", buf[offset:], R, H, W, first_key, key_step, n_keys, B, T, rate, RULES.index(rule), n_total, *window,
                     lut_d, out)
            assert np.array_equal(out.cpu().numpy(), want), (rule, rate, first_key, n_total)
    assert seen == {"wrap", "starts at frame 0", "repeat", "front pad at the end", "end clamp"}


def test_video_clips_ring_refuses_bad_arguments_and_writes_nothing(dev):
    H, W = 6, 12
    ring = torch.zeros(R + 1, H, W, 3, dtype=torch.uint8, device=dev)
    lut = torch.from_numpy(ip.normalize_lut()).to(dev)
    out = torch.full((B, 3, T, H, W), 7.0, dtype=torch.float32, device=dev)
    ok = dict(ring=ring, R=R, H=H, W=W, first_key=0, key_step=1, n_keys=B, B=B, T=T, rate=1, rule=0, n_total=-1, y1=0, x1=0, h=H, w=W, lut=lut, out=out)
    rc = lambda **kw: lib.call_rc("tuber_video_clips_ring", *{**ok, **kw}.values())
    for name in ("ring", "lut", "out"):
        assert rc(**{name: None}) == EINVAL, name
    for name in ("R", "H", "W", "n_keys", "B", "T", "rate", "h", "w"):
        assert rc(**{name: 0}) == EINVAL and rc(**{name: -1}) == EINVAL, name
    for kw in (dict(rule=-1), dict(rule=3), dict(first_key=-1), dict(y1=-1), dict(x1=-1), dict(y1=1), dict(x1=1), dict(y1=3, h=4), dict(x1=8, w=8),
               dict(h=H + 1), dict(w=W + 1)):
        assert rc(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                     # untouched
    assert rc() == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())


# ------------------------------------------------------------------------------------------------------------------------------
# tuber_tube_link_stream
# ------------------------------------------------------------------------------------------------------------------------------
def _state(C, dev):
    return torch.zeros(lib.query("tuber_tube_link_state_bytes", C), dtype=torch.uint8, device=dev)


def _stream_link(fx, v, dev, state, cuts=()):
    """one video of a fixture through ``tuber_tube_link_stream`` in the pieces ``cuts`` make: the records concatenated, as numpy"""
    box, label, score, S = video_rows(fx, v)
    K = fx["K"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    box, label, score = up(box), up(label), up(score)
    head = torch.full((S * K,), 7, dtype=torch.int32, device=dev)
    mean = torch.full((S * K,), 7.0, dtype=torch.float64, device=dev)
    count = torch.full((S * K,), 7, dtype=torch.int32, device=dev)
    edges = [0] + sorted(cuts) + [S]
    for a, b in zip(edges[:-1], edges[1:]):
        lib.call("tuber_tube_link_stream", box[a * K:], label[a * K:], score[a * K:], b - a, K, a, fx["C"], fx["link_iou"], fx["max_gap"], state,
                 head[a * K:], mean[a * K:], count[a * K:])
    return dict(row_head=head.cpu().numpy().astype(np.int64), row_score=mean.cpu().numpy(), row_len=count.cpu().numpy().astype(np.int64))


def _ranked_one_shot(fx, v, dev):
    box, label, score, S = video_rows(fx, v)
    K, N = fx["K"], S * fx["K"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = dict(row_cls=torch.empty(N, dtype=torch.int32, device=dev), row_head=torch.empty(N, dtype=torch.int32, device=dev),
               tube_score=torch.zeros(N, dtype=torch.float64, device=dev), tube_len=torch.zeros(N, dtype=torch.int32, device=dev),
               tube_last=torch.full((N,), -1, dtype=torch.int32, device=dev))
    lib.call("tuber_tube_link_ranked", up(box), up(label), up(score), up((np.arange(S + 1) * K).astype(np.int32)), up(np.array([0, S], dtype=np.int32)), 1, S,
             N, fx["C"], K, fx["link_iou"], fx["max_gap"], out["row_cls"], out["row_head"], out["tube_score"], out["tube_len"], out["tube_last"])
    return {k: t.cpu().numpy() for k, t in out.items()}


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_tube_link_stream_equals_the_host_linker_and_the_one_shot_entry_at_every_cut(dev, name):
    fx = FIXTURES[name]()
    S = fx["videos"][0][1]
    host = pushed(TubeLinker(fx["C"], fx["link_iou"], fx["max_gap"]), fx, 0)
    assert (host["row_head"] >= 0).sum() > 5 and host["row_len"].max() >= 3
    state = _state(fx["C"], dev)
    got = _stream_link(fx, 0, dev, state)
    assert same_records(got, host)
    ranked = _ranked_one_shot(fx, 0, dev)
    assert np.array_equal(got["row_head"], ranked["row_head"].astype(np.int64))
    ends = {int(h): r for r, h in enumerate(got["row_head"].tolist()) if h >= 0}
    for h, r in ends.items():                                           # a tube's score and length are those of its last row
        assert got["row_len"][r] == ranked["tube_len"][h]
        assert got["row_score"][r:r + 1].view(np.int64)[0] == ranked["tube_score"][h:h + 1].view(np.int64)[0]
    for cut in [(c,) for c in range(1, S)] + list(itertools.combinations(range(1, S), 2)):
        state.zero_()
        assert same_records(_stream_link(fx, 0, dev, state, cut), host), cut
    if len(fx["videos"]) > 1:                                           # a zeroed state after a finished video: the next video from ordinal 0
        state.zero_()
        assert same_records(_stream_link(fx, 1, dev, state), pushed(TubeLinker(fx["C"], fx["link_iou"], fx["max_gap"]), fx, 1))
        want = one_shot(fx, 1)
        state.zero_()
        assert np.array_equal(_stream_link(fx, 1, dev, state, (1,))["row_head"], want["row_head"])


def test_tube_link_stream_refuses_beyond_the_linkers_bounds_and_touches_nothing(dev):
    sizes = [lib.query("tuber_tube_link_state_bytes", C) for C in (1, 3, 24, 80)]
    assert sizes[0] > 0 and sizes == sorted(set(sizes))                 # positive, growing with C
    fx = FIXTURES["ranked"]()
    C = fx["C"]
    state = torch.full((lib.query("tuber_tube_link_state_bytes", C),), 7, dtype=torch.uint8, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def call(K, max_gap, S=1, slot_base=0, **kw):
        n = S * K
        a = dict(box=up(np.resize(fx["box"], (n, 4))), label=up(np.resize(fx["label"], n)), score=up(np.resize(fx["score"], n)), state=state,
                 head=torch.full((n,), 7, dtype=torch.int32, device=dev), mean=torch.full((n,), 7.0, dtype=torch.float64, device=dev),
                 count=torch.full((n,), 7, dtype=torch.int32, device=dev))
        a.update(kw)
        code = lib.call_rc("tuber_tube_link_stream", a["box"], a["label"], a["score"], S, K, slot_base, C, fx["link_iou"], max_gap, a["state"], a["head"],
                           a["mean"], a["count"])
        torch.cuda.synchronize()
        return code, all(bool((a[k] == 7).all()) for k in ("head", "mean", "count") if a[k] is not None)
    assert call(33, 1) == (EINVAL, True)                                # 33 * (1 + 1) = 66 active tubes
    assert call(4, 16) == (EINVAL, True)                                # 4 * 17 = 68
    assert call(65, 0) == (EINVAL, True)                                # more rows than tuber_frame_match_max_dets()
    assert call(4, 1, S=2, slot_base=2 ** 29) == (EINVAL, True)         # (slot_base + S) * K beyond an int32
    assert call(4, 1, state=None) == (EINVAL, True) and call(4, 1, head=None)[0] == EINVAL and call(4, -1) == (EINVAL, True)
    assert bool((state == 7).all())                                     # the state untouched by every refusal
    state.zero_()
    assert call(33, 0) == (0, False) and call(4, 1, S=2, slot_base=2 ** 29 - 3) == (0, False)        # within the bounds
    assert bool((state != 0).any())


# ------------------------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------------------------
H0, W0, NFRAMES, STRIDE = 96, 160, 100, 9                               # working resolution 48 x 80; 12 key frames, batch 2: six batches
STRICT_IOU = 0.9999                                                     # links boxes that are identical, and hardly any others


def _feed(vs, frames, pieces, tubes=False):
    """``frames`` pushed in ``pieces``, then ``finish()``: the VideoDetections returned, the tubes of a ``tubes()`` call after every push and after
    ``finish()``, how many of them came before ``finish()``, and whether the ring wrapped"""
    assert sum(pieces) == len(frames)
    outs, found, o = [], [], 0
    for m in pieces:
        outs.append(vs.push(frames[o:o + m]))
        o += m
        if tubes:
            found += vs.tubes()
    early, wrapped, mid = len(found), vs.wrapped, sum(len(vd.keys) for vd in outs if vd is not None)
    outs.append(vs.finish())
    if tubes:
        found += vs.tubes()
    return [vd for vd in outs if vd is not None], found, early, wrapped, mid


def _assert_same_rows(outs, want):
    assert [k for vd in outs for k in vd.keys] == want.keys
    for k in FIELDS:
        got = torch.cat([getattr(vd, k) for vd in outs])
        assert got.shape == getattr(want, k).shape and torch.equal(got, getattr(want, k)), k


@pytest.mark.parametrize("which", ("ava", "jhmdb"))
def test_video_stream_equals_video_detector(dev, which, monkeypatch):
    cfg, model = _model(CONFIGS[which])
    model.engine()
    bias = model.class_fc.bias.data
    saved = bias.clone()
    if which == "jhmdb":
        bias[-1] -= 2.0                                                 # the no-object bias trick of tests/test_video_gpu.py
    try:
        _stream_end_to_end(dev, which, cfg, model, monkeypatch)
    finally:
        bias.copy_(saved)
        model.eval()


def _stream_end_to_end(dev, which, cfg, model, monkeypatch):
    kw = SETTINGS[which]
    frames = np.random.default_rng(11).integers(0, 256, (NFRAMES, H0, W0, 3), dtype=np.uint8)
    second = np.random.default_rng(12).integers(0, 256, (NFRAMES, H0, W0, 3), dtype=np.uint8)
    vdet = VideoDetector(cfg, model, batch=2, **kw)
    want, want2 = vdet(frames, stride=STRIDE), vdet(second, stride=STRIDE)
    want_tubes = want.tubes()
    assert want.tubes_path == "device" and len(want.keys) == 12 and int(want.count.max()) >= 1 and len(want_tubes) >= 1
    vs = VideoStream(cfg, model, batch=2, stride=STRIDE, max_chunk=16, **kw)
    assert vs.rule == vdet.rule and vs.detector.topk == kw["topk"] and vs.R + 1 < NFRAMES         # the ring is smaller than the video
    assert vs.finish() is None                                          # no frames pushed
    # everything in one push (cut inside push: 100 > max_chunk); captures the graph
    outs, _, _, wrapped, mid = _feed(vs, frames, [NFRAMES])
    _assert_same_rows(outs, want)
    assert wrapped and vs.device_bytes() == (vs.R + 1) * 48 * 80 * 3 + lib.query("tuber_tube_link_state_bytes", vs.class_num)
    if which == "ava":
        assert 0 < mid < 12                                             # some keys decided mid-stream, some only once the end is known
    _same_tubes(vs.tubes(), want_tubes)                                 # first called after finish(): every tube of the video, in head order
    # pushes of 7 frames, tubes() after every push
    outs, tubes, early, wrapped, _ = _feed(vs, torch.from_numpy(frames), [7] * 14 + [2], tubes=True)
    _assert_same_rows(outs, want)
    assert wrapped and len(outs) > 2
    for vd in outs:
        assert vd.row_head.shape == vd.scores.shape and vd.row_head.dtype == torch.int32 and vd.row_score.dtype == torch.float64
    print("%s: %d tubes, %d of them before finish()" % (which, len(tubes), early))
    assert all("head" in t for t in tubes)
    _same_tubes(sorted(tubes, key=lambda t: (t["frames"][0], t["head"])), want_tubes)
    assert vs.tubes() == []
    # The boxes of the name-hashed models barely move from key frame to key frame, so at the shipped LINK_IOU every tube runs to the last key
    # and none can close before finish().  A stream that links only boxes that are (all but) identical has tubes that end: under the ava rule
    # the keys 0 .. 27 share one clip (start clamped to 0), hence one set of boxes, and the key after them does not.
    saved_iou = cfg.CONFIG.VAL.VIDEO_MAP.LINK_IOU
    cfg.CONFIG.VAL.VIDEO_MAP.LINK_IOU = STRICT_IOU
    try:
        strict = VideoStream(cfg, model, batch=2, stride=STRIDE, max_chunk=16, **kw)
    finally:
        cfg.CONFIG.VAL.VIDEO_MAP.LINK_IOU = saved_iou
    assert strict.settings["link_iou"] == STRICT_IOU
    outs, tubes, early, _, _ = _feed(strict, frames, [7] * 14 + [2], tubes=True)
    _assert_same_rows(outs, want)
    strict_tubes = want.tubes(link_iou=STRICT_IOU)
    print("%s, LINK_IOU %s: %d tubes, %d of them before finish()" % (which, STRICT_IOU, len(tubes), early))
    assert 1 <= early < len(tubes)                                      # closed tubes come out while the video is still running
    _same_tubes(sorted(tubes, key=lambda t: (t["frames"][0], t["head"])), strict_tubes)
    if which == "ava":
        assert max(t["length"] for t in strict_tubes) >= 2              # the keys that share a clip still link
    # pushes of 1, 50 and 49 frames under the launch hook: a device tensor, the middle push cut into pieces
    (got, seen) = _launches(lambda: _feed(vs, torch.from_numpy(frames).to(dev), [1, 50, 49]))
    outs = got[0]
    _assert_same_rows(outs, want)
    assert seen.count("tuber_video_clips_ring") == 6 and seen.count("tuber_video_clips") == 0      # a launch per batch
    assert seen.count("tuber_tube_link_stream") == len(outs)            # one per push (or finish) that decided keys
    vs.tubes()
    # a second video of the same size: nothing new allocated or captured; no host read and no wait while it is pushed
    (got, syncs) = _count_syncs(monkeypatch, lambda: _feed(vs, second, [30, 30, 40]))
    assert syncs == [], syncs
    _assert_same_rows(got[0], want2)
    assert len(vs._bufs) == 1 and vs.detector.eval.captures == 1 and vs.detector.eval.eager_calls == 0
    _same_tubes(vs.tubes(), want2.tubes())                              # after finish(): everything that remains, in head order
    # errors
    assert vs.push(frames[:3]) is None
    with pytest.raises(ValueError):
        vs.push(frames[:2, :50])                                        # another frame size inside a video
    with pytest.raises(ValueError):
        vs.push(frames.astype(np.float32))
    model.train()
    with pytest.raises(RuntimeError):
        vs.push(frames[:2])
    model.eval()
    assert vs.finish() is not None and vs.finish() is None


def test_video_stream_links_on_the_host_beyond_the_linkers_bounds(dev, capsys):
    cfg, model = _model(CONFIGS["ava"])
    kw = dict(SETTINGS["ava"], topk=33, graphed=False)                   # 33 * (MAX_GAP + 1) = 99 active tubes: beyond the linker
    frames = np.random.default_rng(11).integers(0, 256, (70, H0, W0, 3), dtype=np.uint8)
    want = VideoDetector(cfg, model, batch=2, **kw)(frames, stride=30)
    capsys.readouterr()
    vs = VideoStream(cfg, model, batch=2, stride=30, max_chunk=16, **kw)
    outs, tubes, _, _, _ = _feed(vs, frames, [40, 30], tubes=True)
    assert capsys.readouterr().err.count("linking on the host") == 1    # one line, not one per push
    _assert_same_rows(outs, want)
    _same_tubes(sorted(tubes, key=lambda t: (t["frames"][0], t["head"])), want.tubes())
