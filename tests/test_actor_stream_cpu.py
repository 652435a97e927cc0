"""Host side of the streaming actor tracks, no GPU: ``evaluation.ActorTracker`` -- the definition of
``tuber_track_actions_stream`` -- in one piece and cut at every subset of the cut points against ``evaluation.actor_tracks`` on the hand-written
video of tests/test_actors_cpu.py and on a random one that makes the ring wrap; ``smooth_range``; ``video.TrackAssembler`` on host arrays against
``VideoActors.tracks``; the option's signature and the three C-ABI entries in the header and the built library.  Every comparison is exact."""
import inspect
import itertools
import os
import types

import numpy as np
import pytest
import torch

from test_actors_cpu import LINK_IOU, TRACKS, _seq_mean, track_fixture
from test_actors_gpu import _same_tracks
from tubelet_transformer_amd import lib
from tubelet_transformer_amd.config import load_cfg
from tubelet_transformer_amd.evaluation import ActorTracker, TubeLinker, actor_tracks, smooth_range, track_ring_slots
from tubelet_transformer_amd.video import TrackAssembler, VideoActors, VideoStream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = ((1, 0), (1, 1), (1, 2), (0, 3), (2, 1), (1, 100))            # (max_gap, window)
CUTTINGS = [c for k in range(6) for c in itertools.combinations(range(1, 6), k)]      # every subset of the cut points 1 .. 5: 32
RANDOM_CUTS = ((), (7,), (1, 2, 3), tuple(range(1, 14)), (5, 6, 12))


def random_fixture(C=3, seed=5):
    """S = 14 key frames of A = 5 rows: three people who walk slowly, leave for one or several key frames and come back, and a passer-by now
    and then; action values spread over sixteen orders of magnitude, as in ``track_fixture``"""
    rng = np.random.default_rng(seed)
    S, A = 14, 5
    box, actor, queries = np.zeros((S * A, 4), dtype=np.float32), np.zeros(S * A, dtype=np.float32), np.full(S * A, -1, dtype=np.int32)
    homes = [(0, 0), (40, 0), (0, 40)]
    for s in range(S):
        rows = []
        for p, (x, y) in enumerate(homes):
            if rng.random() < 0.7:
                dx = float(rng.integers(0, 3))
                rows.append(((x + dx, y, x + dx + 10, y + 10), 0.5 + 0.1 * p + 0.01 * s, p))
        if rng.random() < 0.3:
            rows.append(((80, 80, 90, 90), 0.4, 7))
        for a, (b, pr, q) in enumerate(rows):
            box[s * A + a], actor[s * A + a], queries[s * A + a] = b, pr, q
    mag = 10.0 ** rng.integers(-16, 0, (S * A, C))
    actions = (rng.uniform(0.1, 0.99, (S * A, C)) * mag).astype(np.float32)
    actions[queries < 0] = 0.0
    return dict(box=box, actor=actor, queries=queries, actions=actions, S=S, A=A, C=C)


def stream_records(tracker, fx, cuts=(), flush_empty=False):
    """the fixture through ``tracker`` in the pieces ``cuts`` make (``flush_empty``: the flush in a push of its own, without rows): the per-row
    records concatenated, ``smooth`` concatenated, and the smooth ranges"""
    S, A = fx["S"], fx["A"]
    edges = [0] + sorted(cuts) + [S]
    parts, ranges = [], []
    for a, b in zip(edges[:-1], edges[1:]):
        sl = slice(a * A, b * A)
        parts.append(tracker.push(fx["box"][sl], fx["actor"][sl], fx["queries"][sl], fx["actions"][sl], A, flush=b == S and not flush_empty))
        ranges.append(smooth_range(a, b - a, tracker.window, b == S and not flush_empty))
    if flush_empty:
        parts.append(tracker.push(fx["box"][:0], fx["actor"][:0], fx["queries"][:0], fx["actions"][:0], A, flush=True))
        ranges.append(smooth_range(S, 0, tracker.window, True))
    assert [(p["smooth_lo"], p["smooth_hi"]) for p in parts] == ranges
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("row_head", "row_score", "row_len", "row_mean", "row_peak", "smooth")}
    out["ranges"] = ranges
    return out


def _same_bits(a, b, view):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(view), b[~nan].view(view))


def assert_is_actor_tracks(got, want, fx):
    """the stream's records against ``actor_tracks`` of the whole video: heads, ``smooth`` concatenated = ``row_smooth``, and at every track's
    last row the running records = the track's"""
    N = fx["S"] * fx["A"]
    head = want["row_head"]
    assert np.array_equal(got["row_head"], head)
    assert got["smooth"].shape == (N, fx["C"]) and got["smooth"].dtype == np.float64 and got["row_mean"].dtype == np.float64
    assert got["row_peak"].dtype == np.float32
    assert _same_bits(got["smooth"], want["row_smooth"], np.int64)
    last = {int(h): r for r, h in enumerate(head.tolist()) if h >= 0}
    assert last
    for h, r in last.items():
        assert _same_bits(got["row_mean"][r], want["track_mean"][h], np.int64), (h, r)
        assert _same_bits(got["row_peak"][r], want["track_peak"][h], np.int32), (h, r)
        assert got["row_len"][r] == want["tube_len"][h]
        assert got["row_score"][r:r + 1].view(np.int64)[0] == want["tube_score"][h:h + 1].view(np.int64)[0]
    assert not got["row_mean"][head < 0].any() and not got["row_peak"][head < 0].any() and not got["smooth"][head < 0].any()
    lo = [a for a, _ in got["ranges"]]
    assert got["ranges"][0][0] == 0 and got["ranges"][-1][1] == fx["S"] and lo[1:] == [b for _, b in got["ranges"][:-1]]


def same_stream_records(a, b):
    return (np.array_equal(a["row_head"], b["row_head"]) and np.array_equal(a["row_len"], b["row_len"])
            and np.array_equal(a["row_score"].view(np.int64), b["row_score"].view(np.int64)) and _same_bits(a["row_mean"], b["row_mean"], np.int64)
            and _same_bits(a["row_peak"], b["row_peak"], np.int32) and _same_bits(a["smooth"], b["smooth"], np.int64))


def _want(fx, max_gap, window):
    return actor_tracks(fx["box"], fx["actor"], fx["queries"], fx["actions"], fx["S"], fx["A"], LINK_IOU, max_gap, window)


# ------------------------------------------------------------------------------------------------------------------------------
# ActorTracker
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_gap,window", SETTINGS)
def test_actor_tracker_in_one_piece_equals_actor_tracks(max_gap, window):
    fx = track_fixture()
    want = _want(fx, max_gap, window)
    head = want["row_head"]
    if max_gap == 1:                                                    # the fixture holds what it is there for
        assert {h: np.nonzero(head == h)[0].tolist() for h in sorted(set(head[head >= 0].tolist()))} == TRACKS
    tracker = ActorTracker(LINK_IOU, max_gap, window)
    assert tracker.H == track_ring_slots(max_gap, window) == max(2 * window, max_gap + 1) + 1
    got = stream_records(tracker, fx)
    assert_is_actor_tracks(got, want, fx)
    linker = TubeLinker(1, LINK_IOU, max_gap).push(fx["box"], np.where(fx["queries"] >= 0, 0, -1), fx["actor"], 4)
    for k in ("row_head", "row_len"):
        assert np.array_equal(got[k], linker[k]), k
    assert np.array_equal(got["row_score"].view(np.int64), linker["row_score"].view(np.int64))
    # the running mean at every row, last or not: the prefix of the track, summed with Python floats
    members = {}
    for r in np.nonzero(head >= 0)[0].tolist():
        members.setdefault(int(head[r]), []).append(r)
        prefix = members[int(head[r])]
        assert np.array_equal(got["row_mean"][r].view(np.int64), _seq_mean(fx["actions"], prefix).view(np.int64)), r
        assert np.array_equal(got["row_peak"][r], fx["actions"][prefix].max(axis=0)), r
    assert max(len(v) for v in members.values()) >= 3
    # a second video after reset(): the same records
    tracker.reset()
    assert same_stream_records(stream_records(tracker, fx), got)


@pytest.mark.parametrize("max_gap,window", SETTINGS)
def test_actor_tracker_cut_at_every_subset_of_the_cut_points_gives_the_same_records(max_gap, window):
    fx = track_fixture()
    want = _want(fx, max_gap, window)
    whole = stream_records(ActorTracker(LINK_IOU, max_gap, window), fx)
    tracker = ActorTracker(LINK_IOU, max_gap, window)
    assert len(CUTTINGS) == 32
    for cuts in CUTTINGS:
        for flush_empty in (False, True):
            tracker.reset()
            got = stream_records(tracker, fx, cuts, flush_empty)
            assert_is_actor_tracks(got, want, fx)
            assert same_stream_records(got, whole), (cuts, flush_empty)


def test_actor_tracker_propagates_nan_like_actor_tracks_at_every_cut():
    fx = track_fixture()
    fx["actions"][12, 4] = np.nan
    want = _want(fx, 1, 1)
    assert np.isnan(want["track_mean"][0, 4]) and np.isnan(want["track_peak"][0, 4]) and np.isnan(want["row_smooth"][[8, 12, 16], 4]).all()
    tracker = ActorTracker(LINK_IOU, 1, 1)
    for cuts in CUTTINGS:
        tracker.reset()
        got = stream_records(tracker, fx, cuts)
        assert_is_actor_tracks(got, want, fx)
        assert np.isnan(got["row_mean"][[12, 16, 21], 4]).all() and not np.isnan(got["row_mean"][[0, 8], 4]).any()
        assert np.isnan(got["row_peak"][[12, 16, 21], 4]).all() and not np.isnan(got["row_peak"][[0, 8], 4]).any()


@pytest.mark.parametrize("max_gap,window", ((1, 1), (2, 3), (0, 0), (3, 1)))
def test_actor_tracker_on_a_longer_video_whose_ring_wraps(max_gap, window):
    fx = random_fixture()
    want = _want(fx, max_gap, window)
    lens = want["tube_len"][want["row_head"] == np.arange(70)]
    H = track_ring_slots(max_gap, window)
    assert fx["S"] > 2 * H or window == 3                               # the ring wraps more than once
    if (max_gap, window) == (1, 1):
        assert lens.max() > H > lens.min()                              # tracks longer and shorter than the ring
    tracker = ActorTracker(LINK_IOU, max_gap, window)
    for cuts in RANDOM_CUTS:
        tracker.reset()
        assert_is_actor_tracks(stream_records(tracker, fx, cuts), want, fx)


def test_smooth_ranges_partition_the_slots_in_order():
    for window, pushes in ((2, [1, 1, 4, 0, 3]), (3, [2, 2, 2]), (0, [3, 1, 2]), (1, [6]), (5, [1, 2]), (100, [2, 3])):
        for flush_empty in (False, True):
            base, ranges = 0, []
            for i, n in enumerate(pushes):
                ranges.append(smooth_range(base, n, window, flush=i == len(pushes) - 1 and not flush_empty))
                base += n
            if flush_empty:
                ranges.append(smooth_range(base, 0, window, flush=True))
            assert ranges[0][0] == 0 and ranges[-1][1] == base
            assert all(lo <= hi for lo, hi in ranges) and [lo for lo, _ in ranges[1:]] == [hi for _, hi in ranges[:-1]]
            for (lo, hi), end in zip(ranges[:-1], np.cumsum(pushes)):
                assert hi == max(end - window, 0)                       # a row waits for the `window` slots behind it
    assert smooth_range(0, 1, 2) == (0, 0) and smooth_range(1, 1, 2) == (0, 0) and smooth_range(2, 4, 2) == (0, 4)      # a first push shorter than window
    assert smooth_range(6, 0, 2, flush=True) == (4, 6) and smooth_range(6, 0, 2) == (4, 4)
    assert smooth_range(3, 2, 0) == (3, 5) == smooth_range(3, 2, 0, flush=True)
    with pytest.raises(ValueError):
        smooth_range(-1, 1, 1)


# ------------------------------------------------------------------------------------------------------------------------------
# TrackAssembler
# ------------------------------------------------------------------------------------------------------------------------------
KEYS = [0, 30, 60, 90, 120, 150]


def _cpu_store(fx, **settings):
    t = lambda a, *shape: torch.from_numpy(np.ascontiguousarray(a)).reshape(*shape)
    S, A, C = fx["S"], fx["A"], fx["C"]
    count = t((fx["queries"].reshape(S, A) >= 0).sum(1).astype(np.int32), S)
    return VideoActors([30 * s for s in range(S)], t(fx["box"], S, A, 4), t(fx["actor"], S, A), t(fx["queries"], S, A), t(fx["actions"], S, A, C),
                       count, count.clone(), settings=dict(dict(link_iou=LINK_IOU, max_gap=1, min_len=1, window=1, label_thr=0.2), **settings))


def assemble(fx, cuts, max_gap, window, min_len=1, label_thr=0.2, take_every_push=True, flush_empty=False):
    """the fixture through ``ActorTracker`` and ``TrackAssembler`` cut by cut -> (tracks in the order they came out, [(next key ordinal, the
    tracks a take() after that push returned)]); ``flush_empty``: the flush in a record of its own, without keys, as a ``finish()`` that has no
    key left to run makes it"""
    S, A, C = fx["S"], fx["A"], fx["C"]
    tracker = ActorTracker(LINK_IOU, max_gap, window)
    asm = TrackAssembler(A, max_gap, window, min_len, label_thr)
    edges = [0] + sorted(cuts) + [S] + ([S] if flush_empty else [])
    out, seen = [], []
    for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        sl = slice(a * A, b * A)
        last = i == len(edges) - 2
        rec = tracker.push(fx["box"][sl], fx["actor"][sl], fx["queries"][sl], fx["actions"][sl], A, flush=last)
        n = b - a
        asm.add(a, [30 * s for s in range(a, b)], fx["box"][sl].reshape(n, A, 4), fx["actor"][sl].reshape(n, A), fx["queries"][sl].reshape(n, A),
                fx["actions"][sl].reshape(n, A, C), rec["row_head"].reshape(n, A), rec["row_score"].reshape(n, A), rec["row_len"].reshape(n, A),
                rec["row_mean"].reshape(n, A, C), rec["row_peak"].reshape(n, A, C), rec["smooth"].reshape(-1, A, C), rec["smooth_lo"])
        if last:
            asm.end()
        if take_every_push or last:
            got = asm.take()
            seen.append((b, got, last))
            out += got
    assert asm.take() == []
    return out, seen


def _strip(tracks):
    return [{k: v for k, v in t.items() if k != "head"} for t in tracks]


@pytest.mark.parametrize("max_gap,window", ((1, 1), (1, 0), (0, 3), (2, 1), (1, 100)))
def test_the_assembler_returns_video_actors_tracks_and_no_track_before_it_is_closed(max_gap, window, capsys):
    fx = track_fixture()
    want = _cpu_store(fx).tracks(max_gap=max_gap, window=window)
    heads = sorted(int(h) for h in set(_want(fx, max_gap, window)["row_head"].tolist()) if h >= 0)
    assert len(want) == len(heads) >= 3
    early = 0
    for cuts in CUTTINGS:
        got, seen = assemble(fx, cuts, max_gap, window)
        got.sort(key=lambda t: t["head"])
        assert [t["head"] for t in got] == heads
        _same_tracks(_strip(got), want)
        last = {h: t["frames"][-1] // 30 for h, t in zip(heads, want)}   # the key ordinal of a track's last row
        done = set()
        for next_ord, tracks, ended in seen:
            assert [t["head"] for t in tracks] == sorted(t["head"] for t in tracks)        # head order within a call
            assert not done & {t["head"] for t in tracks}               # a track comes out once
            done |= {t["head"] for t in tracks}
            if not ended:                                               # closed, no sooner and no later: no key to come extends it, its last smooth is out
                early += len(tracks)
                assert done == {h for h in heads if next_ord - last[h] > max(max_gap + 1, window)}, (cuts, next_ord)
        assert done == set(heads)
    # some tracks come out while the video runs, where the video has a key far enough behind one (the last cut point is key 5)
    assert (early > 0) == any(5 - o > max(max_gap + 1, window) for o in last.values())
    assert early > 0 or (max_gap, window) in ((2, 1), (1, 100))
    # one take() at the end: everything, in head order
    got, seen = assemble(fx, (2, 4), max_gap, window, take_every_push=False)
    assert len(seen) == 1 and [t["head"] for t in got] == heads
    _same_tracks(_strip(got), want)


def test_the_assembler_honours_min_len_and_label_thr():
    fx = track_fixture()
    store = _cpu_store(fx)
    for min_len, label_thr in ((2, 0.2), (1, 0.0), (3, 0.5)):
        want = store.tracks(min_len=min_len, label_thr=label_thr)
        got, _ = assemble(fx, (1, 3), 1, 1, min_len=min_len, label_thr=label_thr)
        _same_tracks(_strip(sorted(got, key=lambda t: t["head"])), want)
    assert [t["length"] for t in store.tracks(min_len=2)] == [5, 2] and len(store.tracks(label_thr=0.0)[0]["labels"]) == 5
    # the flush in a record without keys: the smoothed rows that waited for the end of the video
    got, seen = assemble(fx, (2,), 1, 2, flush_empty=True)
    assert len(seen) == 3 and seen[1][0] == seen[2][0] == 6 and len(seen[2][1]) >= 2
    _same_tracks(_strip(sorted(got, key=lambda t: t["head"])), store.tracks(window=2))
    # the longer video
    asm_fx = random_fixture()
    want = _cpu_store(asm_fx).tracks(max_gap=2, window=2)
    got, _ = assemble(asm_fx, (3, 4, 9), 2, 2)
    _same_tracks(_strip(sorted(got, key=lambda t: t["head"])), want)


# ------------------------------------------------------------------------------------------------------------------------------
# signatures, the C ABI
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_option_is_off_by_default_and_refuses_what_video_detector_refuses():
    assert inspect.signature(VideoStream.__init__).parameters["actors"].default is None
    cfg = load_cfg(os.path.join(ROOT, "configuration", "Tuber_CSN152_JHMDB.yaml"))
    stub = types.SimpleNamespace(dataset_mode="jhmdb", training=False, query_embed=types.SimpleNamespace(num_embeddings=10))
    assert VideoStream(cfg, stub, graphed=False).detector.actors is None
    with pytest.raises(ValueError, match="actors"):
        VideoStream(cfg, stub, graphed=False, actors=4)
    ava = types.SimpleNamespace(dataset_mode="ava", training=False, query_embed=types.SimpleNamespace(num_embeddings=15))
    cfg = load_cfg(os.path.join(ROOT, "configuration", "TubeR_CSN50_AVA21.yaml"))
    vs = VideoStream(cfg, ava, graphed=False, actors=15)
    assert vs.detector.actors == 15 and vs.actor_settings == dict(link_iou=0.2, max_gap=2, min_len=1, window=1, label_thr=0.05)
    assert vs.tracks_path is None and vs.tracks() == [] and vs.device_bytes() == 0
    with pytest.raises(ValueError, match="actors"):
        VideoStream(cfg, ava, graphed=False, actors=15, link=False)
    for v in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="actors"):
            VideoStream(cfg, ava, graphed=False, actors=v)
    with pytest.raises(RuntimeError, match="actors"):
        VideoStream(cfg, ava, graphed=False).tracks()


def test_the_three_entries_are_declared_and_exported():
    protos = {name: (ret, args) for ret, name, args in lib.header_prototypes()}
    ret, args = protos["tuber_track_actions_stream"]
    assert ret == "int" and [n for _, n in args] == ["actions", "row_head", "S", "A", "C", "slot_base", "max_gap", "window", "flush", "state", "row_mean",
                                                     "row_peak", "smooth", "stream"]
    assert protos["tuber_track_stream_state_bytes"] == ("long", [("int", "A"), ("int", "C"), ("int", "max_gap"), ("int", "window")])
    assert protos["tuber_track_stream_limits"] == ("int", [("int", "which")])
    loaded = lib.load()
    for name in ("tuber_track_actions_stream", "tuber_track_stream_state_bytes", "tuber_track_stream_limits"):
        assert hasattr(loaded, name), name
    active = lib.query("tuber_tube_link_max_active")
    max_a, max_c, max_w, other = (lib.query("tuber_track_stream_limits", w) for w in (0, 1, 2, 3))
    assert (max_a, max_c, other) == (active, 4096, -1) == (lib.query("tuber_track_actions_limits", 0), lib.query("tuber_track_actions_limits", 1), -1)
    assert max_w >= 1 and track_ring_slots(0, max_w) <= 64 < track_ring_slots(0, max_w + 1)       # the largest window whose ring has 64 slots at most
    size = lambda *a: lib.query("tuber_track_stream_state_bytes", *a)
    assert size(15, 80, 2, 1) > 0 and size(15, 80, 2, 1) % 16 == 0
    assert size(15, 80, 2, 1) < size(15, 80, 2, 3) < size(15, 300, 2, 3)           # growing with the ring and with the classes
    assert size(max_a, max_c, 0, max_w) > 0 and size(1, 1, active - 1, 0) > 0
    for bad in ((0, 80, 2, 1), (max_a + 1, 80, 0, 1), (15, 0, 2, 1), (15, max_c + 1, 2, 1), (15, 80, -1, 1), (15, 80, 2, -1), (15, 80, 2, max_w + 1),
                (15, 80, active // 15, 1)):                             # the last one: A * (max_gap + 1) beyond the linker's active tubes
        assert size(*bad) == 0, bad
