"""Dense action tubes on the host: ``evaluation.dense_rows`` / ``dense_tube`` by hand and against each other, the host
path of ``tubes(dense=True)`` / ``tracks(dense=True)``, the assemblers of the stream, ``CONFIG.VAL.VIDEO_MAP.DENSE`` and the linkage of
``tuber_tube_dense``.  Every comparison of fp32 data is one of bytes.  No GPU."""
import inspect

import numpy as np
import pytest
import torch

from test_tube_nms_cpu import padded_actors, padded_detections
from tubelet_transformer_amd import lib
from tubelet_transformer_amd.config import actor_settings, dense_setting, get_cfg_defaults, video_map_settings
from tubelet_transformer_amd.evaluation import ActorTracker, TubeLinker, actor_tracks, dense_extent, dense_from_rows, dense_rows, dense_tube, link_rows
from tubelet_transformer_amd.video import TrackAssembler, TubeAssembler, VideoActors, VideoDetections, VideoStream

DENSE_KEYS = {"frames", "boxes", "frame_scores", "key_index"}
TUBE_KEYS = {"cls", "score", "frames", "boxes", "length"}
TRACK_KEYS = {"score", "frames", "boxes", "actor", "queries", "actions", "smooth", "mean", "peak", "labels", "length"}
ADDED = {"keys", "key_boxes", "frame_scores", "key_index"}
QNAN = 0x7FC00000


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:8].tolist()


def same_dense(got, want):
    """two dense dicts (``dense_tube``'s four fields), byte for byte"""
    assert list(got["frames"]) == list(want["frames"]) and np.array_equal(got["key_index"], want["key_index"])
    same_bits(got["boxes"], want["boxes"])
    same_bits(got["frame_scores"], want["frame_scores"])


# ------------------------------------------------------------------------------------------------------------------------------
# records
# ------------------------------------------------------------------------------------------------------------------------------
PLANTED_KEYS = [3, 4, 9, 10, 140, 141]


def planted_dense():
    """S = 6, K = 3, max_gap = 2 over the keys 3, 4, 9, 10, 140, 141 -> (box, score, row_head, {name: rows}).  ``through`` sits at position 0 of
    every slot (its step from key 10 to key 140 takes a wave three times round its loop); ``bridged`` goes from slot 0 to slot 3, exactly
    max_gap + 1 slots ahead, and on to slot 4; ``ended`` lives in slots 1 and 2 at position 2; ``heir`` starts at position 2 of slot 3, the
    place ``ended`` vacated, and runs into the last slot; the remaining rows are not counted."""
    S, K = 6, 3
    rng = np.random.default_rng(11)
    xy = rng.uniform(0, 300, (S * K, 2))
    box = np.concatenate([xy, xy + rng.uniform(20, 90, (S * K, 2))], axis=1).astype(np.float32)
    score = rng.uniform(0.05, 1.0, S * K).astype(np.float32)
    tubes = dict(through=[0, 3, 6, 9, 12, 15], bridged=[1, 10, 13], ended=[5, 8], heir=[11, 14, 17])
    head = np.full(S * K, -1, dtype=np.int64)
    for rows in tubes.values():
        head[rows] = rows[0]
    return box, score, head, tubes


def seeded(seed, S=12, K=5, C=2, max_gap=2, link_iou=0.2):
    """a seeded padded store and its links: three drifting anchors, a row per anchor and slot with probability 0.7, every coordinate jittered,
    random classes and fp32 scores, keys ascending in steps of 1..9 -> dict(box [S * K, 4], score, label [S * K], keys, S, K, C, max_gap,
    link_iou, link: ``link_rows``' record)"""
    rng = np.random.default_rng(seed)
    keys = np.cumsum(rng.integers(1, 10, S)).tolist()
    box, score, label = np.zeros((S, K, 4), np.float32), np.zeros((S, K), np.float32), np.full((S, K), -1, np.int32)
    anchor = np.asarray([[60.0, 70.0], [200.0, 110.0], [330.0, 190.0]]) + rng.uniform(-15, 15, (3, 2))
    vel = rng.uniform(-2.0, 2.0, (3, 2))
    for s in range(S):
        n = 0
        for k in range(3):
            for _ in range(2 if rng.random() < 0.25 else 1):                # now and then a second detection on one anchor
                if rng.random() < 0.7 and n < K:
                    c = anchor[k] + vel[k] * s
                    box[s, n] = np.asarray([c[0] - 20, c[1] - 30, c[0] + 20, c[1] + 30]) + rng.normal(0, 3, 4)
                    score[s, n], label[s, n] = rng.uniform(0.05, 1.0), k % C
                    n += 1
    box, score, label = box.reshape(-1, 4), score.reshape(-1), label.reshape(-1)
    link = link_rows(box, label, score, np.repeat(np.arange(S), K), [0, S], C, link_iou, max_gap)
    return dict(box=box, score=score, label=label, keys=keys, S=S, K=K, C=C, max_gap=max_gap, link_iou=link_iou, link=link)


def members(head):
    out = {}
    for r in np.nonzero(np.asarray(head) >= 0)[0].tolist():
        out.setdefault(int(head[r]), []).append(r)
    return out


def cpu_detections(fx, dev="cpu", **kw):
    S, K = fx["S"], fx["K"]
    t = lambda a, *shape: torch.from_numpy(np.ascontiguousarray(a)).reshape(*shape).to(dev)
    count = t((fx["label"].reshape(S, K) >= 0).sum(1).astype(np.int32), S)
    return VideoDetections(fx["keys"], t(fx["box"], S, K, 4), t(fx["score"], S, K), t(fx["label"], S, K), t(np.where(fx["label"] >= 0, 0, -1).astype(np.int32), S, K),
                           t(np.zeros(S * K, np.float32), S, K), count, count.clone(), class_num=fx["C"],
                           settings=dict(link_iou=fx["link_iou"], max_gap=fx["max_gap"], min_len=1), **kw)


def cpu_actors(fx, n_actions=4, dev="cpu", **kw):
    S, K = fx["S"], fx["K"]
    t = lambda a, *shape: torch.from_numpy(np.ascontiguousarray(a)).reshape(*shape).to(dev)
    count = t((fx["label"].reshape(S, K) >= 0).sum(1).astype(np.int32), S)
    actions = np.random.default_rng(5).random((S, K, n_actions)).astype(np.float32)
    return VideoActors(fx["keys"], t(fx["box"], S, K, 4), t(fx["score"], S, K), t(np.where(fx["label"] >= 0, 0, -1).astype(np.int32), S, K), t(actions, S, K, n_actions),
                       count, count.clone(), settings=dict(link_iou=fx["link_iou"], max_gap=fx["max_gap"], min_len=1, window=1, label_thr=0.2), **kw)


# ------------------------------------------------------------------------------------------------------------------------------
# the definition
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_worked_example():
    box = np.asarray([[0, 0, 8, 8], [4, 4, 12, 12]], dtype=np.float32)
    score = np.asarray([0.25, 0.75], dtype=np.float32)
    d = dense_tube([10, 14], box, score)
    assert set(d) == DENSE_KEYS and d["frames"] == [10, 11, 12, 13, 14] and d["key_index"].tolist() == [0, 0, 0, 0, 1]
    assert d["boxes"].dtype == np.float32 and d["boxes"][1].tolist() == [1, 1, 9, 9] and d["boxes"].tolist() == [[j, j, 8 + j, 8 + j] for j in range(5)]
    assert d["frame_scores"].dtype == np.float32 and d["frame_scores"].tolist() == [0.25, 0.375, 0.5, 0.625, 0.75]
    rows = dense_rows(box, score, [0, 0], [10, 14], 1, 2)
    assert rows["row_span"].tolist() == [4, 1] and rows["row_next"].tolist() == [1, -1] and rows["dense_box"].shape == (2, 4, 4)
    same_dense(dense_from_rows([0, 1], [10, 14], 1, rows), d)


def test_every_key_frame_carries_its_rows_bytes_and_the_frames_are_the_range():
    box, score, head, tubes = planted_dense()
    assert dense_extent(PLANTED_KEYS, 2) == 136 == max(1, max(PLANTED_KEYS[min(s + 3, 5)] - PLANTED_KEYS[s] for s in range(6)))
    assert dense_extent(PLANTED_KEYS, 0) == 130 and dense_extent([7], 2) == 1 and dense_extent([], 2) == 1 and dense_extent([2, 5, 6], 5) == 4
    fill_box, fill_score = np.full((18, 136, 4), np.float32(-7.5)), np.full((18, 136), np.float32(-7.5))
    d = dense_rows(box, score, head, PLANTED_KEYS, 3, 2, dense_box=fill_box, dense_score=fill_score)
    assert d["dense_box"] is fill_box and d["dense_score"] is fill_score
    span, nxt = d["row_span"], d["row_next"]
    assert span[[0, 3, 6, 9, 12, 15]].tolist() == [1, 5, 1, 130, 1, 1] and nxt[[0, 3, 6, 9, 12, 15]].tolist() == [3, 6, 9, 12, 15, -1]
    assert span[[1, 10, 13]].tolist() == [7, 130, 1] and nxt[[1, 10, 13]].tolist() == [10, 13, -1]        # bridged over two slots: filled
    assert span[[5, 8]].tolist() == [5, 1] and nxt[[5, 8]].tolist() == [8, -1]
    assert span[[11, 14, 17]].tolist() == [130, 1, 1] and nxt[[11, 14, 17]].tolist() == [14, 17, -1]      # not ended's successor
    rest = np.setdiff1d(np.arange(18), np.concatenate(list(tubes.values())))
    assert (span[rest] == 0).all() and (nxt[rest] == -1).all()
    for r in range(18):                                                   # behind the span: as the caller allocated it
        assert (fill_box[r, span[r]:] == -7.5).all() and (fill_score[r, span[r]:] == -7.5).all()
        if span[r]:
            assert bits(fill_box[r, 0]).tolist() == bits(box[r]).tolist() and bits(fill_score[r, :1]).tolist() == bits(score[r:r + 1]).tolist()
    for rows in tubes.values():
        t = dense_from_rows(rows, PLANTED_KEYS, 3, d)
        first, last = PLANTED_KEYS[rows[0] // 3], PLANTED_KEYS[rows[-1] // 3]
        assert t["frames"] == list(range(first, last + 1)) and len(t["boxes"]) == len(t["frame_scores"]) == len(t["key_index"]) == last - first + 1
        for i, r in enumerate(rows):
            at = PLANTED_KEYS[r // 3] - first
            assert t["key_index"][at] == i and bits(t["boxes"][at]).tolist() == bits(box[r]).tolist()
            assert bits(t["frame_scores"][at:at + 1]).tolist() == bits(score[r:r + 1]).tolist()
        assert (np.diff(t["key_index"]) >= 0).all() and t["key_index"][-1] == len(rows) - 1
    # the arithmetic, spelt out for one in-between frame: one subtraction, one product, one sum, one conversion
    a, b, j, g = box[9].astype(np.float64), box[12].astype(np.float64), 77, 130
    want = (a + (b - a) * (np.float64(j) / np.float64(g))).astype(np.float32)
    assert bits(fill_box[9, j]).tolist() == bits(want).tolist()


def test_a_one_row_tube_is_one_frame():
    d = dense_tube([42], [[1, 2, 3, 4]], [0.5])
    assert d["frames"] == [42] and d["boxes"].tolist() == [[1, 2, 3, 4]] and d["frame_scores"].tolist() == [0.5] and d["key_index"].tolist() == [0]
    rows = dense_rows([[1, 2, 3, 4], [5, 6, 7, 8]], [0.5, 0.25], [0, 1], [42, 50], 1, 2)
    assert rows["row_span"].tolist() == [1, 1] and rows["row_next"].tolist() == [-1, -1]
    empty = dense_tube([], np.zeros((0, 4), np.float32), np.zeros(0, np.float32))
    assert empty["frames"] == [] and empty["boxes"].shape == (0, 4)


def test_an_infinite_coordinate_stays_infinite_at_its_key_frame():
    box = np.asarray([[0, 0, np.inf, 8], [4, 4, 12, 12]], dtype=np.float32)
    d = dense_tube([0, 4], box, [0.5, np.nan])
    assert bits(d["boxes"][0]).tolist() == bits(box[0]).tolist() and np.isinf(d["boxes"][0, 2])
    assert d["boxes"][1:4, :2].tolist() == [[1, 1], [2, 2], [3, 3]]
    assert (bits(d["boxes"][1:4, 2]) == QNAN).all() and (bits(d["frame_scores"][1:4]) == QNAN).all()       # inf + -inf: one NaN, always the same
    assert bits(d["boxes"][4]).tolist() == bits(box[1]).tolist() and np.isnan(d["frame_scores"][4]) and d["frame_scores"][0] == 0.5


def test_bad_arguments():
    for keys in ([3, 3], [5, 4], [0, 2, 1]):
        with pytest.raises(ValueError, match="ascending"):
            dense_tube(keys, np.zeros((len(keys), 4)), np.zeros(len(keys)))
        with pytest.raises(ValueError, match="ascending"):
            dense_rows(np.zeros((len(keys), 4)), np.zeros(len(keys)), [-1] * len(keys), keys, 1, 0)
        with pytest.raises(ValueError, match="ascending"):
            dense_extent(keys, 0)
    with pytest.raises(ValueError):
        dense_rows(np.zeros((2, 4)), np.zeros(2), [0, 0], [1, 2], 1, 0, G=0)


def test_a_G_too_small_is_the_escape():
    box, score, head, _ = planted_dense()
    full = dense_rows(box, score, head, PLANTED_KEYS, 3, 2)
    d = dense_rows(box, score, head, PLANTED_KEYS, 3, 2, G=129)
    gone = full["row_span"] > 129
    assert np.nonzero(gone)[0].tolist() == [9, 10, 11] and (d["row_span"][gone] == -1).all() and (d["dense_box"][gone] == 0).all()
    assert np.array_equal(d["row_span"][~gone], full["row_span"][~gone]) and np.array_equal(d["row_next"][~gone], full["row_next"][~gone])
    same_bits(d["dense_box"][~gone], full["dense_box"][~gone][:, :129])


@pytest.mark.parametrize("seed", range(1, 9))
def test_dense_tube_equals_dense_rows(seed):
    fx = seeded(seed)
    rows_of = members(fx["link"]["row_head"])
    assert len(rows_of) >= 3 and max(len(r) for r in rows_of.values()) >= 4
    d = dense_rows(fx["box"], fx["score"], fx["link"]["row_head"], fx["keys"], fx["K"], fx["max_gap"])
    assert d["dense_box"].shape == (fx["S"] * fx["K"], dense_extent(fx["keys"], fx["max_gap"]), 4)
    bridged = 0
    for h, rows in rows_of.items():
        bridged += sum(b // fx["K"] - a // fx["K"] > 1 for a, b in zip(rows[:-1], rows[1:]))
        assert [int(d["row_next"][r]) for r in rows] == rows[1:] + [-1]
        same_dense(dense_from_rows(rows, fx["keys"], fx["K"], d), dense_tube([fx["keys"][r // fx["K"]] for r in rows], fx["box"][rows], fx["score"][rows]))
    print("seed %d: %d tubes, %d bridged gaps" % (seed, len(rows_of), bridged))


def test_the_seeded_records_bridge_gaps():
    assert sum(b // 5 - a // 5 > 1 for seed in range(1, 9) for rows in members(seeded(seed)["link"]["row_head"]).values()
               for a, b in zip(rows[:-1], rows[1:])) >= 8


# ------------------------------------------------------------------------------------------------------------------------------
# the host path of tubes(dense=True) / tracks(dense=True)
# ------------------------------------------------------------------------------------------------------------------------------
def wanted(plain, keys, K, box, score, head):
    """the dense dicts the definition gives for the plain tubes / tracks ``plain`` of a store: ``dense_rows`` over the store, the tube's rows
    found through its first row"""
    d = dense_rows(box, score, head, keys, K, 99)                          # any max_gap at least the linker's finds the same successors
    rows_of = members(head)
    by_first = {(keys[rows[0] // K], bits(box[rows[0]]).tobytes()): rows for rows in rows_of.values()}
    return [dense_from_rows(by_first[(t["frames"][0], bits(t["boxes"][0]).tobytes())], keys, K, d) for t in plain]


def assert_densified(got, plain, want, key_set):
    assert len(got) == len(plain) == len(want) >= 2
    for g, p, w in zip(got, plain, want):
        assert set(p) == key_set and set(g) == key_set | ADDED
        assert g["keys"] == p["frames"] and g["length"] == p["length"] == len(g["keys"]) and g["score"] == p["score"]
        same_bits(g["key_boxes"], p["boxes"])
        same_dense(g, w)
        assert g["frames"] == list(range(g["keys"][0], g["keys"][-1] + 1))
        for k in key_set - {"frames", "boxes"}:
            assert np.array_equal(np.asarray(g[k]), np.asarray(p[k]), equal_nan=True) if isinstance(p[k], np.ndarray) else g[k] == p[k], k


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_the_host_path_equals_the_definition(seed, capsys):
    fx = seeded(seed)
    vd = cpu_detections(fx)
    plain, got = vd.tubes(), vd.tubes(dense=True)
    assert vd.tubes_path == "host" and [set(t) for t in plain] == [TUBE_KEYS] * len(plain)
    assert_densified(got, plain, wanted(plain, fx["keys"], fx["K"], fx["box"], fx["score"], fx["link"]["row_head"]), TUBE_KEYS)
    assert [set(t) for t in vd.tubes(dense=False)] == [TUBE_KEYS] * len(plain)
    va = cpu_actors(fx)
    plain, got = va.tracks(), va.tracks(dense=True)
    assert va.tracks_path == "host" and [set(t) for t in plain] == [TRACK_KEYS] * len(plain)
    link = actor_tracks(va.boxes.numpy(), va.actor.numpy(), va.queries.numpy(), va.actions.numpy(), fx["S"], fx["K"], fx["link_iou"], fx["max_gap"], 1)
    assert_densified(got, plain, wanted(plain, fx["keys"], fx["K"], fx["box"], fx["score"], link["row_head"]), TRACK_KEYS)
    for t in got:                                                          # a per-key field per frame, through key_index
        assert t["smooth"][t["key_index"]].shape == (len(t["frames"]), 4) and t["actor"][t["key_index"]].shape == (len(t["frames"]),)
    capsys.readouterr()


def test_the_padded_stores_of_the_nms_tests(capsys):
    vd = padded_detections()
    plain, got = vd.tubes(), vd.tubes(dense=True)
    assert [t["frames"] for t in got] == [list(range(0, 51)), list(range(0, 51)), list(range(10, 41)), list(range(20, 51))]
    assert [t["keys"] for t in got] == [t["frames"] for t in plain] and all(np.array_equal(t["key_index"], np.arange(len(t["frames"])) // 10) for t in got)
    kept = vd.tubes(nms=0.3, dense=True)                                   # NMS decides on the key rows; only the kept tubes are made dense
    assert [t["frames"][0] for t in kept] == [0, 0, 20] and set(kept[0]) == TUBE_KEYS | ADDED
    for k, i in zip(kept, (0, 1, 3)):
        same_dense(k, got[i])
    tracks = padded_actors().tracks(nms=0.3, dense=True)
    assert [len(t["frames"]) for t in tracks] == [151, 91] and [t["length"] for t in tracks] == [6, 4]
    capsys.readouterr()


def test_the_default_comes_from_the_record_and_unsorted_keys_are_refused(capsys):
    for cls, fn in ((VideoDetections, "tubes"), (VideoActors, "tracks"), (VideoStream, "tubes"), (VideoStream, "tracks")):
        assert inspect.signature(getattr(cls, fn)).parameters["dense"].default is None
    fx = seeded(1)
    on = cpu_detections(fx, dense=True)
    assert set(on.tubes()[0]) == TUBE_KEYS | ADDED and set(on.tubes(dense=False)[0]) == TUBE_KEYS and cpu_detections(fx).dense is False
    assert set(cpu_actors(fx, dense=True).tracks()[0]) == TRACK_KEYS | ADDED
    bad = dict(fx, keys=fx["keys"][:3] + [fx["keys"][2]] + fx["keys"][4:])
    for rec, fn in ((cpu_detections(bad), "tubes"), (cpu_actors(bad), "tracks")):
        assert len(getattr(rec, fn)()) >= 2                                # without dense nobody minds
        with pytest.raises(ValueError, match="ascending"):
            getattr(rec, fn)(dense=True)
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------------------------------------
# the stream's assemblers
# ------------------------------------------------------------------------------------------------------------------------------
CUTS = ((), (1,), (4, 5), (2, 7, 11), tuple(range(1, 12)))


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_the_tube_assembler_fed_piecewise_gives_the_whole_video_dense_tubes(seed, capsys):
    fx = seeded(seed)
    S, K = fx["S"], fx["K"]
    vd = cpu_detections(fx)
    want, plain = vd.tubes(dense=True), vd.tubes()
    heads = sorted(members(fx["link"]["row_head"]))
    box, label, score = fx["box"].reshape(S, K, 4), fx["label"].reshape(S, K), fx["score"].reshape(S, K)
    for dense in (True, False):
        for cuts in CUTS:
            linker, asm = TubeLinker(fx["C"], fx["link_iou"], fx["max_gap"]), TubeAssembler(fx["max_gap"], 1)
            edges, got = [0] + list(cuts) + [S], []
            for a, b in zip(edges[:-1], edges[1:]):
                rec = linker.push(box[a:b].reshape(-1, 4), label[a:b].reshape(-1), score[a:b].reshape(-1), K)
                asm.add(a, fx["keys"][a:b], box[a:b], label[a:b], rec["row_head"].reshape(-1, K), rec["row_score"].reshape(-1, K), rec["row_len"].reshape(-1, K),
                        scores=score[a:b])
                got += asm.take(dense)
            asm.end()
            got = sorted(got + asm.take(dense), key=lambda t: t["head"])
            assert [t["head"] for t in got] == heads and len(got) == len(want)
            for g, w, p in zip(got, want, plain):
                assert set(g) == (TUBE_KEYS | ADDED if dense else TUBE_KEYS) | {"head"}
                if dense:
                    same_dense(g, w)
                    same_bits(g["key_boxes"], w["key_boxes"])
                    assert (g["keys"], g["cls"], g["length"], g["score"]) == (w["keys"], w["cls"], w["length"], w["score"])
                else:
                    assert g["frames"] == p["frames"] and g["score"] == p["score"]
                    same_bits(g["boxes"], p["boxes"])
    asm = TubeAssembler(2, 1)                                              # fed as before this option existed: plain tubes, and a clear refusal
    asm.add(0, [0], box[:1], label[:1], np.asarray([[0, -1, -1, -1, -1]]), np.full((1, K), 0.5), np.ones((1, K), np.int64))
    asm.end()
    with pytest.raises(RuntimeError, match="scores"):
        asm.take(True)
    capsys.readouterr()


@pytest.mark.parametrize("seed", (1, 2))
def test_the_track_assembler_fed_piecewise_gives_the_whole_video_dense_tracks(seed, capsys):
    fx = seeded(seed)
    S, A, C = fx["S"], fx["K"], 4
    va = cpu_actors(fx, C)
    want = va.tracks(dense=True)
    box, actor, query, act = va.boxes.numpy(), va.actor.numpy(), va.queries.numpy(), va.actions.numpy()
    for cuts in CUTS:
        tracker, asm = ActorTracker(fx["link_iou"], fx["max_gap"], 1), TrackAssembler(A, fx["max_gap"], 1, 1, 0.2)
        edges, got = [0] + list(cuts) + [S], []
        for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
            last = i == len(edges) - 2
            rec = tracker.push(box[a:b].reshape(-1, 4), actor[a:b].reshape(-1), query[a:b].reshape(-1), act[a:b].reshape(-1, C), A, flush=last)
            n = b - a
            asm.add(a, fx["keys"][a:b], box[a:b], actor[a:b], query[a:b], act[a:b], rec["row_head"].reshape(n, A), rec["row_score"].reshape(n, A),
                    rec["row_len"].reshape(n, A), rec["row_mean"].reshape(n, A, C), rec["row_peak"].reshape(n, A, C), rec["smooth"].reshape(-1, A, C), rec["smooth_lo"])
            if last:
                asm.end()
            got += asm.take(True)
        got = sorted(got, key=lambda t: t["head"])
        assert len(got) == len(want) >= 2
        for g, w in zip(got, want):
            assert set(g) == TRACK_KEYS | ADDED | {"head"}
            same_dense(g, w)
            same_bits(g["key_boxes"], w["key_boxes"])
            same_bits(g["actor"], w["actor"])
            assert (g["keys"], g["length"], g["score"], g["labels"]) == (w["keys"], w["length"], w["score"], w["labels"])
            assert np.array_equal(g["smooth"], w["smooth"]) and np.array_equal(g["mean"], w["mean"])
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------------------------------------
# settings and the C ABI
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_config_key():
    cfg = get_cfg_defaults()
    assert cfg.CONFIG.VAL.VIDEO_MAP.DENSE is False and dense_setting(cfg) is False
    assert video_map_settings(cfg) == dict(link_iou=0.2, max_gap=2, min_len=1, thresholds=(0.2, 0.5, 0.75, "0.5:0.95"))      # the evaluators' keywords
    assert set(actor_settings(cfg)) == {"topk", "link_iou", "max_gap", "min_len", "window", "label_thr"}
    cfg.CONFIG.VAL.VIDEO_MAP.DENSE = True
    assert dense_setting(cfg) is True and "dense" not in video_map_settings(cfg)
    for v in (1, 0, "yes", None, 1.0, [True]):
        cfg = get_cfg_defaults()
        cfg.CONFIG.VAL.VIDEO_MAP.DENSE = v
        for fn in (dense_setting, video_map_settings, actor_settings):
            with pytest.raises(ValueError, match=r"CONFIG\.VAL\.VIDEO_MAP\.DENSE "):
                fn(cfg)


def test_tuber_tube_dense_is_declared_and_exported():
    declared = {name: (ret, args) for ret, name, args in lib.header_prototypes()}
    assert "tuber_tube_dense" in declared and hasattr(lib.load(), "tuber_tube_dense")
    ret, args = declared["tuber_tube_dense"]
    assert ret == "int" and [a[1] for a in args] == ["det_box", "det_score", "row_head", "slot_frame", "S", "K", "max_gap", "G", "dense_box", "dense_score",
                                                     "row_span", "row_next", "stream"]
    assert [a[0] for a in args[:4]] == ["const float*", "const float*", "const int*", "const int*"] and args[-1][0] == "hipStream_t"
