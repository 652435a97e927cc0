"""Host side of the actor tracks, no GPU: ``detect.decode_actors_host`` -- the definition of ``tuber_detect_actors`` -- against
``decode_topk_host``, whose scores its action rows are by construction; its torch restatement; ``evaluation.actor_tracks`` -- the definition of
``tuber_track_actions`` -- against ``link_rows`` and against sums worked out here on a hand-written video; ``CONFIG.VAL.ACTORS`` and its
validator; the option's signature defaults and the four C-ABI entries in the header and the built library."""
import inspect
import os
import types

import numpy as np
import pytest
import torch

from tubelet_transformer_amd import lib
from tubelet_transformer_amd.config import actor_settings, get_cfg_defaults, load_cfg
from tubelet_transformer_amd.detect import ACTOR_FIELDS, Actors, Detector, _decode_actors_torch, decode_actors_host, decode_topk_host
from tubelet_transformer_amd.evaluation import actor_tracks, link_rows
from tubelet_transformer_amd.video import VideoActors, VideoDetector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 2.0 ** -22
THR = 0.5


# ------------------------------------------------------------------------------------------------------------------------------
# decode_actors_host
# ------------------------------------------------------------------------------------------------------------------------------
def decode_fixture(seed=0, B=3, Qtot=12, C=7):
    """clip 0: queries 2 and 9 share one logits_b row (a tie between actors), query 4 has a NaN actor logit, query 5 one NaN class logit;
    clip 2: no actor"""
    rng = np.random.default_rng(seed)
    lg = rng.normal(0.0, 2.0, (B, Qtot, C)).astype(np.float32)
    lb = rng.normal(0.0, 1.0, (B, Qtot, 3)).astype(np.float32)
    lb[:, :, 1] += 1.5                                                  # most queries pass THR ...
    lb[2, :, 1] = -4.0                                                  # ... none of the last clip
    lb[0, 9] = lb[0, 2] = [0.0, 3.0, -1.0]                              # the clip's best actor, twice
    lb[0, 5] = [0.0, 2.0, -1.0]
    lb[0, 4, 1] = np.nan
    lg[0, 5, 3] = np.nan
    bx = np.concatenate([rng.uniform(0.2, 0.8, (B, Qtot, 2)), rng.uniform(0.05, 0.4, (B, Qtot, 2))], axis=-1).astype(np.float32)
    sizes = np.array([[64, 96], [240, 320], [255, 341]], dtype=np.int64)[:B]
    return lg, lb, bx, sizes


def _softmax64(x):
    x = x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        e = np.exp(x - np.max(x, axis=-1, keepdims=True))
        return e / e.sum(-1, keepdims=True)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _assert_rows_are_the_ranked_decodes(got, lg, lb, bx, sizes, q_begin, Qs):
    """every kept actor's action row, actor probability and box against decode_topk_host(score_thr = 0, K = Qs * C): the same bits at (q, c)"""
    B, _, C = lg.shape
    ranked = decode_topk_host(lg, lb, bx, sizes, "ava", THR, 0.0, Qs * C, q_begin=q_begin, Qs=Qs)
    for b in range(B):
        n = int(ranked["count"][b])
        at = {(int(q), int(c)): i for i, (q, c) in enumerate(zip(ranked["queries"][b, :n], ranked["labels"][b, :n]))}
        for a in range(int(got["count"][b])):
            q = int(got["queries"][b, a])
            for c in range(C):
                v = got["actions"][b, a, c]
                if np.isnan(v):
                    assert (q, c) not in at                             # a NaN score is no candidate of the ranked decode
                    continue
                i = at[q, c]
                assert _bits(v) == _bits(ranked["scores"][b, i])
                assert _bits(got["actor"][b, a]) == _bits(ranked["aux"][b, i])
                assert np.array_equal(_bits(got["boxes"][b, a]), _bits(ranked["boxes"][b, i]))


def test_decode_actors_rows_are_decode_topk_scores_in_actor_order():
    lg, lb, bx, sizes = decode_fixture()
    B, Q, C = lg.shape
    pb = _softmax64(lb)[..., 1]
    for A in (Q, 4, Q + 3):                                            # everything; a cut; A > Qs
        got = decode_actors_host(lg, lb, bx, sizes, THR, A)
        assert sorted(got) == sorted(ACTOR_FIELDS)
        assert got["boxes"].shape == (B, A, 4) and got["actions"].shape == (B, A, C) and got["actions"].dtype == np.float32
        _assert_rows_are_the_ranked_decodes(got, lg, lb, bx, sizes, None, Q)
        for b in range(B):
            with np.errstate(invalid="ignore"):
                actors = [q for q in range(Q) if pb[b, q] > THR]
            want = sorted(actors, key=lambda q: (-pb[b, q], q))         # pb descending, then query ascending
            n = min(len(want), A)
            assert got["total"][b] == len(want) and got["count"][b] == n
            assert got["queries"][b, :n].tolist() == want[:n]
            assert (got["queries"][b, n:] == -1).all() and not got["boxes"][b, n:].any() and not got["actor"][b, n:].any()
            assert not got["actions"][b, n:].any()
    assert got["total"].tolist()[2] == 0                                # the clip without an actor
    full = decode_actors_host(lg, lb, bx, sizes, THR, Q)
    assert full["queries"][0, :2].tolist() == [2, 9] and _bits(full["actor"][0, 0]) == _bits(full["actor"][0, 1])      # the tie, in query order
    assert 4 not in full["queries"][0]                                  # a NaN actor logit: no actor
    row5 = full["actions"][0, full["queries"][0].tolist().index(5)]
    assert np.isnan(row5[3]) and not np.isnan(np.delete(row5, 3)).any()  # a NaN class logit: NaN in the row, the row kept
    cut = decode_actors_host(lg, lb, bx, sizes, THR, 1)                # the cut in the middle of the tie keeps the smaller query
    assert cut["queries"][0].tolist() == [2] and cut["total"][0] == full["total"][0] and cut["count"][0] == 1


def test_decode_actors_takes_the_key_frames_slice_and_an_outside_slice_is_empty():
    lg, lb, bx, sizes = decode_fixture(seed=1, Qtot=12)
    qb = np.array([0, 8, 9])                                           # the last one runs out of the 12 queries
    got = decode_actors_host(lg, lb, bx, sizes, THR, 4, q_begin=qb, Qs=4)
    _assert_rows_are_the_ranked_decodes(got, lg, lb, bx, sizes, qb, 4)
    assert got["total"][1] > 0 and got["queries"][1].max() < 4
    one = decode_actors_host(lg[1:2, 8:12], lb[1:2, 8:12], bx[1:2, 8:12], sizes[1:2], THR, 4)
    for k in ACTOR_FIELDS:
        assert np.array_equal(got[k][1], one[k][0], equal_nan=True), k
    assert got["total"][2] == 0 and got["count"][2] == 0 and (got["queries"][2] == -1).all() and not got["actions"][2].any()
    neg = decode_actors_host(lg, lb, bx, sizes, THR, 4, q_begin=np.array([-1, 0, 0]), Qs=4)
    assert neg["total"][0] == 0 and neg["total"][1] > 0
    per_clip = decode_actors_host(lg, lb[:, 0], bx, sizes, THR, 4)      # logits_b [B, NB]: one probability per clip
    p = _softmax64(lb[:, 0])[:, 1]
    assert per_clip["total"].tolist() == [12 if v > THR else 0 for v in p]


def test_the_torch_restatement_equals_the_definition_on_cpu_tensors():
    lg, lb, bx, sizes = decode_fixture(seed=2)
    t = torch.from_numpy
    # the tolerance rule of the detect tests: twice the error of the fp32 torch expression against fp64 on this fixture, at least 2^-22
    pb = _softmax64(lb)[..., 1]
    with np.errstate(over="ignore"):
        s64 = (1.0 / (1.0 + np.exp(-lg.astype(np.float64)))) * pb[:, :, None]
    s32 = (t(lg).sigmoid() * t(lb).softmax(-1)[..., 1:2]).double().numpy()
    err = float(np.nanmax(np.abs(s32 - s64)))
    tol = max(2.0 * err, FLOOR)
    for A, qb, Qs in ((12, None, 12), (4, None, 12), (15, None, 12), (3, np.array([0, 8, 9], dtype=np.int32), 4)):
        want = decode_actors_host(lg, lb, bx, sizes, THR, A, q_begin=qb, Qs=Qs)
        got = _decode_actors_torch(t(lg), t(lb), t(bx), t(sizes), THR, A, None if qb is None else t(qb), Qs)
        got = dict(zip(ACTOR_FIELDS, (g.numpy() for g in got)))
        for k in ("queries", "count", "total"):
            assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
        assert np.array_equal(got["boxes"], want["boxes"])
        assert np.array_equal(np.isnan(got["actions"]), np.isnan(want["actions"]))
        for k in ("actor", "actions"):
            assert got[k].dtype == np.float32
            assert np.nanmax(np.abs(got[k].astype(np.float64) - want[k].astype(np.float64))) <= tol, k


def test_actors_to_host_trims_to_count():
    lg, lb, bx, sizes = decode_fixture()
    want = decode_actors_host(lg, lb, bx, sizes, THR, 4)
    host = Actors(*[torch.from_numpy(want[k]) for k in ACTOR_FIELDS]).to_host()
    assert [h["count"] for h in host] == want["count"].tolist() and [h["total"] for h in host] == want["total"].tolist()
    for b, h in enumerate(host):
        n = h["count"]
        assert h["actions"].shape == (n, lg.shape[2]) and h["boxes"].shape == (n, 4)
        assert np.array_equal(h["queries"], want["queries"][b, :n]) and np.array_equal(h["actions"], want["actions"][b, :n], equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------------------
# actor_tracks
# ------------------------------------------------------------------------------------------------------------------------------
LINK_IOU, MAX_GAP = 0.25, 1
P, P1, Q, R = (0, 0, 10, 10), (1, 0, 11, 10), (100, 0, 110, 10), (50, 50, 60, 60)
PAD = ((0, 0, 0, 0), 0.0, -1)
# the tracks of the fixture below, by hand: head row -> its rows (row = slot * 4 + position)
TRACKS = {0: [0, 8, 12, 16, 21], 1: [1], 13: [13, 20], 17: [17]}
# ... and the rows of the same track at most 1 slot away, per row
NEAR1 = {0: [0], 8: [8, 12], 12: [8, 12, 16], 16: [12, 16, 21], 21: [16, 21], 1: [1], 13: [13], 20: [20], 17: [17]}


def track_fixture(C=5, seed=3):
    """S = 6 key frames of A = 4 rows, max_gap = 1: (box, actor probability, query) per row.  Person P is there throughout, over an empty key
    frame (bridged); person Q leaves after key 0 and comes back at key 3, beyond the gap: a length-1 track and a new one; R appears once; the
    third row of key 5 has a query but a degenerate box: not counted.  Action values span sixteen orders of magnitude: fp32 values add exactly in
    fp64 while their exponents are less than 29 apart, so 1e-12 and smaller sit beside 0.9 -- the order of a sum then shows in its last bits."""
    slots = [
        [(P, 0.9, 3), (Q, 0.8, 1), PAD, PAD],
        [PAD, PAD, PAD, PAD],
        [(P1, 0.85, 3), PAD, PAD, PAD],
        [(P, 0.7, 2), (Q, 0.6, 1), PAD, PAD],
        [(P, 0.95, 3), (R, 0.5, 0), PAD, PAD],
        [(Q, 0.75, 1), (P, 0.65, 3), ((5, 0, 5, 10), 0.9, 2), PAD],
    ]
    box = np.array([r[0] for s in slots for r in s], dtype=np.float32)
    actor = np.array([r[1] for s in slots for r in s], dtype=np.float32)
    queries = np.array([r[2] for s in slots for r in s], dtype=np.int32)
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.integers(-16, 0, (24, C))
    actions = (rng.uniform(0.1, 0.99, (24, C)) * mag).astype(np.float32)
    actions[0, :2], actions[8, :2], actions[12, :2], actions[16, :2], actions[21, :2] = [0.9, 1e-12], [1e-12, 0.9], [0.3, 0.3], [2.5e-14, 0.7], [0.5, 3e-11]
    actions[queries < 0] = 0.0                                          # what the decode leaves behind a key's count
    return dict(box=box, actor=actor, queries=queries, actions=actions, S=6, A=4, C=C)


def _seq_mean(actions, rows, reverse=False):
    """the fp64 sum of the rows' fp32 values one after the other, divided by their number: Python floats, no numpy reduction"""
    out = []
    for c in range(actions.shape[1]):
        acc = 0.0
        for r in (rows[::-1] if reverse else rows):
            acc = acc + float(actions[r, c])
        out.append(acc / len(rows))
    return np.array(out, dtype=np.float64)


def expected_tracks(fx, window):
    """row_smooth, track_mean, track_peak of the fixture from TRACKS / NEAR1, worked out with Python floats"""
    act, N, C = fx["actions"], 24, fx["C"]
    smooth, mean, peak = np.zeros((N, C)), np.zeros((N, C)), np.zeros((N, C), dtype=np.float32)
    for h, rows in TRACKS.items():
        mean[h] = _seq_mean(act, rows)
        peak[h] = [max(float(act[r, c]) for r in rows) for c in range(C)]
        for r in rows:
            near = [r] if window == 0 else NEAR1[r] if window == 1 else rows
            smooth[r] = _seq_mean(act, near)
    return smooth, mean, peak


def test_actor_tracks_links_like_link_rows_and_aggregates_in_slot_order():
    fx = track_fixture()
    slot = np.repeat(np.arange(6), 4)
    link = link_rows(fx["box"], np.where(fx["queries"] >= 0, 0, -1), fx["actor"], slot, [0, 6], 1, LINK_IOU, MAX_GAP)
    head = link["row_head"]
    # the fixture holds what it is there for
    assert {h: np.nonzero(head == h)[0].tolist() for h in sorted(set(head[head >= 0].tolist()))} == TRACKS
    assert (fx["queries"][4:8] == -1).all() and head[8] == 0                               # an empty key frame, bridged
    assert head[1] == 1 and head[13] == 13 and slot[13] - slot[1] == 3 > MAX_GAP + 1        # a gap beyond max_gap: a new track
    assert link["tube_len"][17] == 1 and link["tube_len"][1] == 1                            # length-1 tracks
    assert fx["queries"][22] >= 0 and head[22] == -1                                         # a row that is not counted
    assert link["tube_len"][0] == 5 and link["tube_last"][0] == 5 and link["tube_last"][13] == 5
    for window in (0, 1, 6, 100):
        got = actor_tracks(fx["box"], fx["actor"], fx["queries"], fx["actions"], 6, 4, LINK_IOU, MAX_GAP, window)
        for k in ("row_head", "tube_len", "tube_last"):
            assert np.array_equal(got[k], link[k]), k
        assert np.array_equal(got["tube_score"].view(np.int64), link["tube_score"].view(np.int64))
        smooth, mean, peak = expected_tracks(fx, window)
        assert got["row_smooth"].dtype == got["track_mean"].dtype == np.float64 and got["track_peak"].dtype == np.float32
        assert np.array_equal(got["row_smooth"].view(np.int64), smooth.view(np.int64)), window
        assert np.array_equal(got["track_mean"].view(np.int64), mean.view(np.int64))
        assert np.array_equal(got["track_peak"].view(np.int32), peak.view(np.int32))
        assert not got["row_smooth"][head < 0].any()
        assert not got["track_mean"][head != np.arange(24)].any() and not got["track_peak"][head != np.arange(24)].any()
    # window 0 is the row itself, a window over the whole video the track's mean
    w0 = actor_tracks(fx["box"], fx["actor"], fx["queries"], fx["actions"], 6, 4, LINK_IOU, MAX_GAP, 0)
    assert np.array_equal(w0["row_smooth"][head >= 0], fx["actions"][head >= 0].astype(np.float64))
    assert np.array_equal(got["row_smooth"][21], got["track_mean"][0])
    # the order of the sum is part of the definition: summed backwards, the mean of the long track is another number
    rev = _seq_mean(fx["actions"], TRACKS[0], reverse=True)
    assert (rev.view(np.int64) != expected_tracks(fx, 0)[1][0].view(np.int64)).any()
    assert np.allclose(rev, got["track_mean"][0], rtol=1e-12)


def test_actor_tracks_propagates_nan_like_numpy():
    fx = track_fixture()
    fx["actions"][12, 4] = np.nan
    got = actor_tracks(fx["box"], fx["actor"], fx["queries"], fx["actions"], 6, 4, LINK_IOU, MAX_GAP, 1)
    assert np.isnan(got["track_mean"][0, 4]) and np.isnan(got["track_peak"][0, 4]) and not np.isnan(got["track_mean"][0, :4]).any()
    assert np.isnan(got["row_smooth"][[8, 12, 16], 4]).all() and not np.isnan(got["row_smooth"][[0, 21], 4]).any()


def test_video_actors_tracks_on_a_cpu_store_answers_on_the_host(capsys):
    fx = track_fixture()
    t = lambda a, *shape: torch.from_numpy(np.ascontiguousarray(a)).reshape(*shape)
    count = t((fx["queries"].reshape(6, 4) >= 0).sum(1).astype(np.int32), 6)
    keys = [0, 30, 60, 90, 120, 150]
    va = VideoActors(keys, t(fx["box"], 6, 4, 4), t(fx["actor"], 6, 4), t(fx["queries"], 6, 4), t(fx["actions"], 6, 4, 5), count, count.clone(),
                     settings=dict(link_iou=LINK_IOU, max_gap=MAX_GAP, min_len=1, window=1, label_thr=0.2))
    tracks = va.tracks()
    assert va.tracks_path == "host" and "tracks on the host" in capsys.readouterr().err
    smooth, mean, peak = expected_tracks(fx, 1)
    assert [tr["frames"] for tr in tracks] == [[0, 60, 90, 120, 150], [0], [90, 150], [120]]
    assert [tr["length"] for tr in tracks] == [5, 1, 2, 1]
    for tr, (h, rows) in zip(tracks, sorted(TRACKS.items())):
        assert np.array_equal(tr["boxes"], fx["box"][rows]) and np.array_equal(tr["actor"], fx["actor"][rows])
        assert tr["queries"].tolist() == fx["queries"][rows].tolist() and np.array_equal(tr["actions"], fx["actions"][rows])
        assert np.array_equal(tr["smooth"], smooth[rows]) and np.array_equal(tr["mean"], mean[h]) and np.array_equal(tr["peak"], peak[h])
        assert tr["score"] == _seq_mean(fx["actor"][:, None], rows)[0]
        keep = [c for c in range(5) if mean[h][c] >= 0.2]
        assert tr["labels"] == sorted(keep, key=lambda c: (-mean[h][c], c))
    assert tracks[0]["labels"][:2] == [1, 0] and tracks[0]["mean"][1] > tracks[0]["mean"][0] >= 0.2
    assert [tr["length"] for tr in va.tracks(min_len=2)] == [5, 2]
    assert [tr["frames"] for tr in va.tracks(max_gap=2)][1] == [0, 90, 150]                  # a longer gap: Q is one track
    host = va.to_host()
    assert [h["key"] for h in host] == keys and [h["count"] for h in host] == [2, 0, 1, 2, 2, 3] and host[5]["actions"].shape == (3, 5)


# ------------------------------------------------------------------------------------------------------------------------------
# settings, signatures, the C ABI
# ------------------------------------------------------------------------------------------------------------------------------
def test_actor_settings_defaults_and_validation():
    cfg = get_cfg_defaults()
    a = cfg.CONFIG.VAL.ACTORS
    assert sorted(a) == ["LABEL_THR", "LINK_IOU", "MAX_GAP", "MIN_LEN", "TOPK", "WINDOW"]
    assert actor_settings(cfg) == dict(topk=15, link_iou=0.2, max_gap=2, min_len=1, window=1, label_thr=0.05)
    for name in ("TubeR_CSN152_AVA21.yaml", "TubeR_CSN50_AVA21.yaml"):
        assert actor_settings(load_cfg(os.path.join(ROOT, "configuration", name)))["topk"] == 15      # min(QUERY_NUM, 64 // 3)
    cfg.CONFIG.VAL.VIDEO_MAP.MAX_GAP, cfg.CONFIG.VAL.VIDEO_MAP.LINK_IOU, cfg.CONFIG.VAL.DETECT.SCORE_THR = 7, 0.4, 0.3
    assert actor_settings(cfg) == dict(topk=8, link_iou=0.4, max_gap=7, min_len=1, window=1, label_thr=0.3)          # inherited; 64 // 8
    a.TOPK, a.LINK_IOU, a.MAX_GAP, a.MIN_LEN, a.WINDOW, a.LABEL_THR = 5, 0.5, 0, 3, 4, 0.25
    assert actor_settings(cfg) == dict(topk=5, link_iou=0.5, max_gap=0, min_len=3, window=4, label_thr=0.25)
    bad = dict(TOPK=(0, -1, 2.5, True, "3"), LINK_IOU=(-0.1, 1.5, "x", True, float("nan")), MAX_GAP=(-1, 1.5, True), MIN_LEN=(0, 2.5, False),
               WINDOW=(-1, 0.5, None, True), LABEL_THR=(-0.1, 1.1, "y", float("nan")))
    for key, values in bad.items():
        for v in values:
            cfg = get_cfg_defaults()
            cfg.CONFIG.VAL.ACTORS[key] = v
            with pytest.raises(ValueError, match=r"CONFIG\.VAL\.ACTORS\.%s" % key):
                actor_settings(cfg)


def test_the_option_is_off_by_default_and_refuses_a_single_label_model():
    assert inspect.signature(Detector.__init__).parameters["actors"].default is None
    assert inspect.signature(VideoDetector.__init__).parameters["actors"].default is None
    cfg = load_cfg(os.path.join(ROOT, "configuration", "Tuber_CSN152_JHMDB.yaml"))
    stub = types.SimpleNamespace(dataset_mode="jhmdb", training=False, query_embed=types.SimpleNamespace(num_embeddings=10))
    assert Detector(cfg, stub, graphed=False).actors is None
    with pytest.raises(ValueError, match="actors"):
        Detector(cfg, stub, graphed=False, actors=4)
    with pytest.raises(ValueError, match="actors"):
        VideoDetector(cfg, stub, graphed=False, actors=4)
    ava = types.SimpleNamespace(dataset_mode="ava", training=False, query_embed=types.SimpleNamespace(num_embeddings=15))
    cfg = load_cfg(os.path.join(ROOT, "configuration", "TubeR_CSN50_AVA21.yaml"))
    assert Detector(cfg, ava, graphed=False, actors=15).actors == 15
    for v in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="actors"):
            Detector(cfg, ava, graphed=False, actors=v)


def test_the_four_entries_are_declared_and_exported():
    protos = {name: (ret, args) for ret, name, args in lib.header_prototypes()}
    ava, act = protos["tuber_detect_ava"][1], protos["tuber_detect_actors"][1]
    assert act[:13] == ava[:13] and [n for _, n in act[13:]] == ["A", "det_box", "det_actor", "det_query", "det_actions", "det_count", "det_total", "stream"]
    assert [n for _, n in protos["tuber_track_actions"][1]] == ["actions", "row_head", "tube_last", "S", "A", "C", "window", "row_smooth", "track_mean",
                                                                "track_peak", "stream"]
    assert protos["tuber_detect_actors_limits"] == ("int", [("int", "which")]) == protos["tuber_track_actions_limits"]
    loaded = lib.load()
    for name in ("tuber_detect_actors", "tuber_detect_actors_limits", "tuber_track_actions", "tuber_track_actions_limits"):
        assert hasattr(loaded, name), name
    assert [lib.query("tuber_detect_actors_limits", w) for w in (0, 1, 2, 3)] == [1024, 1024, 8, -1]
    assert [lib.query("tuber_track_actions_limits", w) for w in (0, 1, 2)] == [lib.query("tuber_tube_link_max_active"), 4096, -1]
    assert lib.query("tuber_detect_limits", 2) == 8                     # the siblings' query is what it was
