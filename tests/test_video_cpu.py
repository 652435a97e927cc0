"""Whole-video inference without a GPU (tubelet_transformer_amd/video.py): ``clip_indices`` against values worked out by hand
from the reference's lines and against a literal restatement of them, the val geometry, the refactor of ``evaluation.VideoMAP.link`` into
``evaluation.link_rows`` pinned against a copy of the loop as it was, a hand-filled CPU ``VideoDetections`` answering ``tubes()`` through the
host definition, and the declaration / export of the two new entry points."""
import numpy as np
import pytest
import torch

from tubelet_transformer_amd import lib
from tubelet_transformer_amd.evaluation import VideoMAP, _iou_one_to_many, link_rows, tube_layout, tubes_from_link
from tubelet_transformer_amd.video import VideoDetections, clip_indices, working_geometry


# ------------------------------------------------------------------------------------------------------------------------------
# clip_indices
# ------------------------------------------------------------------------------------------------------------------------------
BY_HAND = [
    ("ava", dict(T=8, rate=2, n=20), 3, [0, 2, 4, 6, 8, 10, 12, 14]),
    ("ava", dict(T=8, rate=2, n=20), 10, [2, 4, 6, 8, 10, 12, 14, 16]),
    ("ava", dict(T=8, rate=2, n=20), 18, [10, 12, 14, 16, 18, 19, 19, 19]),
    ("jhmdb", dict(T=8, rate=1, n=10), 1, [0, 0, 1, 2, 3, 4, 5, 5]),
    ("jhmdb", dict(T=8, rate=1, n=10), 8, [0, 4, 5, 6, 7, 8, 9, 9]),           # the reference's frame-0 front pad
    ("jhmdb", dict(T=8, rate=1, n=20), 5, [1, 2, 3, 4, 5, 6, 7, 8]),
    ("jhmdb", dict(T=8, rate=1, n=5), 2, [0, 0, 0, 1, 2, 3, 4, 4]),
    ("edge", dict(T=8, rate=2, n=20), 18, [10, 12, 14, 16, 18, 19, 19, 19]),
    ("edge", dict(T=8, rate=2, n=20), 1, [0, 0, 0, 0, 1, 3, 5, 7]),
]


@pytest.mark.parametrize("rule,kw,key,want", BY_HAND, ids=["%s_n%d_key%d" % (r, kw["n"], k) for r, kw, k, _ in BY_HAND])
def test_clip_indices_by_hand(rule, kw, key, want):
    got = clip_indices(kw["n"], [key], kw["T"], kw["rate"], rule)
    assert got.dtype == np.int32 and got.shape == (1, kw["T"])
    assert got[0].tolist() == want
    if rule == "ava" and key == 10:
        assert got[0, 4] == key                                         # the key frame at position T // 2


def _ava_lines(n, key, T, rate):
    """datasets/ava_frame.py:43,143-145 with timef * 30 = key, clip_len = T, frame_sample_rate = rate, len(video_frame_list) = n"""
    start_img = np.max((key - T // 2 * rate, 0))
    start_img = np.max(start_img, 0)
    end_img = start_img + T * rate
    return list(np.clip(range(start_img, end_img, rate), 0, n - 1))


def _jhmdb_lines(n, key, T):
    """datasets/jhmdb_frame.py:201-208 with mid_point = key, p_t = T // 2, clip_len = T, nframes = n (ids 0-based)"""
    p_t = T // 2
    start = max(key - p_t, 0)
    end = min(key + T - p_t, n - 1)
    frame_ids_ = [s for s in range(start, end)]
    if len(frame_ids_) < T:
        front_size = (T - len(frame_ids_)) // 2
        front = [0 for _ in range(front_size)]
        back = [end for _ in range(T - len(frame_ids_) - front_size)]
        frame_ids_ = front + frame_ids_ + back
    assert len(frame_ids_) == T
    return frame_ids_


@pytest.mark.parametrize("n,T,rate", [(20, 8, 2), (7, 8, 1), (40, 32, 2), (33, 32, 1), (100, 8, 3), (9, 5, 2)])
def test_clip_indices_sweep_against_the_cited_lines(n, T, rate):
    keys = list(range(n))
    ava = clip_indices(n, keys, T, rate, "ava")
    jh = clip_indices(n, keys, T, 1, "jhmdb")
    edge = clip_indices(n, keys, T, rate, "edge")
    for k in keys:
        assert ava[k].tolist() == [int(v) for v in _ava_lines(n, k, T, rate)], ("ava", k)
        assert jh[k].tolist() == _jhmdb_lines(n, k, T), ("jhmdb", k)
        assert edge[k].tolist() == [min(max(k + (i - T // 2) * rate, 0), n - 1) for i in range(T)], ("edge", k)
        assert edge[k, T // 2] == k
    for a in (ava, jh, edge):
        assert a.min() >= 0 and a.max() <= n - 1


def test_clip_indices_refuses_what_it_cannot_answer():
    with pytest.raises(ValueError, match="outside"):
        clip_indices(10, [10], 8, 1, "ava")
    with pytest.raises(ValueError, match="rule"):
        clip_indices(10, [1], 8, 1, "nearest")
    with pytest.raises(ValueError, match=">= 1"):
        clip_indices(10, [1], 8, 0, "ava")
    assert clip_indices(10, [], 8, 1, "ava").shape == (0, 8)


def test_working_geometry_is_the_val_pipeline():
    # datasets/ava_frame.py:86-91,127 then Resize_Custom (video_transforms.py:210-227), by hand
    assert working_geometry(96, 160, 48) == (48, 80, 0, 0, 48, 80)
    assert working_geometry(48, 80, 48) == (48, 80, 0, 0, 48, 80)
    assert working_geometry(256, 340, 256) == (256, 340, 0, 0, 256, 340)
    assert working_geometry(240, 320, 256) == (256, 341, 0, 0, 256, 341)         # 256 * (320 / 240) = 341.33
    assert working_geometry(320, 240, 256) == (341, 256, 0, 0, 341, 256)
    nh, nw, y1, x1, h, w = working_geometry(360, 486, 256)                        # 345.6 -> 345; the window: int(256 * (345 / 256))
    assert (nh, nw, h) == (256, 345, 256) and w in (344, 345) and x1 == int(round((345 - w) / 2.0)) and y1 == 0


# ------------------------------------------------------------------------------------------------------------------------------
# the refactor of VideoMAP.link
# ------------------------------------------------------------------------------------------------------------------------------
def _old_link_loop(ev):
    """``VideoMAP.link`` as it stood before ``link_rows`` was factored out of it, kept here word for word (without the tube list)"""
    self = ev
    C, N = self.class_num, len(self.det_keys)
    lay = tube_layout(self.det_keys, self.gt_keys)
    box = np.concatenate(self._box) if self._box else np.zeros((0, 4), np.float32)
    prob = np.concatenate(self._prob) if self._prob else np.zeros((0, C + 1), np.float32)
    order = np.argsort(lay["det_slot"], kind="stable")
    box, prob, slot = box[order], prob[order], lay["det_slot"][order]
    cls = prob.argmax(axis=1) if N else np.zeros(0, dtype=np.int64)
    score = prob[np.arange(N), cls]
    counted = (cls != C) & (box[:, 0] < box[:, 2]) & (box[:, 1] < box[:, 3]) & ~np.isnan(score)
    box64 = box.astype(np.float64)
    video = np.searchsorted(lay["video_off"], slot, side="right") - 1
    head = np.full(N, -1, dtype=np.int64)
    tscore, tlen, tlast = np.zeros(N), np.zeros(N, dtype=np.int64), np.full(N, -1, dtype=np.int64)
    groups = {}
    for r in np.nonzero(counted)[0].tolist():
        groups.setdefault((int(video[r]), int(cls[r])), []).append(r)
    for rows in groups.values():
        tubes, i = [], 0
        while i < len(rows):
            s, j = slot[rows[i]], i
            while j < len(rows) and slot[rows[j]] == s:
                j += 1
            cur, i = rows[i:j], j
            active = [t for t in tubes if s - t[3] <= self.max_gap + 1]
            for t in tubes:
                if s - t[3] > self.max_gap + 1:
                    tscore[t[0]], tlen[t[0]], tlast[t[0]] = t[1] / t[2], t[2], t[3]
            active.sort(key=lambda t: (-(t[1] / t[2]), t[0]))
            claimed = set()
            for t in active:
                cand = [r for r in cur if r not in claimed]
                if not cand:
                    break
                with np.errstate(all="ignore"):
                    iou = _iou_one_to_many(box64[t[4]], box64[cand])
                best = None
                for r, u in zip(cand, iou):
                    if u >= self.link_iou and (best is None or score[r] > score[best]):
                        best = r
                if best is not None:
                    claimed.add(best)
                    head[best] = t[0]
                    t[1] += float(score[best]); t[2] += 1; t[3] = s; t[4] = best
            tubes = active
            for r in cur:
                if r not in claimed:
                    head[r] = r
                    tubes.append([r, float(score[r]), 1, s, r])
        for t in tubes:
            tscore[t[0]], tlen[t[0]], tlast[t[0]] = t[1] / t[2], t[2], t[3]
    return dict(order=order, det_box=box, det_prob=prob, row_slot=slot, row_cls=cls, row_head=head, tube_score=tscore, tube_len=tlen,
                tube_last=tlast, layout=lay)


def _seeded_store(seed=7, C=3, max_gap=1):
    """two videos, frames with gaps (some wider than max_gap), a few boxes jittered around three anchors so that tubes form and cross, scores on a
    coarse lattice (ties within a frame and between tubes), a NaN score, a no-object row, a box that is no box"""
    rng = np.random.default_rng(seed)
    ev = VideoMAP(class_num=C, link_iou=0.2, max_gap=max_gap)
    anchors = np.array([[10, 10, 50, 60], [30, 15, 70, 65], [100, 20, 140, 80]], dtype=np.float32)
    n = 0
    for video, frames in (("a", [1, 2, 3, 5, 6, 9, 10, 14]), ("b_x", [4, 5, 7, 8, 9])):
        for f in frames:
            for _ in range(int(rng.integers(2, 6))):
                box = anchors[rng.integers(3)] + rng.integers(-6, 7, 4).astype(np.float32)
                prob = np.full(C + 1, 0.01, dtype=np.float32)
                prob[rng.integers(0, C + 1 if n % 9 == 4 else C)] = np.float32(rng.integers(2, 10)) / np.float32(10)      # lattice: ties
                if n == 11:
                    prob[:] = np.nan
                if n == 17:
                    box[2] = box[0]
                ev.add_detections(["%s-%d" % (video, f)], [box], [prob])
                n += 1
    ev.add_ground_truth(["a-1", "b_x-9"], [[10, 10, 50, 60], [30, 15, 70, 65]], [0, 1])
    return ev


@pytest.mark.parametrize("max_gap", (0, 1, 2))
def test_link_is_what_it_was_and_link_rows_is_its_body(max_gap):
    ev = _seeded_store(max_gap=max_gap)
    old = _old_link_loop(ev)
    # the fixture holds what it claims: ties in a slot, equal tube means, gaps on both sides of max_gap, a NaN, a no-object row, a bad box
    score = old["det_prob"][np.arange(len(old["row_cls"])), old["row_cls"]]
    assert np.isnan(score).any() and (old["row_cls"] == ev.class_num).any() and (old["det_box"][:, 0] >= old["det_box"][:, 2]).any()
    assert any(len(s) != len(set(s)) for s in ([score[old["row_slot"] == k].tolist() for k in np.unique(old["row_slot"])]))
    heads = np.nonzero(old["row_head"] == np.arange(len(score)))[0]
    assert len(set(old["tube_score"][heads].tolist())) < len(heads) and old["tube_len"].max() >= 3
    new = ev.link()
    assert sorted(k for k in new if k != "tubes") == sorted(old)
    for k in ("order", "det_box", "det_prob", "row_slot", "row_cls", "row_head", "tube_len", "tube_last"):
        assert np.array_equal(new[k], old[k], equal_nan=k == "det_prob"), k
        assert new[k].dtype == old[k].dtype, k
    assert np.array_equal(new["tube_score"].view(np.int64), old["tube_score"].view(np.int64))
    assert [t["rows"] for t in new["tubes"]] == [t["rows"] for t in tubes_from_link(old)]
    rows = link_rows(old["det_box"], old["row_cls"], score, old["row_slot"], old["layout"]["video_off"], ev.class_num, ev.link_iou, ev.max_gap)
    assert sorted(rows) == ["row_head", "tube_last", "tube_len", "tube_score"]
    for k in ("row_head", "tube_len", "tube_last"):
        assert np.array_equal(rows[k], old[k]), k
    assert np.array_equal(rows["tube_score"].view(np.int64), old["tube_score"].view(np.int64))
    # a label outside [0, C) is not counted, whatever side it is on
    lab = old["row_cls"].astype(np.int32)
    lab[lab == ev.class_num] = -1
    again = link_rows(old["det_box"], lab, score, old["row_slot"], old["layout"]["video_off"], ev.class_num, ev.link_iou, ev.max_gap)
    assert np.array_equal(again["row_head"], old["row_head"])


# ------------------------------------------------------------------------------------------------------------------------------
# VideoDetections on the CPU
# ------------------------------------------------------------------------------------------------------------------------------
A, B2 = (0, 0, 10, 10), (40, 0, 54, 10)


def _hand_store(K=3):
    """key frames 0, 30, 60, 90, 120: class 1 follows box A through 0, 30, (gap) 90; class 0 sits at B2 in 30 and 60; 120 is empty"""
    rows = {0: [(A, 1, 0.9)], 30: [((1, 0, 11, 10), 1, 0.7), (B2, 0, 0.6)], 60: [(B2, 0, 0.8)], 90: [((2, 0, 12, 10), 1, 0.5)], 120: []}
    keys = sorted(rows)
    n = len(keys)
    boxes, scores = torch.zeros(n, K, 4), torch.zeros(n, K)
    labels, queries = torch.full((n, K), -1, dtype=torch.int32), torch.full((n, K), -1, dtype=torch.int32)
    count = torch.zeros(n, dtype=torch.int32)
    for i, k in enumerate(keys):
        for j, (box, c, s) in enumerate(rows[k]):
            boxes[i, j], scores[i, j], labels[i, j], queries[i, j] = torch.tensor(box, dtype=torch.float32), s, c, j
        count[i] = len(rows[k])
    return VideoDetections(keys, boxes, scores, labels, queries, torch.zeros(n, K), count, count.clone(), class_num=2)


def test_a_cpu_store_answers_tubes_by_the_host_definition(capsys):
    vd = _hand_store()
    assert vd.tubes_path is None
    tubes = vd.tubes(link_iou=0.2, max_gap=1, min_len=1)
    assert vd.tubes_path == "host"
    assert "linking on the host" in capsys.readouterr().err
    assert [(t["cls"], t["frames"], t["length"]) for t in tubes] == [(2, [0, 30, 90], 3), (1, [30, 60], 2)]      # head order, cls 1-based
    f32 = lambda v: float(np.float32(v))
    assert tubes[0]["score"] == (f32(0.9) + f32(0.7) + f32(0.5)) / 3 and tubes[1]["score"] == (f32(0.6) + f32(0.8)) / 2
    assert tubes[0]["boxes"].tolist() == [list(map(float, A)), [1, 0, 11, 10], [2, 0, 12, 10]]
    # max_gap counts KEY frames: with none allowed the tube of class 2 splits at the empty key frame 60
    assert [(t["cls"], t["frames"]) for t in vd.tubes(max_gap=0)] == [(2, [0, 30]), (1, [30, 60]), (2, [90])]
    assert [(t["cls"], t["frames"]) for t in vd.tubes(max_gap=0, min_len=2)] == [(2, [0, 30]), (1, [30, 60])]
    assert len(vd.tubes()) == 2                                         # the defaults: link_iou 0.2, max_gap 2, min_len 1
    host = vd.to_host()
    assert [h["key"] for h in host] == [0, 30, 60, 90, 120] and [h["count"] for h in host] == [1, 2, 1, 1, 0]
    assert host[1]["labels"].tolist() == [1, 0] and host[4]["boxes"].shape == (0, 4)
    with pytest.raises(ValueError, match="keys"):
        VideoDetections([0], vd.boxes, vd.scores, vd.labels, vd.queries, vd.aux, vd.count, vd.total, class_num=2)


def test_the_new_entry_points_are_declared_and_exported():
    declared = {name: args for _, name, args in lib.header_prototypes()}
    assert [a[1] for a in declared["tuber_video_clips"]] == ["frames", "nframes", "H", "W", "index", "B", "T", "y1", "x1", "h", "w", "lut", "out",
                                                             "stream"]
    link, ranked = declared["tuber_tube_link"], declared["tuber_tube_link_ranked"]
    assert [a[1] for a in ranked][:3] == ["det_box", "det_label", "det_score"]
    assert ranked[3:] == link[2:]                                       # everything else is tuber_tube_link's
    loaded = lib.load()
    assert hasattr(loaded, "tuber_video_clips") and hasattr(loaded, "tuber_tube_link_ranked")
