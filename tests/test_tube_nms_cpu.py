"""Spatio-temporal tube NMS on the host: ``evaluation.tube_nms`` by hand on planted link records, ``VideoMAP(tube_nms=)``,
``CONFIG.VAL.TUBE_NMS`` and the linkage of ``tuber_tube_nms`` / ``tuber_tube_nms_work_bytes``.  No GPU."""
import inspect
import os
import types

import numpy as np
import pytest
import torch

from test_video_map_cpu import _bits, _case_evaluator, _ev, _same_results
from tubelet_transformer_amd import lib, synth
from tubelet_transformer_amd.config import actor_settings, get_cfg_defaults, load_cfg, tube_nms_settings, video_map_settings
from tubelet_transformer_amd.evaluation import VideoMAP, tube_nms
from tubelet_transformer_amd.video import VideoActors, VideoDetections, VideoDetector, VideoStream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_ENTRY_POINTS = ("tuber_tube_nms", "tuber_tube_nms_work_bytes")
BOX = (20.0, 10.0, 60.0, 70.0)
FAR = (200.0, 10.0, 240.0, 70.0)


def shifted(box, dx):
    return (box[0] + dx, box[1], box[2] + dx, box[3])


def record(tubes, videos, slots):
    """A link record by hand, as ``VideoMAP.link()`` leaves it: ``tubes`` = [(video, class, score, {slot in the video: box})]; the rows in layout
    order (video, slot, then the order of ``tubes``), a tube's head its first row.  -> (record, the head row of every tube)"""
    rows = sorted((v * slots + s, i) for i, (v, c, sc, boxes) in enumerate(tubes) for s in boxes)
    N = len(rows)
    rec = dict(det_box=np.zeros((N, 4), np.float32), row_slot=np.zeros(N, np.int64), row_cls=np.zeros(N, np.int64), row_head=np.full(N, -1, np.int64),
               tube_score=np.zeros(N), tube_len=np.zeros(N, np.int64), tube_last=np.full(N, -1, np.int64),
               layout=dict(videos=["v%d" % v for v in range(videos)], V=videos, S=videos * slots, video_off=np.arange(videos + 1, dtype=np.int64) * slots,
                           first_frame=np.zeros(videos, np.int64), parsed=True))
    heads = {}
    for r, (g, i) in enumerate(rows):
        v, c, sc, boxes = tubes[i]
        h = heads.setdefault(i, r)
        rec["det_box"][r], rec["row_slot"][r], rec["row_cls"][r], rec["row_head"][r] = boxes[g - v * slots], g, c, h
        rec["tube_score"][h], rec["tube_len"][h], rec["tube_last"][h] = sc, rec["tube_len"][h] + 1, g
    return rec, [heads[i] for i in range(len(tubes))]


def span(box, first, last, step=1):
    return {s: box for s in range(first, last + 1, step)}


def planted():
    """the planted cases 1-5 as ONE record of 10 videos, 8 slots each, C = 3 -> (record, {name: head row})"""
    near = shifted(BOX, 2.0)                                               # IoU 38 / 42 with BOX
    tubes = [
        # 1: duplicates -- different scores, equal scores, different classes, different videos
        ("dup_hi", 0, 1, 0.9, span(BOX, 0, 3)), ("dup_lo", 0, 1, 0.8, span(near, 0, 3)),
        ("tie_first", 1, 2, 0.7, span(BOX, 0, 3)), ("tie_second", 1, 2, 0.7, span(near, 0, 3)),
        ("cls_a", 2, 0, 0.9, span(BOX, 0, 3)), ("cls_b", 2, 1, 0.8, span(near, 0, 3)),
        ("vid_a", 3, 0, 0.9, span(BOX, 0, 3)), ("vid_b", 4, 0, 0.8, span(near, 0, 3)),
        # 2: slots 0..3 against slots 2..5, the same boxes: stIoU = 2.0 / 6.0
        ("edge_a", 5, 0, 0.9, span(BOX, 0, 3)), ("edge_b", 5, 0, 0.8, span(BOX, 2, 5)),
        # 3: a chain -- IoU(a, b) = IoU(b, c) = 28 / 52, IoU(a, c) = 16 / 64
        ("chain_a", 6, 2, 0.9, span(BOX, 0, 3)), ("chain_b", 6, 2, 0.8, span(shifted(BOX, 12.0), 0, 3)), ("chain_c", 6, 2, 0.7, span(shifted(BOX, 24.0), 0, 3)),
        # 4: a one-row tube with the best score on a long tube's box; a two-row tube that overlaps only the short one above the threshold
        ("long", 7, 1, 0.8, span(BOX, 0, 4)), ("short", 7, 1, 0.95, {2: BOX}), ("beside", 7, 1, 0.6, {2: BOX, 6: FAR}),
        # 5: interleaved rows share no slot
        ("even", 8, 0, 0.9, span(BOX, 0, 6, 2)), ("odd", 8, 0, 0.8, span(BOX, 1, 7, 2)),
        # a NaN score ranks last
        ("nan", 9, 0, float("nan"), span(BOX, 0, 2)), ("number", 9, 0, 0.1, span(near, 0, 2)),
    ]
    rec, heads = record([t[1:] for t in tubes], 10, 8)
    return rec, {t[0]: h for t, h in zip(tubes, heads)}


def keep_of(rec, where, nms_iou, min_len=1):
    keep = tube_nms(rec, nms_iou, min_len)
    heads = set(where.values())
    assert keep.dtype == np.uint8 and all(keep[r] == 2 for r in range(len(keep)) if r not in heads)
    return {name: int(keep[h]) for name, h in where.items()}


def test_a_duplicate_is_suppressed_within_its_video_and_class():
    rec, where = planted()
    k = keep_of(rec, where, 0.3)
    assert (k["dup_hi"], k["dup_lo"]) == (1, 0)
    assert where["tie_first"] < where["tie_second"] and (k["tie_first"], k["tie_second"]) == (1, 0)      # equal scores: the later head goes
    assert (k["cls_a"], k["cls_b"], k["vid_a"], k["vid_b"]) == (1, 1, 1, 1)
    assert (k["number"], k["nan"]) == (1, 0)                              # a NaN score is visited last


def test_the_threshold_is_strict():
    rec, where = planted()
    third = 2.0 / 6.0
    k = keep_of(rec, where, third)
    assert (k["edge_a"], k["edge_b"]) == (1, 1)
    k = keep_of(rec, where, float(np.nextafter(third, 0.0)))
    assert (k["edge_a"], k["edge_b"]) == (1, 0)


def test_a_suppressed_tube_suppresses_nothing():
    rec, where = planted()
    k = keep_of(rec, where, 0.3)
    assert 16.0 / 64.0 < 0.3 < 28.0 / 52.0
    assert (k["chain_a"], k["chain_b"], k["chain_c"]) == (1, 0, 1)
    k = keep_of(rec, where, 0.2)                                           # below IoU(a, c): a suppresses both
    assert (k["chain_a"], k["chain_b"], k["chain_c"]) == (1, 0, 0)


def test_tubes_shorter_than_min_len_take_no_part():
    rec, where = planted()
    # min_len 1: the short tube goes first; stIoU(long, short) = 1 / 5, stIoU(beside, short) = 1 / 2, stIoU(beside, long) = 1 / 6
    k = keep_of(rec, where, 0.3, min_len=1)
    assert (k["short"], k["long"], k["beside"]) == (1, 1, 0)
    k = keep_of(rec, where, 0.3, min_len=2)
    assert (k["short"], k["long"], k["beside"]) == (2, 1, 1)
    k = keep_of(rec, where, 0.1, min_len=2)                                # under a threshold the long tube reaches, it is the long tube that suppresses
    assert (k["short"], k["long"], k["beside"]) == (2, 1, 0)


def test_interleaved_tubes_share_no_slot():
    rec, where = planted()
    for thr in (0.0, 0.3):
        k = keep_of(rec, where, thr)
        assert (k["even"], k["odd"]) == (1, 1), thr


def test_bad_arguments():
    rec, _ = planted()
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            tube_nms(rec, bad)
    with pytest.raises(ValueError):
        tube_nms(rec, 0.3, 0)


def _planted_evaluator(dup_score, **kw):
    """one ground-truth tube over frames 1..4, a true positive on it and a duplicate two pixels beside it"""
    dets = [("v", f, BOX, 0, 0.9) for f in range(1, 5)] + [("v", f, shifted(BOX, 2.0), 0, dup_score) for f in range(1, 5)]
    return _ev(dets, [("v", f, BOX, 0, 0) for f in range(1, 5)], max_gap=0, thresholds=(0.5,), **kw)


def test_video_map_with_tube_nms():
    """One ground-truth tube, a true-positive tube and its lower-scored duplicate.  With NMS the duplicate is neither matched nor ranked
    (flag 2) and the same tube takes the ground truth in both runs.  The class's AP is 1.0 in BOTH runs: a false positive ranked behind the
    last true positive does not lower VOC AP (``test_a_tube_shorter_than_min_len_is_not_counted``: only one ranked in front costs), so the
    figure 0.5 "without NMS" cannot come from this case; the second case below is the one where the AP moves."""
    plain, nms = _planted_evaluator(0.8), _planted_evaluator(0.8, tube_nms=0.3)
    assert "tube_keep" not in plain.link() and nms.link()["tube_keep"].tolist() == [1, 0, 2, 2, 2, 2, 2, 2]
    (_, fp, _), (_, fn, _) = plain.match(), nms.match()
    assert fp[0.5].tolist() == [1, 0, 2, 2, 2, 2, 2, 2] and fn[0.5].tolist() == [1, 2, 2, 2, 2, 2, 2, 2]     # the same tube takes the ground truth
    print("planted duplicate: AP without NMS %r, with NMS %r" % (plain.evaluate()[0.5][1], nms.evaluate()[0.5][1]))
    assert plain.evaluate()[0.5] == (1.0, {1: 1.0}) and nms.evaluate()[0.5] == (1.0, {1: 1.0})
    # a tube beside the ground truth with the best score and its duplicate, both ranked in front of the true positive, which neither
    # suppresses (IoU 12 / 68 < 0.3): two false positives in front without NMS, one with it
    off = shifted(BOX, 28.0)
    dets = ([("v", f, off, 0, 0.99) for f in range(1, 5)] + [("v", f, shifted(off, 2.0), 0, 0.95) for f in range(1, 5)] +
            [("v", f, BOX, 0, 0.9) for f in range(1, 5)])
    gts = [("v", f, BOX, 0, 0) for f in range(1, 5)]
    assert _ev(dets, gts, max_gap=0, thresholds=(0.5,)).evaluate()[0.5][1] == {1: 1.0 / 3.0}
    with_nms = _ev(dets, gts, max_gap=0, thresholds=(0.5,), tube_nms=0.3)
    assert with_nms.evaluate()[0.5][1] == {1: 0.5} and with_nms.link()["tube_keep"][:3].tolist() == [1, 0, 1]
    # a link record without the key (the device's, read back) is completed by match()
    link = {k: v for k, v in with_nms.link().items() if k != "tube_keep"}
    assert with_nms.match(link)[1][0.5][:3].tolist() == [0, 2, 1]


def test_without_the_keyword_nothing_changes():
    case = synth.synthetic_video_map_case(6, 16, 10, 21, seed=5)
    want = _case_evaluator(case).evaluate()
    _same_results(_case_evaluator(case, tube_nms=None).evaluate(), want)
    _same_results(VideoMAP.evaluate(_case_evaluator(case)), want)
    ev = _case_evaluator(case, tube_nms=0.3)
    n_gt, flags, link = ev.match()
    keep = link["tube_keep"]
    assert np.array_equal(keep, tube_nms(link, 0.3, 1)) and (keep == 0).sum() >= 1
    for thr, fl in flags.items():
        assert (fl[keep == 0] == 2).all() and ((fl == 2) == (keep != 1)).all(), thr
    got = ev.evaluate()
    assert list(got) == list(want) and any(_bits(got[t][0]) != _bits(want[t][0]) for t in want)


def test_tube_nms_settings():
    cfg = get_cfg_defaults()
    t = cfg.CONFIG.VAL.TUBE_NMS
    assert t.IOU is None and t.ACTORS_IOU is None and tube_nms_settings(cfg) == dict(iou=None, actors_iou=None)
    cfg.CONFIG.VAL.TUBE_NMS.IOU, cfg.CONFIG.VAL.TUBE_NMS.ACTORS_IOU = 0.3, 1
    assert tube_nms_settings(cfg) == dict(iou=0.3, actors_iou=1.0)
    for key in ("IOU", "ACTORS_IOU"):
        for v in (-0.1, 1.5, "0.3", float("nan"), True, [0.3]):
            cfg = get_cfg_defaults()
            cfg.CONFIG.VAL.TUBE_NMS[key] = v
            with pytest.raises(ValueError, match=r"CONFIG\.VAL\.TUBE_NMS\.%s " % key):
                tube_nms_settings(cfg)
    cfg = get_cfg_defaults()
    assert video_map_settings(cfg) == dict(link_iou=0.2, max_gap=2, min_len=1, thresholds=(0.2, 0.5, 0.75, "0.5:0.95"))
    assert set(actor_settings(cfg)) == {"topk", "link_iou", "max_gap", "min_len", "window", "label_thr"}


def _padded(tubes, S, K):
    """the padded [S][K] tensors of hand-made tubes [(label, score, {slot: box})]: a tube's rows carry its score"""
    box, score, label = np.zeros((S, K, 4), np.float32), np.zeros((S, K), np.float32), np.full((S, K), -1, np.int32)
    fill = [0] * S
    for lab, sc, boxes in tubes:
        for s, b in boxes.items():
            box[s, fill[s]], score[s, fill[s]], label[s, fill[s]] = b, sc, lab
            fill[s] += 1
    return box, score, label, np.asarray(fill, np.int32)


PADDED_TUBES = [(0, 0.9, span(BOX, 0, 5)), (0, 0.6, span(shifted(BOX, 3.0), 1, 4)), (1, 0.8, span(shifted(BOX, 3.0), 0, 5)), (0, 0.5, span(FAR, 2, 5))]


def padded_detections(dev="cpu", **kw):
    box, score, label, count = _padded(PADDED_TUBES, 6, 4)
    t = lambda a: torch.from_numpy(a).to(dev)
    return VideoDetections([10 * s for s in range(6)], t(box), t(score), t(label), t(np.where(label >= 0, 0, -1).astype(np.int32)), t(np.zeros((6, 4), np.float32)),
                           t(count), t(count.copy()), class_num=2, settings=dict(link_iou=0.2, max_gap=0, min_len=1), **kw)


def padded_actors(dev="cpu", **kw):
    box, score, label, count = _padded(PADDED_TUBES, 6, 4)
    rng = np.random.default_rng(3)
    actions = rng.random((6, 4, 5)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)
    return VideoActors([30 * s for s in range(6)], t(box), t(score), t(np.where(label >= 0, 0, -1).astype(np.int32)), t(actions), t(count), t(count.copy()),
                       settings=dict(link_iou=0.2, max_gap=0, min_len=1, window=1, label_thr=0.2), **kw)


def test_tubes_and_tracks_on_a_cpu_store(capsys):
    vd = padded_detections()
    plain = vd.tubes()
    assert vd.tubes_path == "host" and [(t["cls"], t["length"]) for t in plain] == [(1, 6), (2, 6), (1, 4), (1, 4)]
    kept = vd.tubes(nms=0.3)                                              # the class-0 copy on slots 1..4 goes: 4 * IoU / 6 > 0.3; class 1 stays
    assert [(t["cls"], t["length"]) for t in kept] == [(1, 6), (2, 6), (1, 4)] and kept[2]["boxes"][0].tolist() == list(FAR)
    assert [_bits(t["score"]) for t in kept] == [_bits(plain[i]["score"]) for i in (0, 1, 3)]
    assert len(padded_detections(nms_iou=0.3).tubes()) == 3 and len(padded_detections(nms_iou=0.3).tubes(nms=1.0)) == 4
    with pytest.raises(ValueError, match="nms"):
        vd.tubes(nms=1.5)
    va = padded_actors()
    tracks = va.tracks()
    assert va.tracks_path == "host" and [t["length"] for t in tracks] == [6, 6, 4, 4]
    kept = va.tracks(nms=0.3)                                             # class-agnostic: both copies go
    assert [t["length"] for t in kept] == [6, 4] and kept[0]["score"] == tracks[0]["score"] and kept[1]["boxes"][0].tolist() == list(FAR)
    assert np.array_equal(kept[0]["mean"], tracks[0]["mean"]) and np.array_equal(kept[1]["smooth"], tracks[3]["smooth"])
    assert len(padded_actors(nms_iou=0.3).tracks()) == 2
    capsys.readouterr()


def test_the_detector_carries_the_defaults_and_the_stream_ignores_them(capsys):
    assert inspect.signature(VideoDetections.tubes).parameters["nms"].default is None
    assert inspect.signature(VideoActors.tracks).parameters["nms"].default is None
    assert "nms" not in inspect.signature(VideoStream.tubes).parameters and "nms" not in inspect.signature(VideoStream.tracks).parameters
    stub = types.SimpleNamespace(dataset_mode="jhmdb", training=False, query_embed=types.SimpleNamespace(num_embeddings=10))
    cfg = load_cfg(os.path.join(ROOT, "configuration", "Tuber_CSN152_JHMDB.yaml"))
    vd = VideoDetector(cfg, stub, graphed=False)
    assert vd.nms == dict(iou=None, actors_iou=None) and vd.settings == dict(link_iou=0.2, max_gap=2, min_len=1)
    VideoStream(cfg, stub, graphed=False)
    assert "TUBE_NMS" not in capsys.readouterr().err
    cfg.CONFIG.VAL.TUBE_NMS.IOU = 0.3
    vd = VideoDetector(cfg, stub, graphed=False)
    assert vd.nms == dict(iou=0.3, actors_iou=None) and vd.settings == dict(link_iou=0.2, max_gap=2, min_len=1)
    vs = VideoStream(cfg, stub, graphed=False)
    err = capsys.readouterr().err
    assert err.count("CONFIG.VAL.TUBE_NMS is ignored") == 1 and vs.settings == dict(link_iou=0.2, max_gap=2, min_len=1)
    cfg.CONFIG.VAL.TUBE_NMS.IOU = 1.5
    with pytest.raises(ValueError, match="TUBE_NMS.IOU"):
        VideoDetector(cfg, stub, graphed=False)


def test_new_entry_points_are_declared_and_exported():
    declared = {name: (ret, args) for ret, name, args in lib.header_prototypes()}
    L = lib.load()
    for name in NEW_ENTRY_POINTS:
        assert name in declared and hasattr(L, name), name
    ret, args = declared["tuber_tube_nms"]
    assert ret == "int" and [a[1] for a in args] == ["det_box", "slot_off", "video_off", "row_cls", "row_head", "tube_score", "tube_len", "tube_last", "V", "S",
                                                     "N", "C", "max_rows", "min_len", "nms_iou", "work", "tube_keep", "stream"]
    assert declared["tuber_tube_nms_work_bytes"] == ("long", [("long", "N")])
    assert lib.query("tuber_tube_nms_work_bytes", 0) == 0 and lib.query("tuber_tube_nms_work_bytes", -3) == 0
    sizes = [lib.query("tuber_tube_nms_work_bytes", n) for n in (1, 2, 3, 100, 101, 5000)]
    assert sizes == sorted(sizes) and all(s % 16 == 0 for s in sizes) and sizes[0] >= 65 * 4
