"""Video-mAP on the GPU (csrc/tube_map.hip, device_map.DeviceVideoMAP): ``tuber_tube_link`` and ``tuber_tube_match`` directly against the host
definition ``evaluation.VideoMAP`` on planted fixtures, ``DeviceVideoMAP.evaluate_video()`` against ``VideoMAP.evaluate()``, the bounds
(negative return codes: nothing is launched; the store falls back to the host) and ``validate_tuber_ucf_detection`` with
``CONFIG.VAL.VIDEO_MAP``.

Bounds: classes, heads, lengths, last slots and flags are decisions: equal exactly.  A tube's score is the same sequential fp64 sum in slot
order on both sides, divided once: equal bit for bit.  AP: the derived bounds of tests/test_device_map_ucf_gpu.py, nothing measured: per class
|AP_device - AP_host| <= 2 * (n_gt + 3) * 2^-53; a mean over K classes: the mean of those bounds plus 2 * (K + 1) * 2^-53; "0.5:0.95", a mean
of ten such means: the mean of their bounds plus 2 * 11 * 2^-53."""
import os

import numpy as np
import pytest
import torch

from test_tube_nms_cpu import BOX, FAR, planted, record, shifted, span
from test_video_map_cpu import _bits, _case_evaluator, _same_results, _store
from tubelet_transformer_amd import device_map, lib, synth
from tubelet_transformer_amd.config import load_cfg, video_map_settings
from tubelet_transformer_amd.device_map import DeviceFrameMAPUCF, DeviceVideoMAP
from tubelet_transformer_amd.evaluation import VIDEO_MAP_RANGE, VideoMAP, tubes_from_link, validate_tuber_ucf_detection
from tubelet_transformer_amd.tuber import build_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
U = 2.0 ** -53
THRESHOLDS = (0.2, 0.5, 0.75)
SLOTS_A = (1, 2, 17, 40, 70, 5, 9)


def rc(name, *args):
    """the launcher's return code, without lib.call's raise"""
    fn = getattr(lib.load(), name)
    sig = lib._sigs[name]
    if len(args) == len(sig) - 1:
        args = args + (lib.current_stream(),)
    return fn(*[lib._conv(v, t) for v, (t, _) in zip(args, sig)])


def ap_bound(n_gt):
    return 2 * (n_gt + 3) * U


def mean_bound(n_gts):
    return float(np.mean([ap_bound(n) for n in n_gts])) + 2 * (len(n_gts) + 1) * U


# ------------------------------------------------------------------------------------------------------------------------------
# fixtures for the kernels
# ------------------------------------------------------------------------------------------------------------------------------
def _prob_rows(rng, tops, classes, C):
    """[n, C + 1] fp32: ``tops[i]`` in column ``classes[i]``, the rest well below it"""
    p = rng.uniform(0.0, 0.04, (len(tops), C + 1)).astype(np.float32)
    p[np.arange(len(tops)), classes] = tops
    return p


def _fixture_a(seed=1):
    """7 videos of 1, 2, 17, 40, 70, 5 and 9 slots, C = 3, 0..10 rows per slot.  Video 0: one frame.  Video 1: the link whose IoU is exactly
    LINK_IOU.  Video 2: scores in eighths (equal scores inside a slot and across tubes) and the planted rows that are not counted.  Video 3:
    two ground-truth tubes of one class with different extents (explicit ids 8 and 3).  Video 4: longer than a wave is wide, with three
    empty slots.  Video 5: detections only.  Video 6: ground truth only.  -> (VideoMAP settings-free case dict, planted rows by name)"""
    C = 3
    rng = np.random.default_rng(seed)
    det, gt, planted = [], [], {}                           # det: (key, box, prob row); gt: (key, box, class, tube id)

    def moving(u, c0, vel, wh):
        ctr = c0 + vel * u
        return np.concatenate([ctr - wh / 2, ctr + wh / 2]).astype(np.float32).astype(np.float64)

    def video(v, frames, tubes, eighths=False, empty=(), with_gt=True, with_det=True, spurious=3, jitter=0.02, drop=0.1, echo=0.5, exact=None):
        for f in range(1, frames + 1):
            key, rows = "vid%d-%d" % (v, f), []
            u = (f - 1) / max(frames - 1, 1)
            for t in tubes:
                if not t["first"] <= f <= t["last"]:
                    continue
                gb = moving(u, t["c0"], t["vel"], t["wh"])
                if with_gt:
                    gt.append((key, gb, t["cls"], t["id"]))
                if f in (t["first"], t["last"]) or rng.random() >= drop:
                    rows.append((gb + rng.normal(0, jitter, 4) * np.tile(t["wh"], 2), t["cls"], rng.uniform(0.7, 0.95)))
                    if rng.random() < echo:                 # a competing, looser copy
                        rows.append((gb + rng.normal(0, 0.08, 4) * np.tile(t["wh"], 2), t["cls"], rng.uniform(0.5, 0.8)))
            for _ in range(int(rng.integers(0, spurious + 1))):
                p = rng.uniform(0, 200, 2)
                rows.append((np.concatenate([p, p + rng.uniform(20, 80, 2)]), int(rng.integers(0, C)), rng.uniform(0.3, 0.7)))
            while exact and f in exact and len(rows) < exact[f]:
                p = rng.uniform(0, 200, 2)
                rows.append((np.concatenate([p, p + rng.uniform(20, 80, 2)]), int(rng.integers(0, C)), rng.uniform(0.3, 0.7)))
            if not with_det or f in empty:
                rows = []
            rows = [rows[i] for i in rng.permutation(len(rows))][:exact[f] if exact and f in exact else 10]
            for box, c, s in rows:
                s = np.float32(round(s * 8) / 8) if eighths else np.float32(s)
                det.append((key, np.asarray(box, dtype=np.float32), _prob_rows(rng, [s], [c], C)[0]))

    tube = lambda i, cls, first, last: dict(id=i, cls=cls, first=first, last=last, c0=rng.uniform(80, 160, 2), vel=rng.uniform(-40, 40, 2),
                                            wh=rng.uniform(40, 70, 2))
    video(0, 1, [tube(0, 1, 1, 1)], echo=1.0)
    # video 1: (0, 0, 5, 4) lies inside (0, 0, 10, 10): IoU = 20 / (100 + 20 - 20) = 0.2 = LINK_IOU, exactly; its twin one pixel shorter misses
    gt.append(("vid1-1", np.asarray([0.0, 0, 10, 10]), 0, 0)); gt.append(("vid1-2", np.asarray([0.0, 0, 10, 10]), 0, 0))
    planted["exact_head"] = len(det); det.append(("vid1-1", np.asarray([0, 0, 10, 10], np.float32), _prob_rows(rng, [np.float32(0.9)], [0], C)[0]))
    planted["below"] = len(det); det.append(("vid1-2", np.asarray([0, 0, 5, 3.5], np.float32), _prob_rows(rng, [np.float32(0.95)], [0], C)[0]))
    planted["exact"] = len(det); det.append(("vid1-2", np.asarray([0, 0, 5, 4], np.float32), _prob_rows(rng, [np.float32(0.6)], [0], C)[0]))
    n1 = len(det)
    video(2, 17, [tube(0, 0, 1, 17), tube(1, 2, 3, 14)], eighths=True, spurious=4, exact={9: 6})
    # planted in video 2, frame 9 (rows are appended: they come last in their slot, which then has 10 rows)
    box = np.asarray([100, 100, 150, 150], np.float32)
    planted["no_object"] = len(det); det.append(("vid2-9", box, _prob_rows(rng, [np.float32(0.9)], [C], C)[0]))
    nan = _prob_rows(rng, [np.float32(0.5)], [0], C)[0]; nan[1] = np.nan
    planted["nan"] = len(det); det.append(("vid2-9", box, nan))
    planted["x1_eq_x2"] = len(det); det.append(("vid2-9", np.asarray([100, 100, 100, 150], np.float32), _prob_rows(rng, [np.float32(0.9)], [0], C)[0]))
    planted["y1_gt_y2"] = len(det); det.append(("vid2-9", np.asarray([100, 150, 150, 100], np.float32), _prob_rows(rng, [np.float32(0.9)], [2], C)[0]))
    n2 = len(det)
    video(3, 40, [tube(8, 1, 1, 30), tube(3, 1, 15, 40)], jitter=0.015, drop=0.0)
    video(4, 70, [tube(0, 2, 1, 70), tube(1, 0, 10, 60)], empty=(20, 21, 22), jitter=0.015)
    video(5, 5, [tube(0, 1, 1, 5)], with_gt=False)
    video(6, 9, [tube(0, 0, 1, 9), tube(1, 2, 2, 7)], with_det=False)
    case = dict(C=C, det_keys=[d[0] for d in det], det_boxes=np.stack([d[1] for d in det]), det_probs=np.stack([d[2] for d in det]),
                gt_keys=[g[0] for g in gt], gt_boxes=np.stack([g[1] for g in gt]), gt_classes=[g[2] for g in gt], gt_tubes=[g[3] for g in gt])
    assert n1 < planted["no_object"] < n2
    return case, planted


def _fixture_b():
    """one video of 3 slots, C = 3: 64 rows of one class in slots 0 and 1 (with max_gap = 0 the active-tube bound, met exactly), 5 in slot 2"""
    C = 3
    rng = np.random.default_rng(8)
    grid = np.asarray([[40.0 * (i % 8), 40.0 * (i // 8), 40.0 * (i % 8) + 30, 40.0 * (i // 8) + 30] for i in range(64)])
    det_keys, boxes, classes, tops = [], [], [], []
    for f, n in ((1, 64), (2, 64), (3, 5)):
        idx = rng.permutation(64)[:n]
        for k, i in enumerate(idx):
            det_keys.append("big-%d" % f)
            boxes.append(grid[i] + rng.normal(0, 1.5, 4) + ([25.0, 0, 25.0, 0] if f == 2 and k < 8 else [0.0] * 4))    # 8 rows of slot 1 slide to the neighbour
            classes.append(1)
            tops.append(np.float32(0.5 + 0.45 * rng.random()))
    gt = [("big-%d" % f, grid[j] + 1.0, 1, j) for f in (1, 2, 3) for j in (0, 9)]
    return dict(C=C, det_keys=det_keys, det_boxes=np.asarray(boxes, dtype=np.float32), det_probs=_prob_rows(rng, tops, classes, C),
                gt_keys=[g[0] for g in gt], gt_boxes=np.stack([g[1] for g in gt]), gt_classes=[g[2] for g in gt], gt_tubes=[g[3] for g in gt])


def _host(case, max_gap, min_len):
    ev = VideoMAP(class_num=case["C"], link_iou=0.2, max_gap=max_gap, min_len=min_len, thresholds=THRESHOLDS)
    ev.add_detections(case["det_keys"], case["det_boxes"], case["det_probs"])
    ev.add_ground_truth(case["gt_keys"], case["gt_boxes"], case["gt_classes"], case["gt_tubes"])
    return ev


def _operands(ev, link, dev):
    """the kernels' operands from the host evaluator's layout, built here (not by device_map.py)"""
    lay = link["layout"]
    S, V = lay["S"], lay["V"]
    gt, _ = ev.st_iou(link)
    rank, per = {}, {}
    for key in sorted(gt):
        rank[key] = per[key[:2]] = per.get(key[:2], 0)
        per[key[:2]] += 1
    flat = sorted((s, key[1], rank[key], key) for key, g in gt.items() for s in g)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(dev)
    off = lambda slots: np.concatenate([[0], np.cumsum(np.bincount(np.asarray(slots, dtype=np.int64), minlength=S))])
    rows, grows = off(link["row_slot"]), off([f[0] for f in flat])
    return dict(V=V, S=S, N=len(link["row_slot"]), G=len(flat), det_box=up(link["det_box"], np.float32), det_prob=up(link["det_prob"], np.float32),
                slot_off=up(rows, np.int32), video_off=up(lay["video_off"], np.int32), max_rows=int(np.diff(rows).max()),
                gt_box=up(np.asarray([gt[f[3]][f[0]] for f in flat]).reshape(-1, 4), np.float64), gt_cls=up([f[1] for f in flat], np.int32),
                gt_tube=up([f[2] for f in flat], np.int32), gt_off=up(grows, np.int32), max_gt_rows=int(np.diff(grows).max()),
                max_gt_tubes=max(per.values()))


def _device_link(o, C, max_gap, dev):
    N = o["N"]
    out = dict(row_cls=torch.full((N,), -99, dtype=torch.int32, device=dev), row_head=torch.full((N,), -99, dtype=torch.int32, device=dev),
               tube_score=torch.zeros(N, dtype=torch.float64, device=dev), tube_len=torch.zeros(N, dtype=torch.int32, device=dev),
               tube_last=torch.full((N,), -1, dtype=torch.int32, device=dev))
    lib.call("tuber_tube_link", o["det_box"], o["det_prob"], o["slot_off"], o["video_off"], o["V"], o["S"], N, C, o["max_rows"], 0.2, max_gap,
             out["row_cls"], out["row_head"], out["tube_score"], out["tube_len"], out["tube_last"])
    return out


def _device_match(o, d, C, min_len, dev):
    T, N = len(THRESHOLDS), o["N"]
    flags = torch.full((T, N), 77, dtype=torch.uint8, device=dev)
    work = torch.full((N * max(o["max_gt_tubes"], 1),), float("nan"), dtype=torch.float64, device=dev)
    thr = torch.tensor(THRESHOLDS, dtype=torch.float64, device=dev)
    lib.call("tuber_tube_match", o["det_box"], o["slot_off"], o["video_off"], d["row_cls"], d["row_head"], d["tube_score"], d["tube_len"],
             d["tube_last"], o["gt_box"], o["gt_cls"], o["gt_tube"], o["gt_off"], thr, o["V"], o["S"], N, o["G"], C, T, o["max_rows"],
             o["max_gt_rows"], o["max_gt_tubes"], min_len, work, flags)
    return flags.cpu().numpy()


def _check_not_degenerate(ev, link, flags, overlaps):
    """what the fixture must exercise, asserted on the host evaluator"""
    values = [x for row in overlaps.values() for x in row.values()]
    for thr in THRESHOLDS:
        assert min(abs(x - thr) for x in values) > 1e-9, thr             # the order of the stIoU sum is free: no decision may hang on it
        assert (flags[thr] == 1).sum() >= 1 and (flags[thr] == 0).sum() >= 1, thr
    assert sum(len(t["frames"]) > 3 for t in link["tubes"]) >= 5
    claims = {}
    for t in link["tubes"]:
        if len(t["frames"]) >= ev.min_len and overlaps[t["head"]]:
            key = max(overlaps[t["head"]], key=lambda k: overlaps[t["head"]][k])
            if overlaps[t["head"]][key] >= THRESHOLDS[0]:
                claims[key] = claims.get(key, 0) + 1
    assert max(claims.values()) >= 2, "no ground-truth tube is contested by two tubes"


def _compare(case, max_gap, min_len, dev, check=True):
    ev = _host(case, max_gap, min_len)
    n_gt, flags, link = ev.match()
    if check:
        _check_not_degenerate(ev, link, flags, ev.st_iou(link)[1])
    o = _operands(ev, link, dev)
    d = _device_link(o, case["C"], max_gap, dev)
    got = {k: v.cpu().numpy() for k, v in d.items()}
    for k in ("row_cls", "row_head", "tube_len", "tube_last"):
        assert np.array_equal(got[k], link[k]), (k, np.argwhere(got[k] != link[k])[:10].ravel())
    assert np.array_equal(got["tube_score"].view(np.int64), link["tube_score"].view(np.int64))
    dflags = _device_match(o, d, case["C"], min_len, dev)
    for i, thr in enumerate(THRESHOLDS):
        assert np.array_equal(dflags[i], flags[thr]), (thr, np.argwhere(dflags[i] != flags[thr])[:10].ravel())
    again = _device_match(o, _device_link(o, case["C"], max_gap, dev), case["C"], min_len, dev)
    assert np.array_equal(again, dflags)
    return ev, link, flags, got


@pytest.fixture(scope="module")
def fixture_a():
    return _fixture_a()


@pytest.mark.parametrize("max_gap,min_len", [(0, 1), (2, 1), (2, 3), (0, 3)])
def test_tube_link_and_match_equal_the_host_on_fixture_a(dev, fixture_a, max_gap, min_len):
    case, planted = fixture_a
    ev, link, flags, got = _compare(case, max_gap, min_len, dev)
    lay = link["layout"]
    assert np.diff(lay["video_off"]).tolist() == list(SLOTS_A) and lay["V"] == 7
    per_slot = np.bincount(link["row_slot"], minlength=lay["S"])
    assert per_slot.max() == 10 and (per_slot == 0).sum() >= 12 and per_slot[lay["video_off"][6]:].sum() == 0
    assert not [k for k in case["gt_keys"] if k.startswith("vid5-")] and not [k for k in case["det_keys"] if k.startswith("vid6-")]
    # the planted rows, by layout row
    where = {name: int(np.nonzero(link["order"] == r)[0][0]) for name, r in planted.items()}
    head, cls = got["row_head"], got["row_cls"]
    assert head[where["exact"]] == where["exact_head"] and head[where["below"]] == where["below"]      # IoU == LINK_IOU links; the higher score just under it does not
    assert cls[where["no_object"]] == case["C"] and head[where["no_object"]] == -1
    assert cls[where["nan"]] == 1 and head[where["nan"]] == -1
    assert head[where["x1_eq_x2"]] == -1 and head[where["y1_gt_y2"]] == -1 and cls[where["x1_eq_x2"]] == 0 and cls[where["y1_gt_y2"]] == 2
    # equal scores inside a slot and across tubes (video 2), two same-class ground-truth tubes with different extents (video 3)
    v2 = (link["row_slot"] >= lay["video_off"][2]) & (link["row_slot"] < lay["video_off"][3]) & (head >= 0)
    tops = link["det_prob"][v2].max(axis=1)
    assert len(np.unique(tops)) <= 8 < v2.sum()
    means = got["tube_score"][np.nonzero(v2 & (head == np.arange(len(head))))[0]]
    assert len(np.unique(means)) < len(means)
    gt, _ = ev.st_iou(link)
    assert sorted(k for k in gt if k[0] == 3) == [(3, 1, 3), (3, 1, 8)] and len(gt[(3, 1, 3)]) == 26 and len(gt[(3, 1, 8)]) == 30
    if max_gap == 2:
        assert any(t["frames"][-1] - t["frames"][0] + 1 > len(t["frames"]) for t in link["tubes"])       # a bridged gap
    if min_len == 3:
        short = [t["head"] for t in link["tubes"] if len(t["frames"]) < 3]
        assert short and (flags[0.2][short] == 2).all()


def test_tube_link_and_match_at_the_active_tube_bound(dev):
    case = _fixture_b()
    assert lib.query("tuber_tube_link_max_active") == 64 == lib.query("tuber_frame_match_max_dets")
    ev, link, flags, got = _compare(case, 0, 1, dev, check=False)
    per_slot = np.bincount(link["row_slot"])
    assert per_slot.tolist() == [64, 64, 5] and (got["row_cls"] == 1).all() and (got["row_head"] >= 0).all()
    lens = got["tube_len"][got["row_head"] == np.arange(len(got["row_head"]))]
    assert (lens >= 2).sum() >= 32 and (lens == 1).sum() >= 1 and (flags[0.2] == 1).sum() >= 1


# ------------------------------------------------------------------------------------------------------------------------------
# link records made by hand (tests/test_tube_nms_cpu.py ``record``): what no linker writes
# ------------------------------------------------------------------------------------------------------------------------------
def _with_ground_truth(rec, gts, C, slots, thresholds):
    """``rec`` completed to what ``VideoMAP.match`` and ``_operands`` read, with the ground-truth tubes ``gts`` = [(video, class, id, {slot in
    the video: box})] -> the evaluator that holds them"""
    ev = VideoMAP(class_num=C, min_len=1, thresholds=thresholds)
    rows = [(v, s, c, i, b) for v, c, i, boxes in gts for s, b in boxes.items()]
    ev.add_ground_truth(["v%d-%d" % (v, s) for v, s, _, _, _ in rows], [r[4] for r in rows], [r[2] for r in rows], [r[3] for r in rows])
    rec["layout"]["gt_slot"] = np.asarray([v * slots + s for v, s, _, _, _ in rows], dtype=np.int64)
    rec["det_prob"] = np.zeros((len(rec["row_head"]), C + 1), np.float32)
    rec["tubes"] = tubes_from_link(rec)
    return ev


def _match_record(o, rec, C, thresholds, dev, max_rows=None):
    """``tuber_tube_match`` over the host record ``rec`` with the operands ``o`` -> (tube_flag [T, N], work) read back; both start from a pattern"""
    T, N, i32 = len(thresholds), o["N"], np.int32
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(dev)
    flags = torch.full((T, N), 77, dtype=torch.uint8, device=dev)
    work = torch.full((N * max(o["max_gt_tubes"], 1),), 12345.0, dtype=torch.float64, device=dev)
    lib.call("tuber_tube_match", o["det_box"], o["slot_off"], o["video_off"], up(rec["row_cls"], i32), up(rec["row_head"], i32),
             up(rec["tube_score"], np.float64), up(rec["tube_len"], i32), up(rec["tube_last"], i32), o["gt_box"], o["gt_cls"], o["gt_tube"], o["gt_off"],
             torch.tensor(thresholds, dtype=torch.float64, device=dev), o["V"], o["S"], N, o["G"], C, T, o["max_rows"] if max_rows is None else max_rows,
             o["max_gt_rows"], o["max_gt_tubes"], 1, work, flags)
    return flags.cpu().numpy(), work.cpu().numpy().reshape(N, -1)


def test_more_live_tubes_than_lanes_are_flagged_not_decided(dev):
    """tests/test_tube_nms_gpu.py's record of the same name, matched: 33 one-row heads in slot 0 and 33 in slot 1 of class 0, every one with
    tube_last = 5, are 66 tubes live at slot 1 with max_rows = 33.  No link inside the linker's bounds looks like this; the kernel answers with
    byte 3 in every threshold plane and decides the video's other class as usual."""
    thresholds = (0.2, 0.5)
    grid = lambda i: (50.0 * (i % 8), 80.0 * (i // 8), 50.0 * (i % 8) + 40, 80.0 * (i // 8) + 60)
    tubes = [(0, 0, 0.5, {s: grid(i)}) for s in (0, 1) for i in range(33)]
    tubes += [(0, 1, 0.9, span(BOX, 2, 5)), (0, 1, 0.8, span(shifted(BOX, 2.0), 2, 5)), (0, 1, 0.7, span(FAR, 2, 5))]
    rec, heads = record(tubes, 1, 6)
    rec["tube_last"][heads[:66]] = 5
    ev = _with_ground_truth(rec, [(0, 0, 0, span(grid(0), 0, 1)), (0, 1, 0, span(BOX, 2, 5))], 2, 6, thresholds)
    _, want, _ = ev.match(rec)
    o = _operands(ev, rec, dev)
    assert o["max_rows"] == 33 and o["N"] == 78
    got, _ = _match_record(o, rec, 2, thresholds, dev, max_rows=33)
    rest = np.setdiff1d(np.arange(o["N"]), heads)
    for i, thr in enumerate(thresholds):
        assert (got[i][heads[:66]] == 3).all() and (want[thr][heads[:66]] != 2).all()
        assert got[i][heads[66:]].tolist() == want[thr][heads[66:]].tolist() == [1, 0, 0]
        assert (got[i][rest] == 2).all()


def test_malformed_heads_are_not_counted(dev):
    """tests/test_tube_nms_gpu.py's plants (a head beyond the record, a head that points forward), and a row of class 1 whose head is the
    head row of a class-0 tube of its video: the flags are those of the record with these rows and their followers at head -1, and no
    `work` row is written that the cleaned record leaves alone -- a head of another class is another wave's row."""
    rec, where = planted()
    N = len(rec["row_head"])
    beyond, forward, other = where["vid_a"], where["cls_b"], where["cls_a"]
    crossed = int(np.nonzero(rec["row_head"] == forward)[0][-1])            # the last row of cls_b: class 1, video 2
    assert rec["row_cls"][crossed] == 1 and rec["row_cls"][other] == 0 and other < crossed and rec["row_head"][beyond + 1] == beyond
    bad = dict(rec, row_head=rec["row_head"].copy(), layout=dict(rec["layout"]))
    bad["row_head"][beyond] = N + 5
    bad["row_head"][forward] = forward + 1
    bad["row_head"][crossed] = other
    clean = dict(rec, row_head=rec["row_head"].copy(), layout=dict(rec["layout"]))
    for h in (beyond, forward):
        clean["row_head"][rec["row_head"] == h] = -1
    near = shifted(BOX, 2.0)
    gts = [(0, 1, 0, span(BOX, 0, 3)), (2, 0, 0, span(BOX, 0, 3)), (2, 1, 0, span(near, 0, 3)), (3, 0, 0, span(BOX, 0, 3)), (5, 0, 4, span(BOX, 0, 5)),
           (6, 2, 0, span(BOX, 0, 3)), (6, 2, 1, span(shifted(BOX, 24.0), 0, 3)), (7, 1, 0, span(BOX, 0, 5))]
    ev = _with_ground_truth(clean, gts, 3, 8, THRESHOLDS)
    _, want, _ = ev.match(clean)
    assert min(abs(x - t) for row in ev.st_iou(clean)[1].values() for x in row.values() for t in THRESHOLDS) > 1e-9    # no decision on an edge
    assert all(want[t][beyond] == want[t][forward] == 2 for t in THRESHOLDS) and (want[0.5] == 1).sum() >= 5 and (want[0.5] == 0).sum() >= 3
    o = _operands(ev, clean, dev)
    assert o["max_gt_tubes"] == 2
    clean_flags, clean_work = _match_record(o, clean, 3, THRESHOLDS, dev)
    for i, thr in enumerate(THRESHOLDS):
        assert np.array_equal(clean_flags[i], want[thr]), thr
    bad_flags, bad_work = _match_record(o, bad, 3, THRESHOLDS, dev)
    assert np.array_equal(bad_flags, clean_flags), np.argwhere(bad_flags != clean_flags)[:10]
    heads = np.nonzero(clean["row_head"] == np.arange(N))[0]
    assert (clean_work[other] != 12345.0).all() and (clean_work[np.setdiff1d(np.arange(N), heads)] == 12345.0).all()
    for c in range(3):                                                       # the rows of the heads of every class, the other classes' among them
        rows = heads[clean["row_cls"][heads] == c]
        assert np.array_equal(bad_work[rows].view(np.int64), clean_work[rows].view(np.int64)), c
    assert np.array_equal(bad_work.view(np.int64), clean_work.view(np.int64))


# ------------------------------------------------------------------------------------------------------------------------------
# the store
# ------------------------------------------------------------------------------------------------------------------------------
def _check_results(got, want, n_gt):
    assert list(got) == list(want)
    for t in want:
        (gm, gp), (wm, wp) = got[t], want[t]
        assert gp.keys() == wp.keys() and len(wp) > 0
        for c in wp:
            assert abs(gp[c] - wp[c]) <= ap_bound(n_gt[c]), (t, c, gp[c], wp[c])
        b = mean_bound([n_gt[c] for c in wp]) + (2 * 11 * U if t == "0.5:0.95" else 0.0)
        print("video-mAP@%s: device %.17g host %.17g |diff| %.3g bound %.3g" % (t, gm, wm, abs(gm - wm), b))
        assert abs(gm - wm) <= b


def test_device_store_equals_the_host_evaluator_on_the_synthetic_case(dev):
    case = synth.synthetic_video_map_case(12, 24, 10, 21, seed=5)
    ev = _case_evaluator(case)
    want = ev.evaluate()
    n_gt, flags, link = ev.match()
    st = _store(case, device=dev)
    got = st.evaluate_video()
    assert st.video_path == "device"
    _check_results(got, want, n_gt)
    assert want[0.2][0] > want[0.75][0] and (flags[0.5] == 1).sum() >= 5 and (flags[0.5] == 0).sum() >= 5
    # the decisions behind the numbers
    a = st.video_arrays()
    dl = st.link(a)
    for k in ("row_cls", "row_head", "tube_len", "tube_last"):
        assert np.array_equal(dl[k].cpu().numpy(), link[k]), k
    assert np.array_equal(dl["tube_score"].cpu().numpy().view(np.int64), link["tube_score"].view(np.int64))
    df = st.match_video(a, dl).cpu().numpy()
    for i, thr in enumerate(a["thr"]):
        assert np.array_equal(df[i], flags[thr]), thr
    # evaluate() is still the frame metric
    frame = _store(case, device=dev, cls=DeviceFrameMAPUCF, tubes=False)
    (fm, fp), (gm, gp) = frame.evaluate(), st.evaluate()
    assert st.path == "device" and _bits(fm) == _bits(gm) and all(_bits(fp[c]) == _bits(gp[c]) for c in fp) and fp.keys() == gp.keys()
    # the same bits again
    _same_results(_store(case, device=dev).evaluate_video(), got)
    # tubes() is link() read back
    tubes = st.tubes()
    assert [t["head"] for t in tubes] == [t["head"] for t in link["tubes"]]
    for t, w in zip(tubes, link["tubes"]):
        assert (t["video"], t["cls"], t["frames"], t["rows"]) == (w["video"], w["cls"], w["frames"], w["rows"])
        assert _bits(t["score"]) == _bits(w["score"]) and np.array_equal(t["boxes"], w["boxes"])
    timings = {}
    _same_results(st.evaluate_video(timings=timings), got)
    assert {"layout_and_uploads_ms", "tuber_tube_link_ms", "tuber_tube_match_ms", "rank_sort_and_scatter_ms", "tuber_ranked_ap_ms", "read_back_ms"} <= set(timings)


# ------------------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------------------
def test_bounds_are_refused_without_a_launch(dev):
    max_thr, max_gt = lib.query("tuber_tube_match_max_thresholds"), lib.query("tuber_tube_match_max_gt")
    assert (max_thr, max_gt, lib.query("tuber_tube_link_max_active"), lib.query("tuber_frame_match_max_gt")) == (16, 32, 64, 32)
    C, n = 3, 65
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    box, prob = z(n, 4), z(n, C + 1)
    soff, voff = torch.tensor([0, n], dtype=torch.int32, device=dev), torch.tensor([0, 1], dtype=torch.int32, device=dev)
    cls, head = (torch.full((n,), -99, dtype=torch.int32, device=dev) for _ in range(2))
    score, tlen, tlast = z(n, dt=torch.float64), z(n, dt=torch.int32), z(n, dt=torch.int32)
    names = "det_box det_prob slot_off video_off V S N C max_rows link_iou max_gap row_cls row_head tube_score tube_len tube_last".split()
    ok = (box, prob, soff, voff, 1, 1, n, C, n, 0.2, 0, cls, head, score, tlen, tlast)
    bad = lambda **kw: tuple(kw.get(k, v) for k, v in zip(names, ok))
    assert rc("tuber_tube_link", *ok) == EINVAL                                     # 65 rows in a slot
    assert rc("tuber_tube_link", *bad(N=65, max_rows=64)) == EINVAL                 # ... whatever the caller claims
    assert rc("tuber_tube_link", *bad(N=33, max_rows=33, max_gap=1)) == EINVAL      # 33 rows x 2 slots of history: 66 active tubes
    assert rc("tuber_tube_link", *bad(N=64, max_rows=64, max_gap=1)) == EINVAL
    for kw in (dict(C=0), dict(max_gap=-1), dict(link_iou=float("nan")), dict(V=-1), dict(S=0)):
        assert rc("tuber_tube_link", *bad(N=32, max_rows=32, **kw)) == EINVAL, kw
    for name in ("det_box", "det_prob", "slot_off", "video_off", "row_cls", "row_head", "tube_score", "tube_len", "tube_last"):
        assert rc("tuber_tube_link", *bad(N=32, max_rows=32, **{name: None})) == EINVAL, name
    assert rc("tuber_tube_link", *bad(N=0, max_rows=0)) == 0                        # nothing to do: no launch either
    G, T = 4, 3
    gbox, gcls, gtube = z(G, 4, dt=torch.float64), z(G, dt=torch.int32), z(G, dt=torch.int32)
    goff = torch.tensor([0, G], dtype=torch.int32, device=dev)
    thr = z(17, dt=torch.float64)
    work, flags = z(n * 33, dt=torch.float64), torch.full((17, n), 77, dtype=torch.uint8, device=dev)
    names = ("det_box slot_off video_off row_cls row_head tube_score tube_len tube_last gt_box gt_cls gt_tube gt_off thresholds V S N G C T max_rows "
             "max_gt_rows max_gt_tubes min_len work tube_flag").split()
    ok = (box, soff, voff, cls, head, score, tlen, tlast, gbox, gcls, gtube, goff, thr, 1, 1, 32, G, C, T, 32, G, 1, 1, work, flags)
    bad = lambda **kw: tuple(kw.get(k, v) for k, v in zip(names, ok))
    assert rc("tuber_tube_match", *bad(T=max_thr + 1)) == EINVAL                    # 17 thresholds
    assert rc("tuber_tube_match", *bad(max_gt_tubes=max_gt + 1)) == EINVAL          # 33 ground-truth tubes in one (video, class)
    assert rc("tuber_tube_match", *bad(N=65, max_rows=65)) == EINVAL
    assert rc("tuber_tube_match", *bad(G=33, max_gt_rows=33)) == EINVAL
    for kw in (dict(T=0), dict(C=0), dict(N=33), dict(G=5)):
        assert rc("tuber_tube_match", *bad(**kw)) == EINVAL, kw
    for name in ("det_box", "slot_off", "video_off", "row_cls", "row_head", "tube_score", "tube_len", "tube_last", "gt_box", "gt_cls", "gt_tube",
                 "gt_off", "thresholds", "work", "tube_flag"):
        assert rc("tuber_tube_match", *bad(**{name: None})) == EINVAL, name
    assert rc("tuber_tube_match", *bad(N=0)) == 0
    torch.cuda.synchronize()
    assert (flags == 77).all() and (cls == -99).all() and (head == -99).all()       # nothing ran


@pytest.mark.parametrize("which", ["65_rows", "33_rows_gap_1", "17_thresholds", "33_gt_tubes", "unparsed_key"])
def test_a_store_beyond_a_bound_is_evaluated_on_the_host(dev, caplog, which):
    case = synth.synthetic_video_map_case(3, 8, 10, 21, seed=2)
    kw = {}
    if which == "65_rows":
        case["det_keys"] = [case["det_keys"][0]] * 65 + case["det_keys"][65:]
        kw = dict(max_gap=0)
    elif which == "33_rows_gap_1":
        case["det_keys"] = [case["det_keys"][0]] * 33 + case["det_keys"][33:]
        kw = dict(max_gap=1)
    elif which == "17_thresholds":
        kw = dict(thresholds=tuple(round(0.1 + 0.05 * i, 2) for i in range(17)))
    elif which == "33_gt_tubes":
        extra = 33
        case["gt_keys"] = list(case["gt_keys"]) + ["video0000-%d" % (1 + i % 8) for i in range(extra)]
        case["gt_boxes"] = np.concatenate([case["gt_boxes"], np.tile([[10.0, 10, 60, 60]], (extra, 1))])
        lab = np.zeros((extra, case["gt_labels"].shape[1])); lab[:, 4] = 1.0
        case["gt_labels"] = np.concatenate([case["gt_labels"], lab])
        case["gt_tubes"] = np.concatenate([case["gt_tubes"], 100 + np.arange(extra)])
    else:
        case["det_keys"] = [k.replace("-", "_") if k.startswith("video0001") else k for k in case["det_keys"]]
    want = _case_evaluator(case, **kw).evaluate()
    st = _store(case, device=dev, **kw)
    with caplog.at_level("WARNING"):
        got = st.evaluate_video()
    assert st.video_path == "host" and len([r for r in caplog.records if "video-mAP on the host" in r.getMessage()]) == 1
    _same_results(got, want)
    assert st.n == len(case["det_keys"])                                            # no row was dropped
    inside = _store(synth.synthetic_video_map_case(3, 8, 10, 21, seed=2), device=dev, max_gap=2)
    inside.evaluate_video()
    assert inside.video_path == "device"


# ------------------------------------------------------------------------------------------------------------------------------
# the validation loop
# ------------------------------------------------------------------------------------------------------------------------------
def _loader(nc, H=64, W=64):
    """two videos x 3 frames in three batches of two clips, keys "<video>-<frame>": the loader of tests/test_device_map_ucf_gpu.py with tube keys"""
    loader, clip = [], 0
    for i in range(3):
        clips = synth.synthetic_clips(2, 32, H, W, seed=10 + i)
        tg = synth.synthetic_targets(2, "jhmdb", nc, seed=20 + i, device="cpu", hw=(H, W))
        for b, t in enumerate(tg):
            kp = (7 * i + 3 * b) % 32
            t["key_pos"] = torch.tensor(kp, dtype=torch.int64)
            t["image_id"] = ["clip%d-%d" % (clip // 3, 5 + clip % 3), kp]
            t["size"] = torch.tensor([H, W])
            raw = torch.zeros(1, 6)
            raw[:, 0] = 2 * i + b
            raw[:, 1] = kp
            raw[:, 2:] = torch.tensor([4.0 + b, 6.0, 40.0 + 3 * i, 50.0])
            t["raw_boxes"] = raw
            t["labels"] = torch.full_like(t["labels"], 8)
            clip += 1
        loader.append((clips, tg))
    return loader


@pytest.fixture(scope="module")
def loop_model():
    dev = torch.device("cuda:0")
    cfg = load_cfg(os.path.join(ROOT, "configuration", "Tuber_CSN152_JHMDB.yaml"))
    cfg.CONFIG.MODEL.BACKBONE_NAME = "CSN-TEST"
    model, crit, post = build_model(cfg)
    synth.load_name_hashed(model)
    model.to(dev)
    crit.to(dev)
    return cfg, model, crit, post


class _Writer:
    def __init__(self):
        self.scalars = {}

    def add_scalar(self, name, value, epoch):
        self.scalars[name] = value


def _run(loop_model, tmp_path, name, video, device_map_on=False, results=None, writer=None):
    cfg, model, crit, post = loop_model
    cfg.CONFIG.LOG.BASE_PATH, cfg.CONFIG.LOG.RES_DIR = str(tmp_path), name
    cfg.CONFIG.VAL.VIDEO_MAP.ENABLE, cfg.CONFIG.VAL.DEVICE_MAP.ENABLE = video, device_map_on
    names = []

    def hook(fn, args, launch):
        names.append(fn)
        return launch(fn, *args)
    lib.set_launch_hook(hook)
    try:
        kw = {} if results is None else dict(results=results)
        mAP = validate_tuber_ucf_detection(cfg, model, crit, post, _loader(cfg.CONFIG.DATA.NUM_CLASSES), epoch=0, writer=writer, verbose=False, **kw)
    finally:
        lib.set_launch_hook(None)
        cfg.CONFIG.VAL.VIDEO_MAP.ENABLE, cfg.CONFIG.VAL.DEVICE_MAP.ENABLE = False, False
    return mAP, names, os.path.join(str(tmp_path), name)


def test_ucf_validation_loop_with_video_map(dev, loop_model, tmp_path, monkeypatch):
    cfg = loop_model[0]
    nc, Q = cfg.CONFIG.DATA.NUM_CLASSES, cfg.CONFIG.MODEL.QUERY_NUM
    results, writer = {}, _Writer()
    video_map, names, d1 = _run(loop_model, tmp_path, "video", True, results=results, writer=writer)
    assert "tuber_tube_link" in names and "tuber_tube_match" in names
    # off: the store class is not even looked up, and none of the new kernels is launched
    def boom(*a, **k):
        raise AssertionError("DeviceVideoMAP built with VIDEO_MAP off")
    monkeypatch.setattr(device_map, "DeviceVideoMAP", boom)
    plain_map, names, d0 = _run(loop_model, tmp_path, "plain", False)
    dm_map, dm_names, _ = _run(loop_model, tmp_path, "dm", False, device_map_on=True)
    monkeypatch.undo()
    assert not [n for n in names + dm_names if n.startswith("tuber_tube_")]
    assert _bits(video_map) == _bits(plain_map)                                    # still frame-mAP, from the same files
    for f in ("0.txt", "binary_0.txt", "GT_0.txt"):
        assert open(os.path.join(d0, f)).read() == open(os.path.join(d1, f)).read()
    both_map, _, _ = _run(loop_model, tmp_path, "both", True, device_map_on=True)
    assert _bits(both_map) == _bits(dm_map)
    # the video-mAPs: a host VideoMAP fed the rows of the result files (the store's fp32 rows, printed exactly)
    settings = video_map_settings(cfg)
    ev = VideoMAP(class_num=nc, **settings)
    from tubelet_transformer_amd.evaluation import _parse
    dets = [_parse(l) for l in open(os.path.join(d1, "0.txt"))]
    gts = [_parse(l) for l in open(os.path.join(d1, "GT_0.txt"))]
    assert len(dets) == 6 * Q and len(gts) == 6
    ev.add_detections([k for k, _ in dets], np.asarray([v[:4] for _, v in dets]), np.asarray([v[4:5 + nc] for _, v in dets]))
    ev.add_ground_truth([k for k, _ in gts], np.asarray([v[2:6] for _, v in gts]), [int(np.argmax(v[6:])) for _, v in gts])
    want = ev.evaluate()
    n_gt, flags, link = ev.match()
    lay = link["layout"]
    assert lay["videos"] == ["clip0", "clip1"] and np.diff(lay["video_off"]).tolist() == [3, 3] and n_gt == {9: 2}
    assert list(results["video_mAP"]) == list(settings["thresholds"]) == [0.2, 0.5, 0.75, "0.5:0.95"]
    print("loop: %d tubes, %d counted rows, video-mAP %s" % (len(link["tubes"]), (link["row_head"] >= 0).sum(), results["video_mAP"]))
    assert (link["row_head"] >= 0).sum() >= 1, "no row of the run is counted: the comparison would be vacuous"
    _check_results({t: (results["video_mAP"][t], results["video_AP"][t]) for t in want}, want, n_gt)
    assert {"val/video_mAP@%s" % t: results["video_mAP"][t] for t in want}.items() <= writer.scalars.items()
    assert "val/val_mAP_epoch" in writer.scalars
    assert VIDEO_MAP_RANGE[0] == 0.5
