"""The JHMDB / UCF101-24 device frame-mAP evaluator on the GPU (csrc/frame_map.hip, device_map.DeviceFrameMAPUCF): ``tuber_frame_match_top1``
directly against a sequential host restatement, ``DeviceFrameMAPUCF.evaluate()`` against ``evaluation.FrameMAPUCF`` on result files, the bounds
(negative return codes: nothing is launched) and ``validate_tuber_ucf_detection`` with ``CONFIG.VAL.DEVICE_MAP``.

Bounds: the derived ones of tests/test_device_map_gpu.py, nothing measured.  Classes and flags are decisions: equal exactly.  Per class
|AP_device - AP_host| <= 2 * (n_gt + 3) * 2^-53; the mean over K classes: the mean of those bounds plus 2 * (K + 1) * 2^-53."""
import json
import os

import numpy as np
import pytest
import torch

from test_device_map_ucf_cpu import _bits, _from_files, _golden_files, _golden_store, _golden_values, _ucf_files, _ucf_store
from tubelet_transformer_amd import lib, synth
from tubelet_transformer_amd.config import load_cfg
from tubelet_transformer_amd.device_map import DeviceFrameMAPUCF
from tubelet_transformer_amd.evaluation import FrameMAPUCF, _iou_one_to_many, validate_tuber_ucf_detection
from tubelet_transformer_amd.tuber import build_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
U = 2.0 ** -53
NAN = float("nan")


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
# 1. tuber_frame_match_top1
# ------------------------------------------------------------------------------------------------------------------------------
DET_COUNTS = (15, 0, 1, 16, 64, 10, 10, 10)
GT_COUNTS = (3, 1, 0, 32, 3, 1, 3, 2)
FAR = 500.0


def _top1_fixture(C, tied):
    """8 frames: generic with the planted arg-max cases; ground truth only; detections only; 16 x 32; 64 x 3; the IoU == 0.5 case with
    degenerate boxes; twin boxes and a contested box; a frame on the exclude list.  ``rows``: the planted rows by name."""
    rng = np.random.default_rng(300 + C)
    n, g = sum(DET_COUNTS), sum(GT_COUNTS)
    d_off, g_off = np.concatenate([[0], np.cumsum(DET_COUNTS)]), np.concatenate([[0], np.cumsum(GT_COUNTS)])
    gxy = rng.uniform(0, 50, (g, 2))
    gt_box = np.concatenate([gxy, gxy + rng.uniform(8, 40, (g, 2))], axis=1)
    gt_cls = rng.integers(0, C, g).astype(np.int32)
    gt_cls[g_off[3] + 5] = C + 2                                       # a class outside [0, C): matches nothing
    prob = rng.random((n, C + 1)).astype(np.float32)
    det_box = np.zeros((n, 4), dtype=np.float32)
    for f in range(8):
        for i in range(d_off[f], d_off[f + 1]):
            if GT_COUNTS[f] and rng.random() < 0.6:
                j = rng.integers(g_off[f], g_off[f + 1])
                det_box[i] = gt_box[j] + rng.normal(0, 0.1, 4) * np.tile(gt_box[j, 2:] - gt_box[j, :2], 2)
                if gt_cls[j] < C and rng.random() < 0.8:
                    prob[i, gt_cls[j]] += 1.0
            else:
                p = rng.uniform(0, 60, 2)
                det_box[i] = np.concatenate([p, p + rng.uniform(5, 30, 2)])
            if rng.random() < 0.25:
                prob[i, C] += 2.0
    if tied:
        prob = (np.round(prob * 4) / 4).astype(np.float32)

    def top(r, c, v=0.875, others=0.125):
        prob[r] = others
        prob[r, c] = v
    rows = {}
    c1 = min(1, C - 1)
    # frame 0: the arg-max rule
    d0, g0 = d_off[0], g_off[0]
    gt_box[g0], gt_cls[g0] = [0.0, 0.0, 20.0, 20.0], 0
    gt_box[g0 + 1], gt_cls[g0 + 1] = [100.0, 100.0, 130.0, 140.0], c1
    gt_box[g0 + 2], gt_cls[g0 + 2] = [200.0, 0.0, 230.0, 40.0], 0
    rows["no_object_on_top"] = d0
    top(d0, C)
    det_box[d0] = [0.0, 0.0, 20.0, 20.0]
    rows["no_object_equals_best_class"] = d0 + 1
    top(d0 + 1, C)
    prob[d0 + 1, 0] = prob[d0 + 1, C]
    det_box[d0 + 1] = [FAR, FAR, FAR + 10, FAR + 10]
    if C > 1:
        rows["two_classes_equal"] = d0 + 2
        top(d0 + 2, C - 1)
        prob[d0 + 2, c1 if c1 < C - 1 else 0] = prob[d0 + 2, C - 1]
        det_box[d0 + 2] = [FAR, FAR, FAR + 10, FAR + 10]
    rows["nan_class"], rows["beats_nan"] = d0 + 3, d0 + 5
    top(d0 + 3, C)                                                     # NaN beats even a larger no-object entry
    prob[d0 + 3, c1] = NAN
    det_box[d0 + 3] = [100.0, 100.0, 130.0, 140.0]
    top(d0 + 5, c1, v=0.5, others=0.0625)                              # a low finite score of the same class on the same box: ranks above NaN
    det_box[d0 + 5] = [100.0, 100.0, 130.0, 139.0]
    rows["nan_no_object_only"] = d0 + 4
    top(d0 + 4, 0)
    prob[d0 + 4, C] = NAN
    det_box[d0 + 4] = [0.0, 0.0, 20.0, 20.0]
    for r in range(d0 + 6, d_off[1]):
        if np.argmax(prob[r]) == c1:                                    # nobody else contests the NaN rows' box
            det_box[r] = [FAR, FAR, FAR + 10, FAR + 10]
    # frame 5: one ground-truth box [0, 0, 2, 1] of class 0; detection [0, 0, 1, 1] has IoU exactly 0.5 with it; everything else far away
    d5, g5 = d_off[5], g_off[5]
    det_box[d5:d_off[6]] += FAR
    gt_box[g5], gt_cls[g5] = [0.0, 0.0, 2.0, 1.0], 0
    rows["iou_exactly_half"], rows["x1_eq_x2"], rows["y1_gt_y2"] = d5, d5 + 1, d5 + 2
    det_box[d5], det_box[d5 + 1], det_box[d5 + 2] = [0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 0.0, 1.0], [0.0, 1.0, 1.0, 0.5]
    for r in (d5, d5 + 1, d5 + 2):
        top(r, 0)
    # frame 6: twin ground-truth boxes of class 0 with two detections exactly on them; a box two detections of its class contest
    d6, g6 = d_off[6], g_off[6]
    det_box[d6:d_off[7]] += FAR
    gt_box[g6] = gt_box[g6 + 1] = [10.0, 10.0, 30.0, 30.0]
    gt_cls[g6] = gt_cls[g6 + 1] = 0
    gt_box[g6 + 2], gt_cls[g6 + 2] = [60.0, 60.0, 80.0, 90.0], c1
    rows["twin_high"], rows["twin_low"], rows["contest_high"], rows["contest_low"] = d6 + 1, d6, d6 + 3, d6 + 2
    det_box[d6] = det_box[d6 + 1] = [10.0, 10.0, 30.0, 30.0]
    top(d6, 0, v=0.75)
    top(d6 + 1, 0, v=0.875)
    det_box[d6 + 2], det_box[d6 + 3] = [60.0, 60.0, 80.0, 90.0], [60.0, 61.0, 80.0, 90.0]
    top(d6 + 2, c1, v=0.625)                                           # the better IoU, the lower score: a false positive
    top(d6 + 3, c1, v=0.6875)
    if C > 2:
        rows["class_without_gt"] = d6 + 4
        top(d6 + 4, 2)
        det_box[d6 + 4] = [10.0, 10.0, 30.0, 30.0]
    skip = np.zeros(8, dtype=np.uint8)
    skip[7] = 1
    return dict(C=C, det_box=det_box, prob=prob, det_off=d_off.astype(np.int32), gt_box=gt_box.astype(np.float64), gt_cls=gt_cls,
                gt_off=g_off.astype(np.int32), skip=skip, rows=rows)


def _top1_host(fx, thr=0.5):
    """the UCF counting rule and the matching restated on the host, sequentially: np.argmax, the counted rows of a frame visited by
    (-score, row) with NaN last, _iou_one_to_many, first arg-max, a ground-truth row taken once"""
    C, n = fx["C"], len(fx["det_box"])
    cls, flag = np.full(n, -7, dtype=np.int32), np.full(n, 2, dtype=np.uint8)
    for f in range(len(fx["det_off"]) - 1):
        d0, d1, g0, g1 = fx["det_off"][f], fx["det_off"][f + 1], fx["gt_off"][f], fx["gt_off"][f + 1]
        counted = []
        for r in range(d0, d1):
            p, b = fx["prob"][r].astype(np.float64), fx["det_box"][r].astype(np.float64)
            cls[r] = int(np.argmax(p))
            if cls[r] != C and b[0] < b[2] and b[1] < b[3] and not fx["skip"][f]:
                counted.append((bool(np.isnan(p[cls[r]])), -p[cls[r]], r))
        taken = set()
        for _, _, r in sorted(counted):
            cand = [j for j in range(g0, g1) if fx["gt_cls"][j] == cls[r]]
            flag[r] = 0
            if cand:
                iou = _iou_one_to_many(fx["det_box"][r].astype(np.float64), fx["gt_box"][cand])
                j = int(np.argmax(iou))
                if iou[j] >= thr and cand[j] not in taken:
                    taken.add(cand[j])
                    flag[r] = 1
    return cls, flag


def _top1_device(fx, dev, thr=0.5):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n = len(fx["det_box"])
    cls = torch.full((n,), -99, dtype=torch.int32, device=dev)
    flag = torch.full((n,), 77, dtype=torch.uint8, device=dev)
    lib.call("tuber_frame_match_top1", up(fx["det_box"]), up(fx["prob"]), up(fx["det_off"]), up(fx["gt_box"]), up(fx["gt_cls"]), up(fx["gt_off"]),
             up(fx["skip"]), len(fx["det_off"]) - 1, n, len(fx["gt_box"]), fx["C"], thr, cls, flag)
    return cls.cpu().numpy(), flag.cpu().numpy()


@pytest.mark.parametrize("C", [1, 21, 24, 130])
def test_frame_match_top1_equals_the_sequential_host_matching(dev, C):
    fx = _top1_fixture(C, tied=False)
    R, c1 = fx["rows"], min(1, C - 1)
    keep = np.ones(len(fx["prob"]), dtype=bool)
    keep[list(R.values())] = False
    tops = fx["prob"][keep].max(axis=1)
    assert len(np.unique(tops)) == len(tops)                            # apart from the planted rows no two scores are equal
    want_cls, want = _top1_host(fx)
    got_cls, got = _top1_device(fx, dev)
    assert np.array_equal(got_cls, want_cls), np.argwhere(got_cls != want_cls)[:10]
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]
    assert got_cls[R["no_object_on_top"]] == C and got[R["no_object_on_top"]] == 2
    assert got_cls[R["no_object_equals_best_class"]] == 0 and got[R["no_object_equals_best_class"]] == 0     # the class comes first
    if C > 1:
        lower = c1 if c1 < C - 1 else 0
        assert got_cls[R["two_classes_equal"]] == lower and got[R["two_classes_equal"]] != 2
    assert got_cls[R["nan_class"]] == c1 and got[R["nan_class"]] == 0 and got[R["beats_nan"]] == 1              # a NaN score ranks last
    assert got_cls[R["nan_no_object_only"]] == C and got[R["nan_no_object_only"]] == 2
    assert got[R["iou_exactly_half"]] == 1 and got[R["x1_eq_x2"]] == 2 and got[R["y1_gt_y2"]] == 2
    assert got_cls[R["x1_eq_x2"]] == 0 and got_cls[R["y1_gt_y2"]] == 0
    assert got[R["twin_high"]] == 1 and got[R["twin_low"]] == 0         # the twin box is free, but the first arg-max is taken
    assert got[R["contest_high"]] == 1 and got[R["contest_low"]] == 0   # one best box, the higher score takes it
    if C > 2:
        assert got_cls[R["class_without_gt"]] == 2 and got[R["class_without_gt"]] == 0
    d2 = fx["det_off"][2]
    assert got[d2] == (2 if got_cls[d2] == C else 0)                    # a frame without ground truth: a false positive at best
    assert (got[fx["det_off"][7]:] == 2).all() and (got_cls[fx["det_off"][7]:] >= 0).all()                     # the skipped frame
    assert fx["det_off"][1] == fx["det_off"][2] and GT_COUNTS[1] == 1   # a frame with ground truth only: no row, nothing written
    assert {0, 1, 2} <= set(np.unique(got)) and not (got == 77).any() and not (got_cls == -99).any()
    # equal scores (quarters): by row
    fx = _top1_fixture(C, tied=True)
    tops = fx["prob"].max(axis=1)
    assert len(np.unique(tops[~np.isnan(tops)])) <= 16
    (want_cls, want), (got_cls, got) = _top1_host(fx), _top1_device(fx, dev)
    assert np.array_equal(got_cls, want_cls) and np.array_equal(got, want), np.argwhere(got != want)[:10]


# ------------------------------------------------------------------------------------------------------------------------------
# 2. DeviceFrameMAPUCF.evaluate()
# ------------------------------------------------------------------------------------------------------------------------------
def _n_gt(ev):
    n = {}
    for items in ev.gt.values():
        for cls, _ in items:
            n[cls] = n.get(cls, 0) + 1
    return n


def _check_aps(got, per_class, want, want_pc, n_gt):
    assert per_class.keys() == want_pc.keys() and len(want_pc) > 0
    for c in want_pc:
        print("class %d n_gt %d: device %.17g host %.17g bound %.3g" % (c, n_gt[c], per_class[c], want_pc[c], ap_bound(n_gt[c])))
        assert abs(per_class[c] - want_pc[c]) <= ap_bound(n_gt[c]), (c, per_class[c], want_pc[c])
    b = mean_bound([n_gt[c] for c in want_pc])
    print("mAP: device %.17g host %.17g |diff| %.3g bound %.3g" % (got, want, abs(got - want), b))
    assert abs(got - want) <= b


def _host_decisions_in_store_order(ev, st):
    """the host evaluator's (class, flag) per row of the store in frame order: flag 2 where the row is in none of its lists"""
    a = st.device_arrays()
    C = a["C"]
    off = a["det_off"].cpu().numpy()
    box = a["det_box"].cpu().numpy().astype(np.float64)
    prob = a["det_prob"].cpu().numpy().astype(np.float64)
    cls = prob.argmax(axis=1).astype(np.int32)
    _, scores, tps = ev.match()
    assert list(ev.det) == [k for k in st.frame_keys if k in ev.det]
    flag = np.full(a["N"], 2, dtype=np.uint8)
    cursor = {}
    for f, key in enumerate(st.frame_keys):
        if key not in ev.det:
            assert key in ev.exclude or (cls[off[f]:off[f + 1]] == C).all()
            continue
        valid = [r for r in range(off[f], off[f + 1]) if cls[r] != C and box[r, 0] < box[r, 2] and box[r, 1] < box[r, 3]]
        for c in sorted({int(cls[r]) for r in valid}):
            k = cursor.get(c, 0)
            s, t = scores[c + 1][k], tps[c + 1][k]
            cursor[c] = k + 1
            order = sorted([r for r in valid if cls[r] == c], key=lambda r: (-prob[r, c], r))
            assert np.array_equal(s, prob[order, c])
            flag[order] = t
    assert all(cursor.get(c - 1, 0) == len(v) for c, v in scores.items())
    return cls, flag


def test_device_ucf_evaluator_on_the_golden_case(dev, tmp_path):
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "frame_map_ucf_case.json")))
    gt, det = _golden_files(g, tmp_path)
    ref = _from_files(gt, det, g["class_num"], stable=True)
    want, want_pc = _golden_values(g)
    st = _golden_store(g, device=dev)
    got, per_class = st.evaluate()
    assert st.path == "device"
    _check_aps(got, per_class, want, want_pc, _n_gt(ref))
    for k in ref.det:                                                    # the store's fp32
        ref.det[k] = [(c, b.astype(np.float32).astype(np.float64), float(np.float32(s))) for c, b, s in ref.det[k]]
    want_cls, want_flag = _host_decisions_in_store_order(ref, st)
    cls, flag = st.match_flags()
    assert np.array_equal(cls.cpu().numpy(), want_cls) and np.array_equal(flag.cpu().numpy(), want_flag)
    assert {0, 1, 2} <= set(np.unique(want_flag)) and sum(st.ties.values()) == 0
    again, again_pc = _golden_store(g, device=dev).evaluate()
    assert _bits(again) == _bits(got) and all(_bits(again_pc[c]) == _bits(per_class[c]) for c in per_class)


def test_device_ucf_evaluator_equals_the_unmodified_host_evaluator_on_the_synthetic_case(dev, tmp_path):
    case = synth.synthetic_frame_map_ucf_case(48, seed=11)
    gp, dp = _ucf_files(case, tmp_path, "synth")
    ref = _from_files(gp, dp, 21)                                       # stable=False: the reference's own order
    want, want_pc = ref.evaluate()
    st = _ucf_store(case, device=dev)
    got, per_class = st.evaluate()
    assert st.path == "device" and sum(st.ties.values()) == 0
    want_cls, want_flag = _host_decisions_in_store_order(ref, st)
    cls, flag = st.match_flags()
    assert np.array_equal(cls.cpu().numpy(), want_cls) and np.array_equal(flag.cpu().numpy(), want_flag)
    assert (want_flag == 1).sum() >= 20 and len(ref.exclude) >= 1
    _check_aps(got, per_class, want, want_pc, _n_gt(ref))


# ------------------------------------------------------------------------------------------------------------------------------
# 3. bounds
# ------------------------------------------------------------------------------------------------------------------------------
def test_top1_bounds_are_refused_without_a_launch_and_evaluated_on_the_host(dev, tmp_path, caplog):
    max_dets, max_gt = lib.query("tuber_frame_match_max_dets"), lib.query("tuber_frame_match_max_gt")
    assert (max_dets, max_gt) == (64, 32)
    C, n = 5, max_dets + 1
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    box, prob, gbox, gcls, skip = z(n, 4), z(n, C + 1), z(1, 4, dt=torch.float64), z(1, dt=torch.int32), z(1, dt=torch.uint8)
    off = torch.tensor([0, n], dtype=torch.int32, device=dev)
    goff = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    cls = torch.full((n,), -99, dtype=torch.int32, device=dev)
    flag = torch.full((n,), 77, dtype=torch.uint8, device=dev)
    names = "det_box det_prob det_off gt_box gt_cls gt_off frame_skip F N G C iou_thr det_cls det_flag".split()
    ok = (box, prob, off, gbox, gcls, goff, skip, 1, n, 1, C, 0.5, cls, flag)
    bad = lambda **kw: tuple(kw.get(k, v) for k, v in zip(names, ok))
    assert rc("tuber_frame_match_top1", *ok) == EINVAL                             # one frame of max_dets + 1 rows
    assert rc("tuber_frame_match_top1", *bad(N=max_dets, G=max_gt + 1)) == EINVAL
    assert rc("tuber_frame_match_top1", *bad(N=max_dets, C=0)) == EINVAL
    assert rc("tuber_frame_match_top1", *bad(N=max_dets, C=-3)) == EINVAL
    assert rc("tuber_frame_match_top1", *bad(N=max_dets, iou_thr=NAN)) == EINVAL
    for name in ("det_box", "det_prob", "det_off", "gt_box", "gt_cls", "gt_off", "det_cls", "det_flag"):
        assert rc("tuber_frame_match_top1", *bad(N=max_dets, **{name: None})) == EINVAL, name
    assert rc("tuber_frame_match_top1", *bad(N=0)) == 0                            # nothing to do: no launch either
    torch.cuda.synchronize()
    assert (flag == 77).all() and (cls == -99).all()                               # nothing ran
    # a store with a 75-row frame: the host value, through the fallback
    case = synth.synthetic_frame_map_ucf_case(12, seed=2)
    case["det_keys"] = [case["det_keys"][0]] * 75 + case["det_keys"][75:]
    gp, dp = _ucf_files(case, tmp_path, "big")
    want, want_pc = _from_files(gp, dp, 21, stable=True).evaluate()
    st = _ucf_store(case, device=dev)
    with caplog.at_level("WARNING"):
        got, per_class = st.evaluate()
    assert st.path == "host" and len([r for r in caplog.records if "evaluating on the host" in r.getMessage()]) == 1
    assert len(want_pc) > 0 and _bits(got) == _bits(want) and per_class.keys() == want_pc.keys()
    assert all(_bits(per_class[c]) == _bits(want_pc[c]) for c in want_pc)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the validation loop
# ------------------------------------------------------------------------------------------------------------------------------
def _loader(nc, H=64, W=64):
    """the two-batch loader of test_boundary_gpu.test_ucf_validation_loop_writes_reference_format_and_scores, with one raw box of 3 x 3 px:
    its frame goes on the exclude list.  The name-hashed weights put a class, not no-object, on top of the key frames' rows (margin about
    0.02 in probability on the CPU oracle), so the no-object bias of the class head needs no lowering for rows to be counted; the test asserts
    that some are."""
    loader = []
    for i in range(2):
        clips = synth.synthetic_clips(2, 32, H, W, seed=10 + i)
        tg = synth.synthetic_targets(2, "jhmdb", nc, seed=20 + i, device="cpu", hw=(H, W))
        for b, t in enumerate(tg):
            kp = (7 * i + 3 * b) % 32
            t["key_pos"] = torch.tensor(kp, dtype=torch.int64)
            t["image_id"] = ["clip%d_%05d" % (i, 10 + b), kp]
            t["size"] = torch.tensor([H, W])
            raw = torch.zeros(1, 6)
            raw[:, 0] = 2 * i + b
            raw[:, 1] = kp
            raw[:, 2:] = torch.tensor([4.0 + b, 6.0, 40.0 + 3 * i, 50.0])
            if (i, b) == (1, 1):
                raw[:, 2:] = torch.tensor([20.0, 30.0, 23.0, 33.0])
            t["raw_boxes"] = raw
            t["labels"] = torch.full_like(t["labels"], 8)   # the class these weights put on top of most key frames (CPU oracle): the run then
        loader.append((clips, tg))                          # has true positives and a mAP above 0 to compare (printed; not a condition)
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


def _run(loop_model, tmp_path, name, enable, files):
    cfg, model, crit, post = loop_model
    cfg.CONFIG.LOG.BASE_PATH, cfg.CONFIG.LOG.RES_DIR = str(tmp_path), name
    cfg.CONFIG.VAL.DEVICE_MAP.ENABLE, cfg.CONFIG.VAL.DEVICE_MAP.FILES = enable, files
    try:
        mAP = validate_tuber_ucf_detection(cfg, model, crit, post, _loader(cfg.CONFIG.DATA.NUM_CLASSES), epoch=0, verbose=False)
    finally:
        cfg.CONFIG.VAL.DEVICE_MAP.ENABLE, cfg.CONFIG.VAL.DEVICE_MAP.FILES = False, True
    d = os.path.join(str(tmp_path), name)
    read = lambda f: open(os.path.join(d, f)).read() if os.path.exists(os.path.join(d, f)) else None
    return mAP, [read("0.txt"), read("binary_0.txt"), read("GT_0.txt")], d


def test_ucf_validation_loop_with_the_device_evaluator(dev, loop_model, tmp_path):
    cfg = loop_model[0]
    nc, Q = cfg.CONFIG.DATA.NUM_CLASSES, cfg.CONFIG.MODEL.QUERY_NUM
    host_map, f0, d0 = _run(loop_model, tmp_path, "host", False, True)
    dev_map, f1, d1 = _run(loop_model, tmp_path, "dev", True, True)
    assert all(f0) and f0 == f1                                                     # three byte-identical files
    assert len(f0[0].splitlines()) == 4 * Q and len(f0[2].splitlines()) == 4
    ref = _from_files(os.path.join(d1, "GT_0.txt"), os.path.join(d1, "0.txt"), nc, stable=True)
    want, want_pc = ref.evaluate()
    counted = sum(len(v) for v in ref.det.values())
    n_gt = _n_gt(ref)
    assert ref.exclude == {"clip1_00011"} and counted >= 1, "no row of the run is counted: the comparison would be vacuous"
    assert len(want_pc) > 0
    b = mean_bound([n_gt[c] for c in want_pc])
    print("loop: %d true positives" % sum(int(t.sum()) for ts in ref.match()[2].values() for t in ts))
    print("loop: %d counted rows; mAP host (reference order) %.17g, stable %.17g, device %.17g, bound %.3g" % (counted, host_map, want, dev_map, b))
    assert abs(dev_map - want) <= b
    nofile_map, f2, d2 = _run(loop_model, tmp_path, "nofiles", True, False)
    assert f2 == [None, None, None] and not [f for f in os.listdir(d2) if f.endswith(".txt")]
    assert _bits(nofile_map) == _bits(dev_map)
