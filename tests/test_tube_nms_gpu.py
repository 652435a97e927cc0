"""Spatio-temporal tube NMS on the device: ``tuber_tube_nms`` called directly and held, byte for byte, to
``evaluation.tube_nms`` on the same link record; then its three consumers.  Every comparison is one of decisions and therefore exact; the
only bound is the AP bound ``tests/test_video_map_gpu.py`` derives."""
import numpy as np
import pytest
import torch

from test_tube_nms_cpu import BOX, FAR, padded_actors, padded_detections, planted, record, shifted, span
from test_video_map_cpu import _bits, _case_evaluator, _onehot, _store
from test_video_map_gpu import _check_results, rc
from tubelet_transformer_amd import lib
from tubelet_transformer_amd.evaluation import tube_nms

pytestmark = pytest.mark.gpu
SCORES = np.asarray([0.3, 0.5, 0.5, 0.7, 0.9], dtype=np.float32)
SEEDS = tuple(range(1, 9))


# ------------------------------------------------------------------------------------------------------------------------------
# the kernel's operands from a host link record
# ------------------------------------------------------------------------------------------------------------------------------
def operands(rec, dev):
    lay = rec["layout"]
    S, N = lay["S"], len(rec["row_head"])
    per_slot = np.bincount(np.asarray(rec["row_slot"], dtype=np.int64), minlength=S)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(dev)
    return dict(V=lay["V"], S=S, N=N, max_rows=int(per_slot.max()) if S else 0, det_box=up(rec["det_box"], np.float32),
                slot_off=up(np.concatenate([[0], np.cumsum(per_slot)]), np.int32), video_off=up(lay["video_off"], np.int32), row_cls=up(rec["row_cls"], np.int32),
                row_head=up(rec["row_head"], np.int32), tube_score=up(rec["tube_score"], np.float64), tube_len=up(rec["tube_len"], np.int32),
                tube_last=up(rec["tube_last"], np.int32))


def scratch(N, dev):
    """the caller-owned work buffer, full of bytes that are no partner and no status"""
    return torch.full((max(lib.query("tuber_tube_nms_work_bytes", N), 16),), 0x7F, dtype=torch.uint8, device=dev)


def args_of(o, C, min_len, nms_iou, work, keep, over=()):
    a = dict(o, C=C, min_len=min_len, nms_iou=nms_iou, work=work, keep=keep)
    a.update(dict(over))
    return (a["det_box"], a["slot_off"], a["video_off"], a["row_cls"], a["row_head"], a["tube_score"], a["tube_len"], a["tube_last"], a["V"], a["S"], a["N"],
            a["C"], a["max_rows"], a["min_len"], a["nms_iou"], a["work"], a["keep"])


def device_keep(rec, C, min_len, nms_iou, dev):
    o = operands(rec, dev)
    keep = torch.full((o["N"],), 0xAA, dtype=torch.uint8, device=dev)
    lib.call("tuber_tube_nms", *args_of(o, C, min_len, nms_iou, scratch(o["N"], dev), keep))
    return keep.cpu().numpy()


def same(got, want):
    assert np.array_equal(got, want), np.argwhere(got != want)[:10].ravel()


# ------------------------------------------------------------------------------------------------------------------------------
# planted records
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nms_iou,min_len", [(0.3, 1), (0.3, 2), (0.2, 1), (0.1, 2), (2.0 / 6.0, 1), (float(np.nextafter(2.0 / 6.0, 0.0)), 1), (0.0, 1), (1.0, 1)])
def test_planted_cases_equal_the_definition(dev, nms_iou, min_len):
    rec, where = planted()
    assert rec["layout"]["V"] == 10 and len(set(rec["row_cls"].tolist())) == 3
    want = tube_nms(rec, nms_iou, min_len)
    got = device_keep(rec, 3, min_len, nms_iou, dev)
    same(got, want)
    k = {name: int(got[h]) for name, h in where.items()}
    if (nms_iou, min_len) == (0.3, 1):
        assert (k["dup_lo"], k["tie_second"], k["cls_b"], k["vid_b"], k["chain_b"], k["chain_c"], k["beside"], k["odd"], k["nan"]) == (0, 0, 1, 1, 0, 1, 0, 1, 0)
    if nms_iou == 2.0 / 6.0:
        assert k["edge_b"] == 1
    elif nms_iou not in (0.0, 1.0) and 0.33 < nms_iou < 0.34:
        assert k["edge_b"] == 0
    same(device_keep(rec, 3, min_len, nms_iou, dev), got)                  # the same bytes again


def test_a_lane_handed_to_a_new_tube_starts_from_zero(dev):
    """max_gap 0, at most 3 rows per slot.  P (lane 0) and Q (lane 1) run through the video; D takes lane 2 over slots 1..4 on P's box and
    is suppressed; E takes the SAME lane over slots 6..9, far from P, and ends with P: a column of P's table row that kept D's sum would
    give stIoU(P, E) = 4 / (10 + 4 - 8) and suppress E."""
    tubes = [(0, 0, 0.9, span(BOX, 0, 9)), (0, 0, 0.7, span(FAR, 0, 9)), (0, 0, 0.6, span(shifted(BOX, 2.0), 1, 4)), (0, 0, 0.5, span(shifted(BOX, 100.0), 6, 9))]
    rec, (p, q, d, e) = record(tubes, 1, 10)
    assert np.bincount(rec["row_slot"]).max() == 3
    want = tube_nms(rec, 0.3, 1)
    assert (want[p], want[q], want[d], want[e]) == (1, 1, 0, 1)
    same(device_keep(rec, 1, 1, 0.3, dev), want)
    # the mirror image: the late tube is the duplicate and the early one is not
    tubes[2], tubes[3] = (0, 0, 0.6, span(shifted(BOX, 100.0), 1, 4)), (0, 0, 0.5, span(shifted(BOX, 2.0), 6, 9))
    rec, (p, q, d, e) = record(tubes, 1, 10)
    want = tube_nms(rec, 0.3, 1)
    assert (want[p], want[q], want[d], want[e]) == (1, 1, 1, 0)
    same(device_keep(rec, 1, 1, 0.3, dev), want)


# ------------------------------------------------------------------------------------------------------------------------------
# random stores
# ------------------------------------------------------------------------------------------------------------------------------
def random_case(seed, V=3, C=3, slots=12):
    """V videos of 12 slots, 0..6 rows per slot: boxes of about 40 x 60 px around three anchors per video (an anchor a class), every coordinate
    jittered by a normal of sigma 4 px, the anchors drifting 1.5 px per slot; scores from SCORES, so that ties occur; the anchors' paths are
    the ground-truth tubes"""
    rng = np.random.default_rng(seed)
    det_keys, det_boxes, det_probs, gt_keys, gt_boxes, gt_cls, gt_tubes = [], [], [], [], [], [], []
    for v in range(V):
        anchor = np.asarray([[80.0, 90.0], [240.0, 130.0], [400.0, 210.0]]) + rng.uniform(-20, 20, (3, 2))
        angle = rng.uniform(0, 2 * np.pi, 3)
        vel = 1.5 * np.stack([np.cos(angle), np.sin(angle)], axis=1)
        for s in range(slots):
            key = "rv%d-%d" % (v, s + 1)
            for k in range(3):
                ctr = anchor[k] + vel[k] * s
                gt_keys.append(key); gt_boxes.append([ctr[0] - 20, ctr[1] - 30, ctr[0] + 20, ctr[1] + 30]); gt_cls.append(k % C); gt_tubes.append(k)
            for _ in range(int(rng.integers(0, 7))):
                k = int(rng.integers(0, 3))
                ctr = anchor[k] + vel[k] * s
                det_keys.append(key)
                det_boxes.append(np.asarray([ctr[0] - 20, ctr[1] - 30, ctr[0] + 20, ctr[1] + 30]) + rng.normal(0, 4, 4))
                p = np.zeros(C + 1, dtype=np.float32)
                p[k % C] = rng.choice(SCORES)
                det_probs.append(p)
    return dict(det_keys=det_keys, det_boxes=np.asarray(det_boxes, dtype=np.float32), det_probs=np.stack(det_probs), gt_keys=gt_keys,
                gt_boxes=np.asarray(gt_boxes, dtype=np.float64), gt_labels=_onehot(gt_cls), gt_tubes=np.asarray(gt_tubes))


@pytest.fixture(scope="module")
def random_links():
    """per seed the case and its host link record (link settings 0.2 / 2), computed once; asserted here, on the host alone, that the
    comparison below is not all-kept against all-kept"""
    out, total = {}, 0
    for seed in SEEDS:
        case = random_case(seed)
        link = _case_evaluator(case, link_iou=0.2, max_gap=2).link()
        gone = int((tube_nms(link, 0.3, 1) == 0).sum())
        assert gone >= 2, (seed, gone)
        total += gone
        out[seed] = (case, link)
    assert total >= 40, total
    return out


@pytest.mark.parametrize("min_len", [1, 2])
@pytest.mark.parametrize("seed", SEEDS)
def test_random_stores_equal_the_definition(dev, random_links, seed, min_len):
    case, link = random_links[seed]
    assert link["layout"]["V"] == 3 and np.bincount(link["row_slot"]).max() <= 6
    want = tube_nms(link, 0.3, min_len)
    got = device_keep(link, 3, min_len, 0.3, dev)
    same(got, want)
    print("seed %d min_len %d: %d tubes counted, %d suppressed" % (seed, min_len, (want != 2).sum(), (want == 0).sum()))


# ------------------------------------------------------------------------------------------------------------------------------
# the padded [S][K] form: VideoDetections.tubes / VideoActors.tracks
# ------------------------------------------------------------------------------------------------------------------------------
def test_tubes_and_tracks_with_nms_on_a_device_store(dev, capsys):
    seen = []
    lib.set_launch_hook(lambda name, args, launch: (seen.append(name), launch(name, *args))[1])
    try:
        vd, cpu = padded_detections(dev), padded_detections()
        plain = vd.tubes()
        assert seen == ["tuber_tube_link_ranked"]                          # the default path launches what it launched
        del seen[:]
        got = vd.tubes(nms=0.3)
        assert seen == ["tuber_tube_link_ranked", "tuber_tube_nms"] and vd.tubes_path == "device"
        want = cpu.tubes(nms=0.3)
        assert cpu.tubes_path == "host"
        assert len(plain) == 4 and len(got) == len(want) == 3              # without nms the duplicate is there
        for g, w in zip(got, want):
            assert (g["cls"], g["frames"], g["length"]) == (w["cls"], w["frames"], w["length"])
            assert _bits(g["score"]) == _bits(w["score"]) and np.array_equal(g["boxes"], w["boxes"])
        assert [(t["cls"], t["length"]) for t in plain] == [(1, 6), (2, 6), (1, 4), (1, 4)]
        assert len(padded_detections(dev, nms_iou=0.3).tubes()) == 3
        va, cpu_a = padded_actors(dev), padded_actors()
        del seen[:]
        plain = va.tracks()
        assert seen == ["tuber_tube_link_ranked", "tuber_track_actions"]
        del seen[:]
        got = va.tracks(nms=0.3)
        assert seen == ["tuber_tube_link_ranked", "tuber_track_actions", "tuber_tube_nms"] and va.tracks_path == "device"
        want = cpu_a.tracks(nms=0.3)
        assert cpu_a.tracks_path == "host" and len(plain) == 4 and len(got) == len(want) == 2
        for g, w in zip(got, want):
            assert (g["frames"], g["length"], g["labels"]) == (w["frames"], w["length"], w["labels"]) and _bits(g["score"]) == _bits(w["score"])
            assert np.array_equal(g["boxes"], w["boxes"]) and np.array_equal(g["mean"].view(np.int64), w["mean"].view(np.int64))
            assert np.array_equal(g["peak"].view(np.int32), w["peak"].view(np.int32))
    finally:
        lib.set_launch_hook(None)
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------------------------------------
# DeviceVideoMAP
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS[:3])
def test_device_video_map_with_tube_nms(dev, random_links, seed):
    case, _ = random_links[seed]
    kw = dict(link_iou=0.2, max_gap=2, min_len=1, thresholds=(0.2, 0.5, 0.75))
    ev = _case_evaluator(case, tube_nms=0.3, **kw)
    want = ev.evaluate()
    n_gt, flags, link = ev.match()
    st = _store(case, device=dev, tube_nms=0.3, **kw)
    timings = {}
    got = st.evaluate_video(timings=timings)
    assert st.video_path == "device" and "tuber_tube_nms_ms" in timings
    _check_results(got, want, n_gt)
    # the decisions behind the numbers
    a = st.video_arrays()
    dl = st.link(a)
    keep = st.nms(a, dl)
    same(keep.cpu().numpy(), link["tube_keep"])
    df = st.match_video(a, dict(dl, tube_len=dl["tube_len"].masked_fill(keep == 0, 0))).cpu().numpy()
    gone = link["tube_keep"] == 0
    assert gone.sum() >= 2
    for i, thr in enumerate(a["thr"]):
        same(df[i], flags[thr])
        assert (df[i][gone] == 2).all(), thr
    heads = [t["head"] for t in st.tubes()]
    assert heads == [t["head"] for t in link["tubes"] if link["tube_keep"][t["head"]] != 0]
    merged = type(st).merge([st])
    assert merged.tube_nms == 0.3
    # without the keyword: the parent's path and the parent's numbers
    plain_ev = _case_evaluator(case, **kw)
    plain = _store(case, device=dev, **kw)
    seen = []
    lib.set_launch_hook(lambda name, args, launch: (seen.append(name), launch(name, *args))[1])
    try:
        got_plain = plain.evaluate_video()
    finally:
        lib.set_launch_hook(None)
    assert seen == ["tuber_tube_link", "tuber_tube_match", "tuber_ranked_ap"] and plain.video_path == "device" and plain.tube_nms is None
    _check_results(got_plain, plain_ev.evaluate(), plain_ev.match()[0])
    assert len(plain.tubes()) == len(link["tubes"]) > len(heads)


# ------------------------------------------------------------------------------------------------------------------------------
# the contract's edges
# ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(dev):
    rec, _ = planted()
    o = operands(rec, dev)
    N = o["N"]
    keep = torch.full((N,), 0xAA, dtype=torch.uint8, device=dev)
    work = scratch(N, dev)
    for over in (dict(max_rows=65), dict(min_len=0), dict(nms_iou=float("nan")), dict(nms_iou=-0.1), dict(nms_iou=1.5), dict(work=None),
                 dict(work=work[4:]), dict(N=-1), dict(S=-1), dict(V=-1), dict(C=0), dict(max_rows=0), dict(row_head=None), dict(keep=None)):
        code = rc("tuber_tube_nms", *args_of(o, 3, 1, 0.3, work, keep, over))
        assert code < 0, (over, code)
    torch.cuda.synchronize()
    assert (keep == 0xAA).all() and (work == 0x7F).all()
    assert lib.query("tuber_tube_nms_work_bytes", 0) == 0
    sizes = [lib.query("tuber_tube_nms_work_bytes", n) for n in (1, 7, 64, 65, 1000, 100000)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    for over in (dict(N=0), dict(V=0)):
        assert rc("tuber_tube_nms", *args_of(o, 3, 1, 0.3, work, keep, over)) == 0
    torch.cuda.synchronize()
    assert (keep == 0xAA).all() and (work == 0x7F).all()
    assert rc("tuber_tube_nms", *args_of(o, 3, 1, 0.3, work, keep)) == 0   # and the call itself is fine
    torch.cuda.synchronize()
    same(keep.cpu().numpy(), tube_nms(rec, 0.3, 1))


def test_more_live_tubes_than_lanes_are_flagged_not_decided(dev):
    """33 one-row heads in slot 0 and 33 in slot 1 of class 0, every one with tube_last = 5: 66 tubes live at slot 1 with max_rows = 33.  A link
    inside the linker's bounds cannot look like this; the kernel says so with byte 3 and decides the video's other class as usual."""
    grid = lambda i: (50.0 * (i % 8), 80.0 * (i // 8), 50.0 * (i % 8) + 40, 80.0 * (i // 8) + 60)
    tubes = [(0, 0, 0.5, {s: grid(i)}) for s in (0, 1) for i in range(33)]
    tubes += [(0, 1, 0.9, span(BOX, 2, 5)), (0, 1, 0.8, span(shifted(BOX, 2.0), 2, 5)), (0, 1, 0.7, span(FAR, 2, 5))]
    rec, heads = record(tubes, 1, 6)
    rec["tube_last"][heads[:66]] = 5
    want = tube_nms(rec, 0.3, 1)
    got = device_keep(rec, 2, 1, 0.3, dev)
    assert (got[heads[:66]] == 3).all() and (want[heads[:66]] == 1).all()
    assert got[heads[66:]].tolist() == want[heads[66:]].tolist() == [1, 0, 1]
    rest = np.setdiff1d(np.arange(len(got)), heads)
    assert (got[rest] == 2).all()


def test_malformed_heads_are_not_counted(dev):
    rec, where = planted()
    N = len(rec["row_head"])
    beyond, forward = where["vid_a"], where["cls_b"]                       # both are heads of tubes that suppress nothing and are not suppressed
    follower = beyond + 1
    assert rec["row_head"][follower] == beyond
    bad = dict(rec, row_head=rec["row_head"].copy())
    bad["row_head"][beyond] = N + 5
    bad["row_head"][forward] = forward + 1
    # the definition's view: those rows gone, and with them the tubes they headed (a follower whose head is no head row is not counted)
    clean = dict(rec, row_head=rec["row_head"].copy())
    for h in (beyond, forward):
        clean["row_head"][rec["row_head"] == h] = -1
    want = tube_nms(clean, 0.3, 1)
    assert want[beyond] == want[forward] == 2 and (want == 0).sum() >= 5
    o = operands(bad, dev)
    keep = torch.full((N,), 0xAA, dtype=torch.uint8, device=dev)
    assert rc("tuber_tube_nms", *args_of(o, 3, 1, 0.3, scratch(N, dev), keep)) == 0
    same(keep.cpu().numpy(), want)
