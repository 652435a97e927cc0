"""Actor tracks on the GPU: ``tuber_detect_actors`` (csrc/detect.hip; bounds from ``tuber_detect_actors_limits``) on synthetic
head outputs against ``detect.decode_actors_host`` -- the definition -- and, bit for bit, against ``tuber_detect_ava``'s scores and
``PostProcessAVA.decode``'s boxes; ``tuber_track_actions`` (csrc/tube_map.hip; ``tuber_track_actions_limits``) behind ``tuber_tube_link_ranked``
against ``evaluation.actor_tracks``, bit for bit; and ``VideoDetector(..., actors=A)`` with ``VideoActors.tracks()`` end to end on the name-hashed
AVA model of tests/test_video_gpu.py.

Fixtures of the decode.  Actor probabilities lie on a lattice, (0.85, 0.98) for an actor and (0.10, 0.65) otherwise, away from the gate at 0.8,
are converted to logits in fp64 and rounded to the input dtype; everything compared is then recomputed in fp64 FROM THE ROUNDED INPUTS, and
before any launch ``_assert_separated`` checks on the CPU that no actor probability lies within the tolerance of the gate and no two distinct
ones within the tolerance of each other (tied ones are bit-equal by construction: duplicated ``logits_b`` rows).  Under that condition the set
of actors and their order are determined and must equal the definition exactly.

Tolerance of the floats: measured, not fixed -- the rule of tests/test_detect_gpu.py.  ``err`` is the largest error of the fp32 torch expression
``sigmoid(logits) * softmax(logits_b)[..., 1]`` (and of its second factor) against the fp64 formula on the fixture at hand; the kernel may err
by at most ``max(2 x err, 2^-22)``.  Both figures are printed (run with -s; profiles/actor_score_error.txt keeps the lines)."""
import os

import numpy as np
import pytest
import torch

from test_actors_cpu import LINK_IOU, MAX_GAP, TRACKS, track_fixture
from test_video_gpu import H0, KEYS, NFRAMES, SIZE, W0, _gather, _launches, _model
from tubelet_transformer_amd import input_pipeline as ip
from tubelet_transformer_amd import lib
from tubelet_transformer_amd.config import load_cfg
from tubelet_transformer_amd.criterion import PostProcessAVA
from tubelet_transformer_amd.detect import ACTOR_FIELDS, FIELDS, Detector, actors_launch, decode_actors_host, empty_actors, empty_detections
from tubelet_transformer_amd.evaluation import actor_tracks
from tubelet_transformer_amd.misc import NestedTensor
from tubelet_transformer_amd.tuber import build_model
from tubelet_transformer_amd.video import VideoActors, VideoDetector, clip_indices, working_geometry

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 2.0 ** -22
GATE = 0.8
EINVAL, EBOUNDS = -1, -2
SIZES = np.array([[64, 96], [240, 320], [255, 341]], dtype=np.int64)


def _round(a, dtype):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).to(torch.float32).to(dtype).float().numpy()


def _softmax64(x):
    x = x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        e = np.exp(x - np.max(x, axis=-1, keepdims=True))
        return e / e.sum(-1, keepdims=True)


# ------------------------------------------------------------------------------------------------------------------------------
# tuber_detect_actors
# ------------------------------------------------------------------------------------------------------------------------------
def actor_fixture(seed, Qtot, Qs, C, q_begin=None, dtype=torch.float32, B=3, empty_clip=True, nans=True, ties=False):
    """clip 0 generic; clip 1 (``nans``, Qs >= 4): an actor whose row holds one NaN logit, a query with a NaN actor logit; the last clip
    (``empty_clip``): no actor.  ``ties`` (clip 0, Qs >= 10): queries 3 and 7 share the clip's best ``logits_b`` row, 5 and 9 another one."""
    rng = np.random.default_rng(seed)
    lg = rng.normal(0.0, 2.0, (B, Qtot, C))
    lb = np.empty((B, Qtot, 3))
    qb = np.zeros(B, dtype=np.int64) if q_begin is None else np.asarray(q_begin, dtype=np.int64)
    for b in range(B):
        q0 = int(min(max(qb[b], 0), Qtot - Qs))                         # where an outside slice would be if it were inside
        gated = rng.random(Qtot) < 0.6
        if empty_clip and b == B - 1:
            gated[:] = False
        else:
            gated[q0 + rng.integers(Qs)] = True
        if nans and b == 1 and Qs >= 4:
            gated[q0:q0 + 3] = True
        if ties and b == 0:
            gated[[q0 + 3, q0 + 5, q0 + 7, q0 + 9]] = True
        u = (rng.permutation(Qtot) + 0.5) / Qtot
        pb = np.where(gated, 0.85 + 0.13 * u, 0.10 + 0.55 * u)
        if ties and b == 0:
            pb[q0 + 3] = 0.985
        lb[b, :, 0], lb[b, :, 2] = 0.0, -1.0
        lb[b, :, 1] = np.log(pb * (1.0 + np.exp(-1.0)) / (1.0 - pb))
    lg, lb = _round(lg, dtype), _round(lb, dtype)
    if ties:
        q0 = int(qb[0])
        lb[0, q0 + 7], lb[0, q0 + 9] = lb[0, q0 + 3], lb[0, q0 + 5]
    if nans and B > 1 and Qs >= 4:
        q0 = int(qb[1])
        lg[1, q0 + 1, C // 2] = np.nan
        lb[1, q0 + 2, 1] = np.nan
    bx = _round(np.concatenate([rng.uniform(0.2, 0.8, (B, Qtot, 2)), rng.uniform(0.05, 0.4, (B, Qtot, 2))], axis=-1), dtype)
    return dict(lg=lg, lb=lb, bx=bx, sizes=SIZES[:B], qb=None if q_begin is None else qb.astype(np.int32), Qs=Qs, C=C, dtype=dtype, ties=ties)


def exact64(fx):
    """(action score [B, Qtot, C], actor probability [B, Qtot]) in fp64 from the rounded inputs"""
    pb = _softmax64(fx["lb"])[..., 1]
    with np.errstate(over="ignore"):
        return (1.0 / (1.0 + np.exp(-fx["lg"].astype(np.float64)))) * pb[:, :, None], pb


def _slices(fx):
    B, Qtot = fx["lg"].shape[:2]
    for b in range(B):
        q0 = 0 if fx["qb"] is None else int(fx["qb"][b])
        if 0 <= q0 <= Qtot - fx["Qs"]:
            yield b, q0


def _assert_separated(fx, tol):
    """the condition of the fixture (module docstring), in fp64 on the CPU; bit-equal probabilities are ties, near-equal ones are not allowed"""
    _, pb = exact64(fx)
    for b, q0 in _slices(fx):
        p = pb[b, q0:q0 + fx["Qs"]]
        p = np.sort(p[~np.isnan(p)])
        assert np.abs(p - GATE).min() > tol, "an actor probability within the tolerance of the gate"
        d = np.diff(p)
        if fx["ties"]:
            d = d[d != 0.0]
        assert len(d) == 0 or d.min() > tol, "two distinct actor probabilities within the tolerance of each other"


def _dev(fx, dev):
    t = lambda a: torch.from_numpy(a).to(dev).to(fx["dtype"]).contiguous()
    return (t(fx["lg"]), t(fx["lb"]), t(fx["bx"]), torch.from_numpy(fx["sizes"]).to(dev).float(),
            None if fx["qb"] is None else torch.from_numpy(fx["qb"]).to(dev))


def _torch_error(fx, dev):
    """largest error of the fp32 torch expression (module docstring) against fp64 on this fixture, measured on the device"""
    lg, lb, _, _, _ = _dev(fx, dev)
    s, pb = exact64(fx)
    pbt = lb.float().softmax(-1)[..., 1]
    st = lg.float().sigmoid() * pbt[:, :, None]
    return max(float(np.nanmax(np.abs(st.double().cpu().numpy() - s))), float(np.nanmax(np.abs(pbt.double().cpu().numpy() - pb))))


def _launch(fx, A, dev, out=None, over=()):
    lg, lb, bx, sizes, qb = _dev(fx, dev)
    B, Qtot, C = lg.shape
    out = empty_actors(B, A, C, dev) if out is None else out
    args = dict(lg=lg, lb=lb, bx=bx, sizes=sizes, qb=qb, B=B, Qtot=Qtot, Qs=fx["Qs"], C=C, NB=lb.shape[-1], lb_rows=Qtot,
                dtypes=7 if fx["dtype"] == torch.bfloat16 else 0, actor_thr=GATE, A=A)
    args.update(zip(("o_box", "o_actor", "o_query", "o_actions", "o_count", "o_total"), out.tensors()))
    args.update(over)
    code = lib.call_rc("tuber_detect_actors", *args.values())
    torch.cuda.synchronize()
    return code, out


def _check_kernel(fx, A, dev, label):
    """the whole comparison of one fixture at one A; returns the definition's result"""
    err = _torch_error(fx, dev)
    tol = max(2.0 * err, FLOOR)
    _assert_separated(fx, tol)                                          # before the launch: a condition of the fixture, not a measurement
    code, out = _launch(fx, A, dev)
    assert code == 0
    want = decode_actors_host(fx["lg"], fx["lb"], fx["bx"], fx["sizes"], GATE, A, q_begin=fx["qb"], Qs=fx["Qs"])
    got = {k: t.cpu().numpy() for k, t in zip(ACTOR_FIELDS, out.tensors())}
    for k in ("count", "total", "queries"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["boxes"].view(np.int32), want["boxes"].view(np.int32))          # fp32 numpy, operation for operation
    assert np.array_equal(np.isnan(got["actions"]), np.isnan(want["actions"]))
    s, pb = exact64(fx)
    kerr = 0.0
    for b in range(len(want["count"])):
        n, q0 = int(want["count"][b]), 0 if fx["qb"] is None else int(fx["qb"][b])
        if n:
            q = q0 + want["queries"][b, :n]
            ea = np.abs(got["actor"][b, :n].astype(np.float64) - pb[b, q])
            es = np.abs(got["actions"][b, :n].astype(np.float64) - s[b, q])
            kerr = max(kerr, float(ea.max()), float(np.nanmax(es)) if not np.isnan(es).all() else 0.0)
        assert not got["boxes"][b, n:].any() and not got["actor"][b, n:].any() and not got["actions"][b, n:].any()
    print("actors %s A=%d: torch fp32 max error %.3e, kernel max error %.3e, tolerance %.3e, actors %s" % (label, A, err, kerr, tol, want["total"].tolist()))
    assert kerr <= tol
    return want


ACTOR_CASES = {
    "Q15_C80_A8": (dict(seed=1, Qtot=15, Qs=15, C=80), 8),
    "Q15_C80_A16": (dict(seed=1, Qtot=15, Qs=15, C=80), 16),                     # A > Qs
    "Q1_C1": (dict(seed=3, Qtot=1, Qs=1, C=1), 8),
    "Qs15_of_60": (dict(seed=4, Qtot=60, Qs=15, C=80, q_begin=[0, 15, 50], empty_clip=False), 8),       # 50 + 15 > 60: outside
    "bf16_Q5_C12": (dict(seed=7, Qtot=5, Qs=5, C=12, dtype=torch.bfloat16), 8),
    "C7_scalar_stores": (dict(seed=5, Qtot=15, Qs=15, C=7), 8),
    "Q1024_the_largest": (dict(seed=6, Qtot=1024, Qs=1024, C=4, B=2, nans=False), 40),
}


@pytest.mark.parametrize("case", sorted(ACTOR_CASES))
def test_detect_actors_equals_the_definition(dev, case):
    kw, A = ACTOR_CASES[case]
    if case == "Q1024_the_largest":
        assert kw["Qs"] == lib.query("tuber_detect_actors_limits", 0)
    fx = actor_fixture(**kw)
    want = _check_kernel(fx, A, dev, case)
    assert want["total"][-1] == 0 and want["count"][-1] == 0            # the clip with no actor, or with its slice outside the queries
    if case == "Q15_C80_A8":
        assert want["total"][1] > A and want["count"][1] == A           # more actors than A
    if case == "Q15_C80_A16":
        assert 0 < want["total"][0] == want["count"][0] < A
        assert 2 not in want["queries"][1] and 1 in want["queries"][1]  # the NaN actor logit; the row with a NaN logit is kept
        assert np.isnan(want["actions"][1, want["queries"][1].tolist().index(1), 40])
    if case == "Qs15_of_60":
        _, pb = exact64(fx)
        assert (pb[2, 45:60] > GATE).any()                              # the last clip has actors: its result is empty because of the slice
    if case == "Q1024_the_largest":
        assert want["total"][0] > 500 and want["count"].tolist() == [40, 0]


def test_tied_actors_keep_query_order_and_the_cut_falls_inside_the_tie(dev):
    fx = actor_fixture(seed=21, Qtot=15, Qs=15, C=80, ties=True)
    _, pb = exact64(fx)
    assert pb[0, 3] == pb[0, 7] == np.nanmax(pb[0]) and pb[0, 5] == pb[0, 9]          # equal in fp64 as well
    for A in (8, 1, 2):
        want = _check_kernel(fx, A, dev, "ties")
        assert want["queries"][0].tolist()[:2] == [3, 7][:A]
    order = decode_actors_host(fx["lg"], fx["lb"], fx["bx"], fx["sizes"], GATE, 15)["queries"][0].tolist()
    at5 = order.index(5)
    assert order[at5 + 1] == 9
    want = _check_kernel(fx, at5 + 1, dev, "ties")                      # the cut between 5 and 9
    assert want["queries"][0].tolist()[-1] == 5 and 9 not in want["queries"][0]
    _, out = _launch(fx, 8, dev)
    a = out.actor[0].cpu().numpy().view(np.int32)
    assert a[0] == a[1] and a[1] != a[2]


@pytest.mark.parametrize("case", ("Q12_C80", "bf16_Q5_C12"))
def test_action_rows_are_detect_avas_scores_and_decodes_boxes_bit_for_bit(dev, case):
    """device against device: ``tuber_detect_ava`` with score_thr = 0 and K = Qs * C reports every candidate (q, c) of a gated query"""
    fx = actor_fixture(seed=8, Qtot=12, Qs=12, C=80) if case == "Q12_C80" else actor_fixture(seed=7, Qtot=5, Qs=5, C=12, dtype=torch.bfloat16)
    lg, lb, bx, sizes, _ = _dev(fx, dev)
    B, Q, C = lg.shape
    K = Q * C
    assert K <= lib.query("tuber_detect_limits", 1)
    det = empty_detections(B, K, dev)
    lib.call("tuber_detect_ava", lg, lb, bx, sizes, None, B, Q, Q, C, 3, Q, 7 if fx["dtype"] == torch.bfloat16 else 0, GATE, 0.0, K, *det.tensors())
    code, out = _launch(fx, Q, dev)
    assert code == 0
    det = {k: t.cpu().numpy() for k, t in zip(FIELDS, det.tensors())}
    got = {k: t.cpu().numpy() for k, t in zip(ACTOR_FIELDS, out.tensors())}
    _, tboxes, _ = PostProcessAVA().decode({"pred_logits": lg, "pred_logits_b": lb, "pred_boxes": bx}, sizes)
    tboxes = tboxes.cpu().numpy()
    seen = 0
    for b in range(B):
        n = int(det["count"][b])
        assert n == det["total"][b]
        row = {int(q): a for a, q in enumerate(got["queries"][b, :int(got["count"][b])].tolist())}
        assert sorted(row) == sorted(set(det["queries"][b, :n].tolist()) | {q for q in row if np.isnan(got["actions"][b, row[q]]).all()})
        a = np.array([row[int(q)] for q in det["queries"][b, :n]], dtype=np.int64)
        assert np.array_equal(got["actions"][b, a, det["labels"][b, :n]].view(np.int32), det["scores"][b, :n].view(np.int32))
        assert np.array_equal(got["actor"][b, a].view(np.int32), det["aux"][b, :n].view(np.int32))
        assert np.array_equal(got["boxes"][b, a].view(np.int32), det["boxes"][b, :n].view(np.int32))
        assert n == int((~np.isnan(got["actions"][b, :len(row)])).sum())  # every entry that is not NaN is a candidate there
        for q, r in row.items():
            assert np.array_equal(got["boxes"][b, r].view(np.int32), tboxes[b, q].view(np.int32)), "boxes differ from decode()'s"
        seen += n
    assert seen > 100 if case == "Q12_C80" else seen > 10


def test_detect_actors_refuses_bad_calls_and_writes_nothing(dev):
    assert [lib.query("tuber_detect_actors_limits", w) for w in (0, 1, 2, 3)] == [1024, 1024, 8, -1]
    fx = actor_fixture(seed=1, Qtot=15, Qs=15, C=80)
    A = 8
    out = empty_actors(3, A, 80, dev)
    for t in out.tensors():
        t.fill_(7)
    for name in ("lg", "lb", "bx", "sizes", "o_box", "o_actor", "o_query", "o_actions", "o_count", "o_total"):
        assert _launch(fx, A, dev, out, over={name: None})[0] == EINVAL, name
    for kw in (dict(B=0), dict(B=-1), dict(A=0), dict(A=-3), dict(actor_thr=float("nan")), dict(Qs=0), dict(Qs=16), dict(C=0), dict(NB=1), dict(lb_rows=2),
               dict(dtypes=8)):
        assert _launch(fx, A, dev, out, over=kw)[0] == EINVAL, kw
    for kw in (dict(A=1025), dict(NB=9), dict(Qtot=1025, Qs=1025, lb_rows=1025)):       # legal calls beyond the bounds: refused before anything is read
        assert _launch(fx, A, dev, out, over=kw)[0] == EBOUNDS, kw
    assert all(bool((t == 7).all()) for t in out.tensors())            # untouched
    assert _launch(fx, A, dev, out)[0] == 0
    assert not any(bool((t == 7).all()) for t in out.tensors())
    # beyond the bounds the launch helper answers by the torch restatement
    big = actor_fixture(seed=9, Qtot=15, Qs=15, C=12)
    err = _torch_error(big, dev)
    tol = max(2.0 * err, FLOOR)
    _assert_separated(big, tol)
    lg, lb, bx, sizes, _ = _dev(big, dev)
    got = actors_launch(lg, lb, bx, sizes, None, 15, GATE, 1025)
    want = decode_actors_host(big["lg"], big["lb"], big["bx"], big["sizes"], GATE, 1025)
    for k in ("count", "total", "queries", "boxes"):
        assert np.array_equal(getattr(got, k).cpu().numpy(), want[k]), k
    for k in ("actor", "actions"):
        assert np.nanmax(np.abs(getattr(got, k).cpu().numpy().astype(np.float64) - want[k])) <= tol


# ------------------------------------------------------------------------------------------------------------------------------
# tuber_track_actions
# ------------------------------------------------------------------------------------------------------------------------------
def _track_buffers(N, C, dev, fill=None):
    out = dict(row_smooth=torch.zeros(N, C, dtype=torch.float64, device=dev), track_mean=torch.zeros(N, C, dtype=torch.float64, device=dev),
               track_peak=torch.zeros(N, C, dtype=torch.float32, device=dev))
    if fill is not None:
        for t in out.values():
            t.fill_(fill)
    return out


def _link_and_track(fx, dev, window, max_gap=MAX_GAP):
    S, A, C = fx["S"], fx["A"], fx["C"]
    N = S * A
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    i32 = torch.int32
    link = dict(row_cls=torch.empty(N, dtype=i32, device=dev), row_head=torch.empty(N, dtype=i32, device=dev),
                tube_score=torch.zeros(N, dtype=torch.float64, device=dev), tube_len=torch.zeros(N, dtype=i32, device=dev),
                tube_last=torch.full((N,), -1, dtype=i32, device=dev))
    label = up(np.where(fx["queries"] >= 0, 0, -1).astype(np.int32))
    lib.call("tuber_tube_link_ranked", up(fx["box"]), label, up(fx["actor"]), up((np.arange(S + 1) * A).astype(np.int32)), up(np.array([0, S], dtype=np.int32)),
             1, S, N, 1, A, LINK_IOU, max_gap, *link.values())
    out = _track_buffers(N, C, dev, fill=7)
    lib.call("tuber_track_actions", up(fx["actions"]), link["row_head"], link["tube_last"], S, A, C, window, *out.values())
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in {**link, **out}.items()}
    return got


@pytest.mark.parametrize("window", (0, 1, 2, 6, 1 << 30))
@pytest.mark.parametrize("C", (5, 80, 300))
def test_track_actions_equals_the_definition_bit_for_bit(dev, C, window):
    """C = 5: the hand-written video of tests/test_actors_cpu.py; 80: AVA's classes; 300: more classes than the workgroup has threads"""
    fx = track_fixture(C=C)
    want = actor_tracks(fx["box"], fx["actor"], fx["queries"], fx["actions"], 6, 4, LINK_IOU, MAX_GAP, window)
    head = want["row_head"]
    assert {h: np.nonzero(head == h)[0].tolist() for h in sorted(set(head[head >= 0].tolist()))} == TRACKS
    got = _link_and_track(fx, dev, window)
    for k in ("row_head", "tube_len", "tube_last"):
        assert np.array_equal(got[k].astype(np.int64), want[k]), k
    assert np.array_equal(got["tube_score"].view(np.int64), want["tube_score"].view(np.int64))
    for k in ("row_smooth", "track_mean"):
        assert np.array_equal(got[k].view(np.int64), want[k].view(np.int64)), k
    assert np.array_equal(got["track_peak"].view(np.int32), want["track_peak"].view(np.int32))
    assert not got["row_smooth"][head < 0].any()                        # rows that are not counted, over the 7s the buffers held
    no_head = head != np.arange(24)
    assert not got["track_mean"][no_head].any() and not got["track_peak"][no_head].any()
    assert got["track_mean"][0].all() and got["row_smooth"][head >= 0].all()


def test_track_actions_propagates_nan_like_the_definition(dev):
    fx = track_fixture(C=80)
    fx["actions"][12, 4] = np.nan
    want = actor_tracks(fx["box"], fx["actor"], fx["queries"], fx["actions"], 6, 4, LINK_IOU, MAX_GAP, 1)
    got = _link_and_track(fx, dev, 1)
    for k, view in (("row_smooth", np.int64), ("track_mean", np.int64), ("track_peak", np.int32)):
        nan = np.isnan(want[k])
        assert nan.any() and np.array_equal(np.isnan(got[k]), nan), k
        assert np.array_equal(got[k][~nan].view(view), want[k][~nan].view(view)), k
    assert np.isnan(want["track_peak"][0, 4]) and np.isnan(want["row_smooth"][[8, 12, 16], 4]).all()


def test_track_actions_refuses_bad_calls_and_writes_nothing(dev):
    assert [lib.query("tuber_track_actions_limits", w) for w in (0, 1, 2)] == [64, 4096, -1]
    fx = track_fixture()
    S, A, C = 6, 4, 5
    N = S * A
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    want = actor_tracks(fx["box"], fx["actor"], fx["queries"], fx["actions"], S, A, LINK_IOU, MAX_GAP, 1)
    out = _track_buffers(N, C, dev, fill=7)
    ok = dict(actions=up(fx["actions"]), row_head=up(want["row_head"].astype(np.int32)), tube_last=up(want["tube_last"].astype(np.int32)), S=S, A=A, C=C,
              window=1, **out)
    rc = lambda **kw: lib.call_rc("tuber_track_actions", *{**ok, **kw}.values())
    for name in ("actions", "row_head", "tube_last", "row_smooth", "track_mean", "track_peak"):
        assert rc(**{name: None}) == EINVAL, name
    for kw in (dict(S=-1), dict(A=0), dict(A=-1), dict(A=65), dict(C=0), dict(C=4097), dict(window=-1), dict(S=1 << 30, A=64)):
        assert rc(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out.values())             # untouched
    assert rc(S=0) == 0                                                 # nothing to do: no launch either
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out.values())
    assert rc() == 0                                                    # the host definition's link records in, the same bits out
    torch.cuda.synchronize()
    assert np.array_equal(out["row_smooth"].cpu().numpy().view(np.int64), want["row_smooth"].view(np.int64))
    assert np.array_equal(out["track_mean"].cpu().numpy().view(np.int64), want["track_mean"].view(np.int64))


# ------------------------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------------------------
SETTINGS = dict(actor_thr=0.0, score_thr=0.0, topk=8)                   # tests/test_video_gpu.py: every (query, class) is a candidate
ACTORS = 8


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


def _same_tracks(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert sorted(x) == sorted(y) == sorted(("score", "frames", "boxes", "actor", "queries", "actions", "smooth", "mean", "peak", "labels", "length"))
        assert (x["frames"], x["labels"], x["length"]) == (y["frames"], y["labels"], y["length"])
        assert np.float64(x["score"]).view(np.int64) == np.float64(y["score"]).view(np.int64)
        for k, view in (("boxes", np.int32), ("actor", np.int32), ("actions", np.int32), ("peak", np.int32), ("smooth", np.int64), ("mean", np.int64)):
            assert x[k].shape == y[k].shape and np.array_equal(np.ascontiguousarray(x[k]).view(view), np.ascontiguousarray(y[k]).view(view)), k
        assert np.array_equal(x["queries"], y["queries"])


def test_video_detector_with_actors_end_to_end(dev, monkeypatch, capsys):
    cfg, model = _model("TubeR_CSN50_AVA21.yaml")
    T, rate, C = cfg.CONFIG.DATA.TEMP_LEN, cfg.CONFIG.DATA.FRAME_RATE, cfg.CONFIG.DATA.NUM_CLASSES
    frames = np.random.default_rng(11).integers(0, 256, (NFRAMES, H0, W0, 3), dtype=np.uint8)
    nh, nw, y1, x1, h, w = working_geometry(H0, W0, SIZE)
    # the option off: the parent's path
    base = VideoDetector(cfg, model, batch=2, **SETTINGS)(frames, keys=KEYS)
    assert base.actors is None
    base = {k: t.clone() for k, t in zip(FIELDS, base.tensors())}
    # the expected actors: the batches (the padded last one included) gathered in numpy through Detector(actors=8)
    src = torch.from_numpy(frames).to(dev)
    (bh, kh, bv, kv), ksh, ksv, y0, rows = ip._device_coeffs(dev, H0, W0, nh, nw)
    small = torch.empty(NFRAMES, nh, nw, 3, dtype=torch.uint8, device=dev)
    tmp = torch.empty(NFRAMES * rows * nw * 3, dtype=torch.uint8, device=dev)
    lib.call("tuber_frames_resize", src, tmp, small, NFRAMES, H0, W0, nh, nw, bh, kh, ksh, bv, kv, ksv, y0, rows)
    clips = _gather(small.cpu().numpy(), clip_indices(NFRAMES, KEYS + [KEYS[-1]], T, rate, "ava"), (y1, x1, h, w), ip.normalize_lut())
    det = Detector(cfg, model, actors=ACTORS, **SETTINGS)
    want = {k: [] for k in ACTOR_FIELDS}
    mask = torch.zeros(2, h, w, dtype=torch.bool, device=dev)
    for b in range(3):
        d = det(NestedTensor(torch.from_numpy(clips[2 * b:2 * b + 2]).to(dev), mask), [[H0, W0]] * 2, [T // 2] * 2)
        for k, t in zip(ACTOR_FIELDS, d.actors.tensors()):
            want[k].append(t.clone())
        if b == 0:
            for k, t in zip(FIELDS, d.tensors()):
                assert torch.equal(t, base[k][:2]), k
    host = d.actors.to_host()                                           # one copy, trimmed
    assert [hh["count"] for hh in host] == want["count"][-1].tolist() and host[0]["actions"].shape == (host[0]["count"], C)
    want = {k: torch.cat(v)[:len(KEYS)] for k, v in want.items()}
    with capsys.disabled():
        print("actors per key %s, kept %s" % (want["total"].tolist(), want["count"].tolist()))
    assert int(want["count"].min()) >= 1 and want["actions"].shape == (len(KEYS), ACTORS, C)
    # the video path
    vdet = VideoDetector(cfg, model, batch=2, actors=ACTORS, **SETTINGS)
    assert vdet.detector.actors == ACTORS and vdet.actor_settings == dict(link_iou=0.2, max_gap=2, min_len=1, window=1, label_thr=0.05)
    first = vdet(frames, keys=KEYS)                                     # captures the graph
    first = {k: t.clone() for k, t in zip(ACTOR_FIELDS, first.actors.tensors())}
    (vd, seen), syncs = _count_syncs(monkeypatch, lambda: _launches(lambda: vdet(torch.from_numpy(frames), keys=KEYS, chunk=16)))
    assert syncs == [], syncs                                           # a replaying call reads nothing back and waits for nothing
    assert seen.count("tuber_video_clips") == 3 and "tuber_detect_actors" not in seen and "tuber_detect_ava" not in seen      # both inside the replay
    assert vdet.detector.eval.captures == 1 and vdet.detector.eval.eager_calls == 0
    for k, t in zip(FIELDS, vd.tensors()):                              # the seven existing fields are what they are without the option
        assert t.shape == base[k].shape and torch.equal(t, base[k]), k
    va = vd.actors
    assert isinstance(va, VideoActors) and va.keys == KEYS and va.class_num == C
    for k, t in zip(ACTOR_FIELDS, va.tensors()):
        assert t.shape == want[k].shape and torch.equal(t, want[k]), k
        assert torch.equal(first[k], want[k]), k
    # the action rows are the ranked decode's scores: every kept (query, class) pair of the seven fields, bit for bit
    q7, c7, s7, n7 = (getattr(vd, k).cpu().numpy() for k in ("queries", "labels", "scores", "count"))
    qa, act = va.queries.cpu().numpy(), va.actions.cpu().numpy()
    hits = 0
    for i in range(len(KEYS)):
        row = {int(q): a for a, q in enumerate(qa[i].tolist()) if q >= 0}
        for j in range(int(n7[i])):
            if int(q7[i, j]) in row:
                assert act[i, row[int(q7[i, j])], c7[i, j]].view(np.int32) == s7[i, j].view(np.int32)
                hits += 1
    assert hits >= 1
    # tracks: on the device, and what the definition gives on the store read back
    capsys.readouterr()
    (tracks, seen), syncs = _count_syncs(monkeypatch, lambda: _launches(lambda: va.tracks()))
    assert va.tracks_path == "device" and capsys.readouterr().err == ""
    assert seen == ["tuber_tube_link_ranked", "tuber_track_actions"] and syncs.count("cpu") == 1 and "synchronize" not in syncs      # one copy back
    cpu = VideoActors(va.keys, *[t.cpu() for t in va.tensors()], settings=va.settings)
    _same_tracks(tracks, cpu.tracks())
    assert cpu.tracks_path == "host" and "tracks on the host" in capsys.readouterr().err and len(tracks) >= 1
    with capsys.disabled():
        print("%d tracks, lengths %s, labels of the longest %s" % (len(tracks), sorted((t["length"] for t in tracks), reverse=True)[:8],
                                                                max(tracks, key=lambda t: t["length"])["labels"][:5]))
    assert sum(t["length"] for t in tracks) == int(want["count"].sum()) and all(set(t["frames"]) <= set(KEYS) for t in tracks)
    for w_ in (0, 5):
        _same_tracks(va.tracks(window=w_, label_thr=0.0), cpu.tracks(window=w_, label_thr=0.0))
    assert len(va.tracks(label_thr=0.0)[0]["labels"]) == C
    # beyond the bounds the host answers and says so
    capsys.readouterr()
    beyond = va.tracks(max_gap=16)                                      # 8 * 17 = 136 active tracks
    assert va.tracks_path == "host" and "tracks on the host" in capsys.readouterr().err
    _same_tracks(beyond, cpu.tracks(max_gap=16))
    host = va.to_host()
    assert [hh["key"] for hh in host] == KEYS and [hh["count"] for hh in host] == want["count"].tolist()


def test_actors_on_a_single_label_model_raise(dev):
    cfg = load_cfg(os.path.join(ROOT, "configuration", "Tuber_CSN152_JHMDB.yaml"))
    cfg.CONFIG.DATA.IMG_SIZE = SIZE
    model, _, _ = build_model(cfg)
    model.eval()
    with pytest.raises(ValueError, match="actors"):
        Detector(cfg, model, actors=4)
    with pytest.raises(ValueError, match="actors"):
        VideoDetector(cfg, model, actors=4)
    assert VideoDetector(cfg, model, graphed=False).detector.actors is None
