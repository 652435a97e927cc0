"""The detection surface on the GPU: ``tuber_detect_ava`` / ``tuber_detect_top1`` (csrc/detect.hip; bounds from ``tuber_detect_limits``) on
synthetic head outputs against ``detect.decode_topk_host`` -- the definition -- and against the boxes of ``PostProcessAVA.decode`` /
``PostProcess.decode``; then ``GraphedEval``, ``Detector`` and the two validation loops under ``CONFIG.VAL.GRAPHED`` on name-hashed models.

Fixtures.  Target scores lie on a lattice (one point per (q, c), shuffled), are converted to logits in fp64 and rounded to the input dtype;
actor probabilities are drawn from [0.85, 0.98] (gated) or [0.10, 0.65] (not gated), away from the gate at 0.8; ``score_thr`` sits half a
lattice step between two points.  Everything the comparison depends on is then recomputed in fp64 FROM THE ROUNDED INPUTS, and before any
launch ``_assert_separated`` checks that every pair of distinct candidate scores, every score against ``score_thr`` and every actor
probability against the gate differ by more than the score tolerance: under that condition decisions and order are determined, and must
equal the definition exactly.

Score tolerance: measured, not fixed.  ``_torch_error`` is the largest error of ``decode()`` -- the torch path -- against the fp64 formula
on the fixture at hand; the kernel's ``det_score`` / ``det_aux`` may err by at most twice that (the margin is for a different ``exp``),
with a floor of 2^-22.  Both figures are printed (run with -s)."""
import os
import types

import numpy as np
import pytest
import torch

from test_detect_cpu import assert_same_arrays, mixed_parts
from test_video_gpu import _count_syncs
from tubelet_transformer_amd import ab, lib, synth
from tubelet_transformer_amd.config import load_cfg
from tubelet_transformer_amd.criterion import PostProcess, PostProcessAVA
from tubelet_transformer_amd.detect import FIELDS, Detector, GraphedEval, decode_topk_host, empty_detections, host_parts
from tubelet_transformer_amd.misc import NestedTensor
from tubelet_transformer_amd.tuber import build_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 2.0 ** -22
GATE = 0.8                          # PostProcessAVA.decode's constant: the kernel-level tests use it as actor_thr
EBOUNDS = -2
SIZES = np.array([[64, 96], [240, 320], [255, 341]], dtype=np.int64)


def _round(a, dtype):
    """fp64 values rounded to ``dtype``, as fp32 numpy (bf16 values are fp32 values)"""
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).to(torch.float32).to(dtype).float().numpy()


def _softmax64(x):
    x = x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        e = np.exp(x - np.max(x, axis=-1, keepdims=True))
        return e / e.sum(-1, keepdims=True)


def _boxes(rng, B, Qtot, dtype):
    return _round(np.concatenate([rng.uniform(0.2, 0.8, (B, Qtot, 2)), rng.uniform(0.05, 0.4, (B, Qtot, 2))], axis=-1), dtype)


# ------------------------------------------------------------------------------------------------------------------------------
# fixtures from chosen scores
# ------------------------------------------------------------------------------------------------------------------------------
def ava_fixture(seed, Qtot, Qs, C, q_begin=None, dtype=torch.float32, B=3, empty_clip=True, nans=True, ties=False, thr0=False):
    """clip 0 generic; clip 1 (``nans``, Qs >= 4): a gated all-NaN row, a gated row with one NaN entry, a row with a NaN actor logit; the last clip
    (``empty_clip``): no gated query.  ``ties`` (clip 0): query 7 duplicates query 3, whose row holds the clip's best score once and its second
    best twice."""
    rng = np.random.default_rng(seed)
    n = Qtot * C
    lg, lb = np.empty((B, Qtot, C)), np.empty((B, Qtot, 3))
    qb = np.zeros(B, dtype=np.int64) if q_begin is None else np.asarray(q_begin, dtype=np.int64)
    for b in range(B):
        q0 = int(qb[b])
        gated = rng.random(Qtot) < 0.6
        if empty_clip and b == B - 1:
            gated[:] = False
        else:
            gated[q0 + rng.integers(Qs)] = True
        if nans and b == 1 and Qs >= 4:
            gated[q0:q0 + 2] = True
        if ties and b == 0:
            gated[[q0 + 3, q0 + 7]] = True
        u = (rng.permutation(Qtot) + 0.5) / Qtot
        pb = np.where(gated, 0.85 + 0.13 * u, 0.10 + 0.55 * u)
        lb[b, :, 0], lb[b, :, 2] = 0.0, -1.0
        lb[b, :, 1] = np.log(pb * (1.0 + np.exp(-1.0)) / (1.0 - pb))
        t = (0.02 + 0.68 * (rng.permutation(n) + 1.0) / (n + 1)).reshape(Qtot, C)
        if ties and b == 0:
            t[q0 + 3, [5, 9]] = 0.72
            t[q0 + 3, 11] = 0.75
        sg = np.where(gated[:, None], t / pb[:, None], t)              # sigmoid(logit) * pb = t for a gated query
        lg[b] = np.log(sg / (1.0 - sg))
    lg, lb = _round(lg, dtype), _round(lb, dtype)
    if ties:
        q0 = int(qb[0])
        lg[0, q0 + 7], lb[0, q0 + 7] = lg[0, q0 + 3], lb[0, q0 + 3]
    if nans and B > 1 and Qs >= 4:
        q0 = int(qb[1])
        lg[1, q0] = np.nan
        lg[1, q0 + 1, C // 2] = np.nan
        lb[1, q0 + 2, 1] = np.nan
    j0 = n // 2
    thr = 0.0 if thr0 else 0.02 + 0.68 * (j0 + 0.5) / (n + 1)
    return dict(mode="ava", lg=lg, lb=lb, bx=_boxes(rng, B, Qtot, dtype), sizes=SIZES[:B], qb=None if q_begin is None else qb.astype(np.int32), Qs=Qs,
                C=C, thr=thr, dtype=dtype, ties=ties)


def top1_fixture(seed, Qtot, Qs, C, q_begin=None, dtype=torch.float32, B=3, per_clip_b=True, ties=False, thr0=False):
    """every row: label a, probability p on a lattice in (0.55, 0.95), the other columns share 1 - p by random weights.  Clip 0: a no-object row;
    clip 1: a row with a NaN; the last clip: every row no-object.  ``ties`` (clip 0): query 5 duplicates query 4, the clip's best row."""
    rng = np.random.default_rng(seed)
    lg = np.empty((B, Qtot, C + 1))
    qb = np.zeros(B, dtype=np.int64) if q_begin is None else np.asarray(q_begin, dtype=np.int64)
    for b in range(B):
        q0 = int(qb[b])
        p = 0.55 + 0.40 * (rng.permutation(Qtot) + 1.0) / (Qtot + 1)
        if ties and b == 0:
            p[q0 + 4] = 0.97
        for q in range(Qtot):
            a = int(rng.integers(0, C))
            if (b == 0 and q == q0 + 2) or b == B - 1:
                a = C
            w = rng.dirichlet(np.ones(C))
            row = np.log((1.0 - p[q]) * w / p[q])
            lg[b, q] = np.insert(row, a, 0.0)
    lg = _round(lg, dtype)
    if ties:
        lg[0, int(qb[0]) + 5] = lg[0, int(qb[0]) + 4]
    if B > 1:
        lg[1, int(qb[1]) + 1, 3] = np.nan
    lb = _round(rng.standard_normal((B, 2) if per_clip_b else (B, Qtot, 2)) * 2, dtype)
    j0 = Qtot // 2
    thr = 0.0 if thr0 else 0.55 + 0.40 * (j0 + 0.5) / (Qtot + 1)
    return dict(mode="jhmdb", lg=lg, lb=lb, bx=_boxes(rng, B, Qtot, dtype), sizes=SIZES[:B], qb=None if q_begin is None else qb.astype(np.int32), Qs=Qs,
                C=C, thr=thr, dtype=dtype, ties=ties)


def exact64(fx):
    """(score [B, Qtot, C] or [B, Qtot], actor / visibility probability [B, Qtot] or [B], label [B, Qtot] or None) in fp64 from the inputs"""
    pb = _softmax64(fx["lb"])[..., 1]
    if fx["mode"] == "ava":
        with np.errstate(over="ignore"):
            return (1.0 / (1.0 + np.exp(-fx["lg"].astype(np.float64)))) * pb[:, :, None], pb, None
    lab = np.argmax(fx["lg"], axis=-1)
    return np.take_along_axis(_softmax64(fx["lg"]), lab[..., None], -1)[..., 0], pb, lab


def _assert_separated(fx, tol):
    """the condition of the fixture (module docstring), in fp64 on the CPU; with ``ties`` equal scores are allowed, near-equal ones are not"""
    s, pb, lab = exact64(fx)
    B, Qtot = fx["lg"].shape[:2]
    for b in range(B):
        q0 = 0 if fx["qb"] is None else int(fx["qb"][b])
        sl = slice(q0, q0 + fx["Qs"])
        if fx["mode"] == "ava":
            p = pb[b, sl]
            assert np.nanmin(np.abs(p - GATE)) > tol, "an actor probability within the tolerance of the gate"
            with np.errstate(invalid="ignore"):
                v = s[b, sl][p > GATE].reshape(-1)
        else:
            v = s[b, sl][lab[b, sl] != fx["C"]]
        v = np.sort(v[~np.isnan(v)])
        if len(v) == 0:
            continue
        assert np.abs(v - fx["thr"]).min() > tol, "a score within the tolerance of score_thr"
        d = np.diff(v)
        if fx["ties"]:
            d = d[d != 0.0]
        assert len(d) == 0 or d.min() > tol, "two distinct scores within the tolerance of each other"


def _dev(fx, dev):
    t = lambda a: torch.from_numpy(a).to(dev).to(fx["dtype"]).contiguous()
    return (t(fx["lg"]), t(fx["lb"]), t(fx["bx"]), torch.from_numpy(fx["sizes"]).to(dev),
            None if fx["qb"] is None else torch.from_numpy(fx["qb"]).to(dev))


def _torch_error(fx, dev):
    """(largest error of decode() -- the torch path -- against fp64 on this fixture, its boxes [B, Qtot, 4])"""
    lg, lb, bx, sizes, _ = _dev(fx, dev)
    s, pb, lab = exact64(fx)
    outputs = {"pred_logits": lg, "pred_logits_b": lb, "pred_boxes": bx}
    if fx["mode"] == "ava":
        prob, boxes, pbt = PostProcessAVA().decode(outputs, sizes)
        with np.errstate(invalid="ignore"):
            gated = pb > GATE
        e = np.abs(prob.double().cpu().numpy() - s)[gated]
    else:
        prob, boxes, pbt = PostProcess().decode(outputs, sizes)
        e = np.abs(np.take_along_axis(prob.double().cpu().numpy(), lab[..., None], -1)[..., 0] - s)
    eb = np.abs(pbt.double().cpu().numpy()[..., 0] - pb)
    err = max(float(np.nanmax(e)) if e.size else 0.0, float(np.nanmax(eb)))
    return err, boxes


def _launch(fx, K, dev, out=None):
    lg, lb, bx, sizes, qb = _dev(fx, dev)
    B, Qtot = lg.shape[:2]
    out = empty_detections(B, K, dev) if out is None else out
    dtypes = 7 if fx["dtype"] == torch.bfloat16 else 0
    name = "tuber_detect_ava" if fx["mode"] == "ava" else "tuber_detect_top1"
    code = lib.call_rc(name, lg, lb, bx, sizes.float(), qb, B, Qtot, fx["Qs"], fx["C"], lb.shape[-1], Qtot if lb.dim() == 3 else 1, dtypes, GATE, fx["thr"], K,
              *out.tensors())
    torch.cuda.synchronize()
    return code, out


def _check_kernel(fx, K, dev, label):
    """the whole comparison of one fixture at one K; returns the host result"""
    err, tboxes = _torch_error(fx, dev)
    tol = max(2.0 * err, FLOOR)
    _assert_separated(fx, tol)                                          # before the launch: a condition of the fixture, not a measurement
    code, out = _launch(fx, K, dev)
    assert code == 0
    want = decode_topk_host(fx["lg"], fx["lb"], fx["bx"], fx["sizes"], fx["mode"], GATE, fx["thr"], K, q_begin=fx["qb"], Qs=fx["Qs"])
    got = {k: t.cpu().numpy() for k, t in zip(FIELDS, out.tensors())}
    for k in ("count", "total", "labels", "queries"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["boxes"].view(np.int32), want["boxes"].view(np.int32))          # fp32 numpy, operation for operation
    s, pb, _ = exact64(fx)
    kerr = 0.0
    tb = tboxes.cpu().numpy()
    for b in range(len(want["count"])):
        n, q0 = int(want["count"][b]), 0 if fx["qb"] is None else int(fx["qb"][b])
        q, c = q0 + want["queries"][b, :n], want["labels"][b, :n]
        assert np.array_equal(got["boxes"][b, :n].view(np.int32), tb[b, q].view(np.int32)), "boxes differ from decode()'s"
        es = np.abs(got["scores"][b, :n].astype(np.float64) - (s[b, q, c] if fx["mode"] == "ava" else s[b, q]))
        ea = np.abs(got["aux"][b, :n].astype(np.float64) - (pb[b, q] if pb.ndim == 2 else pb[b]))
        kerr = max([kerr] + es.tolist() + ea.tolist())
        assert not got["boxes"][b, n:].any() and not got["scores"][b, n:].any() and not got["aux"][b, n:].any()
    print("%s K=%d: decode() max error %.3e, kernel max error %.3e, tolerance %.3e, candidates %s" % (label, K, err, kerr, tol, want["total"].tolist()))
    assert kerr <= tol
    return want


AVA_CASES = {
    "Q15_C80_K8": (dict(seed=1, Qtot=15, Qs=15, C=80), 8),
    "Q15_C80_K1024_thr0": (dict(seed=2, Qtot=15, Qs=15, C=80, thr0=True), 1024),
    "Q1_C1": (dict(seed=3, Qtot=1, Qs=1, C=1, empty_clip=True), 8),
    "Qs15_of_60": (dict(seed=4, Qtot=60, Qs=15, C=80, q_begin=[0, 15, 45]), 8),
    "C81": (dict(seed=5, Qtot=15, Qs=15, C=81), 100),
    "Q64_C64_4096_keys": (dict(seed=6, Qtot=64, Qs=64, C=64), 1024),
    "bf16_Q5_C12": (dict(seed=7, Qtot=5, Qs=5, C=12, dtype=torch.bfloat16), 8),
}


@pytest.mark.parametrize("case", sorted(AVA_CASES))
def test_detect_ava_equals_the_definition(dev, case):
    kw, K = AVA_CASES[case]
    fx = ava_fixture(**kw)
    want = _check_kernel(fx, K, dev, "ava " + case)
    assert want["total"][-1] == 0 and want["count"][-1] == 0            # the clip with no gated query
    if case == "Q15_C80_K8":
        assert want["total"][0] > K and want["count"][0] == K           # more than K candidates
    if case == "Q15_C80_K1024_thr0":
        assert 0 < want["total"][0] == want["count"][0] < K             # score_thr = 0: every (q, c) of a gated query
        nan_free = 80 * int(np.sum(_softmax64(fx["lb"])[1, :, 1] > GATE)) - 80 - 1
        assert want["total"][1] == nan_free                            # the NaN row and the NaN entry are no candidates, their neighbours are


TOP1_CASES = {
    "Q10_C21_sliced_K3": (dict(seed=11, Qtot=40, Qs=10, C=21, q_begin=[0, 10, 30]), 3),
    "Q10_C24_K16_thr0": (dict(seed=12, Qtot=10, Qs=10, C=24, per_clip_b=False, thr0=True), 16),
    "bf16_Q10_C21": (dict(seed=13, Qtot=10, Qs=10, C=21, dtype=torch.bfloat16), 16),
}


@pytest.mark.parametrize("case", sorted(TOP1_CASES))
def test_detect_top1_equals_the_definition(dev, case):
    kw, K = TOP1_CASES[case]
    fx = top1_fixture(**kw)
    want = _check_kernel(fx, K, dev, "top1 " + case)
    assert want["total"][-1] == 0                                       # every row no-object
    assert 2 not in want["queries"][0] and 1 not in want["queries"][1]  # the no-object row, the NaN row
    if case == "Q10_C21_sliced_K3":
        assert want["total"][0] > K
    if case == "Q10_C24_K16_thr0":
        assert want["total"].tolist() == [9, 9, 0]


def test_exact_ties_keep_query_then_class_order_and_k_cuts_by_it(dev):
    """duplicated logit rows of duplicated queries give bit-equal scores: (q, c) ascending, and K cuts inside the tie by that order"""
    fx = ava_fixture(seed=21, Qtot=15, Qs=15, C=80, ties=True)
    s, _, _ = exact64(fx)
    assert s[0, 3, 11] == s[0, 7, 11] and s[0, 3, 5] == s[0, 3, 9] == s[0, 7, 5] == s[0, 7, 9]          # equal in fp64 as well
    order = [(3, 11), (7, 11), (3, 5), (3, 9), (7, 5), (7, 9)]
    for K in (8, 1, 3, 5):
        want = _check_kernel(fx, K, dev, "ava ties")
        assert list(zip(want["queries"][0].tolist(), want["labels"][0].tolist()))[:6] == order[:K]
    _, out = _launch(fx, 8, dev)
    sc = out.scores[0].cpu().numpy().view(np.int32)
    assert sc[0] == sc[1] and sc[2] == sc[3] == sc[4] == sc[5] and sc[1] != sc[2]
    fx = top1_fixture(seed=22, Qtot=10, Qs=10, C=21, ties=True)
    for K in (4, 1):
        want = _check_kernel(fx, K, dev, "top1 ties")
        assert want["queries"][0].tolist()[:2] == [4, 5][:K]


def test_host_parts_is_one_copy_of_device_tensors(dev, monkeypatch):
    """the mixed list of tests/test_detect_cpu.py on the device: every array as the tensor's own ``.cpu().numpy()``, one ``.cpu()`` in all"""
    parts = [t for _, t in mixed_parts(dev)]
    assert all(t.is_cuda for t in parts) and not parts[5].is_contiguous()
    want = [t.cpu().numpy() for t in parts]
    got, syncs = _count_syncs(monkeypatch, lambda: host_parts(parts))
    assert syncs.count("cpu") == 1 and not {"item", "tolist", "synchronize"} & set(syncs), syncs
    assert_same_arrays(got, want)
    assert_same_arrays(got, [a for a, _ in mixed_parts()])


def test_beyond_the_bounds_nothing_is_launched_and_the_detector_answers_by_the_fallback(dev):
    assert [lib.query("tuber_detect_limits", w) for w in (0, 1, 2)] == [4096, 1024, 8]
    fx = ava_fixture(seed=31, Qtot=17, Qs=17, C=241)                    # Qs * C = 4097
    err, _ = _torch_error(fx, dev)
    tol = max(2.0 * err, FLOOR)
    _assert_separated(fx, tol)
    K = 16
    out = empty_detections(3, K, dev)
    for t in out.tensors():
        t.fill_(7)
    code, out = _launch(fx, K, dev, out)
    assert code == EBOUNDS
    assert all(bool((t == 7).all()) for t in out.tensors())            # untouched
    small = ava_fixture(seed=1, Qtot=15, Qs=15, C=80)
    code, out = _launch(small, 1025, dev, out=empty_detections(3, 1025, dev))
    assert code == EBOUNDS
    top = top1_fixture(seed=32, Qtot=2, Qs=2, C=2049)
    assert _launch(top, 4, dev)[0] == EBOUNDS
    # the Detector on such head outputs (a stand-in for the model: only the decode is exercised)
    cfg = load_cfg(os.path.join(ROOT, "configuration", "TubeR_CSN50_AVA21.yaml"))
    cfg.CONFIG.MODEL.QUERY_NUM = 17
    stub = types.SimpleNamespace(dataset_mode="ava", training=False, query_embed=types.SimpleNamespace(num_embeddings=17))
    det = Detector(cfg, stub, score_thr=fx["thr"], topk=K, actor_thr=GATE, graphed=False)
    lg, lb, bx, sizes, _ = _dev(fx, dev)
    outputs = {"pred_logits": lg, "pred_logits_b": lb, "pred_boxes": bx}
    statics = det.statics(outputs)
    statics["sizes"].copy_(sizes)
    got = det.launch(outputs, statics)
    want = decode_topk_host(fx["lg"], fx["lb"], fx["bx"], fx["sizes"], "ava", GATE, fx["thr"], K)
    assert want["total"][0] > K
    for k in ("count", "total", "labels", "queries", "boxes"):
        assert np.array_equal(getattr(got, k).cpu().numpy(), want[k]), k
    for k in ("scores", "aux"):
        assert np.abs(getattr(got, k).cpu().numpy().astype(np.float64) - want[k]).max() <= tol


# ------------------------------------------------------------------------------------------------------------------------------
# model level
# ------------------------------------------------------------------------------------------------------------------------------
def _model(name):
    dev = torch.device("cuda:0")
    cfg = load_cfg(os.path.join(ROOT, "configuration", name))
    model, crit, post = build_model(cfg)
    synth.load_name_hashed(model)
    model.to(dev).eval()
    crit.to(dev)
    return cfg, model, crit, post


@pytest.fixture(scope="module")
def ava_model():
    return _model("TubeR_CSN50_AVA21.yaml")


@pytest.fixture(scope="module")
def jhmdb_model():
    return _model("Tuber_CSN152_JHMDB.yaml")


def _flat(out):
    """every tensor of a forward's output dict, by name"""
    flat = {k: v for k, v in out.items() if torch.is_tensor(v)}
    for i, t in enumerate(out["_stacked"]):
        flat["_stacked.%d" % i] = t
    for i, layer in enumerate(out.get("aux_outputs", [])):
        for k, v in layer.items():
            flat["aux_outputs.%d.%s" % (i, k)] = v
    return flat


def _eager(model, samples):
    with torch.no_grad():
        return {k: v.clone() for k, v in _flat(model(samples)).items()}


def _assert_same(out, want):
    got = _flat(out)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k


def _count_launches(fn):
    seen = []
    lib.set_launch_hook(lambda name, args, launch: (seen.append(name), launch(name, *args))[1])
    try:
        res = fn()
    finally:
        lib.set_launch_hook(None)
    return res, seen


def _other_shape(dev):
    clips = synth.synthetic_clips(2, 32, 48, 80, seed=12, device=dev)
    mask = torch.zeros(2, 48, 80, dtype=torch.bool, device=dev)
    mask[1, :, 64:] = True                                             # the second clip is 64 wide, padded to 80
    clips[1, :, :, :, 64:] = 0
    return NestedTensor(clips, mask)


@pytest.mark.parametrize("which", ("ava", "jhmdb"))
def test_graphed_eval_equals_the_eager_forward(dev, which, request):
    cfg, model, _, _ = request.getfixturevalue(which + "_model")
    a = synth.synthetic_clips(2, 32, 64, 96, seed=10, device=dev)
    b = synth.synthetic_clips(2, 32, 64, 96, seed=11, device=dev)
    want_a, want_b = _eager(model, a), _eager(model, b)
    assert ("aux_outputs.0.pred_logits" in want_a) == bool(model.aux_loss) and "_stacked.2" in want_a
    ge = GraphedEval(model)
    _assert_same(ge(a), want_a)
    assert (ge.captures, ge.eager_calls) == (1, 0)
    out, seen = _count_launches(lambda: ge(b))                          # the same shape: a replay, no library launch outside it
    assert seen == [] and (ge.captures, ge.eager_calls) == (1, 0)
    _assert_same(out, want_b)
    other = _other_shape(dev)
    want_o = _eager(model, other)
    _assert_same(ge(other), want_o)                                     # another shape, with its mask: its own capture
    assert (ge.captures, ge.eager_calls) == (2, 0)
    _assert_same(ge(a), want_a)
    assert ge.captures == 2
    one = GraphedEval(model, max_shapes=1)
    _assert_same(one(a), want_a)
    out, seen = _count_launches(lambda: one(other))                     # max_shapes reached: eager, and still equal
    assert len(seen) > 10 and (one.captures, one.eager_calls) == (1, 1)
    _assert_same(out, want_o)
    model.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            ge(a)
    finally:
        model.eval()


def test_a_replay_follows_in_place_weight_changes_without_a_recapture(dev, ava_model):
    cfg, model, _, _ = ava_model
    a = synth.synthetic_clips(2, 32, 64, 96, seed=10, device=dev)
    ge = GraphedEval(model)
    before = _eager(model, a)
    _assert_same(ge(a), before)
    saved = model.class_fc.weight.data.clone()
    try:
        model.class_fc.weight.data.add_(0.01)                           # a view of store.flat: the address stays
        after = _eager(model, a)
        assert not torch.equal(after["pred_logits"], before["pred_logits"])
        _assert_same(ge(a), after)
        assert ge.captures == 1
    finally:
        model.class_fc.weight.data.copy_(saved)


def test_coop_off_is_part_of_the_key(dev, ava_model):
    """under the bf16-stream eval form the decoder is the cooperative launch; with ``coop_off`` set by hand (nothing is starved or timed out) the
    key changes and the new capture equals the eager launch chain"""
    cfg, model, _, _ = ava_model
    a = synth.synthetic_clips(2, 32, 64, 96, seed=10, device=dev)
    store = model.engine()[0]
    assert not store.coop_off
    with ab.override("eval_bf16_stream"):
        ge = GraphedEval(model)
        want, seen = _count_launches(lambda: _eager(model, a))
        assert "tuber_decoder_coop_fwd" in seen
        _assert_same(ge(a), want)
        k0 = ge.key_of(NestedTensor(a, torch.zeros(2, 64, 96, dtype=torch.bool, device=dev)))
        try:
            store.coop_off = True
            assert ge.key_of(NestedTensor(a, torch.zeros(2, 64, 96, dtype=torch.bool, device=dev))) != k0
            chain, seen = _count_launches(lambda: _eager(model, a))
            assert "tuber_decoder_coop_fwd" not in seen
            _assert_same(ge(a), chain)
            assert ge.captures == 2
        finally:
            store.coop_off = False
        assert not store.coop_failed()


# The name-hashed weights are no detector.  At 2 x 32 x 64 x 96 (seed 10) the AVA model's actor probabilities are 0.1245 ... 0.1260: the gate at
# 0.8 passes 0 of the 2 x 15 queries (printed), so the gate is set inside that range (it passes some queries of each clip and not others) and
# score_thr under the best scores (about 0.111).  The JHMDB model puts no-object (probability about 0.12, the classes about 0.04 each) on top of all
# 2 x 320 rows: 0 candidates; the test lowers the no-object bias of class_fc by 2 for its duration, so that every row is a candidate of some class.
# (topk = 4 there: with these weights the sixth and seventh best scores of a key frame lie 1.3e-7 apart, inside the tolerance, so a cut below them would
# not be decided; _assert_model_outputs_decided checks the condition on the CPU for whatever is chosen here.)
DETECT_SETTINGS = {"ava": dict(actor_thr=0.1252, score_thr=0.10, topk=16), "jhmdb": dict(actor_thr=0.8, score_thr=0.0, topk=4)}


def _assert_model_outputs_decided(fx, s64, pb64, want, qb, Q, kw, tol):
    """the fixture condition for a model's outputs: every decision the compared result depends on is separated by more than the tolerance --
    every actor probability from the gate, every gated score from score_thr, and the kept scores plus the first one cut from each other
    (pairs that are both cut, or both under score_thr, decide nothing that is compared)"""
    for b in range(len(want["count"])):
        q0 = 0 if qb is None else qb[b]
        sl = slice(q0, q0 + (Q if qb is not None else s64.shape[1]))
        if fx["mode"] == "ava":
            p = pb64[b, sl]
            assert np.abs(p - kw["actor_thr"]).min() > tol, "an actor probability within the tolerance of the gate"
            v = s64[b, sl][p > kw["actor_thr"]].reshape(-1)
        else:
            lab = np.argmax(fx["lg"][b, sl], axis=-1)
            v = s64[b, sl][lab != fx["C"]]
        assert not np.isnan(v).any()
        assert np.abs(v - kw["score_thr"]).min() > tol, "a score within the tolerance of score_thr"
        top = np.sort(v[v >= kw["score_thr"]])[::-1][:kw["topk"] + 1]
        assert len(top) < 2 or (-np.diff(top)).min() > tol, "two of the kept scores (or the first one cut) within the tolerance of each other"


@pytest.mark.parametrize("which", ("ava", "jhmdb"))
def test_detector_graphed_eager_and_definition_agree(dev, which, request):
    cfg, model, _, _ = request.getfixturevalue(which + "_model")
    model.engine()
    bias = model.class_fc.bias.data
    saved = bias.clone()
    if which == "jhmdb":
        bias[-1] -= 2.0
    try:
        _detector_agreement(dev, which, cfg, model)
    finally:
        bias.copy_(saved)


def _detector_agreement(dev, which, cfg, model):
    a = synth.synthetic_clips(2, 32, 64, 96, seed=10, device=dev)
    sizes = [[64, 96], [60, 90]]
    key_pos = None if which == "ava" else [3, 16]
    Q = cfg.CONFIG.MODEL.QUERY_NUM
    kw = DETECT_SETTINGS[which]
    with torch.no_grad():
        out = model(a)
        lg, lb, bx = (out[k].float().cpu().numpy() for k in ("pred_logits", "pred_logits_b", "pred_boxes"))
        err_fx = dict(mode=model.dataset_mode, lg=lg, lb=lb, bx=bx, sizes=np.asarray(sizes), dtype=torch.float32, C=lg.shape[2] - (which != "ava"), qb=None)
        err, tboxes = _torch_error(err_fx, dev)
    tol = max(2.0 * err, FLOOR)
    qb = None if key_pos is None else [k * Q for k in key_pos]
    want = decode_topk_host(lg, lb, bx, sizes, model.dataset_mode, kw["actor_thr"], kw["score_thr"], kw["topk"], q_begin=qb, Qs=Q if qb else None)
    s64, pb64, _ = exact64(err_fx)
    _assert_model_outputs_decided(err_fx, s64, pb64, want, qb, Q, kw, tol)          # on the CPU, before any Detector runs
    if which == "ava":
        pb = _softmax64(lb)[..., 1]
        print("ava: queries per clip with an actor probability above 0.8: %s, above %g: %s" % ((pb > 0.8).sum(1).tolist(), kw["actor_thr"],
                                                                                                (pb > kw["actor_thr"]).sum(1).tolist()))
    print("%s: candidates per clip %s, kept %s (decode() error %.3e)" % (which, want["total"].tolist(), want["count"].tolist(), err))
    assert (want["count"] >= 1).all()
    results = {}
    for graphed in (True, False):
        det = Detector(cfg, model, graphed=graphed, **kw)
        for _ in range(2):                                              # the second call of the graphed detector is a pure replay
            d, seen = _count_launches(lambda: det(a, sizes, key_pos))
        assert det.eval.captures == (1 if graphed else 0)
        assert (seen == []) if graphed else (seen[-1] in ("tuber_detect_ava", "tuber_detect_top1") and seen.count(seen[-1]) == 1)
        results[graphed] = {k: t.clone() for k, t in zip(FIELDS, d.tensors())}
        host = d.to_host()
        assert [h["count"] for h in host] == want["count"].tolist()
        assert all(len(h["scores"]) == h["count"] for h in host)
    for k in FIELDS:
        assert torch.equal(results[True][k], results[False][k]), k        # the same kernel on bit-identical forwards
    got = {k: v.cpu().numpy() for k, v in results[True].items()}
    for k in ("count", "total", "labels", "queries", "boxes"):
        assert np.array_equal(got[k], want[k]), k
    kerr = 0.0                                                          # against fp64, as in the kernel-level tests
    for b in range(2):
        n, q0 = int(want["count"][b]), 0 if qb is None else qb[b]
        q, c = q0 + want["queries"][b, :n], want["labels"][b, :n]
        es = np.abs(got["scores"][b, :n].astype(np.float64) - (s64[b, q, c] if which == "ava" else s64[b, q]))
        ea = np.abs(got["aux"][b, :n].astype(np.float64) - (pb64[b, q] if pb64.ndim == 2 else pb64[b]))
        kerr = max([kerr] + es.tolist() + ea.tolist())
    print("%s: kernel max error %.3e, tolerance %.3e" % (which, kerr, tol))
    assert kerr <= tol
    if which == "jhmdb":
        with pytest.raises(ValueError, match="key_pos"):
            Detector(cfg, model, graphed=False)(a, sizes)


def _ava_loader(H=64, W=96):
    """the two-batch loader of test_model_gpu.test_eval_loop_writes_reference_format_and_scores"""
    loader = []
    gen = torch.Generator().manual_seed(5)
    for i in range(2):
        clips = synth.synthetic_clips(2, 32, H, W, seed=10 + i)
        tg = synth.synthetic_targets(2, "ava", 80, seed=20 + i, device="cpu", hw=(H, W))
        for b, t in enumerate(tg):
            n = t["boxes"].shape[0]
            t["image_id"] = ["vid%d_%04d" % (i, 900 + b), 16]
            t["size"] = torch.tensor([H, W])
            raw = torch.zeros(n, 6)
            raw[:, 0] = b
            raw[:, 1] = 16
            raw[:, 2:] = torch.rand(n, 4, generator=gen).sort(dim=1).values * torch.tensor([W, H, W, H]) / 2 + torch.tensor([0, 0, W / 2, H / 2])
            t["raw_boxes"] = raw
        loader.append((clips, tg))
    return loader


def _same_number(a, b):
    return a == b or (a != a and b != b)


@pytest.mark.parametrize("which", ("ava", "jhmdb"))
def test_validation_loops_are_unchanged_by_graphed(dev, which, request, tmp_path, monkeypatch):
    """mAP and result files of both loops with GRAPHED on and off, with and without the device evaluator; the GRAPHED run builds one
    GraphedEval, captures the first batch and replays the second, the default builds none"""
    import tubelet_transformer_amd.detect as detect_mod
    from test_device_map_ucf_gpu import _loader as _ucf_loader
    built = []

    class Recording(GraphedEval):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            self.calls = 0
            built.append(self)

        def run(self, samples, feed=None):
            self.calls += 1
            return super().run(samples, feed)
    monkeypatch.setattr(detect_mod, "GraphedEval", Recording)
    from tubelet_transformer_amd.evaluation import validate_tuber_detection, validate_tuber_ucf_detection
    cfg, model, crit, post = request.getfixturevalue(which + "_model")
    C = cfg.CONFIG
    if which == "ava":
        loader, loop = _ava_loader(), validate_tuber_detection
    else:
        loader, loop = _ucf_loader(C.DATA.NUM_CLASSES), validate_tuber_ucf_detection
    runs = {}
    try:
        for device_map in (False, True):
            for graphed in (False, True):
                name = "res_%d_%d" % (device_map, graphed)
                C.LOG.BASE_PATH, C.LOG.RES_DIR = str(tmp_path), name
                C.VAL.GRAPHED, C.VAL.DEVICE_MAP.ENABLE = graphed, device_map
                batches = [(c, [dict(t) for t in tg]) for c, tg in loader]
                del built[:]
                _, seen = _count_launches(lambda: runs.__setitem__("mAP", loop(cfg, model, crit, post, batches, epoch=0, verbose=False)))
                mAP = runs.pop("mAP")
                if graphed:                                             # two batches of one shape: a capture, then a replay
                    assert len(built) == 1 and (built[0].calls, built[0].captures, built[0].eager_calls) == (2, 1, 0)
                else:
                    assert built == []
                assert "tuber_cast_f32_bf16" in seen                    # (the forward's refresh: the hook saw the loop)
                d = os.path.join(str(tmp_path), name)
                runs[device_map, graphed] = (mAP, {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))})
    finally:
        C.VAL.GRAPHED, C.VAL.DEVICE_MAP.ENABLE = False, False
        model.eval()
    for device_map in (False, True):
        (m0, f0), (m1, f1) = runs[device_map, False], runs[device_map, True]
        print("%s DEVICE_MAP %s: mAP %.17g eager, %.17g graphed; files %s" % (which, device_map, m0, m1, sorted(f0)))
        assert _same_number(m0, m1)
        assert len(f0) >= 2 and all(len(v) > 0 for v in f0.values()) and f0 == f1          # byte-identical result files
