"""Host side of the detection surface (tubelet_transformer_amd/detect.py), no GPU: ``decode_topk_host`` -- the definition -- against a
brute-force loop on both rules, the ``CONFIG.VAL.DETECT`` / ``GRAPHED`` defaults and their validator, the purity of the capture key, the
trimming of ``Detections.to_host`` and the three C-ABI entries of csrc/detect.hip in the header and the built library."""
import math
import os

import numpy as np
import pytest
import torch

from tubelet_transformer_amd import lib
from tubelet_transformer_amd.config import detect_settings, get_cfg_defaults
from tubelet_transformer_amd.detect import FIELDS, Detections, decode_topk_host, graph_key, host_parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _softmax(row):
    m = max(row)
    e = [math.exp(float(v) - float(m)) for v in row]
    return [v / sum(e) for v in e]


def _brute(logits, logits_b, boxes, sizes, mode, actor_thr, score_thr, K, q_begin, Qs):
    """the rules of detect.py's docstring as nested Python loops over python floats (fp64), candidates sorted by (-score, q, c)"""
    B, Qtot = logits.shape[0], logits.shape[1]
    res = []
    for b in range(B):
        q0 = 0 if q_begin is None else int(q_begin[b])
        cand = []
        if 0 <= q0 and q0 + Qs <= Qtot:
            for q in range(Qs):
                row = logits[b, q0 + q]
                lb = logits_b[b, q0 + q] if logits_b.ndim == 3 else logits_b[b]
                pb = _softmax(lb)[1]
                if mode == "ava":
                    if not pb > actor_thr:
                        continue
                    for c in range(len(row)):
                        x = float(row[c])
                        if x != x:
                            continue
                        s = (1.0 / (1.0 + math.exp(-x))) * pb
                        if s >= score_thr:
                            cand.append((-s, q, c, pb))
                else:
                    if any(float(v) != float(v) for v in row):
                        continue                                       # a NaN in the row: a NaN probability
                    lab = max(range(len(row)), key=lambda c: (float(row[c]), -c))        # the first maximum
                    s = _softmax(row)[lab]
                    if lab != len(row) - 1 and s >= score_thr:
                        cand.append((-s, q, lab, pb))
        cand.sort(key=lambda t: t[:3])
        rows = []
        for ns, q, c, pb in cand[:K]:
            cx, cy, w, h = (np.float32(v) for v in boxes[b, q0 + q])
            H, W = np.float32(sizes[b][0]), np.float32(sizes[b][1])
            half = np.float32(0.5)
            box = [(cx - half * w) * W, (cy - half * h) * H, (cx + half * w) * W, (cy + half * h) * H]
            rows.append((box, np.float32(-ns), c, q, np.float32(pb)))
        res.append((rows, len(cand)))
    return res


def _check(out, want, K):
    for b, (rows, total) in enumerate(want):
        n = len(rows)
        assert out["count"][b] == n and out["total"][b] == total
        for r, (box, s, c, q, pb) in enumerate(rows):
            assert out["labels"][b, r] == c and out["queries"][b, r] == q, (b, r)
            assert out["scores"][b, r] == s and out["aux"][b, r] == pb
            assert np.array_equal(out["boxes"][b, r], np.asarray(box, np.float32))
        assert (out["labels"][b, n:] == -1).all() and (out["queries"][b, n:] == -1).all()
        assert not out["boxes"][b, n:].any() and not out["scores"][b, n:].any() and not out["aux"][b, n:].any()
    assert out["boxes"].shape == (len(want), K, 4) and out["boxes"].dtype == np.float32
    assert out["labels"].dtype == np.int32 and out["count"].dtype == np.int32


@pytest.mark.parametrize("K", (5, 64))
def test_decode_topk_host_equals_a_brute_force_loop_ava(K):
    rng = np.random.default_rng(3)
    B, Qtot, Qs, C = 3, 12, 4, 7
    lg = rng.standard_normal((B, Qtot, C)).astype(np.float32) * 2
    lb = rng.standard_normal((B, Qtot, 3)).astype(np.float32) * 3
    lg[0, 5] = lg[0, 4]                                                # duplicated rows: equal scores, (q, c) order
    lb[0, 4] = lb[0, 5] = np.float32([0.0, 3.0, -1.0])                 # (gated: pb = 0.94)
    lg[1, 2, 3] = np.nan
    lb[2, :, 1] = -9.0                                                 # a clip with no gated query
    bx = rng.uniform(0.1, 0.9, (B, Qtot, 4)).astype(np.float32)
    sizes = np.array([[64, 96], [240, 320], [255, 341]])
    qb = np.array([4, 0, 8])
    out = decode_topk_host(lg, lb, bx, sizes, "ava", 0.5, 0.2, K, q_begin=qb, Qs=Qs)
    want = _brute(lg, lb, bx, sizes, "ava", 0.5, 0.2, K, qb, Qs)
    assert want[0][1] > 5 and want[2][1] == 0
    _check(out, want, K)
    full = decode_topk_host(lg, lb, bx, sizes, "ava", 0.5, 0.0, 200)
    _check(full, _brute(lg, lb, bx, sizes, "ava", 0.5, 0.0, 200, None, Qtot), 200)
    outside = decode_topk_host(lg, lb, bx, sizes, "ava", 0.5, 0.2, K, q_begin=np.array([9, -1, 0]), Qs=Qs)
    assert outside["count"].tolist()[:2] == [0, 0] and outside["count"][2] == 0        # slices outside the clip / the ungated clip


@pytest.mark.parametrize("per_clip", (True, False))
def test_decode_topk_host_equals_a_brute_force_loop_top1(per_clip):
    rng = np.random.default_rng(4)
    B, Qtot, Qs, C = 2, 20, 10, 5
    lg = rng.standard_normal((B, Qtot, C + 1)).astype(np.float32) * 2
    lg[0, 3, C] = 9.0                                                  # a no-object row
    lg[0, 4, 2] = np.nan
    lg[1, 12] = lg[1, 11]                                              # duplicated rows
    lg[1, 13, 1] = lg[1, 13, 3] = 5.0                                  # a duplicated maximum: the first one
    lb = rng.standard_normal((B, 2) if per_clip else (B, Qtot, 2)).astype(np.float32)
    bx = rng.uniform(0.1, 0.9, (B, Qtot, 4)).astype(np.float32)
    sizes = np.array([[64, 96], [240, 320]])
    qb = np.array([0, 10])
    for K, thr in ((4, 0.0), (32, 0.3)):
        out = decode_topk_host(lg, lb, bx, sizes, "jhmdb", 0.8, thr, K, q_begin=qb, Qs=Qs)
        _check(out, _brute(lg, lb, bx, sizes, "jhmdb", 0.8, thr, K, qb, Qs), K)
    assert 3 not in out["queries"][0] and 4 not in out["queries"][0]
    r = out["queries"][1].tolist().index(3)
    assert out["labels"][1, r] == 1


def test_detect_config_defaults_and_validator():
    cfg = get_cfg_defaults()
    V = cfg.CONFIG.VAL
    assert V.GRAPHED is False
    assert V.DETECT.to_dict() == {"SCORE_THR": 0.05, "TOPK": 100, "ACTOR_THR": 0.8}
    assert detect_settings(cfg) == {"score_thr": 0.05, "topk": 100, "actor_thr": 0.8, "graphed": False}
    for key, value in (("DETECT.SCORE_THR", "high"), ("DETECT.SCORE_THR", 1.5), ("DETECT.SCORE_THR", float("nan")), ("DETECT.TOPK", 0),
                       ("DETECT.TOPK", 2.5), ("DETECT.TOPK", True), ("DETECT.ACTOR_THR", 1.0), ("DETECT.ACTOR_THR", None), ("GRAPHED", 1)):
        c = get_cfg_defaults()
        node = c.CONFIG.VAL
        parts = key.split(".")
        for p in parts[:-1]:
            node = node[p]
        node[parts[-1]] = value
        with pytest.raises(ValueError, match=r"CONFIG\.VAL\.%s " % key.replace(".", r"\.")):
            detect_settings(c)


def test_graph_key_is_a_pure_function_of_its_arguments():
    a = graph_key(torch.Size([2, 3, 32, 64, 96]), (2, 64, 96), torch.float32, 11, 4096, False, ["b", "a"], "")
    b = graph_key([2, 3, 32, 64, 96], torch.Size([2, 64, 96]), torch.float32, 11, 4096, False, ("a", "b"), "")
    assert a == b and hash(a) == hash(b)
    base = dict(clip_shape=(2, 3, 32, 64, 96), mask_shape=(2, 64, 96), dtype=torch.float32, store_id=11, flat_ptr=4096, coop_off=False,
                switches=(), precision="")
    k0 = graph_key(**base)
    for name, other in (("clip_shape", (2, 3, 32, 48, 80)), ("mask_shape", (2, 48, 80)), ("dtype", torch.bfloat16), ("store_id", 12),
                        ("flat_ptr", 8192), ("coop_off", True), ("switches", ("no_decoder_coop",)), ("precision", "fp32_class")):
        assert graph_key(**dict(base, **{name: other})) != k0, name
    assert graph_key(**base) == k0


def test_detections_to_host_trims_to_count():
    B, K = 2, 4
    det = Detections(torch.arange(B * K * 4, dtype=torch.float32).view(B, K, 4), torch.tensor([[.9, .5, 0, 0], [0, 0, 0, 0.]]),
                     torch.tensor([[3, 1, -1, -1], [-1] * 4], dtype=torch.int32), torch.tensor([[0, 2, -1, -1], [-1] * 4], dtype=torch.int32),
                     torch.tensor([[.95, .85, 0, 0], [0, 0, 0, 0.]]), torch.tensor([2, 0], dtype=torch.int32), torch.tensor([7, 0], dtype=torch.int32))
    assert det.tensors()[0] is det.boxes and len(det.tensors()) == len(FIELDS)
    host = det.to_host()
    assert len(host) == B
    assert host[0]["count"] == 2 and host[0]["total"] == 7 and host[1]["count"] == 0 and host[1]["total"] == 0
    assert host[0]["boxes"].shape == (2, 4) and host[0]["labels"].tolist() == [3, 1] and host[0]["queries"].tolist() == [0, 2]
    assert np.array_equal(host[0]["scores"], np.float32([.9, .5])) and np.array_equal(host[0]["aux"], np.float32([.95, .85]))
    for k in ("boxes", "scores", "labels", "queries", "aux"):
        assert len(host[1][k]) == 0


def mixed_parts(device="cpu"):
    """[(numpy array, the tensor on ``device`` that holds it)]: fp32 [2, 3, 4] with a NaN and a negative zero, fp64 [5], int32 [2, 3], uint8 [7], a
    tensor of no elements and a non-contiguous view"""
    rng = np.random.default_rng(3)
    f32 = rng.standard_normal((2, 3, 4)).astype(np.float32)
    f32[0, 1, 2], f32[1, 0, 0] = np.nan, -0.0
    wide = rng.integers(-9, 9, (4, 6)).astype(np.int32)
    arrays = [f32, rng.standard_normal(5), rng.integers(-2 ** 31, 2 ** 31 - 1, (2, 3)).astype(np.int32), rng.integers(0, 256, 7).astype(np.uint8),
              np.zeros((0, 4), dtype=np.float32)]
    parts = [(a, torch.from_numpy(a.copy()).to(device)) for a in arrays]
    return parts + [(np.ascontiguousarray(wide.T[1:5:2]), torch.from_numpy(wide.copy()).to(device).t()[1:5:2])]


def assert_same_arrays(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == w.shape
        assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes()


def test_host_parts_keeps_dtype_shape_and_bits():
    parts = mixed_parts()
    assert [str(a.dtype) for a, _ in parts] == ["float32", "float64", "int32", "uint8", "float32", "int32"]
    assert parts[4][1].numel() == 0 and not parts[5][1].is_contiguous() and parts[5][1].shape == (2, 4)
    assert_same_arrays(host_parts([t for _, t in parts]), [a for a, _ in parts])
    assert host_parts([]) == []


def test_header_declares_and_library_exports_the_detect_entries():
    protos = {name: (ret, args) for ret, name, args in lib.header_prototypes()}
    for name in ("tuber_detect_ava", "tuber_detect_top1"):
        ret, args = protos[name]
        assert ret == "int" and args[-1] == ("hipStream_t", "stream")
        assert [a for _, a in args[-8:-1]] == ["det_box", "det_score", "det_label", "det_query", "det_aux", "det_count", "det_total"]
    assert protos["tuber_detect_limits"] == ("int", [("int", "which")])
    header = open(lib.HEADER).read()
    for cite in ("models/criterion.py:447-482", "models/tuber_jhmdb.py:357-389", "evaluates/evaluate_ucf.py:109-126"):
        assert cite in header
    L = lib.load()
    for name in ("tuber_detect_ava", "tuber_detect_top1", "tuber_detect_limits"):
        assert hasattr(L, name), name
    # the bounds are a host query
    assert [lib.query("tuber_detect_limits", w) for w in (0, 1, 2, 3)] == [4096, 1024, 8, -1]


@pytest.mark.parametrize("mode", ("ava", "jhmdb"))
def test_torch_restatement_of_the_definition_equals_it(mode):
    """the path of shapes beyond the kernel's bounds (detect._decode_topk_torch), here on the CPU: decisions exactly, fp64 probabilities"""
    from tubelet_transformer_amd.detect import _decode_topk_torch
    rng = np.random.default_rng(9)
    B, Qtot, Qs, C = 3, 12, 6, 9
    lg = (rng.standard_normal((B, Qtot, C if mode == "ava" else C + 1)) * 2).astype(np.float32)
    lb = (rng.standard_normal((B, Qtot, 3) if mode == "ava" else (B, 2)) * 2).astype(np.float32)
    lg[0, 7] = lg[0, 6]
    if mode == "ava":
        lb[0, 7] = lb[0, 6] = np.float32([0.0, 3.0, -1.0])
    lg[1, 1, 2] = np.nan
    bx = rng.uniform(0.1, 0.9, (B, Qtot, 4)).astype(np.float32)
    sizes = np.array([[64, 96], [240, 320], [255, 341]])
    qb = np.array([6, 0, 7])                                           # the last slice is outside the clip
    for K, thr in ((4, 0.1), (80, 0.0)):
        want = decode_topk_host(lg, lb, bx, sizes, mode, 0.5, thr, K, q_begin=qb, Qs=Qs)
        got = _decode_topk_torch(torch.from_numpy(lg), torch.from_numpy(lb), torch.from_numpy(bx), torch.from_numpy(sizes), mode, 0.5, thr, K,
                                 torch.from_numpy(qb).to(torch.int32), Qs)
        assert want["total"].max() > 4 and want["count"][2] == 0
        for k, t in zip(FIELDS, got):
            if k in ("scores", "aux"):
                assert np.abs(t.numpy().astype(np.float64) - want[k]).max() <= 2.0 ** -23, k
            else:
                assert np.array_equal(t.numpy(), want[k]), k
            assert t.numpy().dtype == want[k].dtype, k


def test_validation_loops_build_a_graphed_eval_only_when_asked_and_refuse_a_non_bool():
    from tubelet_transformer_amd.evaluation import _graphed_eval
    cfg = get_cfg_defaults()
    assert _graphed_eval(cfg, None) is None                            # the default: the loops run the plain forward
    cfg.CONFIG.VAL.GRAPHED = 0                                         # falsy, but not False
    with pytest.raises(ValueError, match=r"CONFIG\.VAL\.GRAPHED "):
        _graphed_eval(cfg, None)
