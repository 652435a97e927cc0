"""Dense action tubes on the device: ``tuber_tube_dense`` called directly and held, byte for byte, to
``evaluation.dense_rows`` on the same record -- every output buffer pre-filled with sentinel bytes, so that an entry behind a row's span
that the kernel touched shows -- then ``tubes(dense=True)`` / ``tracks(dense=True)`` on device stores against their CPU copies, and the
stream against the whole video.  No tolerance appears anywhere: fp32 data is compared as int32."""
import numpy as np
import pytest
import torch

from test_tube_dense_cpu import ADDED, PLANTED_KEYS, TRACK_KEYS, TUBE_KEYS, cpu_actors, cpu_detections, planted_dense, same_bits, same_dense, seeded
from test_tube_nms_cpu import padded_actors, padded_detections
from tubelet_transformer_amd import lib
from tubelet_transformer_amd.evaluation import dense_extent, dense_rows

pytestmark = pytest.mark.gpu
BOX_FILL, INT_FILL = 0xAA, 0x7F
INT_SENTINEL = 0x7F7F7F7F


# ------------------------------------------------------------------------------------------------------------------------------
# the kernel's operands and its sentinel-filled outputs
# ------------------------------------------------------------------------------------------------------------------------------
def filled(dev, byte, dtype, *shape):
    n = int(np.prod(shape)) * 4
    return torch.full((max(n, 16),), byte, dtype=torch.uint8, device=dev)[:n].view(dtype).view(*shape)


def operands(box, score, head, keys, K, dev):
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(dev)
    return dict(det_box=up(np.asarray(box).reshape(-1, 4), np.float32), det_score=up(score, np.float32), row_head=up(head, np.int32), slot_frame=up(keys, np.int32),
                S=len(keys), K=K)


def outputs(N, G, dev):
    return dict(dense_box=filled(dev, BOX_FILL, torch.float32, N, G, 4), dense_score=filled(dev, BOX_FILL, torch.float32, N, G),
                row_span=filled(dev, INT_FILL, torch.int32, N), row_next=filled(dev, INT_FILL, torch.int32, N))


def args_of(o, out, max_gap, G, over=()):
    a = dict(o, **out, max_gap=max_gap, G=G)
    a.update(dict(over))
    return (a["det_box"], a["det_score"], a["row_head"], a["slot_frame"], a["S"], a["K"], a["max_gap"], a["G"], a["dense_box"], a["dense_score"], a["row_span"],
            a["row_next"])


def untouched(out):
    return all(bool((t.contiguous().view(torch.uint8) == byte).all()) for t, byte in ((out["dense_box"], BOX_FILL), (out["dense_score"], BOX_FILL),
                                                                                         (out["row_span"], INT_FILL), (out["row_next"], INT_FILL)))


def device_dense(box, score, head, keys, K, max_gap, G, dev):
    o = operands(box, score, head, keys, K, dev)
    out = outputs(len(keys) * K, G, dev)
    lib.call("tuber_tube_dense", *args_of(o, out, max_gap, G))
    return {k: v.cpu().numpy() for k, v in out.items()}


def definition(box, score, head, keys, K, max_gap, G):
    """``dense_rows`` over buffers pre-filled as the device's are: what the kernel must leave, byte for byte -- but for ``row_next`` at a row
    that took the escape, which the kernel does not write"""
    N = len(keys) * K
    fill = lambda *shape: np.full(int(np.prod(shape)) * 4, BOX_FILL, dtype=np.uint8).view(np.float32).reshape(*shape)
    return dense_rows(box, score, head, keys, K, max_gap, G=G, dense_box=fill(N, G, 4), dense_score=fill(N, G))


def assert_equals_the_definition(got, want):
    span = want["row_span"]
    assert np.array_equal(got["row_span"], span), np.argwhere(got["row_span"] != span)[:10].ravel()
    escaped = span == -1
    assert np.array_equal(got["row_next"][~escaped], want["row_next"][~escaped]) and (got["row_next"][escaped] == INT_SENTINEL).all()
    same_bits(got["dense_box"], want["dense_box"])                          # the frames a row owns AND the sentinels behind them
    same_bits(got["dense_score"], want["dense_score"])
    for r in np.nonzero(span < got["dense_score"].shape[1])[0].tolist():    # said once more, in so many words: nothing behind the span
        assert (got["dense_score"][r, max(span[r], 0):].view(np.uint8) == BOX_FILL).all() and (got["dense_box"][r, max(span[r], 0):].view(np.uint8) == BOX_FILL).all(), r


def chains(seed, S, K, max_gap):
    """a random record of the linker's shape: per slot every tube still within max_gap + 1 slots of its last row goes on with probability 0.6
    at a free position, every position left starts a tube with probability 0.4 -> (box, score, row_head, keys in steps of 1..3)"""
    rng = np.random.default_rng(seed)
    head = np.full((S, K), -1, dtype=np.int64)
    live = []                                                             # [head, last slot]
    for s in range(S):
        free = rng.permutation(K).tolist()
        for t in [t for t in live if s - t[1] <= max_gap + 1]:
            if free and rng.random() < 0.6:
                head[s, free.pop()] = t[0]
                t[1] = s
        for q in free:
            if rng.random() < 0.4:
                head[s, q] = s * K + q
                live.append([s * K + q, s])
    xy = rng.uniform(0, 500, (S * K, 2))
    box = np.concatenate([xy, xy + rng.uniform(5, 200, (S * K, 2))], axis=1).astype(np.float32)
    return box, rng.uniform(0, 1, S * K).astype(np.float32), head.reshape(-1), np.cumsum(rng.integers(1, 4, S)).tolist()


# ------------------------------------------------------------------------------------------------------------------------------
# the kernel against the definition
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_planted_record(dev):
    box, score, head, tubes = planted_dense()
    G = dense_extent(PLANTED_KEYS, 2)
    assert G == 136 > 128                                                  # a wave goes three times round its loop for the 130-frame step
    want = definition(box, score, head, PLANTED_KEYS, 3, 2, G)
    got = device_dense(box, score, head, PLANTED_KEYS, 3, 2, G, dev)
    assert_equals_the_definition(got, want)
    assert got["row_span"].tolist() == [1, 7, 0, 5, 0, 5, 1, 0, 1, 130, 130, 130, 1, 1, 1, 1, 0, 1]
    assert got["row_next"].tolist() == [3, 10, -1, 6, -1, 8, 9, -1, -1, 12, 13, 14, 15, -1, 17, -1, -1, -1]
    again = device_dense(box, score, head, PLANTED_KEYS, 3, 2, G, dev)    # the same bytes again
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k
    roomy = device_dense(box, score, head, PLANTED_KEYS, 3, 2, G + 61, dev)                # a G larger than needed changes the stride, nothing else
    assert_equals_the_definition(roomy, definition(box, score, head, PLANTED_KEYS, 3, 2, G + 61))
    same_bits(roomy["dense_box"][:, :G], got["dense_box"])


@pytest.mark.parametrize("S,K,max_gap", [(7, 16, 3), (5, 64, 0), (70, 1, 63), (1, 5, 2), (9, 3, 0)])
def test_the_bound_shapes(dev, S, K, max_gap):
    assert K <= lib.query("tuber_frame_match_max_dets") and K * (max_gap + 1) <= lib.query("tuber_tube_link_max_active")
    box, score, head, keys = chains(S * 100 + K, S, K, max_gap)
    G = dense_extent(keys, max_gap)
    want = definition(box, score, head, keys, K, max_gap, G)
    assert (want["row_span"] == 0).any() or K == 1
    if S > 1:
        assert (want["row_span"] > 1).any() and (want["row_next"] >= 0).sum() >= 2
    if (K, max_gap) == (1, 63):
        assert (want["row_next"] - np.arange(S) > 8).any()                # a successor far down the lanes of the ballot
    assert_equals_the_definition(device_dense(box, score, head, keys, K, max_gap, G, dev), want)


@pytest.mark.parametrize("seed", range(1, 9))
def test_seeded_records_linked_by_link_rows(dev, seed):
    fx = seeded(seed)
    assert (fx["S"], fx["K"]) == (12, 5) and 1 <= min(np.diff(fx["keys"])) and max(np.diff(fx["keys"])) <= 9
    G = dense_extent(fx["keys"], fx["max_gap"])
    want = definition(fx["box"], fx["score"], fx["link"]["row_head"], fx["keys"], fx["K"], fx["max_gap"], G)
    assert_equals_the_definition(device_dense(fx["box"], fx["score"], fx["link"]["row_head"], fx["keys"], fx["K"], fx["max_gap"], G, dev), want)


def test_a_G_one_too_small_is_the_escape(dev):
    box, score, head, _ = planted_dense()
    full = dense_rows(box, score, head, PLANTED_KEYS, 3, 2)
    G = int(full["row_span"].max()) - 1
    want = definition(box, score, head, PLANTED_KEYS, 3, 2, G)
    got = device_dense(box, score, head, PLANTED_KEYS, 3, 2, G, dev)
    assert np.nonzero(got["row_span"] == -1)[0].tolist() == np.nonzero(full["row_span"] > G)[0].tolist() == [9, 10, 11]
    assert_equals_the_definition(got, want)                                # the escaped rows all sentinel, every other row as before
    assert (got["dense_box"][[9, 10, 11]].view(np.uint8) == BOX_FILL).all() and (got["dense_score"][[9, 10, 11]].view(np.uint8) == BOX_FILL).all()
    rest = np.setdiff1d(np.arange(18), [9, 10, 11])
    for r in rest.tolist():
        same_bits(got["dense_box"][r, :full["row_span"][r]], full["dense_box"][r, :full["row_span"][r]])
    # keys that do not ascend: a span below 1 takes the same way out
    keys = [3, 4, 9, 9, 140, 141]
    got = device_dense(box, score, head, keys, 3, 2, 200, dev)
    assert got["row_span"][[6, 8]].tolist() == [-1, 1] and got["row_span"][[0, 1]].tolist() == [1, 6] and (got["dense_box"][6].view(np.uint8) == BOX_FILL).all()


def test_refusals_write_nothing(dev):
    box, score, head, _ = planted_dense()
    o = operands(box, score, head, PLANTED_KEYS, 3, dev)
    G = 136
    out = outputs(18, G, dev)
    shifted = outputs(19, G, dev)                                          # the same buffers one fp32 further on: valid addresses, 4-byte aligned only
    wide = dict(K=65), dict(K=16, max_gap=4), dict(K=1, max_gap=64), dict(K=64, max_gap=1)
    sizes = dict(G=0), dict(G=-1), dict(S=-1), dict(K=0), dict(K=-3), dict(max_gap=-1), dict(S=1 << 30, K=2, G=1), dict(S=1 << 20, K=64, G=1 << 10)
    null = tuple({k: None} for k in ("det_box", "det_score", "row_head", "slot_frame", "dense_box", "dense_score", "row_span", "row_next"))
    odd = dict(dense_box=shifted["dense_box"].view(-1)[1:1 + 18 * G * 4]), dict(det_box=o["det_box"].view(-1)[1:]), dict(det_score=o["det_score"].view(torch.uint8)[1:])
    for over in wide + sizes + null + odd:
        code = lib.call_rc("tuber_tube_dense", *args_of(o, out, 2, G, over))
        assert code < 0, (over, code)
    torch.cuda.synchronize()
    assert untouched(out) and untouched(shifted)
    assert lib.call_rc("tuber_tube_dense", *args_of(o, out, 2, G, dict(S=0))) == 0 and lib.call_rc("tuber_tube_dense", *args_of(o, out, 2, G, dict(S=0, det_box=None))) == 0
    torch.cuda.synchronize()
    assert untouched(out)
    assert lib.call_rc("tuber_tube_dense", *args_of(o, out, 2, G)) == 0     # and the call itself is fine
    assert_equals_the_definition({k: v.cpu().numpy() for k, v in out.items()}, definition(box, score, head, PLANTED_KEYS, 3, 2, G))


# ------------------------------------------------------------------------------------------------------------------------------
# tubes(dense=True) / tracks(dense=True) on a device store
# ------------------------------------------------------------------------------------------------------------------------------
def assert_same_output(got, want, key_set):
    assert len(got) == len(want) >= 2
    for g, w in zip(got, want):
        assert set(g) == set(w) == key_set
        for k in key_set:
            a, b = g[k], w[k]
            if isinstance(b, np.ndarray):
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
            elif isinstance(b, float):
                assert np.float64(a).tobytes() == np.float64(b).tobytes(), k
            else:
                assert a == b, k


def hooked(fn):
    seen = []
    lib.set_launch_hook(lambda name, args, launch: (seen.append(name), launch(name, *args))[1])
    try:
        return fn(), seen
    finally:
        lib.set_launch_hook(None)


@pytest.mark.parametrize("store", ("padded", "seeded"))
def test_dense_tubes_and_tracks_on_a_device_store(dev, store, capsys):
    fx = seeded(4)
    make_d = (lambda d, **kw: padded_detections(d, **kw)) if store == "padded" else (lambda d, **kw: cpu_detections(fx, dev=d, **kw))
    make_a = (lambda d, **kw: padded_actors(d, **kw)) if store == "padded" else (lambda d, **kw: cpu_actors(fx, dev=d, **kw))
    vd, cpu = make_d(dev), make_d("cpu")
    plain, seen = hooked(lambda: vd.tubes())
    assert seen == ["tuber_tube_link_ranked"] and [set(t) for t in plain] == [TUBE_KEYS] * len(plain)     # without the option: what was launched before
    off, seen = hooked(lambda: vd.tubes(dense=False))
    assert seen == ["tuber_tube_link_ranked"]
    assert_same_output(off, plain, TUBE_KEYS)
    got, seen = hooked(lambda: vd.tubes(dense=True))
    assert seen == ["tuber_tube_link_ranked", "tuber_tube_dense"] and vd.tubes_path == "device"
    want = cpu.tubes(dense=True)
    assert cpu.tubes_path == "host"
    assert_same_output(got, want, TUBE_KEYS | ADDED)
    assert [t["keys"] for t in got] == [t["frames"] for t in plain] and all(len(t["frames"]) == t["keys"][-1] - t["keys"][0] + 1 for t in got)
    got, seen = hooked(lambda: vd.tubes(nms=0.3, dense=True))
    assert seen == ["tuber_tube_link_ranked", "tuber_tube_nms", "tuber_tube_dense"] and vd.tubes_path == "device"
    want = cpu.tubes(nms=0.3, dense=True)
    assert_same_output(got, want, TUBE_KEYS | ADDED)
    if store == "padded":
        assert len(got) == 3 == len(plain) - 1                            # the suppressed tube is absent from both
    assert_same_output(make_d(dev, dense=True).tubes(), vd.tubes(dense=True), TUBE_KEYS | ADDED)         # the record's default
    va, cpu_a = make_a(dev), make_a("cpu")
    plain, seen = hooked(lambda: va.tracks())
    assert seen == ["tuber_tube_link_ranked", "tuber_track_actions"] and [set(t) for t in plain] == [TRACK_KEYS] * len(plain)
    assert_same_output(va.tracks(dense=False), plain, TRACK_KEYS)
    got, seen = hooked(lambda: va.tracks(dense=True))
    assert seen == ["tuber_tube_link_ranked", "tuber_track_actions", "tuber_tube_dense"] and va.tracks_path == "device"
    assert_same_output(got, cpu_a.tracks(dense=True), TRACK_KEYS | ADDED)
    got, seen = hooked(lambda: va.tracks(nms=0.3, dense=True))
    assert seen == ["tuber_tube_link_ranked", "tuber_track_actions", "tuber_tube_nms", "tuber_tube_dense"] and va.tracks_path == "device"
    want = cpu_a.tracks(nms=0.3, dense=True)
    assert_same_output(got, want, TRACK_KEYS | ADDED)
    if store == "padded":
        assert [t["length"] for t in got] == [6, 4] and [len(t["frames"]) for t in got] == [151, 91]
    bad = make_d(dev)
    bad.keys[2] = bad.keys[1]
    def refused():
        with pytest.raises(ValueError, match="ascending"):
            bad.tubes(dense=True)
    _, seen = hooked(refused)
    assert seen == []                                                      # refused before anything is launched
    capsys.readouterr()


def test_video_stream_dense_tubes_equal_the_video_detectors(dev):
    """the name-hashed AVA model of tests/test_video_gpu.py over 64 tiny frames, 8 key frames: the stream's closed tubes, made dense on the
    host, are the whole video's, made dense on the device"""
    from test_video_gpu import CONFIGS, SETTINGS, _model
    from tubelet_transformer_amd.video import VideoDetector, VideoStream
    cfg, model = _model(CONFIGS["ava"])
    kw = dict(SETTINGS["ava"], graphed=False)
    frames = np.random.default_rng(11).integers(0, 256, (64, 96, 160, 3), dtype=np.uint8)
    whole = VideoDetector(cfg, model, batch=2, **kw)(frames, stride=9)
    want, plain = whole.tubes(dense=True), whole.tubes()
    assert whole.tubes_path == "device" and len(want) >= 1 and max(t["length"] for t in want) >= 2
    vs = VideoStream(cfg, model, batch=2, stride=9, max_chunk=16, **kw)
    got = []
    for a in range(0, 64, 20):
        vs.push(frames[a:a + 20])
        got += vs.tubes(dense=True)
    vs.finish()
    got = sorted(got + vs.tubes(dense=True), key=lambda t: t["head"])
    assert len(got) == len(want)
    for g, w, p in zip(got, want, plain):
        assert set(g) == TUBE_KEYS | ADDED | {"head"} and g["keys"] == w["keys"] == p["frames"] and g["cls"] == w["cls"]
        same_dense(g, w)
        same_bits(g["key_boxes"], w["key_boxes"])
        assert np.float64(g["score"]).tobytes() == np.float64(w["score"]).tobytes()
    for a in range(0, 64, 32):                                            # and without the option the stream's tubes are what they were
        vs.push(frames[a:a + 32])
    vs.finish()
    assert [set(t) for t in vs.tubes()] == [TUBE_KEYS | {"head"}] * len(plain)
