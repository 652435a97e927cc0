"""Cost of dense action tubes on two synthetic padded stores of the sizes the video benchmarks run -- no model: the
forward is not what is measured here.

* 18 key frames of a 512-frame video (a key every 30 frames), 21 rows per key, max_gap 2: G = 90 frames per row;
* 1024 key frames (a key on every frame), 21 rows per key, max_gap 2: G = 3.

Per shape, after a warm-up call, the median wall time of ``--repeats`` calls, alternating, of

* ``tubes()``: the link launch, one copy, the host assembly;
* ``tubes(dense=True)``: the link and ``tuber_tube_dense`` launches, one copy, the host assembly;
* ``tubes()`` and then ``evaluation.dense_rows`` + ``dense_from_rows`` on the host: what a caller without the option does;

and the ``tuber_tube_dense`` launch alone from HIP events (the median of ``--launches`` launches).  The device's tubes must equal the host's
byte for byte.  A record, not a gate: nothing is asserted about time.

    python scripts/tube_dense_bench.py [--repeats 7] [--launches 50] [--out profiles/tube_dense_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tubelet_transformer_amd import lib  # noqa: E402
from tubelet_transformer_amd.device_map import DENSE_NAMES, link_ranked, tube_dense_launch  # noqa: E402
from tubelet_transformer_amd.evaluation import dense_extent, dense_from_rows, dense_rows, link_rows  # noqa: E402
from tubelet_transformer_amd.video import VideoDetections  # noqa: E402

SHAPES = ((18, 30), (1024, 1))          # (key frames, frames between two keys)
K, CLASSES, MAX_GAP, LINK_IOU = 21, 24, 2, 0.2


def store_of(S, stride, seed, dev):
    """a padded [S][K] store: 14 anchors that drift a pixel per frame, each seen at a key with probability 0.85 (so that gaps are bridged) at a
    jittered box, a class per anchor; the rows behind a key's count carry label -1"""
    rng = np.random.default_rng(seed)
    box, score, label = np.zeros((S, K, 4), np.float32), np.zeros((S, K), np.float32), np.full((S, K), -1, np.int32)
    anchor = rng.uniform(40, 300, (14, 2))
    angle = rng.uniform(0, 2 * np.pi, 14)
    vel = np.stack([np.cos(angle), np.sin(angle)], axis=1) / 8.0
    for s in range(S):
        n = 0
        for k in range(14):
            if rng.random() < 0.85:
                c = anchor[k] + vel[k] * s * stride
                box[s, n] = np.asarray([c[0] - 20, c[1] - 30, c[0] + 20, c[1] + 30]) + rng.normal(0, 2, 4)
                score[s, n], label[s, n] = rng.uniform(0.05, 1.0), k % CLASSES
                n += 1
    t = lambda a: torch.from_numpy(a).to(dev)
    count = (label >= 0).sum(1).astype(np.int32)
    return VideoDetections([s * stride for s in range(S)], t(box), t(score), t(label), t(np.where(label >= 0, 0, -1).astype(np.int32)), t(np.zeros((S, K), np.float32)),
                           t(count), t(count.copy()), class_num=CLASSES, settings=dict(link_iou=LINK_IOU, max_gap=MAX_GAP, min_len=1))


def host_heads(vd):
    """the store's links by the definition, once, outside every timed region -> (row_head, {head: rows})"""
    host = vd._fetch()[0]
    S = len(vd.keys)
    head = link_rows(host["boxes"].reshape(-1, 4), host["labels"].reshape(-1), host["scores"].reshape(-1), np.repeat(np.arange(S), K), [0, S], CLASSES, LINK_IOU,
                     MAX_GAP)["row_head"]
    rows = {}
    for r in np.nonzero(head >= 0)[0].tolist():
        rows.setdefault(int(head[r]), []).append(r)
    return head, rows


def by_hand(vd, head, rows):
    """``tubes()`` and then the definition on the host over a copy of the store: the loop a caller writes without the option (the links
    given: ``tubes()`` has made them)"""
    tubes = vd.tubes()
    host = vd._fetch()[0]
    d = dense_rows(host["boxes"].reshape(-1, 4), host["scores"].reshape(-1), head, vd.keys, K, MAX_GAP)
    return [dict(t, **dense_from_rows(rows[h], vd.keys, K, d)) for t, h in zip(tubes, sorted(rows))]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def launch_ms(vd, launches):
    link, _, _ = link_ranked(vd.boxes, vd.labels, vd.scores, CLASSES, LINK_IOU, MAX_GAP)
    G = dense_extent(vd.keys, MAX_GAP)
    out = tube_dense_launch(vd.boxes, vd.scores, link["row_head"], vd.keys, MAX_GAP, G)          # warm-up; its buffers are reused below
    S = len(vd.keys)
    slot_frame = torch.tensor(vd.keys, dtype=torch.int32).to(vd.boxes.device)
    boxes, scores = vd.boxes.contiguous(), vd.scores.contiguous()
    times = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        lib.call("tuber_tube_dense", boxes, scores, link["row_head"], slot_frame, S, K, MAX_GAP, G, *(out[k] for k in DENSE_NAMES))
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), G, sum(out[k].numel() * out[k].element_size() for k in DENSE_NAMES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tube_dense_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tube_dense_bench.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    shapes = []
    for S, stride in SHAPES:
        vd = store_of(S, stride, args.seed, dev)
        head, rows = host_heads(vd)
        cases = dict(tubes=lambda: vd.tubes(), tubes_dense=lambda: vd.tubes(dense=True), tubes_then_host_dense=lambda: by_hand(vd, head, rows))
        got = {k: fn() for k, fn in cases.items()}                        # warm-up, and the results to compare
        assert vd.tubes_path == "device"
        for g, w in zip(got["tubes_dense"], got["tubes_then_host_dense"]):
            assert g["frames"] == w["frames"] and g["boxes"].tobytes() == w["boxes"].tobytes() and g["frame_scores"].tobytes() == w["frame_scores"].tobytes()
        walls = {k: [] for k in cases}
        for _ in range(args.repeats):
            for k, fn in cases.items():
                walls[k].append(wall(fn)[0])
        ms, G, out_bytes = launch_ms(vd, args.launches)
        entry = dict(workload="synthetic padded store: %d key frames, a key every %d frames, %d rows per key, %d classes, max_gap %d" % (S, stride, K, CLASSES, MAX_GAP),
                     rows=S * K, G=G, dense_output_bytes=out_bytes, tubes=len(got["tubes"]), frames_in_tubes=sum(len(t["frames"]) for t in got["tubes_dense"]),
                     wall_ms={k: statistics.median(v) for k, v in walls.items()}, wall_ms_all=walls, tuber_tube_dense_ms=ms)
        shapes.append(entry)
        print(json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(repeats=args.repeats, launches=args.launches, shapes=shapes), f, indent=1)


if __name__ == "__main__":
    main()
