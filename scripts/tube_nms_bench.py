"""Cost of spatio-temporal tube NMS on the two synthetic stores of scripts/video_map_bench.py:

* 256 videos x 32 frames x 10 detections x 24 classes;
* 8 videos x 1024 frames x 10 x 24.

Per shape: the host definition ``evaluation.tube_nms`` once on the CPU; the ``tuber_tube_nms`` stage of ``DeviceVideoMAP.evaluate_video()`` from
HIP events and the wall time of ``evaluate_video()`` with NMS off and on (after a warm-up call, the median of ``--repeats`` calls); the
launches of both runs by name -- with NMS off they must be the three of the evaluator without the feature.  The device's bytes must equal the
host's.  A record, not a gate: nothing is asserted about time.

    python scripts/tube_nms_bench.py [--repeats 5] [--iou 0.3] [--out profiles/tube_nms_bench.json]
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

from tubelet_transformer_amd import lib, synth  # noqa: E402
from tubelet_transformer_amd.device_map import DeviceVideoMAP  # noqa: E402
from tubelet_transformer_amd.evaluation import VideoMAP, tube_nms  # noqa: E402

SHAPES = ((256, 32), (8, 1024))
PLAIN_LAUNCHES = ["tuber_tube_link", "tuber_tube_match", "tuber_ranked_ap"]


def store_of(case, classes, dev, nms):
    st = DeviceVideoMAP(class_num=classes, device=dev, tube_nms=nms)
    boxes, probs = torch.from_numpy(case["det_boxes"]).to(dev), torch.from_numpy(case["det_probs"]).to(dev)
    for i in range(0, len(case["det_keys"]), 20):
        st.add_detections(case["det_keys"][i:i + 20], boxes[i:i + 20], probs[i:i + 20])
    st.add_ground_truth(case["gt_keys"], case["gt_boxes"], case["gt_labels"], tubes=case["gt_tubes"])
    return st


def timed(st, repeats):
    seen = []
    lib.set_launch_hook(lambda name, args, launch: (seen.append(name), launch(name, *args))[1])
    try:
        warm = st.evaluate_video()
    finally:
        lib.set_launch_hook(None)
    assert st.video_path == "device"
    walls, parts = [], []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = {}
        t0 = time.perf_counter()
        st.evaluate_video(timings=t)
        walls.append((time.perf_counter() - t0) * 1e3)
        parts.append(t)
    return warm, seen, dict(evaluate_wall_ms=statistics.median(walls), evaluate_wall_ms_all=walls,
                            parts_ms={k: statistics.median(p[k] for p in parts) for k in parts[0]}, launches=seen,
                            video_mAP={str(k): v[0] for k, v in warm.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dets", type=int, default=10)
    ap.add_argument("--classes", type=int, default=24)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iou", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tube_nms_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tube_nms_bench.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    shapes = []
    for videos, frames in SHAPES:
        case = synth.synthetic_video_map_case(videos, frames, args.dets, args.classes, seed=args.seed)
        entry = dict(workload="synthetic store: %d videos x %d frames x %d detections x (%d classes + no-object), nms_iou %g" % (
            videos, frames, args.dets, args.classes, args.iou))
        ev = VideoMAP(class_num=args.classes)
        ev.add_detections(case["det_keys"], case["det_boxes"], case["det_probs"])
        link = ev.link()
        t0 = time.perf_counter()
        want = tube_nms(link, args.iou, 1)
        entry["host"] = dict(tube_nms_s=time.perf_counter() - t0, rows=len(want), tubes=int((want != 2).sum()), suppressed=int((want == 0).sum()))
        _, seen, entry["nms_off"] = timed(store_of(case, args.classes, dev, None), args.repeats)
        assert seen == PLAIN_LAUNCHES, seen
        st = store_of(case, args.classes, dev, args.iou)
        _, seen, entry["nms_on"] = timed(st, args.repeats)
        assert seen == PLAIN_LAUNCHES[:1] + ["tuber_tube_nms"] + PLAIN_LAUNCHES[1:], seen
        a = st.video_arrays()
        got = st.nms(a, st.link(a)).cpu().numpy()
        assert np.array_equal(got, want), "tuber_tube_nms differs from evaluation.tube_nms at %d rows" % int((got != want).sum())
        entry["tuber_tube_nms_ms"] = entry["nms_on"]["parts_ms"]["tuber_tube_nms_ms"]
        shapes.append(entry)
        print(json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(repeats=args.repeats, shapes=shapes), f, indent=1)


if __name__ == "__main__":
    main()
