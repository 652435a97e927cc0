"""Cost of video-mAP over linked action tubes, host path (evaluation.VideoMAP) against device path (device_map.DeviceVideoMAP), on synthetic
stores that need no model (synth.synthetic_video_map_case), for two shapes:

* 256 videos x 32 frames x 10 detections x 24 classes: many short videos, the shape of a JHMDB / UCF101-24 validation pass;
* 8 videos x 1024 frames x 10 x 24: few long videos -- linking is sequential in the frame count, so this is the shape that shows it.

Per shape: the host time of ``VideoMAP.link()`` and of ``evaluate()`` (which links again), once; the device wall time of
``DeviceVideoMAP.evaluate_video()`` (host clock around a call that ends in the read-back) after a warm-up call, the median of ``--repeats``
calls, and its stages from HIP events: layout + uploads (host work included), tuber_tube_link, tuber_tube_match, ranking sorts + scatter,
tuber_ranked_ap, read-back.  Nothing is asserted about time; the results must agree.

    python scripts/video_map_bench.py [--repeats 5] [--out profiles/video_map_bench.json] [--host-only]
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

from tubelet_transformer_amd import synth  # noqa: E402
from tubelet_transformer_amd.evaluation import VideoMAP  # noqa: E402

SHAPES = ((256, 32), (8, 1024))


def host_path(case, classes):
    ev = VideoMAP(class_num=classes)
    ev.add_detections(case["det_keys"], case["det_boxes"], case["det_probs"])
    ev.add_ground_truth(case["gt_keys"], case["gt_boxes"], case["gt_labels"].argmax(axis=1), case["gt_tubes"])
    t0 = time.perf_counter()
    link = ev.link()
    t1 = time.perf_counter()
    res = ev.evaluate()
    t2 = time.perf_counter()
    lens = [len(t["frames"]) for t in link["tubes"]]
    return res, dict(link_s=t1 - t0, evaluate_s=t2 - t1, video_mAP={str(k): v[0] for k, v in res.items()}, rows=len(case["det_keys"]),
                     gt_lines=len(case["gt_keys"]), tubes=len(lens), longest_tube=max(lens))


def device_path(case, classes, repeats):
    import torch
    from tubelet_transformer_amd.device_map import DeviceVideoMAP
    dev = torch.device("cuda:0")
    st = DeviceVideoMAP(class_num=classes, device=dev)
    n, step = len(case["det_keys"]), 20                          # the loop's batches: two clips of ten rows
    boxes, probs = torch.from_numpy(case["det_boxes"]).to(dev), torch.from_numpy(case["det_probs"]).to(dev)
    for i in range(0, n, step):
        st.add_detections(case["det_keys"][i:i + step], boxes[i:i + step], probs[i:i + step])
    st.add_ground_truth(case["gt_keys"], case["gt_boxes"], case["gt_labels"], tubes=case["gt_tubes"])
    warm = st.evaluate_video()
    assert st.video_path == "device"
    walls, parts = [], []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = {}
        t0 = time.perf_counter()
        res = st.evaluate_video(timings=t)
        walls.append((time.perf_counter() - t0) * 1e3)
        parts.append(t)
        assert all(np.float64(res[k][0]).view(np.int64) == np.float64(warm[k][0]).view(np.int64) for k in warm), "evaluate_video() is not reproducible"
    return warm, dict(evaluate_wall_ms=statistics.median(walls), evaluate_wall_ms_all=walls,
                      parts_ms={k: statistics.median(p[k] for p in parts) for k in parts[0]}, video_mAP={str(k): v[0] for k, v in warm.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dets", type=int, default=10)
    ap.add_argument("--classes", type=int, default=24)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-only", action="store_true", help="the host path alone (no GPU needed); nothing is written")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_map_bench.json"))
    args = ap.parse_args()
    if not args.host_only:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("video_map_bench.py measures on the GPU: none found")
    shapes = []
    for videos, frames in SHAPES:
        case = synth.synthetic_video_map_case(videos, frames, args.dets, args.classes, seed=args.seed)
        what = "synthetic store: %d videos x %d frames x %d detections x (%d classes + no-object), 1..2 ground-truth tubes per video" % (
            videos, frames, args.dets, args.classes)
        entry = dict(workload=what)
        if not args.host_only:
            dres, entry["device"] = device_path(case, args.classes, args.repeats)
        hres, entry["host"] = host_path(case, args.classes)
        if not args.host_only:
            entry["max_abs_difference"] = max(abs(dres[k][0] - hres[k][0]) for k in hres)
            assert entry["max_abs_difference"] < 1e-12, entry
        shapes.append(entry)
        print(json.dumps(entry), flush=True)
    if not args.host_only:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(repeats=args.repeats, shapes=shapes), f, indent=1)


if __name__ == "__main__":
    main()
