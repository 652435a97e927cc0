"""Cost of the validation metric at the end of validate_tuber_detection, host path against device path (device_map.py), on a synthetic
store that needs no model: 4096 frames x 15 detections x 80 classes, 0..5 ground-truth boxes per frame with 1..3 labels each, one fifth of
the rows gated to score 0 like the real decode, tie-free otherwise (synth.synthetic_frame_map_case).

* host: write_result_files + FrameMAP.load_gt / load_detections + evaluate(), once, in a child process under a time limit of its own;
* device: DeviceFrameMAP.evaluate() wall time (host clock around a call that ends in the read-back) after a warm-up call, the median of
  ``--repeats`` calls, and its parts from HIP events: frame sort + uploads, tuber_frame_match, ranking sort + gather, tuber_ranked_ap, tie
  count, read-back.

``--ucf`` measures the same quantities for the JHMDB / UCF101-24 loop (validate_tuber_ucf_detection: FrameMAPUCF against
DeviceFrameMAPUCF) on a store of 8192 frames x 10 detections x 24 classes (synth.synthetic_frame_map_ucf_case) and writes
profiles/device_map_ucf_bench.json.

    python scripts/device_map_bench.py [--frames 4096] [--repeats 5] [--host-limit 900] [--out profiles/device_map_bench.json]
    python scripts/device_map_bench.py --ucf [--frames 8192] [--repeats 5] [--out profiles/device_map_ucf_bench.json]
    python scripts/device_map_bench.py --host-only DIR      (the child: prints one JSON line)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tubelet_transformer_amd import synth  # noqa: E402
from tubelet_transformer_amd.evaluation import FrameMAP, FrameMAPUCF, write_result_files  # noqa: E402


def case_of(args):
    if args.ucf:
        case = synth.synthetic_frame_map_ucf_case(args.frames, dets=args.dets, classes=args.classes, seed=args.seed)
        case["det_scores"] = case["det_probs"]
        return case
    return synth.synthetic_frame_map_case(args.frames, dets=args.dets, classes=args.classes, seed=args.seed, gated=0.2)


def host_path(args, d):
    case = case_of(args)
    n, m = len(case["det_keys"]), len(case["gt_keys"])
    t0 = time.perf_counter()
    dp, gp = write_result_files(d, "res", 0, case["det_keys"], case["det_boxes"], case["det_scores"], np.zeros((n, 0 if args.ucf else 1), np.float32),
                                case["gt_keys"], np.concatenate([np.zeros((m, 2)), case["gt_boxes"]], axis=1), case["gt_labels"])
    t1 = time.perf_counter()
    out = {}
    for stable in (False, True):
        ta = time.perf_counter()
        ev = FrameMAPUCF(args.classes, stable=stable) if args.ucf else FrameMAP(args.classes, stable=stable)
        ev.load_gt([gp])
        ev.load_detections([dp])
        tb = time.perf_counter()
        mAP, _ = ev.evaluate()
        tc = time.perf_counter()
        out["stable" if stable else "reference_order"] = dict(load_s=tb - ta, evaluate_s=tc - tb, mAP=mAP)
    ref = out["reference_order"]
    return dict(write_s=t1 - t0, load_s=ref["load_s"], evaluate_s=ref["evaluate_s"], total_s=t1 - t0 + ref["load_s"] + ref["evaluate_s"],
                mAP=ref["mAP"], mAP_stable=out["stable"]["mAP"], detection_lines=n, gt_lines=m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ucf", action="store_true", help="the JHMDB / UCF101-24 evaluator on 8192 frames x 10 detections x 24 classes")
    ap.add_argument("--frames", type=int, default=None)
    ap.add_argument("--dets", type=int, default=None)
    ap.add_argument("--classes", type=int, default=None)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-limit", type=float, default=900.0, help="seconds the host path may take before it is given up")
    ap.add_argument("--host-only", metavar="DIR", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    for k, v in zip(("frames", "dets", "classes"), (8192, 10, 24) if args.ucf else (4096, 15, 80)):
        if getattr(args, k) is None:
            setattr(args, k, v)
    args.out = args.out or os.path.join(ROOT, "profiles", "device_map_ucf_bench.json" if args.ucf else "device_map_bench.json")
    if args.host_only:
        print(json.dumps(host_path(args, args.host_only)))
        return
    import torch
    from tubelet_transformer_amd.device_map import DeviceFrameMAP, DeviceFrameMAPUCF
    if not torch.cuda.is_available():
        raise SystemExit("device_map_bench.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    case = case_of(args)
    st = DeviceFrameMAPUCF(args.classes, device=dev) if args.ucf else DeviceFrameMAP(args.classes, device=dev)
    n = len(case["det_keys"])
    step = 2 * args.dets                                       # the loop's batches: two clips
    t0 = time.perf_counter()
    boxes, scores = torch.from_numpy(case["det_boxes"]).to(dev), torch.from_numpy(case["det_scores"]).to(dev)
    for i in range(0, n, step):
        st.add_detections(case["det_keys"][i:i + step], boxes[i:i + step], scores[i:i + step])
    st.add_ground_truth(case["gt_keys"], case["gt_boxes"], case["gt_labels"])
    torch.cuda.synchronize()
    feed_s = time.perf_counter() - t0
    warm, _ = st.evaluate()
    assert st.path == "device"
    walls, parts, maps = [], [], []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t = {}
        t0 = time.perf_counter()
        mAP, _ = st.evaluate(timings=t)
        walls.append((time.perf_counter() - t0) * 1e3)
        parts.append(t)
        maps.append(mAP)
    assert all(np.float64(m).view(np.int64) == np.float64(warm).view(np.int64) for m in maps), "evaluate() is not reproducible"
    device = dict(evaluate_wall_ms=statistics.median(walls), evaluate_wall_ms_all=walls, feed_s=feed_s, mAP=warm,
                  parts_ms={k: statistics.median(p[k] for p in parts) for k in parts[0]}, tied_rows=sum(st.ties.values()))
    host = None
    with tempfile.TemporaryDirectory() as d:
        cmd = [sys.executable, os.path.abspath(__file__), "--host-only", d, "--frames", str(args.frames), "--dets", str(args.dets),
               "--classes", str(args.classes), "--seed", str(args.seed)] + (["--ucf"] if args.ucf else [])
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.host_limit, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
            host = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else dict(error=r.stderr[-2000:])
        except subprocess.TimeoutExpired:
            host = dict(error="not measured: the host path did not finish in %.0f s" % args.host_limit)
    what = ("synthetic UCF-style store: %d frames x %d detections x (%d classes + no-object), 0..3 ground-truth boxes per frame, 1/4 of the rows no-object"
            if args.ucf else "synthetic store: %d frames x %d detections x %d classes, 0..5 ground-truth boxes per frame, 1/5 of the rows gated to 0")
    result = dict(workload=what % (args.frames, args.dets, args.classes), repeats=args.repeats, device=device, host=host)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
