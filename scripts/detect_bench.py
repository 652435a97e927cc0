"""Cost of getting ranked detections out of an eval forward (detect.py), TubeR_CSN152_AVA21 at 2 x 3 x 32 x 256 x 340, name-hashed weights:

  (a) eager_decode_host       the eager forward + PostProcessAVA.decode() + the three host copies (what PostProcessAVA.forward does)
  (b) detector_eager          Detector(graphed=False): the eager forward + one tuber_detect_ava launch, then to_host()
  (c) detector_graphed        Detector(graphed=True): forward and decode as one hipGraph replay, then to_host()
  (d) loop_eager / loop_graphed   one iteration of validate_tuber_detection with CONFIG.VAL.GRAPHED off / on: (T(6 batches) - T(2 batches)) / 4,
                              so that the capture of the first iteration is not in it

(a) to (d) are measured as same-box interleaved pairs: ``--rounds`` rounds, every variant once per round, host clock around calls that end on
the host.  (b') / (c') are (b) / (c) without to_host(), ended by a device synchronisation.  The decode launch alone (HIP events, --reps
launches) is recorded against the torch launches of decode() it replaces.  Nothing is asserted about time.

    python scripts/detect_bench.py [--rounds 5] [--reps 200] [--out profiles/detect_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tubelet_transformer_amd import synth  # noqa: E402
from tubelet_transformer_amd.config import load_cfg  # noqa: E402
from tubelet_transformer_amd.detect import Detector, detect_launch, empty_detections  # noqa: E402
from tubelet_transformer_amd.evaluation import validate_tuber_detection  # noqa: E402
from tubelet_transformer_amd.tuber import build_model  # noqa: E402

H, W = 256, 340


def wall(fn, n):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


def events(fn, n):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n           # microseconds per call


def loader(n):
    out = []
    for i in range(n):
        clips = synth.synthetic_clips(2, 32, H, W, seed=10 + i)
        tg = synth.synthetic_targets(2, "ava", 80, seed=20 + i, device="cpu", hw=(H, W))
        for b, t in enumerate(tg):
            k = t["boxes"].shape[0]
            t["image_id"] = ["vid%d_%04d" % (i, 900 + b), 16]
            t["size"] = torch.tensor([H, W])
            raw = torch.zeros(k, 6)
            raw[:, 0], raw[:, 1] = b, 16
            raw[:, 2:] = torch.tensor([10.0, 20.0, 200.0, 220.0])
            t["raw_boxes"] = raw
        out.append((clips, tg))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40, help="calls per variant and round")
    ap.add_argument("--reps", type=int, default=200, help="launches of the decode-alone measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("detect_bench.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    cfg = load_cfg(os.path.join(ROOT, "configuration", "TubeR_CSN152_AVA21.yaml"))
    model, criterion, post = build_model(cfg)
    synth.load_name_hashed(model)
    model.to(dev).eval()
    criterion.to(dev).eval()
    clips = synth.synthetic_clips(2, 32, H, W, seed=1, device=dev)
    sizes = torch.tensor([[H, W], [H, W]])
    eager_det = Detector(cfg, model, graphed=False)
    graph_det = Detector(cfg, model, graphed=True)
    tmp = tempfile.mkdtemp(prefix="detect_bench_")
    cfg.CONFIG.LOG.BASE_PATH, cfg.CONFIG.LOG.RES_DIR = tmp, "res"
    batches = loader(6)
    eager_det(clips, sizes)                                        # the engine's lazy buffers exist; what the first capture adds is its private pool
    torch.cuda.synchronize()
    reserved0 = torch.cuda.memory_reserved()
    graph_det(clips, sizes)
    torch.cuda.synchronize()
    pool_mib = (torch.cuda.memory_reserved() - reserved0) / 2 ** 20

    def a():
        with torch.no_grad():
            return post["bbox"](model(clips), sizes)

    def loop(graphed):
        cfg.CONFIG.VAL.GRAPHED = graphed
        t = []
        for n in (2, 6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            validate_tuber_detection(cfg, model, criterion, post, batches[:n], epoch=0, verbose=False)
            t.append(time.perf_counter() - t0)
        cfg.CONFIG.VAL.GRAPHED = False
        return 1e3 * (t[1] - t[0]) / 4

    variants = {
        "eager_decode_host": lambda: wall(a, args.calls),
        "detector_eager": lambda: wall(lambda: eager_det(clips, sizes).to_host(), args.calls),
        "detector_graphed": lambda: wall(lambda: graph_det(clips, sizes).to_host(), args.calls),
        "detector_eager_no_host_copy": lambda: wall(lambda: eager_det(clips, sizes), args.calls),
        "detector_graphed_no_host_copy": lambda: wall(lambda: graph_det(clips, sizes), args.calls),
        "loop_eager": lambda: loop(False),
        "loop_graphed": lambda: loop(True),
    }
    ms = {k: [] for k in variants}
    for rnd in range(args.rounds):
        for k, fn in variants.items():
            ms[k].append(fn())
        print("round %d: %s" % (rnd, ", ".join("%s %.3f" % (k, v[-1]) for k, v in ms.items())), flush=True)

    # the decode launch alone against the torch launches of decode() it replaces
    with torch.no_grad():
        out = model(clips)
        sz = sizes.to(dev, torch.float32)
        dets = empty_detections(2, eager_det.topk, dev)
        one = events(lambda: detect_launch("ava", out["pred_logits"], out["pred_logits_b"], out["pred_boxes"], sz, None, out["pred_logits"].shape[1],
                                           eager_det.actor_thr, eager_det.score_thr, eager_det.topk, out=dets), args.reps)
        torch_us = events(lambda: post["bbox"].decode(out, sz), args.reps)
    model.engine()[0].check_coop()
    res = dict(workload="TubeR_CSN152_AVA21, 2 x 3 x 32 x %d x %d, name-hashed weights, CONFIG.VAL.DETECT defaults (SCORE_THR %g, TOPK %d, ACTOR_THR %g)" %
               (H, W, eager_det.score_thr, eager_det.topk, eager_det.actor_thr), rounds=args.rounds, calls_per_round=args.calls,
               ms_per_batch_median={k: statistics.median(v) for k, v in ms.items()}, ms_per_batch_all=ms,
               decode_launch_us=one, torch_decode_launches_us=torch_us, captures=graph_det.eval.captures,
               capture_private_pool_mib=pool_mib)
    print(json.dumps(res["ms_per_batch_median"]), "decode launch %.1f us, torch decode() %.1f us" % (one, torch_us), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
