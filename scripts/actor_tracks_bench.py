"""Cost of actor tracks (detect.Detector(actors=A), video.VideoActors.tracks) on the workload of scripts/video_detect_bench.py:
TubeR_CSN152_AVA21, name-hashed weights, a synthetic 512-frame 256 x 340 video, a key frame every 30 frames (18 keys, batches of 2):

  (a) video_detector / video_detector_actors   VideoDetector(frames) per video with ``actors`` off -- the path without this feature -- and
                       with ``actors=15``: one more launch per batch inside the replayed graph and six more device-to-device copies
  (b) tuber_detect_actors alone beside tuber_detect_ava alone, on the head outputs of one batch, HIP events over ``--reps`` launches
  (c) VideoActors.tracks() on the device (tuber_tube_link_ranked with one class, tuber_track_actions, one copy back) beside
                       evaluation.actor_tracks on the host over the store read back (host clock: both end on the host)

Same-box interleaved: ``--rounds`` rounds, every variant once per round; medians, the range and every round are recorded.  Expectation written
down before the first run: the forward is about 4.9 ms per batch, so one more small launch per batch should be lost in it.  Nothing is asserted
about time.

    python scripts/actor_tracks_bench.py [--rounds 5] [--reps 200] [--out profiles/actor_tracks_bench.json]
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
from tubelet_transformer_amd.config import load_cfg  # noqa: E402
from tubelet_transformer_amd.detect import empty_actors, empty_detections  # noqa: E402
from tubelet_transformer_amd.tuber import build_model  # noqa: E402
from tubelet_transformer_amd.video import VideoActors, VideoDetector  # noqa: E402

N, H, W, ACTORS = 512, 256, 340, 15


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def events(fn, n):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n           # microseconds per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200, help="launches per round of the kernel-alone measurements")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "actor_tracks_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("actor_tracks_bench.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    cfg = load_cfg(os.path.join(ROOT, "configuration", "TubeR_CSN152_AVA21.yaml"))
    model, _, _ = build_model(cfg)
    synth.load_name_hashed(model)
    model.to(dev).eval()
    B = 2
    frames = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (N, H, W, 3), dtype=np.uint8)).to(dev)
    thr = dict(actor_thr=0.0, score_thr=0.0)                            # name-hashed weights are no detector: every query is an actor
    keys = list(range(0, N, 30))
    plain = VideoDetector(cfg, model, batch=B, **thr)
    witha = VideoDetector(cfg, model, batch=B, actors=ACTORS, **thr)
    variants = {"video_detector": lambda: plain(frames, keys=keys), "video_detector_actors": lambda: witha(frames, keys=keys)}
    for fn in variants.values():                                       # captures, lazy buffers, tables
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for rnd in range(args.rounds):
        for k, fn in variants.items():
            ms[k].append(wall(fn))
        print("round %d: %s" % (rnd, ", ".join("%s %.2f ms" % (k, v[-1]) for k, v in ms.items())), flush=True)

    # the two decode launches alone, on the head outputs of one batch
    with torch.no_grad():
        out = model(synth.synthetic_clips(B, cfg.CONFIG.DATA.TEMP_LEN, 256, 340, seed=3, device=dev))
    lg, lb, bx = (out[k].contiguous() for k in ("pred_logits", "pred_logits_b", "pred_boxes"))
    Q, C = lg.shape[1], lg.shape[2]
    dtypes = sum(bit for t, bit in ((lg, 1), (lb, 2), (bx, 4)) if t.dtype == torch.bfloat16)
    sizes = torch.tensor([[H, W]] * B, dtype=torch.float32, device=dev)
    K = plain.detector.topk
    det, act = empty_detections(B, K, dev), empty_actors(B, ACTORS, C, dev)
    ava = lambda: lib.call("tuber_detect_ava", lg, lb, bx, sizes, None, B, Q, Q, C, lb.shape[-1], Q, dtypes, 0.0, 0.0, K, *det.tensors())
    actors = lambda: lib.call("tuber_detect_actors", lg, lb, bx, sizes, None, B, Q, Q, C, lb.shape[-1], Q, dtypes, 0.0, ACTORS, *act.tensors())
    us = {"tuber_detect_ava": [], "tuber_detect_actors": []}
    for rnd in range(args.rounds):
        us["tuber_detect_ava"].append(events(ava, args.reps))
        us["tuber_detect_actors"].append(events(actors, args.reps))

    # tracks(): the device path beside the host definition, on the video's actors
    va = witha(frames, keys=keys).actors
    cpu = VideoActors(va.keys, *[t.cpu() for t in va.tensors()], settings=va.settings)
    tracks_ms = {"device": [], "host": []}
    err = sys.stderr
    for rnd in range(args.rounds):
        t0 = time.perf_counter(); n_dev = len(va.tracks()); tracks_ms["device"].append(1e3 * (time.perf_counter() - t0))
        sys.stderr = open(os.devnull, "w")                              # the host path says that it is the host path, every time
        try:
            t0 = time.perf_counter(); n_host = len(cpu.tracks()); tracks_ms["host"].append(1e3 * (time.perf_counter() - t0))
        finally:
            sys.stderr.close()
            sys.stderr = err
    assert va.tracks_path == "device" and n_dev == n_host
    model.engine()[0].check_coop()
    med = lambda d: {k: statistics.median(v) for k, v in d.items()}
    rng = lambda d: {k: [min(v), max(v)] for k, v in d.items()}
    res = dict(workload="TubeR_CSN152_AVA21, name-hashed weights, %d frames of %d x %d, %d key frames (stride 30), batches of %d, topk %d, actors %d, "
                        "actor_thr 0, score_thr 0" % (N, H, W, len(keys), B, K, ACTORS), rounds=args.rounds, reps=args.reps,
               expectation="the forward is about 4.9 ms per batch: one more small launch per batch should be lost in it",
               ms_per_video_median=med(ms), ms_per_video_range=rng(ms), ms_per_video_all=ms, kernel_us_median=med(us), kernel_us_range=rng(us),
               kernel_us_all=us, tracks_ms_median=med(tracks_ms), tracks_ms_range=rng(tracks_ms), tracks_ms_all=tracks_ms, tracks=n_dev,
               actors_per_key=[int(c) for c in cpu.count.tolist()])
    print(json.dumps({k: res[k] for k in ("ms_per_video_median", "ms_per_video_range", "kernel_us_median", "tracks_ms_median", "tracks")}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
