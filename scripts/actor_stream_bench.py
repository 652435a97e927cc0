"""Cost of streaming actor tracks (video.py ``VideoStream(..., actors=A)``) on 6h's workload: TubeR_CSN152_AVA21, name-hashed weights,
the synthetic 512-frame 256 x 340 video of scripts/video_stream_bench.py, a key frame every 30 frames (18 keys, batches of 2), 64 frames per push:

  stream               VideoStream(link=True): the parent's path, timed in the same run
  stream_actors        VideoStream(link=True, actors=A): six more device-to-device copies per batch, and per push that decided keys one more
                       tuber_tube_link_stream call (one class) and one tuber_track_actions_stream call

Both variants are same-box interleaved: ``--rounds`` rounds, every variant once per round, host clock around calls that end in a device
synchronise; medians and every round are recorded.  Beside them, with HIP events over ``--reps`` repetitions and interleaved in rounds too: the
per-push pair (``tuber_tube_link_stream`` with C = 1 + ``tuber_track_actions_stream``) summed over a video, a batch of keys per push, against one
``tuber_tube_link_ranked`` + ``tuber_track_actions`` over the same 18 x A store.  Nothing is asserted about time.

    python scripts/actor_stream_bench.py [--rounds 5] [--reps 200] [--out profiles/actor_stream_bench.json]
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
from tubelet_transformer_amd.config import actor_settings, load_cfg  # noqa: E402
from tubelet_transformer_amd.detect import ACTOR_FIELDS  # noqa: E402
from tubelet_transformer_amd.evaluation import smooth_range  # noqa: E402
from tubelet_transformer_amd.tuber import build_model  # noqa: E402
from tubelet_transformer_amd.video import VideoDetector, VideoStream  # noqa: E402

N, H, W, STRIDE, PER_PUSH = 512, 256, 340, 30, 64


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
    return 1e3 * e0.elapsed_time(e1) / n           # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200, help="repetitions per round of the kernel-alone measurements")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "actor_stream_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("actor_stream_bench.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    cfg = load_cfg(os.path.join(ROOT, "configuration", "TubeR_CSN152_AVA21.yaml"))
    model, _, _ = build_model(cfg)
    synth.load_name_hashed(model)
    model.to(dev).eval()
    B = 2
    frames = np.random.default_rng(1).integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    thr = dict(actor_thr=0.0, score_thr=0.0)                            # name-hashed weights are no detector: every query is an actor
    plain = VideoStream(cfg, model, batch=B, stride=STRIDE, max_chunk=64, **thr)
    A = actor_settings(cfg)["topk"]
    acted = VideoStream(cfg, model, batch=B, stride=STRIDE, max_chunk=64, actors=A, **thr)
    vdet = VideoDetector(cfg, model, batch=B, actors=A, **thr)

    def stream(vs):
        def run():
            outs = [vs.push(frames[i:i + PER_PUSH]) for i in range(0, N, PER_PUSH)] + [vs.finish()]
            vs._pending.clear()                                          # tubes() / tracks() are not part of this figure
            vs._pending_tracks.clear()
            return [o for o in outs if o is not None]
        return run
    variants = {"stream": stream(plain), "stream_actors": stream(acted)}
    want = vdet(frames, stride=STRIDE)
    for k, fn in variants.items():                                      # captures, lazy buffers; and the stream's actors are the detector's, bit for bit
        got = fn()
        if k == "stream_actors":
            assert all(torch.equal(torch.cat([getattr(o.actors, f) for o in got]), getattr(want.actors, f)) for f in ACTOR_FIELDS)
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for rnd in range(args.rounds):
        for k, fn in variants.items():
            ms[k].append(wall(fn))
        print("round %d: %s" % (rnd, ", ".join("%s %.2f ms" % (k, v[-1]) for k, v in ms.items())), flush=True)

    # the kernels alone: the per-push pair a batch of keys at a time against the one-shot pair over the video's store
    va, st = want.actors, vdet.actor_settings
    S, A, C = va.actions.shape
    NR = S * A
    f64, i32 = torch.float64, torch.int32
    boxes, actor, actions = va.boxes.contiguous(), va.actor.contiguous(), va.actions.contiguous()
    label = torch.where(va.queries >= 0, 0, -1).to(i32).contiguous()
    slot_off = torch.arange(S + 1, dtype=i32, device=dev) * A
    video_off = torch.tensor([0, S], dtype=i32).to(dev)
    one = dict(row_cls=torch.empty(NR, dtype=i32, device=dev), row_head=torch.empty(NR, dtype=i32, device=dev), tube_score=torch.zeros(NR, dtype=f64, device=dev),
               tube_len=torch.zeros(NR, dtype=i32, device=dev), tube_last=torch.full((NR,), -1, dtype=i32, device=dev),
               row_smooth=torch.empty(NR, C, dtype=f64, device=dev), track_mean=torch.empty(NR, C, dtype=f64, device=dev),
               track_peak=torch.empty(NR, C, dtype=torch.float32, device=dev))

    def one_shot():
        lib.call("tuber_tube_link_ranked", boxes, label, actor, slot_off, video_off, 1, S, NR, 1, A, st["link_iou"], st["max_gap"], one["row_cls"],
                 one["row_head"], one["tube_score"], one["tube_len"], one["tube_last"])
        lib.call("tuber_track_actions", actions, one["row_head"], one["tube_last"], S, A, C, st["window"], one["row_smooth"], one["track_mean"],
                 one["track_peak"])
    link_state = torch.zeros(lib.query("tuber_tube_link_state_bytes", 1), dtype=torch.uint8, device=dev)
    track_state = torch.zeros(lib.query("tuber_track_stream_state_bytes", A, C, st["max_gap"], st["window"]), dtype=torch.uint8, device=dev)
    head, score, length = torch.empty(S, A, dtype=i32, device=dev), torch.empty(S, A, dtype=f64, device=dev), torch.empty(S, A, dtype=i32, device=dev)
    mean, peak = torch.empty(S, A, C, dtype=f64, device=dev), torch.empty(S, A, C, dtype=torch.float32, device=dev)
    smooth = torch.empty(S, A, C, dtype=f64, device=dev)

    def per_push():
        link_state.zero_()
        track_state.zero_()
        for s in range(0, S, B):
            n = min(B, S - s)
            lo, _ = smooth_range(s, n, st["window"], s + n == S)
            lib.call("tuber_tube_link_stream", boxes[s:], label[s:], actor[s:], n, A, s, 1, st["link_iou"], st["max_gap"], link_state, head[s:], score[s:],
                     length[s:])
            lib.call("tuber_track_actions_stream", actions[s:], head[s:], n, A, C, s, st["max_gap"], st["window"], int(s + n == S), track_state, mean[s:],
                     peak[s:], smooth[lo:])
    one_shot(), per_push()
    assert torch.equal(head.reshape(-1), one["row_head"]) and torch.equal(smooth.reshape(NR, C), one["row_smooth"])
    us = {"one_shot_link_ranked_plus_track_actions": [], "per_push_link_stream_plus_track_actions_stream_total": []}
    for rnd in range(args.rounds):
        us["one_shot_link_ranked_plus_track_actions"].append(events(one_shot, args.reps))
        us["per_push_link_stream_plus_track_actions_stream_total"].append(events(per_push, args.reps))
    model.engine()[0].check_coop()
    med = lambda d: {k: statistics.median(v) for k, v in d.items()}
    res = dict(status="measured",
               workload="TubeR_CSN152_AVA21, name-hashed weights, %d frames of %d x %d, %d key frames (stride %d), batches of %d, %d frames per push, "
                        "actors %d, classes %d, max_gap %d, window %d, actor_thr 0, score_thr 0, max_chunk 64" % (
                            N, H, W, S, STRIDE, B, PER_PUSH, A, C, st["max_gap"], st["window"]),
               rounds=args.rounds, reps=args.reps, ms_per_video_median=med(ms), ms_per_video_all=ms, kernel_us_median=med(us), kernel_us_all=us,
               per_push_calls=(S + B - 1) // B,
               device_bytes=dict(stream=plain.device_bytes(), stream_actors=acted.device_bytes(), actor_link_state=int(link_state.numel()),
                                 track_state=int(track_state.numel())))
    print(json.dumps({k: res[k] for k in ("ms_per_video_median", "kernel_us_median", "device_bytes")}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
