"""Cost of streaming video inference (video.py ``VideoStream``) beside whole-video inference (6g): TubeR_CSN152_AVA21, name-hashed
weights, the synthetic 512-frame 256 x 340 video of scripts/video_detect_bench.py, a key frame every 30 frames (18 keys, batches of 2):

  video_detector       VideoDetector(frames, stride=30): the whole video resident, one index table, tuber_video_clips per batch
  stream_16 / _64 / _512   VideoStream fed 16, 64 and 512 frames per push (max_chunk 64), finish() at the end, link=True

All variants are same-box interleaved: ``--rounds`` rounds, every variant once per round, host clock around calls that end in a device
synchronise; medians and every round are recorded.  Beside them, with HIP events over ``--reps`` launches and interleaved in rounds too:
``tuber_video_clips_ring`` against ``tuber_video_clips`` on the same batch (keys 120 and 150: the same clips, from the ring and from the resident
video), and the linker -- one ``tuber_tube_link_ranked`` over the video's 18 x K store against the ``tuber_tube_link_stream`` launches that
link it a batch at a time.  The device bytes held are recorded as well: ring + link state against the resident video.  Nothing is asserted
about time; the comparison base is ``VideoDetector`` in the same run.

    python scripts/video_stream_bench.py [--rounds 5] [--reps 200] [--out profiles/video_stream_bench.json]
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

from tubelet_transformer_amd import input_pipeline as ip  # noqa: E402
from tubelet_transformer_amd import lib, synth  # noqa: E402
from tubelet_transformer_amd.config import load_cfg  # noqa: E402
from tubelet_transformer_amd.detect import FIELDS  # noqa: E402
from tubelet_transformer_amd.tuber import build_model  # noqa: E402
from tubelet_transformer_amd.video import RULES, VideoDetector, VideoStream, clip_indices, working_geometry  # noqa: E402

N, H, W, STRIDE = 512, 256, 340, 30


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
    ap.add_argument("--reps", type=int, default=200, help="launches per round of the kernel-alone measurements")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_stream_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("video_stream_bench.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    cfg = load_cfg(os.path.join(ROOT, "configuration", "TubeR_CSN152_AVA21.yaml"))
    model, _, _ = build_model(cfg)
    synth.load_name_hashed(model)
    model.to(dev).eval()
    T, rate, B = cfg.CONFIG.DATA.TEMP_LEN, cfg.CONFIG.DATA.FRAME_RATE, 2
    frames = np.random.default_rng(1).integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    nh, nw, y1, x1, h, w = working_geometry(H, W, cfg.CONFIG.DATA.IMG_SIZE)
    thr = dict(actor_thr=0.0, score_thr=0.0)                            # name-hashed weights are no detector: every key frame keeps topk rows to link
    vdet = VideoDetector(cfg, model, batch=B, **thr)
    vs = VideoStream(cfg, model, batch=B, stride=STRIDE, max_chunk=64, **thr)

    def stream(per_push):
        def run():
            outs = [vs.push(frames[i:i + per_push]) for i in range(0, N, per_push)] + [vs.finish()]
            vs._pending.clear()                                          # tubes() is not part of this figure: drop the records it would read
            return [o for o in outs if o is not None]
        return run
    variants = {"video_detector": lambda: vdet(frames, stride=STRIDE), "stream_16": stream(16), "stream_64": stream(64), "stream_512": stream(512)}
    want = variants["video_detector"]()
    for k, fn in variants.items():                                      # captures, lazy buffers, tables; and the stream is the detector, bit for bit
        got = fn()
        if k != "video_detector":
            assert all(torch.equal(torch.cat([getattr(o, f) for o in got]), getattr(want, f)) for f in FIELDS), k
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for rnd in range(args.rounds):
        for k, fn in variants.items():
            ms[k].append(wall(fn))
        print("round %d: %s" % (rnd, ", ".join("%s %.2f ms" % (k, v[-1]) for k, v in ms.items())), flush=True)

    # the gather alone: the same two clips from the ring and from the resident video
    lut = ip._device_tables(dev, (ip.MEAN, ip.STD))[0]
    R, keys = vs.R, [120, 150]
    resident = torch.from_numpy(frames).to(dev)                        # 256 x 340 is the working size: no resize
    assert (nh, nw) == (H, W)
    ring = torch.empty(R + 1, nh, nw, 3, dtype=torch.uint8, device=dev)
    for f in range(keys[-1] + T * rate):
        ring[f % R].copy_(resident[f])
    ring[R].copy_(resident[0])
    table = torch.from_numpy(clip_indices(N, keys, T, rate, "ava")).to(dev)
    out_a = torch.empty(B, 3, T, h, w, dtype=torch.float32, device=dev)
    out_b = torch.empty_like(out_a)
    gather = lambda: lib.call("tuber_video_clips", resident, N, nh, nw, table, B, T, y1, x1, h, w, lut, out_a)
    gather_ring = lambda: lib.call("tuber_video_clips_ring", ring, R, nh, nw, keys[0], keys[1] - keys[0], B, B, T, rate, RULES.index("ava"), -1, y1, x1,
                                   h, w, lut, out_b)
    gather(), gather_ring()
    assert torch.equal(out_a, out_b)

    # the linker alone: one launch over the video's store against a launch per batch
    S, K = want.scores.shape
    C, st = want.class_num, vdet.settings
    N_rows = S * K
    slot_off = torch.arange(S + 1, dtype=torch.int32, device=dev) * K
    video_off = torch.tensor([0, S], dtype=torch.int32).to(dev)
    one = dict(row_cls=torch.empty(N_rows, dtype=torch.int32, device=dev), row_head=torch.empty(N_rows, dtype=torch.int32, device=dev),
               tube_score=torch.zeros(N_rows, dtype=torch.float64, device=dev), tube_len=torch.zeros(N_rows, dtype=torch.int32, device=dev),
               tube_last=torch.full((N_rows,), -1, dtype=torch.int32, device=dev))
    boxes, labels, scores = want.boxes.contiguous(), want.labels.contiguous(), want.scores.contiguous()
    state = torch.zeros(lib.query("tuber_tube_link_state_bytes", C), dtype=torch.uint8, device=dev)
    head = torch.empty(S, K, dtype=torch.int32, device=dev)
    mean = torch.empty(S, K, dtype=torch.float64, device=dev)
    count = torch.empty(S, K, dtype=torch.int32, device=dev)
    link_one = lambda: lib.call("tuber_tube_link_ranked", boxes, labels, scores, slot_off, video_off, 1, S, N_rows, C, K, st["link_iou"], st["max_gap"],
                                one["row_cls"], one["row_head"], one["tube_score"], one["tube_len"], one["tube_last"])

    def link_stream():
        state.zero_()
        for s in range(0, S, B):
            n = min(B, S - s)
            lib.call("tuber_tube_link_stream", boxes[s:], labels[s:], scores[s:], n, K, s, C, st["link_iou"], st["max_gap"], state, head[s:], mean[s:],
                     count[s:])
    link_one(), link_stream()
    assert torch.equal(head.reshape(-1), one["row_head"])
    us = {"tuber_video_clips": [], "tuber_video_clips_ring": [], "tuber_tube_link_ranked_once": [], "tuber_tube_link_stream_per_batch_total": []}
    for rnd in range(args.rounds):
        us["tuber_video_clips"].append(events(gather, args.reps))
        us["tuber_video_clips_ring"].append(events(gather_ring, args.reps))
        us["tuber_tube_link_ranked_once"].append(events(link_one, args.reps))
        us["tuber_tube_link_stream_per_batch_total"].append(events(link_stream, args.reps))
    model.engine()[0].check_coop()
    med = lambda d: {k: statistics.median(v) for k, v in d.items()}
    res = dict(status="measured",
               workload="TubeR_CSN152_AVA21, name-hashed weights, %d frames of %d x %d, %d key frames (stride %d), batches of %d, T %d, rate %d, topk %d, "
                        "actor_thr 0, score_thr 0, max_chunk 64" % (N, H, W, S, STRIDE, B, T, rate, K),
               rounds=args.rounds, reps=args.reps, ms_per_video_median=med(ms), ms_per_video_all=ms, kernel_us_median=med(us), kernel_us_all=us,
               link_stream_launches=(S + B - 1) // B,
               device_bytes=dict(resident_video=N * nh * nw * 3, ring=(R + 1) * nh * nw * 3, ring_frames=R + 1, link_state=int(state.numel()),
                                 stream_total=vs.device_bytes()))
    print(json.dumps({k: res[k] for k in ("ms_per_video_median", "kernel_us_median", "device_bytes")}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
