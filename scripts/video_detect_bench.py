"""Cost of whole-video inference (video.py): TubeR_CSN152_AVA21, name-hashed weights, a synthetic 512-frame 256 x 340 video, a key
frame every 30 frames (18 keys, batches of 2):

  (a) clip_loop        the route without video.py: per key a host clip cut with clip_indices' rule, ClipBatch([...]).to(device) (upload +
                       tuber_clip_prepare per batch), the captured Detector, the fields cloned device-to-device; one synchronise at the end
  (b) video_detector   VideoDetector(frames): one upload, one tuber_video_clips launch per batch, the same captured Detector; one synchronise
                       at the end
  (b') video_detector_resident   (b) on frames that are already a device tensor

(a), (b), (b') are same-box interleaved: ``--rounds`` rounds, every variant once per round, host clock around calls that end in a device
synchronise; medians and every round are recorded.  Beside them, with HIP events over ``--reps`` launches: ``tuber_video_clips`` alone and
``tuber_clip_prepare`` alone at the same output size (both write the same bytes; the yardstick), interleaved in rounds too; and
``VideoDetections.tubes()`` on the device beside the host definition (host clock: both end on the host).  Nothing is asserted about time.

    python scripts/video_detect_bench.py [--rounds 5] [--reps 200] [--out profiles/video_detect_bench.json]
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
from tubelet_transformer_amd.detect import Detector  # noqa: E402
from tubelet_transformer_amd.tuber import build_model  # noqa: E402
from tubelet_transformer_amd.video import VideoDetections, VideoDetector, clip_indices, working_geometry  # noqa: E402

N, H, W = 512, 256, 340


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_detect_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("video_detect_bench.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    cfg = load_cfg(os.path.join(ROOT, "configuration", "TubeR_CSN152_AVA21.yaml"))
    model, _, _ = build_model(cfg)
    synth.load_name_hashed(model)
    model.to(dev).eval()
    T, rate, B = cfg.CONFIG.DATA.TEMP_LEN, cfg.CONFIG.DATA.FRAME_RATE, 2
    frames = np.random.default_rng(1).integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    frames_dev = torch.from_numpy(frames).to(dev)
    nh, nw, y1, x1, h, w = working_geometry(H, W, cfg.CONFIG.DATA.IMG_SIZE)
    thr = dict(actor_thr=0.0, score_thr=0.0)                            # name-hashed weights are no detector: every key frame keeps topk rows to link
    vdet = VideoDetector(cfg, model, batch=B, **thr)
    det = Detector(cfg, model, topk=vdet.detector.topk, **thr)
    keys = list(range(0, N, 30))
    index = clip_indices(N, keys, T, rate, "ava")
    transforms = ip.make_transforms("val", cfg)
    sizes = torch.tensor([[H, W]] * B)

    def clip_loop():
        kept = []
        for b in range(0, len(keys), B):
            rows = list(index[b:b + B])
            rows += [rows[-1]] * (B - len(rows))
            clips = []
            for row in rows:
                clip = ip.FrameClip(frames[row]).resize((nw, nh))
                clips.append(transforms(clip, {})[0])
            d = det(ip.ClipBatch(clips).to(dev), sizes, [T // 2] * B)
            kept.append([t.clone() for t in d.tensors()])
        return kept

    variants = {"clip_loop": clip_loop, "video_detector": lambda: vdet(frames, keys=keys), "video_detector_resident": lambda: vdet(frames_dev, keys=keys)}
    for fn in variants.values():                                       # captures, lazy buffers, tables
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for rnd in range(args.rounds):
        for k, fn in variants.items():
            ms[k].append(wall(fn))
        print("round %d: %s" % (rnd, ", ".join("%s %.2f ms" % (k, v[-1]) for k, v in ms.items())), flush=True)

    # the gather alone beside tuber_clip_prepare writing the same bytes
    lut, hsv = ip._device_tables(dev, (ip.MEAN, ip.STD))
    table = torch.from_numpy(index[4:4 + B].copy()).to(dev)
    out = torch.empty(B, 3, T, h, w, dtype=torch.float32, device=dev)
    mask = torch.empty(B, h, w, dtype=torch.bool, device=dev)
    desc = np.zeros(B, ip._DESC)
    for i in range(B):
        desc[i] = (i * T * nh * nw * 3, nh, nw, y1, x1, h, w, 0, 0, 0, 0, 0, 0)
    ddesc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    gather = lambda: lib.call("tuber_video_clips", frames_dev, N, nh, nw, table, B, T, y1, x1, h, w, lut, out)
    prepare = lambda: lib.call("tuber_clip_prepare", frames_dev, ddesc, lut, hsv, out, mask, B, T, h, w)
    us = {"tuber_video_clips": [], "tuber_clip_prepare": []}
    for rnd in range(args.rounds):
        us["tuber_video_clips"].append(events(gather, args.reps))
        us["tuber_clip_prepare"].append(events(prepare, args.reps))
    written = out.numel() * 4

    # tubes(): the device linker beside the host definition, on the video's detections
    vd = vdet(frames_dev, keys=keys)
    cpu = VideoDetections(vd.keys, *[t.cpu() for t in vd.tensors()], class_num=vd.class_num, settings=vd.settings)
    tubes_ms = {"device": [], "host": []}
    for rnd in range(args.rounds):
        t0 = time.perf_counter(); n_dev = len(vd.tubes()); tubes_ms["device"].append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter(); n_host = len(cpu.tubes()); tubes_ms["host"].append(1e3 * (time.perf_counter() - t0))
    assert vd.tubes_path == "device" and n_dev == n_host
    model.engine()[0].check_coop()
    med = lambda d: {k: statistics.median(v) for k, v in d.items()}
    res = dict(workload="TubeR_CSN152_AVA21, name-hashed weights, %d frames of %d x %d, %d key frames (stride 30), batches of %d, T %d, rate %d, topk %d, actor_thr 0, score_thr 0" %
               (N, H, W, len(keys), B, T, rate, vdet.detector.topk), rounds=args.rounds, reps=args.reps,
               ms_per_video_median=med(ms), ms_per_video_all=ms, kernel_us_median=med(us), kernel_us_all=us, bytes_written_per_launch=written,
               kernel_write_gb_per_s={k: written / (v * 1e-6) / 1e9 for k, v in med(us).items()},
               tubes_ms_median=med(tubes_ms), tubes_ms_all=tubes_ms, tubes=n_dev,
               detections_per_key=[int(c) for c in cpu.count.tolist()])
    print(json.dumps({k: res[k] for k in ("ms_per_video_median", "kernel_us_median", "kernel_write_gb_per_s", "tubes_ms_median", "tubes")}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
