"""Cost of cropping tubes out of the resident video -- no model: the forward is not what is measured here.

Workload: the 512-frame 256 x 340 video of the other video benchmarks (random pixels, resident as uint8), the dense tubes of the synthetic padded
store ``scripts/tube_dense_bench.py`` links (18 key frames, a key every 30 frames, 21 rows per key), every frame of every tube cropped at 112 x 112.

The device's bytes must equal ``crops.crop_rows``' first.  Then, interleaved, the median wall time of ``--repeats`` calls of

* ``tube_crops``: the table on the host, one upload, one ``tuber_tube_crops`` launch;
* what a caller writes today on the device: per tube, the tube's frames as fp32, a sampling grid, ``torch.nn.functional.grid_sample``
  (bilinear, border, ``align_corners=False``), rounded to uint8;
* the numpy definition on the host over a host copy of the video (``--host-repeats`` calls);

and the ``tuber_tube_crops`` launch alone from HIP events (the median of ``--launches`` launches), with the bytes it writes and the source bytes
under the boxes computed from the shapes, and the rate those give.  A record, not a gate: nothing is asserted about time.

    python scripts/tube_crops_bench.py [--repeats 7] [--host-repeats 2] [--launches 30] [--out profiles/tube_crops_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tube_dense_bench import store_of  # noqa: E402
from tubelet_transformer_amd import lib  # noqa: E402
from tubelet_transformer_amd.crops import crop_rows, crop_table, tube_crops  # noqa: E402

FRAMES, H, W, SIZE = 512, 256, 340, (112, 112)


def grid_sample_loop(video, tubes, size):
    """the crops of every tube by ``grid_sample``, a tube at a time: fp32, so close to the definition's bytes, not equal to them"""
    h, w = size
    _, Hv, Wv, _ = video.shape
    out = []
    for t in tubes:
        idx = torch.as_tensor(t["frames"], device=video.device).clamp_(0, video.shape[0] - 1)
        box = torch.from_numpy(np.asarray(t["boxes"], np.float32)).to(video.device)
        img = video[idx].permute(0, 3, 1, 2).float()
        u = box[:, None, 0] + (torch.arange(w, device=video.device) + 0.5) * ((box[:, 2] - box[:, 0]) / w)[:, None]
        v = box[:, None, 1] + (torch.arange(h, device=video.device) + 0.5) * ((box[:, 3] - box[:, 1]) / h)[:, None]
        grid = torch.stack([(u / Wv * 2 - 1)[:, None, :].expand(-1, h, -1), (v / Hv * 2 - 1)[:, :, None].expand(-1, -1, w)], dim=-1)
        got = torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=False)
        out.append((got + 0.5).floor_().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous())
    return out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def source_bytes(index, boxes):
    """bytes of the video under the boxes, each clamped to its frame with the bilinear neighbour: what one pass over the crops must read"""
    ok = (index >= 0) & (index < FRAMES) & np.isfinite(boxes).all(1)
    b = boxes[ok].astype(np.float64)
    x1, x2 = np.clip(np.floor(np.minimum(b[:, 0], b[:, 2]) - 0.5), 0, W - 1), np.clip(np.floor(np.maximum(b[:, 0], b[:, 2]) - 0.5) + 1, 0, W - 1)
    y1, y2 = np.clip(np.floor(np.minimum(b[:, 1], b[:, 3]) - 0.5), 0, H - 1), np.clip(np.floor(np.maximum(b[:, 1], b[:, 3]) - 0.5) + 1, 0, H - 1)
    return int(((x2 - x1 + 1) * (y2 - y1 + 1)).sum()) * 3


def launch_ms(video, index, boxes, launches):
    dev, R = video.device, len(index)
    t_index, t_boxes = torch.from_numpy(index).to(dev), torch.from_numpy(boxes).to(dev)
    out = torch.empty(R, SIZE[0], SIZE[1], 3, dtype=torch.uint8, device=dev)
    valid = torch.empty(R, dtype=torch.uint8, device=dev)
    call = lambda: lib.call("tuber_tube_crops", video, FRAMES, H, W, t_index, t_boxes, R, SIZE[0], SIZE[1], 1.0, 1.0, 1.0, 1, None, out, valid)
    call()
    times = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tube_crops_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tube_crops_bench.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    host_video = np.random.default_rng(args.seed).integers(0, 256, (FRAMES, H, W, 3), dtype=np.uint8)
    video = torch.from_numpy(host_video).to(dev)
    tubes = store_of(18, 30, args.seed, dev).tubes(dense=True)
    index, boxes, offsets = crop_table(tubes)
    R = len(index)

    t0 = time.perf_counter()
    want, want_valid = crop_rows(host_video, index, boxes, SIZE)
    host_ms = [(time.perf_counter() - t0) * 1e3]
    got = tube_crops(video, tubes, SIZE)
    pixels, valid = got.to_host()
    assert got.path == "device" and np.array_equal(valid, want_valid) and np.array_equal(pixels, want), "the device's bytes are not the definition's"
    loop = torch.cat(grid_sample_loop(video, tubes, SIZE)).cpu().numpy()             # warm-up, and how far fp32 grid_sample is from the definition
    diff = np.abs(loop.astype(np.int16) - want.astype(np.int16))

    cases = dict(tube_crops=lambda: tube_crops(video, tubes, SIZE), grid_sample_loop=lambda: grid_sample_loop(video, tubes, SIZE))
    walls = {k: [] for k in cases}
    for i in range(args.repeats):
        for k, fn in cases.items():
            walls[k].append(wall(fn)[0])
        if i + 1 < args.host_repeats:
            t0 = time.perf_counter()
            crop_rows(host_video, index, boxes, SIZE)
            host_ms.append((time.perf_counter() - t0) * 1e3)
    walls["numpy_definition_host"] = host_ms
    ms, all_ms = launch_ms(video, index, boxes, args.launches)
    written, read = R * SIZE[0] * SIZE[1] * 3 + R, source_bytes(index, boxes) + R * 20
    entry = dict(workload="%d frames of %d x %d resident; the dense tubes of a synthetic padded store (18 key frames, a key every 30 frames, 21 rows per key) "
                          "cropped at %d x %d, samples 1" % (FRAMES, H, W, SIZE[0], SIZE[1]),
                 tubes=len(tubes), rows=R, bytes_written=written, source_bytes_under_the_boxes=read, tuber_tube_crops_ms=ms, tuber_tube_crops_ms_all=all_ms,
                 gb_per_s=(written + read) / (ms * 1e-3) / 1e9, wall_ms={k: statistics.median(v) for k, v in walls.items()}, wall_ms_all=walls,
                 grid_sample_fp32_bytes_off_by_one=int((diff == 1).sum()), grid_sample_fp32_bytes_off_by_more=int((diff > 1).sum()), bytes_compared=int(want.size),
                 device_equals_definition=True)
    print(json.dumps({k: v for k, v in entry.items() if not k.endswith("_all")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(repeats=args.repeats, host_repeats=args.host_repeats, launches=args.launches, result=entry), f, indent=1)


if __name__ == "__main__":
    main()
