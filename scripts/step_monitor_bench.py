"""Cost of the step monitor (CONFIG.TRAIN.MONITOR, monitor.py) on the default workload (CSN-152 AVA 2.1, 2 clips of 32 x 256 x 340, the
captured hipGraph step, dropout on): ms per step of three configurations of ONE model, measured as same-process interleaved rounds (every
round times each configuration once, in rotating order, after its own warm-up replays):

    off        no monitor attached (the step of a run without CONFIG.TRAIN.MONITOR)
    every_1    a monitor attached, a row recorded at every optimizer step
    every_50   the same captured step, EVERY 50 written to the device state (no new capture): 49 of 50 replays run early-exit workgroups only

``every_50 - off`` is the cost of a non-recording replay.  In the same run: the time of the three monitor launches on their own (the
unconditional form with the moments) and their achieved GB/s at 16 B / element (read g, p, m, v), beside two streaming passes over the same
buffers as yardsticks, ``tuber_weight_average`` at 12 B / element and the ``tuber_adamw_segment`` launches of one optimizer step at 28 B /
element -- HIP events around back-to-back launches, repeated ``--rounds`` times in rotating order.  profiles/weight_avg_bench.json holds the
rates of those two as recorded when the averager was added; they are quoted in the output.

    python scripts/step_monitor_bench.py [--rounds 5] [--steps 60] [--warmup 5] [--out profiles/step_monitor_bench.json]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tubelet_transformer_amd import lib, synth  # noqa: E402
from tubelet_transformer_amd.config import load_cfg  # noqa: E402
from tubelet_transformer_amd.misc import NestedTensor  # noqa: E402
from tubelet_transformer_amd.monitor import StepMonitor  # noqa: E402
from tubelet_transformer_amd.training import GraphedTrainStep, build_optimizer, deploy_model  # noqa: E402
from tubelet_transformer_amd.tuber import build_model  # noqa: E402
from tubelet_transformer_amd.weight_avg import WeightAverage  # noqa: E402

CONFIGS = {"off": None, "every_1": 1, "every_50": 50}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=340)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_monitor_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cfg = load_cfg(os.path.join(ROOT, "configuration", "TubeR_CSN152_AVA21.yaml"))
    torch.manual_seed(0)
    model, crit, _ = build_model(cfg)
    synth.load_name_hashed(model)
    model = deploy_model(model, cfg, True, device=dev)
    crit.to(dev)
    model.train()
    crit.train()
    opt = build_optimizer(model, cfg)
    store = model.engine()[0]
    mon = StepMonitor(model, every=1, history=8)
    hw = (args.height, args.width)
    clips = synth.synthetic_clips(2, 32, hw[0], hw[1], seed=1234, device=dev)
    targets = synth.synthetic_targets(2, "ava", cfg.CONFIG.DATA.NUM_CLASSES, seed=4321, device=dev, hw=hw)
    max_norm = cfg.CONFIG.LOSS_COFS.CLIPS_MAX_NORM

    def select(name):
        every = CONFIGS[name]
        if every is None:
            mon.detach()
        else:
            if opt.monitor is not mon:
                mon.attach(opt)
            mon.configure(every=every)

    step = GraphedTrainStep(model, crit, opt, max_norm)
    resident = {}
    for name in CONFIGS:                                  # capture + the batch resident in the buffers each captured step reads
        select(name)
        step(clips, targets)
        torch.cuda.synchronize()
        bufs = step.input_buffers(clips.shape)
        resident[name] = NestedTensor(bufs[0], bufs[1])
    assert len(step.graphs) == 2, list(step.graphs)       # off, and ONE graph for both cadences
    store.check_coop()
    names = list(CONFIGS)
    ms = {n: [] for n in names}
    recorded = {}
    for r in range(args.rounds):
        for name in names[r % len(names):] + names[:r % len(names)]:
            select(name)
            for _ in range(args.warmup):
                step(resident[name], targets)
            torch.cuda.synchronize()
            mon.reset()
            t0 = opt.t
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                loss, _ = step(resident[name], targets)
            e1.record()
            e1.synchronize()
            assert bool(torch.isfinite(loss)), (name, loss)
            ms[name].append(e0.elapsed_time(e1) / args.steps)
            every = CONFIGS[name]
            want = 0 if every is None else opt.t // every - t0 // every          # rows the cadence owes for these steps
            got = mon.rows()
            assert mon.bad() is None and len(got) == min(want, mon.history), (name, want, [x[0] for x in got])
            recorded[name] = want
    assert len(step.graphs) == 2, "a configuration was captured again inside the timed rounds"
    store.check_coop()
    mon.detach()

    # the streaming passes on their own, over the same buffers (the training state is not used after this point)
    avg = WeightAverage(model, "ema", 0.9999)
    seg_elems = sum(end - o for o, end, _ in opt.segments)
    mon_elems = sum(mon.numels)
    clip = opt.norm_out

    def k_mon():
        mon._launch(opt.exp_avg, opt.exp_avg_sq, None, None)

    def k_avg():
        avg.update()

    def k_adamw():
        for o, end, gi in opt.segments:
            g = opt.param_groups[gi]
            b1, b2 = g["betas"]
            lib.call("tuber_adamw_segment", store.flat.data_ptr() + 4 * o, store.gflat.data_ptr() + 4 * o, opt.exp_avg.data_ptr() + 4 * o,
                     opt.exp_avg_sq.data_ptr() + 4 * o, end - o, clip, float(g["lr"]), float(b1), float(b2), float(g["eps"]),
                     float(g["weight_decay"]), opt.t_dev, 0, opt.hyper.data_ptr() + 8 * gi)

    kernels = {"tuber_tensor_stats": (k_mon, 16 * mon_elems, mon_elems, 3),
               "tuber_weight_average": (k_avg, 12 * store.total, store.total, 2),
               "tuber_adamw_segment": (k_adamw, 28 * seg_elems, seg_elems, len(opt.segments))}
    knames = list(kernels)
    kms = {k: [] for k in knames}
    for r in range(args.rounds):
        for k in knames[r % len(knames):] + knames[:r % len(knames)]:
            fn = kernels[k][0]
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.kernel_reps):
                fn()
            e1.record()
            e1.synchronize()
            kms[k].append(e0.elapsed_time(e1) / args.kernel_reps)
    assert bool(torch.isfinite(store.flat).all())
    gbs = {k: [kernels[k][1] / (t * 1e-3) / 1e9 for t in v] for k, v in kms.items()}
    kstat = {k: {"launches": kernels[k][3], "elements": kernels[k][2], "bytes_per_element": kernels[k][1] // kernels[k][2],
                 "median_ms": round(statistics.median(kms[k]), 4), "rounds_ms": [round(x, 4) for x in kms[k]],
                 "median_GB_per_s": round(statistics.median(gbs[k]), 1), "min_GB_per_s": round(min(gbs[k]), 1), "max_GB_per_s": round(max(gbs[k]), 1)}
             for k in knames}
    gb_med = {k: statistics.median(v) for k, v in gbs.items()}
    earlier = {}
    path = os.path.join(ROOT, "profiles", "weight_avg_bench.json")
    if os.path.exists(path):
        old = json.load(open(path))["kernels"]
        earlier = {k: old[k]["median_GB_per_s"] for k in ("tuber_weight_average", "tuber_adamw_segment") if k in old}

    stat = {n: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "rounds_ms": [round(x, 4) for x in v],
                "rows_owed_in_last_timed_block": recorded[n]} for n, v in ms.items()}
    spread = max(max(v) - min(v) for v in ms.values())
    med = {n: statistics.median(v) for n, v in ms.items()}
    chunks_per_tensor = mon._tensors_host["nchunks"]
    res = {"workload": "CSN-152 AVA2.1, 2 clips x 32 x %d x %d, captured step, dropout on" % hw, "rounds": args.rounds, "steps": args.steps,
           "warmup": args.warmup, "configurations": stat, "spread_ms": round(spread, 4),
           "every_1_minus_off_ms": round(med["every_1"] - med["off"], 4), "every_50_minus_off_ms": round(med["every_50"] - med["off"], 4),
           "early_exit_within_spread": bool(med["every_50"] - med["off"] <= spread),
           "tensors": mon.n_tensors, "chunks": mon.n_chunks, "chunk_elements": mon.chunk,
           "one_chunk_tensors": int((chunks_per_tensor <= 1).sum()), "elements": mon_elems, "kernel_reps": args.kernel_reps, "kernels": kstat,
           "tensor_stats_over_weight_average_rate": round(gb_med["tuber_tensor_stats"] / gb_med["tuber_weight_average"], 3),
           "rates_recorded_in_weight_avg_bench_GB_per_s": earlier,
           "lib_md5": hashlib.md5(open(lib.LIBPATH, "rb").read()).hexdigest()[:12]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
