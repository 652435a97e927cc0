"""Cost of gradient accumulation (accum.py) on the default workload (CSN-152 AVA 2.1, 2 clips of 32 x 256 x 340 per micro-batch, the
captured hipGraph step): ms per micro-batch for ACCUM_STEPS k in {1, 2, 8}, measured as same-process interleaved rounds (every round
times each k once, in rotating order, over a whole number of groups), and the bandwidth of one tuber_grad_accum pass (init / add /
fold) over the trainable windows, from HIP events around back-to-back launches, and the device memory the captured graphs of each k hold.
``--passes-only`` runs nothing but 50 launches of each pass, for a kernel trace:

    python scripts/accum_bench.py [--rounds 6] [--groups 2] [--out profiles/accum_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -o accum -- python scripts/accum_bench.py --passes-only
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tubelet_transformer_amd import synth  # noqa: E402
from tubelet_transformer_amd.config import load_cfg  # noqa: E402
from tubelet_transformer_amd.training import GraphedTrainStep, build_optimizer, deploy_model  # noqa: E402
from tubelet_transformer_amd.tuber import build_model  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--groups", type=int, default=2, help="groups of 8 micro-batches per timed block")
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=340)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum_bench.json"))
    ap.add_argument("--passes-only", action="store_true", help="only the init / add / fold launches (kernel-trace run)")
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
    hw = (args.height, args.width)
    clips = synth.synthetic_clips(2, 32, hw[0], hw[1], seed=1234, device=dev)
    targets = synth.synthetic_targets(2, "ava", cfg.CONFIG.DATA.NUM_CLASSES, seed=4321, device=dev, hw=hw)
    max_norm = cfg.CONFIG.LOSS_COFS.CLIPS_MAX_NORM
    if args.passes_only:
        from tubelet_transformer_amd.accum import GradAccumulator
        acc = GradAccumulator(model.engine()[0], 8)
        for fn in (acc.init, acc.add, acc.fold):
            for _ in range(50):
                fn()
        torch.cuda.synchronize()
        print(json.dumps({"passes_only": True, "trainable_elements": sum(b - a for a, b in acc.windows()), "launches_per_pass": 50}))
        return
    ks = (1, 2, 8)
    steps = {k: GraphedTrainStep(model, crit, opt, max_norm, accum_steps=k) for k in ks}
    n = 8 * args.groups                                   # micro-batches per timed block: whole groups for every k
    graph_gb = {}
    for k in ks:                                          # capture every role + warm up
        torch.cuda.synchronize()
        r0 = torch.cuda.memory_reserved()
        for _ in range(max(2 * k, 4)):
            steps[k](clips, targets)
        torch.cuda.synchronize()
        graph_gb[str(k)] = {"graphs": len(steps[k].graphs), "reserved_GB": round((torch.cuda.memory_reserved() - r0) / 1e9, 2)}
    torch.cuda.synchronize()
    model.engine()[0].check_coop()
    ms = {k: [] for k in ks}
    for r in range(args.rounds):
        order = ks[r % len(ks):] + ks[:r % len(ks)]
        for k in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                steps[k](clips, targets)
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / n)
    model.engine()[0].check_coop()
    med = {k: statistics.median(v) for k, v in ms.items()}
    # one accumulation pass in isolation: bytes = (2 reads + 1 write) x 4 B per trainable element (init: 1 read + 1 write)
    acc = steps[8].accum
    elems = sum(b - a for a, b in acc.windows())
    passes = {}
    for name, fn, rw in (("init", acc.init, 2), ("add", acc.add, 3), ("fold", acc.fold, 3)):
        fn()
        torch.cuda.synchronize()
        reps = 50
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        t = e0.elapsed_time(e1) / reps
        passes[name] = {"ms": round(t, 4), "GB": round(rw * 4 * elems / 1e9, 3), "TB_per_s": round(rw * 4 * elems / (t * 1e-3) / 1e12, 2)}
    res = {"workload": "CSN-152 AVA2.1, 2 clips x 32 x %d x %d per micro-batch, captured step" % hw, "rounds": args.rounds,
           "micro_batches_per_block": n, "ms_per_micro": {str(k): round(med[k], 3) for k in ks},
           "ms_per_micro_rounds": {str(k): [round(x, 3) for x in v] for k, v in ms.items()},
           "clips_per_s": {str(k): round(2 * 1e3 / med[k], 1) for k in ks},
           "k8_vs_k1_clips_per_s": round(med[1] / med[8], 4), "k2_vs_k1_clips_per_s": round(med[1] / med[2], 4),
           "trainable_elements": elems, "accum_pass": passes,
           "graph_memory": graph_gb}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
