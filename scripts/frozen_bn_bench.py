"""Cost of frozen BatchNorm (CONFIG.MODEL.FREEZE_BN, bn_stats.freeze_batchnorm) on the default workload (CSN-152 AVA 2.1, 2 clips of
32 x 256 x 340, the captured hipGraph step, dropout on): ms per step of four configurations of ONE model, measured as same-process
interleaved rounds (every round times each configuration once, in rotating order, after its own warm-up replays):

    a  default                          every tensor trains, every BatchNorm in train mode
    b  pretrained freeze                stem + layer1 + layer2 frozen by requires_grad, BatchNorm in train mode (today's recipe)
    c  b + FREEZE_BN: frozen            ... and their BatchNorm layers frozen
    d  FREEZE_BN: all                   every tensor trains, every backbone BatchNorm frozen

plus the launches of one eager step of each.  Acceptance: c is not slower than b and d not slower than a by more than the spread (the
largest max - min of one configuration in this run).

    python scripts/frozen_bn_bench.py [--rounds 3] [--steps 60] [--warmup 5] [--out profiles/frozen_bn_bench.json]
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
from tubelet_transformer_amd.bn_stats import freeze_batchnorm  # noqa: E402
from tubelet_transformer_amd.config import load_cfg  # noqa: E402
from tubelet_transformer_amd.misc import NestedTensor  # noqa: E402
from tubelet_transformer_amd.training import GraphedTrainStep, build_optimizer, deploy_model, train_step  # noqa: E402
from tubelet_transformer_amd.tuber import build_model  # noqa: E402

CONFIGS = {"a_default": (False, "none"), "b_pretrained_freeze": (True, "none"), "c_pretrained_freeze_bn_frozen": (True, "frozen"),
           "d_bn_all_frozen": (False, "all")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=340)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frozen_bn_bench.json"))
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
    body = model.backbone.body
    low = [p for mod in (body.conv1, body.bn1, body.layer1, body.layer2) for p in mod.parameters()]
    bns = [m for m in body.modules() if isinstance(m, torch.nn.BatchNorm3d)]

    def select(name):
        freeze, policy = CONFIGS[name]
        for p in low:
            p.requires_grad = not freeze
        for m in bns:
            m.training = True
        freeze_batchnorm(model, policy)
        return sum(1 for m in bns if not m.training)

    # launches of one eager step per configuration
    launches, frozen_layers = {}, {}
    for name in CONFIGS:
        frozen_layers[name] = select(name)
        count = [0]

        def hook(entry, a, launch):
            count[0] += 1
            return launch(entry, *a)
        lib.set_launch_hook(hook)
        try:
            train_step(model, crit, opt, clips, targets, max_norm)
            torch.cuda.synchronize()
        finally:
            lib.set_launch_hook(None)
        launches[name] = count[0]
    step = GraphedTrainStep(model, crit, opt, max_norm, max_graphs=len(CONFIGS))
    resident = {}
    for name in CONFIGS:                                  # capture + the batch resident in the buffers each captured step reads
        select(name)
        step(clips, targets)
        torch.cuda.synchronize()
        bufs = step.input_buffers(clips.shape)
        resident[name] = NestedTensor(bufs[0], bufs[1])
    assert len(step.graphs) == len(CONFIGS), list(step.graphs)
    model.engine()[0].check_coop()
    names = list(CONFIGS)
    ms = {n: [] for n in names}
    for r in range(args.rounds):
        for name in names[r % len(names):] + names[:r % len(names)]:
            select(name)
            for _ in range(args.warmup):
                step(resident[name], targets)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                loss, _ = step(resident[name], targets)
            e1.record()
            e1.synchronize()
            assert bool(torch.isfinite(loss)), (name, loss)
            ms[name].append(e0.elapsed_time(e1) / args.steps)
    assert len(step.graphs) == len(CONFIGS), "a configuration was captured again inside the timed rounds"
    model.engine()[0].check_coop()
    stat = {n: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "rounds_ms": [round(x, 4) for x in v],
                "launches_per_eager_step": launches[n], "frozen_bn_layers": frozen_layers[n]} for n, v in ms.items()}
    spread = max(max(v) - min(v) for v in ms.values())
    med = {n: statistics.median(v) for n, v in ms.items()}
    res = {"workload": "CSN-152 AVA2.1, 2 clips x 32 x %d x %d, captured step, dropout on" % hw, "rounds": args.rounds, "steps": args.steps,
           "warmup": args.warmup, "configurations": stat, "spread_ms": round(spread, 4),
           "c_minus_b_ms": round(med["c_pretrained_freeze_bn_frozen"] - med["b_pretrained_freeze"], 4),
           "d_minus_a_ms": round(med["d_bn_all_frozen"] - med["a_default"], 4),
           "accepted": bool(med["c_pretrained_freeze_bn_frozen"] <= med["b_pretrained_freeze"] + spread and med["d_bn_all_frozen"] <= med["a_default"] + spread),
           "lib_md5": hashlib.md5(open(lib.LIBPATH, "rb").read()).hexdigest()[:12]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
