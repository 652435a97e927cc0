"""Record the launch sequence of the schedule: ``python scripts/launch_sequence.py OUTDIR`` writes OUTDIR/<case>.txt, one line per launch =
the entry-point name and every argument (pointers as 0 / p -- addresses depend on the allocator -- everything else by value); a tuber_gemm_tn_group
line goes on with every TnArgs field of its host entries, a tuber_multi_reduce line with "n stride S mode C next" of every entry of its device table.  Two trees that
launch the same kernels with the same scalar operands produce byte-identical files (``cmp``); which buffer went where is what
``bench.py --dump-outputs`` covers.  Smoke shape: CSN-152 / AVA 2.1, synthetic weights, 2 clips of 32 x 64 x 96, eager steps, fixed seeds.
tests/test_launch_sequence_gpu.py holds the default training step and eval forward to tests/golden/launch_sequence_*.txt (written by this script)."""
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tubelet_transformer_amd import ab, lib, synth  # noqa: E402
from tubelet_transformer_amd.config import load_cfg  # noqa: E402
from tubelet_transformer_amd.engine import DeferredReduce, TnArgs  # noqa: E402
from tubelet_transformer_amd.training import build_optimizer, train_step  # noqa: E402
from tubelet_transformer_amd.tuber import build_model  # noqa: E402

DEV = torch.device("cuda:0")
CFG = load_cfg(os.path.join(ROOT, "configuration", "TubeR_CSN152_AVA21.yaml"))
CLIPS = synth.synthetic_clips(2, 32, 64, 96, seed=3).to(DEV)
TARGETS = synth.synthetic_targets(2, "ava", 80, seed=5, device=DEV, hw=(64, 96))


def record(fn):
    """the launches of ``fn()``, one line each"""
    lines = []
    lib.load()

    def hook(name, args, launch):
        word = lambda v, t: ("0" if v is None or (isinstance(v, int) and v == 0) else "p") if "*" in t or t == "hipStream_t" else repr(v)
        words = [name] + [word(v, t) for v, (t, _) in zip(args, lib._sigs[name])]
        if name == "tuber_gemm_tn_group":        # the host argument block: every TnArgs field of every entry, under the same rule
            for e in args[0][:args[1]]:
                words += [word(getattr(e, k), "*" if c is ctypes.c_void_p else "") for k, c in TnArgs._fields_]
        elif name == "tuber_multi_reduce":       # the device table (eager steps: the copy is allowed); the P / out addresses stay unprinted
            for e in args[0].cpu().numpy().view(DeferredReduce._ENTRY):
                words += [str(int(e[k])) for k in ("n", "stride", "S", "mode", "C", "next")]
        lines.append(" ".join(words))
        return launch(name, *args)
    lib.set_launch_hook(hook)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.set_launch_hook(None)
    return lines


def fresh(frozen=()):
    torch.manual_seed(0)
    model, criterion, _ = build_model(CFG)
    synth.load_name_hashed(model)
    for p in (p for prefix in frozen for n, p in model.backbone.body.named_parameters() if n.startswith(prefix)):
        p.requires_grad = False
    return model.to(DEV).train(), criterion.to(DEV).train()


def step(model, criterion):
    opt = build_optimizer(model, CFG)
    return lambda: train_step(model, criterion, opt, CLIPS, TARGETS, CFG.CONFIG.LOSS_COFS.CLIPS_MAX_NORM)


def fwd_bwd(model, criterion):
    loss_dict = criterion(model(CLIPS), TARGETS)
    model.engine()[0].zero_grad()
    criterion.weighted_total(loss_dict, criterion.weight_dict).backward()


def segment(model, lo=1, hi=5):
    """blocks [1, 5): starts at an identity block of layer1 and crosses into layer2"""
    store, runner = model.engine()
    g = torch.Generator().manual_seed(7)
    store.refresh()
    store.begin_step(True)
    store.zero_grad()
    x = torch.randn(2 * 32 * 16 * 24, 256, generator=g).to(DEV, torch.bfloat16)
    y, _, saved = runner.run_blocks(x, (2, 32, 16, 24), lo, hi, train=True)
    runner.backward_blocks(saved, torch.randn(y.shape, generator=g).to(DEV, torch.bfloat16))


def eval_forward(model, mode):
    os.environ["TUBER_EVAL_PRECISION"] = mode
    try:
        with torch.no_grad():
            model.eval()(CLIPS)
    finally:
        del os.environ["TUBER_EVAL_PRECISION"]


def main(out):
    os.makedirs(out, exist_ok=True)

    def write(case, fn):
        lines = record(fn)
        open(os.path.join(out, case + ".txt"), "w").write("\n".join(lines) + "\n")
        print("%-40s %6d launches" % (case, len(lines)), flush=True)
    write("train", step(*fresh()))
    write("train_pretrained_freeze", step(*fresh(("conv1.", "bn1.", "layer1.", "layer2."))))
    write("train_body_frozen", step(*fresh(("",))))
    # the lowest trainable block stops its chain at every depth: everything below layer4's last block frozen, then that block tensor by tensor
    model, criterion = fresh(("conv1.", "bn1.", "layer1.", "layer2.", "layer3.", "layer4.0.", "layer4.1."))
    last = model.backbone.body.layer4[2]
    for depth, mod in zip(range(6, 0, -1), (None, last.conv1, last.bn1, last.conv3, last.bn3, last.conv4)):
        for p in (mod.parameters() if mod is not None else ()):
            p.requires_grad = False
        write("fwd_bwd_depth%d" % depth, lambda: fwd_bwd(model, criterion))
    for mode in ("fp32_stream", "bf16_stream", "fp32_class"):
        model = fresh()[0]
        write("eval_" + mode, lambda: eval_forward(model, mode))
    model = fresh()[0]
    write("segment_1_5", lambda: segment(model))
    for name in sorted(ab.KNOWN):
        with ab.override(name):
            write("train_ab_" + name, step(*fresh()))


if __name__ == "__main__":
    main(sys.argv[1])
