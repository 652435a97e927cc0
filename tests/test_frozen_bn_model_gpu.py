"""Frozen BatchNorm through the model: a backbone BatchNorm whose module is in eval mode inside a training step normalises with its running
statistics, never writes them and back-propagates dx = gamma * invstd * dz (F.batch_norm(training=False) under autograd, reference
ir_CSN_152.py:46,56,64,119,154).  The oracle is patched at run time (its ``batch_norm`` gets ``train and p not in frozen``), the way
parity_util.run_oracle patches ``O.F.conv3d``."""
import importlib.util
import math
import os
import time

import pytest
import torch

from parity_util import compare_gradients, grad_row, host_mem_gb, output_errors, report, rounded_convs, run_oracle, surrogate
from tubelet_transformer_amd import ab, synth
from tubelet_transformer_amd.bn_stats import freeze_batchnorm
from tubelet_transformer_amd.config import load_cfg
from tubelet_transformer_amd.training import GraphedTrainStep, _frozen, build_optimizer, train_step
from tubelet_transformer_amd.tuber import build_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "configuration", "TubeR_CSN152_AVA21.yaml")
LOW = ("backbone.body.conv1.", "backbone.body.bn1.", "backbone.body.layer1.", "backbone.body.layer2.")


def _model(dev, body="CSN-TEST", dropout=False, policy="none"):
    cfg = load_cfg(YAML)
    if body:
        cfg.CONFIG.MODEL.BACKBONE_NAME = body
    cfg.CONFIG.MODEL.FREEZE_BN = policy
    model, crit, _ = build_model(cfg)
    synth.load_name_hashed(model)
    if not dropout:
        synth.zero_dropout(model)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.to(dev).train()
    crit.to(dev).train()
    return cfg, model, crit, state


def _bns(model):
    return {n: m for n, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm3d)}


def _stats(model):
    return {n: (m.running_mean.detach().clone(), m.running_var.detach().clone(), m.num_batches_tracked.detach().clone()) for n, m in _bns(model).items()}


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _freeze(model, names):
    for n in names:
        model.get_submodule(n).eval()


class frozen_oracle:
    """context: the oracle's BatchNorm layers named in ``frozen`` run in eval mode whatever the forward's ``train`` flag says;
    ``momentum``: the oracle's BatchNorm momentum meanwhile"""

    def __init__(self, frozen, momentum=None):
        self.frozen, self.momentum = set(frozen), momentum

    def __enter__(self):
        from oracle import tuber_oracle as O
        self.O, self.orig, self.mom = O, O.batch_norm, O.BN_MOMENTUM
        orig, frozen = self.orig, self.frozen
        O.batch_norm = lambda state, p, x, train: orig(state, p, x, train and p not in frozen)
        if self.momentum is not None:
            O.BN_MOMENTUM = self.momentum
        return self

    def __exit__(self, *exc):
        self.O.batch_norm, self.O.BN_MOMENTUM = self.orig, self.mom
        return False


# ------------------------------------------------------------------------------------------------------------------------------
# 1. buffers: eager and captured steps, gradient accumulation, a flag flipped after the capture
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accum", [1, 2])
def test_frozen_layers_keep_their_buffers_in_eager_and_captured_steps(dev, accum):
    """CSN-TEST body, 2 x 3x32x64x96, a mixed frozen set covering all five BatchNorm roles (affine parameters trainable): after 3 eager and 3
    captured optimisation steps every frozen layer's running_mean / running_var / num_batches_tracked are bit-unchanged and every other
    layer's moved.  One more layer put into eval mode after the capture: its buffers stop moving from the next step (a new graph)."""
    from tubelet_transformer_amd.accum import GradAccumulator
    cfg, model, crit, _ = _model(dev, dropout=True)
    bns = _bns(model)
    names = list(bns)
    frozen = ["backbone.body.bn1", "backbone.body.layer1.0.bn3", "backbone.body.layer1.0.down_sample.1", "backbone.body.layer1.1.bn1",
              "backbone.body.layer2.0.bn4", "backbone.body.layer2.1.bn3", "backbone.body.layer3.0.bn1", "backbone.body.layer3.0.down_sample.1",
              "backbone.body.layer3.1.bn4", "backbone.body.layer4.1.bn1", "backbone.body.layer4.1.bn3", "backbone.body.layer4.1.bn4"]
    late = "backbone.body.layer2.0.bn1"
    assert set(frozen) < set(names) and late not in frozen
    _freeze(model, frozen)
    bns["backbone.body.layer4.1.bn3"].momentum = None          # whatever the momentum: a frozen layer's counter does not advance either
    opt = build_optimizer(model, cfg)
    store, _ = model.engine()
    store.manual_seed(11)
    first = _stats(model)

    def batch(i):
        return (synth.synthetic_clips(2, 32, 64, 96, seed=40 + i, device=dev),
                synth.synthetic_targets(2, "ava", 80, seed=70 + i, device=dev, hw=(64, 96)))

    def check(before, tag, frozen_now):
        after = _stats(model)
        for n in names:
            if n in frozen_now:
                assert _same(after[n], first[n]), (tag, "frozen layer wrote its buffers", n)
            else:
                assert not torch.equal(after[n][0], before[n][0]) and not torch.equal(after[n][1], before[n][1]), (tag, "train-mode layer did not move", n)
                assert int(after[n][2]) > int(before[n][2]), (tag, n)
        return after

    acc = GradAccumulator(store, accum) if accum > 1 else None
    i = 0
    for s in range(3):
        before = _stats(model)
        for _ in range(accum):
            clips, targets = batch(i)
            i += 1
            loss, _ = train_step(model, crit, opt, clips, targets, 0.1, **({"accum": acc} if acc else {}))
        torch.cuda.synchronize()
        assert math.isfinite(float(loss))
        check(before, "eager step %d" % s, frozen)
    step = GraphedTrainStep(model, crit, opt, 0.1, **({"accum_steps": accum} if accum > 1 else {}))
    for s in range(3):
        before = _stats(model)
        for _ in range(accum):
            clips, targets = batch(i)
            i += 1
            loss, _ = step(clips, targets)
        torch.cuda.synchronize()
        assert math.isfinite(float(loss))
        check(before, "captured step %d" % s, frozen)
    ngraphs = len(step.graphs)
    assert all(_frozen(k) and len(_frozen(k)[1]) == len(frozen) for k in step.graphs), list(step.graphs)
    # one more layer frozen after the capture: from the next step on its buffers stand still -> a new graph was captured
    bns[late].eval()
    held = _stats(model)[late]
    for s in range(2):
        before = _stats(model)
        for _ in range(accum):
            clips, targets = batch(i)
            i += 1
            step(clips, targets)
        torch.cuda.synchronize()
        after = _stats(model)
        assert _same(after[late], held), "the layer frozen after the capture still moves: the old graph was replayed"
        for n in names:
            if n in frozen:
                assert _same(after[n], first[n]), n
            elif n != late:
                assert not torch.equal(after[n][0], before[n][0]), n
    assert len(step.graphs) > ngraphs
    # and back: unfreezing takes effect in the next step too
    bns[late].train()
    step(*batch(i))
    torch.cuda.synchronize()
    assert not torch.equal(_stats(model)[late][0], held[0])
    for p in model.parameters():
        assert p.grad is None or bool(torch.isfinite(p.grad).all())


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the forward of an all-frozen body IS the eval forward
# ------------------------------------------------------------------------------------------------------------------------------
def test_all_frozen_training_forward_equals_the_eval_path(dev, monkeypatch):
    """every BatchNorm frozen: the training-mode backbone features (the whole forward: stem + all blocks; and run_blocks over all blocks on
    the stem's output) are bit-identical to the eval forward with the bf16 residual stream (TUBER_EVAL_PRECISION=bf16_stream) on the
    same input -- the same kernels with the same constant affine maps; buffers untouched; momentum plays no part"""
    monkeypatch.setenv("TUBER_EVAL_PRECISION", "bf16_stream")
    cfg, model, _, _ = _model(dev)
    store, runner = model.engine()
    clips = synth.synthetic_clips(2, 32, 64, 96, seed=9, device=dev)
    store.refresh()
    store.begin_step(False)
    with torch.no_grad():
        want, _ = runner.forward(clips, False)
        want = want.clone()
    first = _stats(model)
    assert freeze_batchnorm(model, "all") == list(_bns(model))
    _bns(model)["backbone.body.layer3.0.bn3"].momentum = None
    store.begin_step(True)
    got, saved = runner.forward(clips, True)
    torch.cuda.synchronize()
    assert torch.equal(got, want), "all-frozen training forward differs from the eval forward on %d elements" % int((got != want).sum())
    assert all(_same(a, first[n]) for n, a in _stats(model).items())
    assert len(saved["blocks"]) == len(runner.blocks) and all(s is not None for s in saved["blocks"])      # everything trains: everything is kept
    # run_blocks over all blocks, from the input the eval forward's first block saw
    x0 = saved["blocks"][0].x
    y, geom, _ = runner.run_blocks(x0, (2, 32, 16, 24), 0, len(runner.blocks), train=True)
    torch.cuda.synchronize()
    assert torch.equal(y.view_as(want), want) and geom == tuple(want.shape[1:4])
    # eval-form trunk: below the lowest trainable block an all-frozen block saves nothing (no _Saved, no ReLU mask, no stem argmax)
    for n, p in model.named_parameters():
        if n.startswith(LOW):
            p.requires_grad = False
    got2, saved2 = runner.forward(clips, True)
    torch.cuda.synchronize()
    assert torch.equal(got2, want)
    nlow = len(model.backbone.body.layer1) + len(model.backbone.body.layer2)
    assert all(s is None for s in saved2["blocks"][:nlow]) and all(s is not None for s in saved2["blocks"][nlow:])
    assert saved2["stem"].arg is None and saved2["stem"].clips is None


# ------------------------------------------------------------------------------------------------------------------------------
# 3. teacher-forced gradients at real depth
# ------------------------------------------------------------------------------------------------------------------------------
def _rows(t):
    return t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1]).to(torch.bfloat16).contiguous()


def _unrows(r, like):
    B, C, T, H, W = like.shape
    return r.float().view(B, T, H, W, C).permute(0, 4, 1, 2, 3)


@pytest.mark.parametrize("pattern", ["all", "every_second"])
def test_teacher_forced_frozen_bottleneck_gradients_at_real_depth(dev, pattern):
    """test_teacher_forced_bottleneck_gradients_at_real_depth with frozen BatchNorm layers (all of them / every second one in module
    order), affine parameters trainable: CSN-152, 2 x 3x32x256x340 (1 clip under 100 GB of host memory), the same 50 single-block + 13
    multi-block segments and the same gates -- relerr(hip) <= 2 x relerr(rounded oracle) + 0.05, at most 0.5 % of the tensors between 2x
    and 3x, none beyond 3x or outside norm ratio (0.5, 2), cos >= 0.9 wherever the rounded oracle has >= 0.95; fixture conditions: rounded
    oracle cos >= 0.99 on >= 95 % of the single-block tensors and >= 0.9 on every multi-block tensor.  The running statistics are first set
    to the statistics of the same clips (one no_grad train-mode oracle pass at momentum 1), so frozen layers see the activations they
    were calibrated on."""
    from oracle import tuber_oracle as O
    B = 2 if host_mem_gb() > 100 else 1
    cfg, model, _, state = _model(dev, body=None)
    P = "backbone.body"
    bn_names = [n for n in _bns(model) if n.startswith(P + ".")]
    assert len(bn_names) == 155
    frozen = bn_names if pattern == "all" else bn_names[::2]
    clips = synth.synthetic_clips(B, 32, 256, 340, seed=1234)
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    # --- calibration: running statistics := the statistics of these clips, in the oracle and in the HIP model -------------------------
    bstate = {k: v.clone() for k, v in state.items() if k.startswith(P + ".")}
    with torch.no_grad(), frozen_oracle((), momentum=1.0):
        O.csn_body(bstate, P, clips, "CSN-152", cfg.CONFIG.MODEL.LAST_STRIDE, True)
    model.load_state_dict({k: v for k, v in bstate.items() if "running" in k or "num_batches" in k}, strict=False)
    _freeze(model, frozen)
    store, runner = model.engine()
    assert len(runner.frozen_signature()) == len(frozen)
    pn = [k for k in bstate if "running" not in k and "num_batches" not in k]
    held = {n: tuple(t.clone() for t in _stats(model)[n]) for n in frozen}
    # --- fp32 oracle, whole body, capturing (x_i, dy_i, dx_i) of every bottleneck ------------------------------------------------
    recs = []
    orig = O.bottleneck

    def capture(st, p, x, stride, tstride, has_ds, train):
        y = orig(st, p, x, stride, tstride, has_ds, train)
        rec = {"p": p, "x": x.detach(), "args": (stride, tstride, has_ds)}
        y.register_hook(lambda g, rec=rec: rec.__setitem__("dy", g.detach().clone()))
        x.register_hook(lambda g, rec=rec: rec.__setitem__("dx", g.detach().clone()))
        recs.append(rec)
        return y
    st32 = {k: (v.clone().requires_grad_(True) if k in pn else v.clone()) for k, v in bstate.items()}
    t0 = time.time()
    O.bottleneck = capture
    try:
        with frozen_oracle(frozen):
            feat = O.csn_body(st32, P, clips, "CSN-152", cfg.CONFIG.MODEL.LAST_STRIDE, True)
            (feat * torch.randn(feat.shape, generator=torch.Generator().manual_seed(5))).sum().backward()
    finally:
        O.bottleneck = orig
    g32 = {k: st32[k].grad for k in pn}
    del feat
    assert len(recs) == 50 and all("dy" in r and "dx" in r for r in recs)
    print("fp32 oracle body fwd+bwd (%s frozen) with per-block capture: %.1f s" % (pattern, time.time() - t0))
    segs = [(i, i + 1) for i in range(50)] + [(0, 3), (3, 7), (7, 11)] + [(11 + 4 * k, 15 + 4 * k) for k in range(9)] + [(47, 50)]
    rows, worse, weak = [], [], []
    store.refresh()
    t0 = time.time()
    for lo, hi in segs:
        names = [k for k in pn if any(k.startswith(recs[i]["p"] + ".") for i in range(lo, hi))]
        stb = {k: (v.clone().requires_grad_(True) if k in names else v.clone()) for k, v in bstate.items()
               if any(k.startswith(recs[i]["p"] + ".") for i in range(lo, hi))}
        xb = recs[lo]["x"].to(torch.bfloat16).float().requires_grad_(True)
        with rounded_convs(), frozen_oracle(frozen):
            yb = xb
            for i in range(lo, hi):
                yb = orig(stb, recs[i]["p"], yb, *recs[i]["args"], True)
            yb.backward(recs[hi - 1]["dy"].to(torch.bfloat16).float())
        x = recs[lo]["x"]
        store.begin_step(True)
        store.zero_grad()
        y, _, saved = runner.run_blocks(_rows(x).to(dev), (x.shape[0], x.shape[2], x.shape[3], x.shape[4]), lo, hi, train=True)
        dx = runner.backward_blocks(saved, _rows(recs[hi - 1]["dy"]).to(dev))
        torch.cuda.synchronize()
        params = dict(model.named_parameters())
        tag = "block %d" % lo if hi == lo + 1 else "blocks %d-%d" % (lo, hi - 1)
        items = [(n, params[n].grad, g32[n], stb[n].grad) for n in names] + [(recs[lo]["p"] + ".dx", _unrows(dx.cpu(), x), recs[lo]["dx"], xb.grad)]
        for n, h, a, b in items:
            assert h is not None, (tag, n)                 # no tensor may be left out
            ch, cb, eh, eb, nr = grad_row(h, a, b)
            rows.append((ch, cb, eh, eb, nr, tag + " " + n))
            if eh > 2.0 * eb + 0.05 or not (0.5 < nr < 2.0):
                worse.append((tag, n, "cos %.4f/%.4f" % (ch, cb), "relerr %.3f/%.3f" % (eh, eb), "norm %.3f" % nr,
                              eh > 3.0 * eb + 0.05 or not (0.5 < nr < 2.0)))
            if cb >= 0.95 and ch < 0.9:
                weak.append((tag, n, ch, cb))
    print("50 single-block + %d multi-block teacher-forced segments: %.1f s" % (len(segs) - 50, time.time() - t0))
    rows.sort()
    report(rows, "CSN-152 %dx3x32x256x340 teacher-forced bottlenecks, %s frozen" % (B, pattern))
    single = [r for r in rows if r[5].startswith("block ")]
    multi = [r for r in rows if r[5].startswith("blocks ")]
    good = sum(1 for r in single if r[1] >= 0.99)
    print("   rounded oracle: cos >= 0.99 on %d of %d single-block tensors; min cos over the %d multi-block tensors %.4f; worst rounded relerr %.3f"
          % (good, len(single), len(multi), min(r[1] for r in multi), max(r[3] for r in rows)))
    print("   outside 2x (+0.05): %d of %d tensors: %s" % (len(worse), len(rows), [w[:5] for w in worse[:8]]))
    assert len(single) == 50 * 9 + 4 * 3 + 50 and len(multi) == len(single) - 50 + 13          # 512 single-block tensors; no tensor is left out
    assert good >= 0.95 * len(single), (good, len(single))
    assert min(r[1] for r in multi) >= 0.9
    assert len(worse) <= 0.005 * len(rows), "teacher-forced gradients worse than 2x the bf16-rounded oracle (+0.05): %s" % worse[:20]
    assert not [w for w in worse if w[5]], "teacher-forced gradients worse than 3x the bf16-rounded oracle (+0.05) or off in norm: %s" % [w for w in worse if w[5]][:20]
    assert not weak, weak[:10]
    now = _stats(model)
    assert all(_same(now[n], held[n]) for n in frozen), "a frozen layer wrote its running statistics"


# ------------------------------------------------------------------------------------------------------------------------------
# 4. whole model, every BatchNorm frozen
# ------------------------------------------------------------------------------------------------------------------------------
def test_whole_model_all_frozen_backward_per_parameter(dev):
    """CSN-TEST body at 2 x 3x32x256x340, name-hashed state as loaded, every body BatchNorm frozen (FREEZE_BN: all), surrogate loss: per
    parameter relerr(hip) <= 2 x relerr(rounded oracle) + 0.05 and norm ratio in (0.5, 2) for all tensors (no conditioning filter), at least
    304 of the 306 tensors graded (the other two have a numerically zero fp32 gradient), outputs within 3 x rounded + 2e-2"""
    cfg, model, _, state = _model(dev, policy="all")
    frozen = [n for n in _bns(model)]
    assert all(not m.training for m in _bns(model).values()) and model.training
    pn = [n for n, _ in model.named_parameters()]
    assert len(pn) == 306
    clips = synth.synthetic_clips(2, 32, 256, 340, seed=1234)
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    with frozen_oracle(frozen):
        o32, g32 = run_oracle(cfg, state, clips, train=True, param_names=pn, loss=surrogate)
        obf, gbf = run_oracle(cfg, state, clips, train=True, rounded=True, param_names=pn, loss=surrogate)
    store, _ = model.engine()
    store.zero_grad()
    first = _stats(model)
    out = model(clips.to(dev))
    surrogate(out).backward()
    torch.cuda.synchronize()
    det = lambda o: {k: (v.detach() if torch.is_tensor(v) else [{kk: vv.detach() for kk, vv in a.items()} for a in v]) for k, v in o.items()}
    errs = output_errors(out, det(o32), det(obf))
    print("all-frozen CSN-TEST body at 2x3x32x256x340, train-mode outputs hip / rounded oracle vs fp32: %s" % {k: "%.2e / %.2e" % v for k, v in errs.items()})
    for kind, (eh, eb) in errs.items():
        assert eh <= 3 * eb + 2e-2, (kind, eh, eb)
    rows, worse = compare_gradients([(n, p.grad) for n, p in model.named_parameters()], g32, gbf, min_cb=None)
    report(rows, "all-frozen shallow body, full resolution")
    print("   worst rounded-oracle relerr %.3f" % max(r[3] for r in rows))
    assert len(rows) >= 304, len(rows)
    assert not worse, "gradients worse than 2x a bf16-rounded oracle (+0.05): %s" % worse[:20]
    assert all(_same(a, first[n]) for n, a in _stats(model).items())


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the pretrained recipe with FREEZE_BN: frozen
# ------------------------------------------------------------------------------------------------------------------------------
def test_pretrained_recipe_with_the_frozen_policy(dev):
    """stem / layer1 / layer2 frozen by requires_grad (what load_csn_mat leaves) + FREEZE_BN: frozen: their parameters have grad None, their
    BatchNorm buffers are bit-unchanged after eager and captured steps, layer3 / layer4 behave as today (statistics move, gradients flow);
    eager and captured sequences agree bit for bit -- the standard of test_graph_replay_tracks_batch_state_like_eager"""
    results = []
    for graphed in (False, True):
        cfg, model, crit, _ = _model(dev, dropout=True, policy="frozen")
        for n, p in model.named_parameters():
            if n.startswith(LOW):
                p.requires_grad = False
        model.train()                                           # the training loop's call: the policy is evaluated here
        bns = _bns(model)
        low = [n for n in bns if (n + ".").startswith(LOW)]
        assert low and [n for n, m in bns.items() if not m.training] == low
        opt = build_optimizer(model, cfg)
        store, _ = model.engine()
        store.manual_seed(321)
        step = GraphedTrainStep(model, crit, opt, 0.1) if graphed else None
        first = _stats(model)
        losses = []
        for i in range(3):
            clips = synth.synthetic_clips(2, 32, 64, 96, seed=50 + i, device=dev)
            targets = synth.synthetic_targets(2, "ava", 80, seed=70 + i, device=dev, hw=(64, 96))
            before = _stats(model)
            model.train()
            loss, _ = step(clips, targets) if graphed else train_step(model, crit, opt, clips, targets, 0.1)
            torch.cuda.synchronize()
            losses.append(float(loss))
            after = _stats(model)
            for n in bns:
                if n in low:
                    assert _same(after[n], first[n]), n
                else:
                    assert not torch.equal(after[n][0], before[n][0]) and int(after[n][2]) == int(before[n][2]) + 1, n
        for n, p in model.named_parameters():
            if n.startswith(LOW):
                assert p.grad is None, n
        if not graphed:
            assert all(p.grad is not None for n, p in model.named_parameters() if ".layer3." in n or ".layer4." in n)
        else:
            assert len(step.graphs) == 1 and _frozen(next(iter(step.graphs)))
        results.append((losses, store.flat.detach().clone(), {k: v.clone() for k, v in model.state_dict().items() if "running" in k}))
    (l0, f0, b0), (l1, f1, b1) = results
    assert all(math.isfinite(v) for v in l0) and l0 == l1
    assert torch.equal(f0, f1), "%d parameters differ" % int((f0 != f1).sum())
    for k in b0:
        assert torch.equal(b0[k], b1[k]), k


# ------------------------------------------------------------------------------------------------------------------------------
# 6. launch counts
# ------------------------------------------------------------------------------------------------------------------------------
def test_frozen_layers_launch_no_statistics_kernels(dev):
    """recorded with scripts/launch_sequence.py's record() (CSN-152, 2 x 3x32x64x96, eager step): with every BatchNorm frozen a training step
    contains no tuber_bn_finalize*, tuber_dwconv_tile_fwd_bn* or tuber_bn_count_advance launch; with the `frozen` policy on the pretrained
    recipe it finalises exactly the 119 BatchNorm layers of layer3 + layer4 (today: all 155) and launches less than the same recipe with
    train-mode BatchNorm; the frozen table is one launch per forward and absent when no layer is frozen"""
    spec = importlib.util.spec_from_file_location("launch_sequence", os.path.join(ROOT, "scripts", "launch_sequence.py"))
    ls = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ls)
    stat = ("tuber_bn_finalize", "tuber_dwconv_tile_fwd_bn", "tuber_bn_count_advance")

    def count(lines, *prefixes):
        return sum(1 for l in lines if l.split()[0].startswith(prefixes))
    low = ("conv1.", "bn1.", "layer1.", "layer2.")
    model, crit = ls.fresh()
    base = ls.record(ls.step(model, crit))
    assert count(base, "tuber_bn_finalize", "tuber_dwconv_tile_fwd_bn") == 155 and count(base, "tuber_bn_frozen") == 0
    assert count(base, "tuber_bn_bwd_fa_frozen", "tuber_dwconv_tile_bwd_data_bn_frozen", "tuber_dwconv_tile_bwd_both_bn_frozen") == 0
    model, crit = ls.fresh()
    for m in _bns(model).values():
        m.momentum = None                                       # (would need tuber_bn_count_advance in train mode)
    freeze_batchnorm(model, "all")
    every = ls.record(ls.step(model, crit))
    assert count(every, *stat) == 0, [l.split()[0] for l in every if l.split()[0].startswith(stat)][:5]
    assert count(every, "tuber_bn_frozen_affine_multi") == 1 and count(every, "tuber_bn_bwd_finalize") == 0
    assert count(every, "tuber_dwconv_tile_bwd_both_bn_frozen") == count(base, "tuber_dwconv_tile_bwd_both_bn") > 0      # no layer fell off the fused path
    assert count(every, "tuber_dwconv_tile_bwd_both_bn") == count(every, "tuber_dwconv_tile_bwd_both_bn_frozen")
    assert len(every) < len(base)
    model, crit = ls.fresh(low)
    recipe = ls.record(ls.step(model, crit))
    model, crit = ls.fresh(low)
    names = freeze_batchnorm(model, "frozen")
    assert len(names) == 155 - 119
    policy = ls.record(ls.step(model, crit))
    assert count(recipe, "tuber_bn_finalize", "tuber_dwconv_tile_fwd_bn") == 155
    assert count(policy, "tuber_bn_finalize", "tuber_dwconv_tile_fwd_bn") == 119 and count(policy, "tuber_bn_frozen_affine_multi") == 1
    assert len(policy) < len(recipe), (len(policy), len(recipe))
    print("launches per eager step: default %d, every BatchNorm frozen %d; pretrained recipe %d, with FREEZE_BN frozen %d"
          % (len(base), len(every), len(recipe), len(policy)))


# ------------------------------------------------------------------------------------------------------------------------------
# 7. the A/B switches that reroute a backbone BatchNorm kernel, on the every-second pattern
# ------------------------------------------------------------------------------------------------------------------------------
AB_BN = ["no_bn_bwd_fa", "no_bn_bwd_fa_after_reduce", "no_bn3_in_dw", "no_dw_bwd_one_launch", "no_bn1_in_dw_fwd", "dw_register_tiled",
         "no_conv4_bwd_fused", "no_proj_bwd_fused", "no_conv1_bwd_fused", "no_join_fusion", "no_entry_conv", "no_blockout_conv1", "no_join_mask"]
_AB_FORWARD = {"dw_register_tiled", "no_blockout_conv1", "no_entry_conv"}
_AB_DEFAULT = {}


def _ab_loss_noise():
    """||outputs(bf16-rounded oracle) - outputs(fp32 oracle)||_2 over every output of this fixture, from the oracle alone.  The surrogate
    loss is a fixed N(0, 1)-weighted sum of the outputs, so an output displacement d moves it like a N(0, ||d||^2) draw: this norm is the
    scale of what a change of the forward's rounding points moves the loss by.  Checked with the oracle on the CPU: 1.40 (the same
    with 4 and 16 threads) at ||outputs|| = 78; the loss itself nearly cancels on the every-second pattern -- fp32 1.43, bf16-rounded 0.77
    with 16 threads / 0.74 with 4 / 0.94 on another host, 1.16 with the gradients rounded too -- so a bound relative to the loss
    (6 % of 39.5 = 2.4 where every layer is in train mode) would grade the cancellation, not the kernels."""
    import numpy as np
    from parity_util import flat_outputs
    cfg = load_cfg(YAML)
    cfg.CONFIG.MODEL.BACKBONE_NAME = "CSN-TEST"
    model = build_model(cfg)[0]
    synth.load_name_hashed(model)
    synth.zero_dropout(model)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    frozen = list(_bns(model))[::2]
    clips = synth.synthetic_clips(2, 32, 64, 96, seed=21)
    with frozen_oracle(frozen):
        o32, _ = run_oracle(cfg, state, clips, train=True)
        obf, _ = run_oracle(cfg, state, clips, train=True, rounded=True)
    a, b = flat_outputs(o32), flat_outputs(obf)
    return float(np.sqrt(sum(float(((a[k] - b[k]) ** 2).sum()) for k in a))), float(surrogate(o32)), float(surrogate(obf))


def _ab_run(dev, names):
    with ab.override(*names):
        cfg, model, crit, _ = _model(dev)
        bn_names = list(_bns(model))
        store, _ = model.engine()
        clips = synth.synthetic_clips(2, 32, 64, 96, seed=21, device=dev)
        # every BatchNorm frozen, training mode: the backbone's forward is the eval path's arithmetic (bit for bit, see
        # test_all_frozen_training_forward_equals_the_eval_path), so these outputs are held like the existing test's eval-mode outputs
        _freeze(model, bn_names)
        with torch.no_grad():
            frz = {k: v.detach().float().clone() for k, v in model(clips).items() if k in ("pred_logits", "pred_boxes", "pred_logits_b")}
        model.train()
        _freeze(model, bn_names[::2])
        store.zero_grad()
        out = model(clips)
        loss = surrogate(out)
        loss.backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None}
        bufs = {n: b.detach().float().clone() for n, b in model.named_buffers() if n.endswith("running_mean")}
        return float(loss.detach()), grads, bufs, frz


@pytest.mark.parametrize("name", AB_BN)
def test_bn_ab_switches_reproduce_the_default_path_with_frozen_layers(dev, name):
    """every second BatchNorm (module order) frozen: each TUBER_AB switch that reroutes a backbone BatchNorm kernel reproduces the default
    path's training-mode gradients and running statistics to the bounds of test_every_ab_switch_reproduces_the_default_path.  The loss:
    1e-4 for the switches that only regroup launches, as there; for the three that move the forward's rounding points the surrogate loss
    of this fixture nearly cancels, so it is held to 2 x the output displacement of the bf16-rounded oracle (_ab_loss_noise: 2 x 1.40,
    about what 6 % is in absolute terms on the all-train fixture) instead of to 6 % of itself -- a bound that wide cannot fail for a
    realistic error, so it only guards against a non-finite or runaway loss; the sharp checks are the gradient bounds and the
    all-frozen training-mode outputs (2e-2 / 1e-6, the existing test's eval-output bound).  (MI355X: default path 1.72,
    dw_register_tiled 1.56, no_entry_conv 0.77 -- the oracle's own executions spread over 0.74 - 1.43.)"""
    assert name in ab.KNOWN
    if not _AB_DEFAULT:
        _AB_DEFAULT["ref"] = _ab_run(dev, ())
        _AB_DEFAULT["noise"] = _ab_loss_noise()
    l0, g0, b0, f0 = _AB_DEFAULT["ref"]
    noise, l32, lbf = _AB_DEFAULT["noise"]
    l1, g1, b1, f1 = _ab_run(dev, (name,))
    fwd = name in _AB_FORWARD
    # training-mode outputs with EVERY BatchNorm frozen against the default path's: the bound of the existing test's eval-output check
    # (2e-2 for the switches that move the forward's rounding points, 1e-6 for the others) -- the direct check on the forward that the
    # nearly-cancelling loss below cannot give
    for k in f0:
        err = float((f1[k] - f0[k]).abs().max())
        print("TUBER_AB=%s, every BatchNorm frozen: %s max |switch - default| = %.3e" % (name, k, err))
        assert err <= (2e-2 if fwd else 1e-6), (k, err)
    print("TUBER_AB=%s, every second BatchNorm frozen: loss %.6f vs %.6f (oracle fp32 %.4f, bf16-rounded %.4f, output displacement %.4f)" % (name, l1, l0, l32, lbf, noise))
    assert math.isfinite(l1) and abs(l1 - l0) <= (2.0 * noise if fwd else 1e-4 * max(abs(l0), 1.0)), (l0, l1, noise)
    assert set(g0) == set(g1)
    rels = []
    gmax = max(float(v.norm()) for v in g0.values())
    for n in g0:
        den = float(g0[n].norm())
        if den < 1e-12:
            continue
        floor = 1e-4 * gmax
        rels.append((float((g1[n] - g0[n]).norm()) / max(den, floor), n))
        if den > floor:
            assert 0.5 < float(g1[n].norm()) / den < 2.0, n
        else:
            assert float(g1[n].norm()) <= 2.0 * floor, (n, float(g1[n].norm()), floor)
    rels.sort(reverse=True)
    med = rels[len(rels) // 2][0]
    print("   median / worst gradient relerr %.2e / %.2e (%s)" % (med, rels[0][0], rels[0][1]))
    if fwd:
        assert med <= 0.15 and rels[0][0] <= 1.0, (med, rels[:3])
    else:
        assert rels[0][0] <= 0.15 and med <= 1e-3, (med, rels[:3])
    for n in b0:
        assert torch.allclose(b0[n], b1[n], rtol=2e-2 if fwd else 1e-5, atol=2e-3 if fwd else 1e-6), n


# ------------------------------------------------------------------------------------------------------------------------------
# 8. partial rows nobody reads are not requested where the producer takes NULL
# ------------------------------------------------------------------------------------------------------------------------------
def test_fully_frozen_bn1_requests_no_rows_from_the_depthwise_data_gradient(dev):
    """every BatchNorm frozen and the depthwise weights frozen (so the data gradient is a launch of its own): with the BatchNorm affine
    parameters frozen too, the LDS-staged data-gradient kernels get NULL statistics rows (bn1 reads none) and bn3's frozen form NULL
    partial rows; every remaining gradient is bit-identical to the run whose affine parameters train (the rows do not enter the data path)"""
    from tubelet_transformer_amd import lib
    runs = []
    for affine in (True, False):
        cfg, model, _, _ = _model(dev, policy="all")
        for n, p in model.named_parameters():
            if ".conv3." in n or (not affine and isinstance(model.get_submodule(n.rsplit(".", 1)[0]), torch.nn.BatchNorm3d)):
                p.requires_grad = False
        store, _ = model.engine()
        clips = synth.synthetic_clips(2, 32, 64, 96, seed=21, device=dev)
        seen = []

        def hook(name, args, launch):
            if name.startswith("tuber_dwconv_tile_bwd_data"):
                seen.append((name, {a: v for v, (_, a) in zip(args, lib._sigs[name])}))
            return launch(name, *args)
        store.zero_grad()
        lib.set_launch_hook(hook)
        try:
            surrogate(model(clips)).backward()
            torch.cuda.synchronize()
        finally:
            lib.set_launch_hook(None)
        # (layer1 at this clip size has too many partial rows for the bn3 fold: its blocks take the plain LDS-staged kernel)
        names = {name for name, _ in seen}
        assert names == {"tuber_dwconv_tile_bwd_data_bn_frozen", "tuber_dwconv_tile_bwd_data"}, names
        for name, a in seen:
            assert (a["st0"] is None) == (not affine) and (a["st1"] is None) == (not affine), name
            if name.endswith("_frozen"):
                assert (a["bst0"] is None) == (not affine) and (a["dgamma"] is None) == (not affine)
        runs.append({n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
    ga, gb = runs
    assert gb and set(gb) < set(ga) and not any(".bn" in n or "down_sample.1" in n for n in gb if n.startswith("backbone."))
    for n in gb:
        assert torch.equal(ga[n], gb[n]), n
