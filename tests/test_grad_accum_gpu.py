"""Gradient accumulation on the device (csrc/grad_accum.hip, accum.py): one k-micro-batch step equals the mean of k independent
2-clip backward passes bit for bit -- eager, captured, with frozen windows, through the training loop and under a world-2 reducer.
Small shapes (2 x 32 x 64 x 96 clips, the CSN-TEST body), dropout off."""
import os

import numpy as np
import pytest
import torch

from tubelet_transformer_amd import lib, synth
from tubelet_transformer_amd.accum import GradAccumulator
from tubelet_transformer_amd.config import load_cfg
from tubelet_transformer_amd.optim import FusedClipAdamW
from tubelet_transformer_amd.training import GraphedTrainStep, build_optimizer, train_step, train_tuber_detection
from tubelet_transformer_amd.tuber import build_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(dev, yaml_name="TubeR_CSN152_AVA21.yaml"):
    cfg = load_cfg(os.path.join(ROOT, "configuration", yaml_name))
    cfg.CONFIG.MODEL.BACKBONE_NAME = "CSN-TEST"
    model, crit, _ = build_model(cfg)
    synth.load_name_hashed(model)
    synth.zero_dropout(model)
    model.to(dev).train()
    crit.to(dev).train()
    return cfg, model, crit


def _batch(i, dev):
    return (synth.synthetic_clips(2, 32, 64, 96, seed=40 + i, device=dev),
            synth.synthetic_targets(2, "ava", 80, seed=60 + i, device=dev, hw=(64, 96)))


def _plain_grad(model, crit, clips, targets):
    store, _ = model.engine()
    out = model(clips)
    loss = crit.weighted_total(crit(out, targets), crit.weight_dict)
    store.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    return store.gflat.detach().clone()


def _freeze_body_bottom(model):
    body = model.backbone.body
    for mod in (body.conv1, body.bn1, body.layer1, body.layer2):
        for p in mod.parameters():
            p.requires_grad = False


def _bn_state(model):
    return {n: b.detach().clone() for n, b in model.named_buffers() if "running_" in n or "num_batches_tracked" in n}


# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dev_scale", [False, True])
def test_kernel_modes_bit_exact_over_odd_windows(dev, mode, dev_scale):
    n = 300_017
    gen = torch.Generator(device=dev).manual_seed(11)
    g0 = torch.randn(n, device=dev, generator=gen)
    a0 = torch.randn(n, device=dev, generator=gen)
    wins = [(1, 6), (13, 100_003), (100_010, 100_011), (150_002, 150_003 + 4 * 1000 + 3), (200_001, n - 3)]
    table = torch.tensor(np.asarray(wins, dtype=np.int64)).to(dev)
    s = 1.0 / 3.0
    scale_dev = torch.tensor([s], dtype=torch.float32, device=dev) if dev_scale else None
    g, a = g0.clone(), a0.clone()
    lib.call("tuber_grad_accum", g, a, table, len(wins), mode, scale_dev, 0.0 if dev_scale else s)
    torch.cuda.synchronize()
    want_g, want_a = g0.clone(), a0.clone()
    for lo, hi in wins:
        if mode == 0:
            want_a[lo:hi] = g0[lo:hi]
        elif mode == 1:
            want_a[lo:hi] = a0[lo:hi] + g0[lo:hi]
        else:
            want_g[lo:hi] = (a0[lo:hi] + g0[lo:hi]) * s
    assert torch.equal(g, want_g)                  # inside the windows, and every byte outside them unchanged
    assert torch.equal(a, want_a)


@pytest.mark.parametrize("k", [2, 3])
def test_eager_fold_is_the_mean_of_plain_backward_passes(dev, k):
    cfg, model, crit = _model(dev)
    store, _ = model.engine()
    batches = [_batch(i, dev) for i in range(k)]
    gs = [_plain_grad(model, crit, c, t) for c, t in batches]
    opt = build_optimizer(model, cfg)
    acc = GradAccumulator(store, k)
    t0 = opt.t
    for i, (c, t) in enumerate(batches):
        train_step(model, crit, opt, c, t, 0.1, accum=acc)
        assert acc.micro == (i + 1) % k
        assert opt.t == t0 + (1 if i == k - 1 else 0)
    torch.cuda.synchronize()
    want = gs[0]
    for g in gs[1:]:
        want = want + g
    want = want * (1.0 / k)
    assert torch.equal(store.gflat, want)


def test_graph_step_matches_eager_and_adamw_on_the_mean(dev):
    batches = [_batch(i, dev) for i in range(2)]
    cfg, me, ce = _model(dev)
    oe = build_optimizer(me, cfg)
    acc = GradAccumulator(me.engine()[0], 2)
    for c, t in batches:
        train_step(me, ce, oe, c, t, 0.1, accum=acc)
    torch.cuda.synchronize()
    _, mg, cg = _model(dev)
    og = build_optimizer(mg, cfg)
    step = GraphedTrainStep(mg, cg, og, 0.1, accum_steps=2)
    for c, t in batches:
        step(c, t)
    torch.cuda.synchronize()
    sg, se = mg.engine()[0], me.engine()[0]
    assert {k[-1] for k in step.graphs} == {"first", "last"}
    assert torch.equal(sg.gflat, se.gflat)
    assert torch.equal(sg.flat, se.flat)
    assert og.t == 1 and oe.t == 1
    be, bg = _bn_state(me), _bn_state(mg)
    assert all(torch.equal(be[n], bg[n]) for n in be)
    # the same AdamW step applied by hand to the mean buffer
    _, mr, cr = _model(dev)
    orf = build_optimizer(mr, cfg)
    sr = mr.engine()[0]
    gs = [_plain_grad(mr, cr, c, t) for c, t in batches]
    with torch.no_grad():
        sr.gflat.copy_((gs[0] + gs[1]) * 0.5)
    FusedClipAdamW.step(orf, max_norm=0.1)
    torch.cuda.synchronize()
    assert torch.equal(sr.flat, sg.flat)


def test_batchnorm_statistics_follow_micro_batch_zero(dev):
    batches = [_batch(i, dev) for i in range(2)]
    cfg, ma, ca = _model(dev)
    with torch.no_grad():
        ma(batches[0][0])
    torch.cuda.synchronize()
    want = _bn_state(ma)
    cfg, mb, cb = _model(dev)
    ob = build_optimizer(mb, cfg)
    acc = GradAccumulator(mb.engine()[0], 2)
    before = _bn_state(mb)
    for c, t in batches:
        train_step(mb, cb, ob, c, t, 0.1, accum=acc)
    torch.cuda.synchronize()
    got = _bn_state(mb)
    assert len(got) > 20
    assert all(torch.equal(got[n], want[n]) for n in want)
    assert any(not torch.equal(got[n], before[n]) for n in got if "running_mean" in n)


def test_frozen_windows_are_never_written(dev):
    batches = [_batch(i, dev) for i in range(2)]
    cfg, model, crit = _model(dev)
    cfg.CONFIG.TRAIN.LR_BACKBONE = 0.0
    _freeze_body_bottom(model)
    store, _ = model.engine()
    gs = [_plain_grad(model, crit, c, t) for c, t in batches]
    opt = build_optimizer(model, cfg)
    acc = GradAccumulator(store, 2)
    acc.acc.fill_(7.0)                             # sentinel: the accumulation buffer outside the trainable windows is never touched
    for c, t in batches:
        train_step(model, crit, opt, c, t, 0.1, accum=acc)
    torch.cuda.synchronize()
    want = (gs[0] + gs[1]) * 0.5
    inside = torch.zeros(store.total, dtype=torch.bool, device=dev)
    for a, b in store.trainable_ranges():
        inside[a:b] = True
    assert not bool(inside.all()) and bool(inside.any())
    assert torch.equal(store.gflat[inside], want[inside])
    assert bool((store.gflat[~inside] == 0).all())
    assert bool((acc.acc[~inside] == 7.0).all())


def test_flush_closes_a_pending_group_with_its_mean(dev):
    batches = [_batch(i, dev) for i in range(2)]
    cfg, model, crit = _model(dev)
    store, _ = model.engine()
    gs = [_plain_grad(model, crit, c, t) for c, t in batches]
    opt = build_optimizer(model, cfg)
    acc = GradAccumulator(store, 3)
    for c, t in batches:                           # two micro-batches of a group of three, then the loader ends
        train_step(model, crit, opt, c, t, 0.1, accum=acc)
    assert opt.t == 0 and acc.micro == 2
    assert acc.flush(lambda: opt.step(max_norm=0.1))
    torch.cuda.synchronize()
    assert torch.equal(store.gflat, (gs[0] + gs[1]) * 0.5)
    assert opt.t == 1 and acc.micro == 0 and acc.steps == 1
    assert not acc.flush(lambda: opt.step(max_norm=0.1))


def test_reallocated_batchnorm_buffers_are_refused(dev):
    cfg, model, crit = _model(dev)
    acc = GradAccumulator(model.engine()[0], 2)
    bn = next(m for m in model.modules() if isinstance(m, torch.nn.BatchNorm3d))
    bn.running_mean = bn.running_mean.clone()      # what a checkpoint load that replaces buffers does
    with pytest.raises(RuntimeError, match="BatchNorm buffers"):
        acc.begin_micro()


def test_captured_fold_precedes_the_all_reduce_on_the_own_rccl_communicator(dev, monkeypatch):
    """the cut-graph step on a forced one-rank RCCL communicator with the default edge mode (a device counter orders the first cut): the
    bytes every all-reduce reads on the transport stream are the FOLDED mean, and the step equals the local fold bit for bit"""
    from tubelet_transformer_amd.ddp import attach_reducer
    for k in ("TUBER_RCCL_IN_GRAPH", "TUBER_DDP_BF16", "TUBER_FORCE_SPLIT_GRAPH", "TUBER_NO_SPLIT_GRAPH", "TUBER_DDP_EDGE", "TUBER_DDP_CUTS"):
        monkeypatch.delenv(k, raising=False)
    batches = [_batch(i, dev) for i in range(2)]
    cfg, model, crit = _model(dev, "TubeR_CSN50_AVA21.yaml")
    store, _ = model.engine()

    def zero_lr(opt):
        for g in opt.param_groups:
            g["lr"] = 0.0
            g["weight_decay"] = 0.0                # parameters stay put: both runs differentiate at the same point
        return opt
    opt = zero_lr(build_optimizer(model, cfg))
    acc = GradAccumulator(store, 2)
    for c, t in batches:
        train_step(model, crit, opt, c, t, 0.1, accum=acc)
    torch.cuda.synchronize()
    want = store.gflat.clone()
    red = attach_reducer(store, force=True)
    try:
        assert red is not None and red.comm is not None and red.world == 1 and red.flag_points() == frozenset([0])
        seen = []
        orig = red.comm.all_reduce

        def spy(ptr, count, bf16=False, stream=None):
            orig(ptr, count, bf16=bf16, stream=stream)
            o = (ptr - store.gflat.data_ptr()) // 4
            with torch.cuda.stream(stream or red.comm.stream):
                seen.append((o, store.gflat[o:o + count].clone()))      # what the transport stream sees, in its own order
        red.comm.all_reduce = spy
        step = GraphedTrainStep(model, crit, zero_lr(build_optimizer(model, cfg)), 0.1, accum_steps=2)
        for c, t in batches:
            step(c, t)
        torch.cuda.synchronize()
        g = step.graphs[next(k for k in step.graphs if k[-1] == "last")]
        assert g.parts and 0 in g.flag_edges       # the cut graph with the counter-ordered first cut
        assert red.issued == sum(b - a for a, b in store.trainable_ranges())
        assert seen and sum(x.numel() for _, x in seen) == red.issued
        for o, x in seen:
            assert torch.equal(x, want[o:o + x.numel()]), "window at %d reached the transport before its fold" % o
        assert torch.equal(store.gflat, want)
    finally:
        red.comm.close()
        store.reducer = None


class _Sched:
    def __init__(self):
        self.calls = []

    def step_update(self, i):
        self.calls.append(i)


@pytest.mark.parametrize("graphed", [False, None])
def test_training_loop_steps_every_k_batches_and_folds_the_partial_group(dev, graphed):
    batches = [_batch(i, dev) for i in range(5)]
    cfg, model, crit = _model(dev)
    cfg.CONFIG.TRAIN.ACCUM_STEPS = 2
    cfg.CONFIG.TRAIN.LR_POLICY = "cosine"
    cfg.DDP_CONFIG.GPU_WORLD_RANK = 0
    opt = build_optimizer(model, cfg)
    sched = _Sched()
    train_tuber_detection(cfg, model, crit, list(batches), opt, 0, 0.1, lr_scheduler=sched, graphed=graphed, print_freq=100)
    torch.cuda.synchronize()
    assert opt.t == 3 and sched.calls == [0, 1, 2]
    _, mr, cr = _model(dev)
    orf = build_optimizer(mr, cfg)
    acc = GradAccumulator(mr.engine()[0], 2)
    for i, (c, t) in enumerate(batches):
        train_step(mr, cr, orf, c, t, 0.1, accum=acc, last=i == len(batches) - 1)
    torch.cuda.synchronize()
    assert orf.t == 3
    assert torch.equal(model.engine()[0].flat, mr.engine()[0].flat)


# ------------------------------------------------------------------------------------------------------------------------------
# world size 2 on ONE GPU (gloo, both ranks on cuda:0), k = 2: each rank's gradient after the group equals the mean over the ranks of
# their local folds, and every trainable window is sent exactly once (only by the last micro-batch)
# ------------------------------------------------------------------------------------------------------------------------------
_WORKER = r"""
import os, sys, torch, torch.distributed as dist
root, port, rank, mode, out = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4], sys.argv[5]
sys.path.insert(0, root)
from tubelet_transformer_amd import synth
from tubelet_transformer_amd.accum import GradAccumulator
from tubelet_transformer_amd.config import load_cfg
from tubelet_transformer_amd.ddp import attach_reducer, broadcast_parameters
from tubelet_transformer_amd.training import GraphedTrainStep, build_optimizer, train_step
from tubelet_transformer_amd.tuber import build_model
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
cfg = load_cfg(os.path.join(root, "configuration", "TubeR_CSN50_AVA21.yaml"))
cfg.CONFIG.MODEL.BACKBONE_NAME = "CSN-TEST"
model, crit, _ = build_model(cfg)
synth.load_name_hashed(model)
synth.zero_dropout(model)
model.to(dev).train(); crit.to(dev).train()
store, _ = model.engine()
batches = [(synth.synthetic_clips(2, 32, 64, 96, seed=3 + 10 * rank + i, device=dev),
            synth.synthetic_targets(2, "ava", 80, seed=5 + 10 * rank + i, device=dev, hw=(64, 96))) for i in range(2)]

def folded(reduced):
    red = store.reducer if reduced else None
    keep, store.reducer = store.reducer, red
    try:
        opt = build_optimizer(model, cfg)
        for g in opt.param_groups:
            g["lr"] = 0.0; g["weight_decay"] = 0.0
        flat0 = store.flat.clone()
        if mode == "graph":
            step = GraphedTrainStep(model, crit, opt, 0.1, accum_steps=2)
            for c, t in batches:
                step(c, t)
        else:
            acc = GradAccumulator(store, 2)
            for c, t in batches:
                train_step(model, crit, opt, c, t, 0.1, accum=acc)
        torch.cuda.synchronize()
        store.flat.copy_(flat0)
        return store.gflat.detach().clone()
    finally:
        store.reducer = keep

local = folded(False)
os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", port
dist.init_process_group("gloo", rank=rank, world_size=2)
broadcast_parameters(store)
red = attach_reducer(store)
assert red is not None and red.comm is None and red.world == 2
got = folded(True)
both = [torch.zeros_like(local).cpu() for _ in range(2)]
dist.all_gather(both, local.cpu())
want = (both[0] + both[1]) * 0.5
torch.save({"got": got.cpu(), "want": want, "issued": red.issued, "trainable": sum(b - a for a, b in store.trainable_ranges()),
            "names": store.names, "offsets": [store.offsets[n] for n in store.names]}, out + ".%d" % rank)
dist.barrier()
dist.destroy_process_group()
"""


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_world2_accumulated_gradients_equal_the_mean_of_the_ranks_folds(tmp_path, dev, mode):
    import subprocess
    import sys
    script = str(tmp_path / "w2a.py")
    open(script, "w").write(_WORKER)
    port = str(29500 + os.getpid() % 150 + (0 if mode == "eager" else 1))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", TUBER_SHARE_GPU="1")
    for k in ("TUBER_RCCL_IN_GRAPH", "TUBER_DDP_BF16", "TUBER_FORCE_DDP", "TUBER_NO_SPLIT_GRAPH"):
        env.pop(k, None)
    out = str(tmp_path / "res")
    procs = [subprocess.Popen([sys.executable, script, ROOT, port, str(r), mode, out], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = [p.communicate(timeout=900)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-3000:] for l in logs)
    for r in range(2):
        res = torch.load(out + ".%d" % r)
        got, want = res["got"], res["want"]
        assert res["issued"] == res["trainable"], (res["issued"], res["trainable"])
        bad = []
        for n, o, e in zip(res["names"], res["offsets"], res["offsets"][1:] + [got.numel()]):
            if not torch.equal(got[o:e], want[o:e]):
                bad.append((n, float((got[o:e] - want[o:e]).abs().max()), float(want[o:e].abs().max())))
        assert not bad, "rank %d: %d tensors differ from the mean of the ranks' folds, e.g. %s" % (r, len(bad), bad[:6])
