"""BatchNorm momentum on the MI355X: the module's ``momentum`` (any value, or None = cumulative average) reaches the finalisation kernels
(tuber_bn_finalize_ex, tuber_dwconv_tile_fwd_bn_ex, tuber_bn_count_advance), ``torch.optim.swa_utils.update_bn`` and
``bn_stats.recompute_bn_stats`` produce the plain average of the per-batch statistics, and a captured training step re-captures when a
momentum changes.  Small shapes (2 x 32 x 64 x 96 clips, the CSN-TEST body), dropout off."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tubelet_transformer_amd import lib, synth
from tubelet_transformer_amd.bn_stats import recompute_bn_stats
from tubelet_transformer_amd.config import load_cfg
from tubelet_transformer_amd.training import GraphedTrainStep, build_optimizer, train_step
from tubelet_transformer_amd.tuber import build_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


def _rnd(*shape, dev, seed, scale=1.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(*shape, device=dev, generator=g) * scale


# ------------------------------------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------------------------------------
class _Layer:
    """one BatchNorm layer's device state and a batch generator for the two finalisation kernels"""

    def __init__(self, dev, C, nbt0, shape=None):
        self.dev, self.C = dev, C
        self.gamma, self.beta = 1 + 0.1 * _rnd(C, dev=dev, seed=3), 0.1 * _rnd(C, dev=dev, seed=4)
        self.rm, self.rv = 0.1 * _rnd(C, dev=dev, seed=5), 1 + 0.1 * _rnd(C, dev=dev, seed=6).abs()
        self.nbt = torch.full((1,), nbt0, dtype=torch.int64, device=dev)
        self.outs = [torch.empty(C, device=dev) for _ in range(4)]         # scale, shift, mean, invstd
        self.table = torch.tensor([self.nbt.data_ptr()], dtype=torch.int64).to(dev)
        self.shape = shape                                                 # (N, T, H, W): the depthwise kernel's input

    def batch(self, seed, R):
        """rows x [M, C] (bf16-exact values, per-channel offsets), their R partial rows (sum x, sum x^2) and the fp64 batch statistics"""
        M = int(np.prod(self.shape)) if self.shape else 3000
        x = (_rnd(M, self.C, dev=self.dev, seed=seed, scale=1.5) + 0.3 * _rnd(self.C, dev=self.dev, seed=seed + 1)).to(BF)
        xf = x.float()
        b = torch.linspace(0, M, R + 1).long().tolist()
        p0 = torch.stack([xf[b[i]:b[i + 1]].sum(0) for i in range(R)])
        p1 = torch.stack([(xf[b[i]:b[i + 1]] ** 2).sum(0) for i in range(R)])
        x64 = xf.double()
        return x, p0, p1, M, x64.mean(0), x64.var(0, unbiased=True)

    def finalize(self, name, x, p0, p1, R, M, mom):
        if name.startswith("tuber_bn_finalize"):
            lib.call(name, p0, p1, R, self.C, float(M), self.gamma, self.beta, self.rm, self.rv, self.nbt, mom, 1e-3, *self.outs)
            return None
        N, T, H, W = self.shape
        w = _rnd(self.C, 27, dev=self.dev, seed=2, scale=27 ** -0.5)
        out = torch.empty(N, T, H, W, self.C, device=self.dev, dtype=BF)
        nblk = lib.query("tuber_dwconv_tile_blocks", N, T, H, W, self.C)
        st0, st1 = torch.zeros(nblk, self.C, device=self.dev), torch.zeros(nblk, self.C, device=self.dev)
        lib.call(name, x, p0, p1, R, float(M), self.gamma, self.beta, self.rm, self.rv, self.nbt, mom, 1e-3, *self.outs, w, out, st0, st1,
                 N, T, H, W, self.C)
        return out, st0, st1


# (kernel, C, R, input geometry): C = 2048 -> 64 finalize workgroups; the depthwise launch has 8 channel groups x hundreds of tiles
KERNELS = [("tuber_bn_finalize", 2048, 7, None), ("tuber_bn_finalize", 2048, 300, None),
           ("tuber_dwconv_tile_fwd_bn", 512, 88, (2, 8, 16, 22)), ("tuber_dwconv_tile_fwd_bn", 256, 150, (1, 4, 32, 44))]


@pytest.mark.parametrize("kernel,C,R,shape", KERNELS)
@pytest.mark.parametrize("nbt0", [0, 7])
def test_cumulative_mode_matches_torch_over_three_batches(dev, kernel, C, R, shape, nbt0):
    """momentum=None: factor 1 / (n + 1) from the counter BEFORE the batch, the counter left alone by the finalisation and advanced by
    tuber_bn_count_advance -- against a float64 model of _BatchNorm.forward (num_batches_tracked += 1, then factor 1 / num_batches_tracked)"""
    L = _Layer(dev, C, nbt0, shape)
    rm, rv = L.rm.double(), L.rv.double()
    n = nbt0
    for k in range(3):
        x, p0, p1, M, mean, var = L.batch(11 + 7 * k, R)
        L.finalize(kernel + "_ex", x, p0, p1, R, M, -1.0)
        torch.cuda.synchronize()
        assert int(L.nbt) == n, "the cumulative finalisation must not write the counter"
        lib.call("tuber_bn_count_advance", L.table, 1)
        n += 1
        f = 1.0 / n
        rm, rv = (1 - f) * rm + f * mean, (1 - f) * rv + f * var
        torch.cuda.synchronize()
        assert int(L.nbt) == n
        for got, want, what in ((L.rm, rm, "running_mean"), (L.rv, rv, "running_var")):
            err = float((got.double() - want).abs().max() / want.abs().max())
            assert err < 5e-6, "%s after batch %d: relative error %.3g" % (what, k + 1, err)


@pytest.mark.parametrize("kernel,C,R,shape", KERNELS[1:3])
@pytest.mark.parametrize("mom", [0.0, 0.3, 1.0])
def test_momentum_is_honoured(dev, kernel, C, R, shape, mom):
    L = _Layer(dev, C, 5, shape)
    rm0, rv0 = L.rm.clone(), L.rv.clone()
    x, p0, p1, M, mean, var = L.batch(21, R)
    L.finalize(kernel + "_ex", x, p0, p1, R, M, mom)
    torch.cuda.synchronize()
    assert int(L.nbt) == 6
    if mom == 0.0:
        assert torch.equal(L.rm, rm0) and torch.equal(L.rv, rv0)
    for got, r0, b in ((L.rm, rm0, mean), (L.rv, rv0, var)):
        want = (1 - mom) * r0.double() + mom * b
        assert float((got.double() - want).abs().max() / want.abs().max()) < 5e-6


@pytest.mark.parametrize("kernel,C,R,shape", KERNELS)
def test_new_export_at_default_momentum_is_the_old_export_bit_for_bit(dev, kernel, C, R, shape):
    res = []
    for name in (kernel, kernel + "_ex"):
        L = _Layer(dev, C, 41, shape)
        x, p0, p1, M, _, _ = L.batch(31, R)
        conv = L.finalize(name, x, p0, p1, R, M, 0.1)
        torch.cuda.synchronize()
        res.append([L.rm, L.rv, L.nbt] + L.outs + list(conv or ()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert int(res[0][2]) == 42


def test_cumulative_mode_checks_its_counter(dev):
    L = _Layer(dev, 64, 0)
    x, p0, p1, M, _, _ = L.batch(1, 4)
    with pytest.raises(RuntimeError):           # the factor comes from the counter: there must be one
        lib.call("tuber_bn_finalize_ex", p0, p1, 4, 64, float(M), L.gamma, L.beta, L.rm, L.rv, None, -1.0, 1e-3, *L.outs)


# ------------------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------------------
def _model(dev):
    cfg = load_cfg(os.path.join(ROOT, "configuration", "TubeR_CSN152_AVA21.yaml"))
    cfg.CONFIG.MODEL.BACKBONE_NAME = "CSN-TEST"
    model, crit, _ = build_model(cfg)
    synth.load_name_hashed(model)
    synth.zero_dropout(model)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.to(dev).train()
    crit.to(dev).train()
    return cfg, model, crit, state


def _clips(i, dev):
    return synth.synthetic_clips(2, 32, 64, 96, seed=40 + i, device=dev)


def _bns(model):
    return {n: m for n, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm3d)}


def _stats(model):
    return {n: (m.running_mean.detach().clone(), m.running_var.detach().clone(), int(m.num_batches_tracked)) for n, m in _bns(model).items()}


def _batch_stats(model, clips):
    """the engine's per-batch statistics of every layer: one train-mode forward with momentum 1.0 (running = batch mean / unbiased var)"""
    bns = _bns(model)
    keep = {n: m.momentum for n, m in bns.items()}
    for m in bns.values():
        m.momentum = 1.0
    try:
        with torch.no_grad():
            model(clips)
        torch.cuda.synchronize()
        return _stats(model)
    finally:
        for n, m in bns.items():
            m.momentum = keep[n]


def test_update_bn_gives_the_mean_of_the_per_batch_statistics(dev):
    """torch.optim.swa_utils.update_bn (reset, momentum=None, train-mode forwards) over 3 batches: every layer's running statistics are
    the arithmetic mean of its 3 per-batch statistics (before this change: an EMA with factor 0.1 from zeros / ones)"""
    _, model, _, _ = _model(dev)
    clips = [_clips(i, dev) for i in range(3)]
    per = [_batch_stats(model, c) for c in clips]
    torch.optim.swa_utils.update_bn([(c,) for c in clips], model)
    torch.cuda.synchronize()
    got = _stats(model)
    bad = []
    for n, (rm, rv, nbt) in got.items():
        assert nbt == 3, (n, nbt)
        for i, v in ((0, rm), (1, rv)):
            want = torch.stack([p[n][i].double() for p in per]).mean(0)
            err = float((v.double() - want).abs().max() / max(1.0, float(want.abs().max())))
            if err > 2e-6:
                bad.append((n, i, err))
    assert not bad, "%d of %d layers are not the mean of their batch statistics, e.g. %s" % (len(bad), len(got), bad[:4])
    assert all(m.momentum == 0.1 for m in _bns(model).values())


def test_batch_statistics_at_momentum_one_match_the_oracle(dev):
    """the per-batch statistics the update_bn test averages, pinned against the fp32 oracle's train-mode csn_body (its 0.1 update undone:
    b = (r1 - 0.9 r0) / 0.1) with the yardstick of the full-size running-statistics test (2 x the bf16-rounded oracle's error + 1e-2)"""
    from oracle import tuber_oracle as O
    from parity_util import RoundBF
    import torch.nn.functional as F
    cfg, model, _, state = _model(dev)
    clips = _clips(0, dev)
    got = _batch_stats(model, clips)
    x = clips.cpu()
    st2 = {k: v.clone() for k, v in state.items()}
    st3 = {k: v.clone() for k, v in state.items()}
    with torch.no_grad():
        O.csn_body(st2, "backbone.body", x, "CSN-TEST", cfg.CONFIG.MODEL.LAST_STRIDE, True)
        oc = F.conv3d
        O.F.conv3d = lambda x_, w, *a, **k: RoundBF.apply(oc(RoundBF.apply(x_), RoundBF.apply(w), *a, **k))
        try:
            O.csn_body(st3, "backbone.body", x, "CSN-TEST", cfg.CONFIG.MODEL.LAST_STRIDE, True)
        finally:
            O.F.conv3d = oc
    worst, yard = 0.0, 0.0
    for n, (rm, rv, _) in got.items():
        for i, (v, key) in enumerate(((rm, "running_mean"), (rv, "running_var"))):
            k = "%s.%s" % (n, key)
            r0 = state[k].double()
            b = (st2[k].double() - 0.9 * r0) / 0.1
            b3 = (st3[k].double() - 0.9 * r0) / 0.1
            sc = max(1.0, float(b.abs().max()))
            worst = max(worst, float((v.double().cpu() - b).abs().max()) / sc)
            yard = max(yard, float((b3 - b).abs().max()) / sc)
    print("batch statistics: worst relative error hip %.3e / bf16-rounded oracle %.3e" % (worst, yard))
    assert worst <= 2.0 * yard + 1e-2


def test_recompute_bn_stats_leaves_the_model_as_a_checkpoint_load_would(dev):
    cfg, model, crit, state = _model(dev)
    store, _ = model.engine()
    flat0 = store.flat.detach().clone()
    _bns(model)["backbone.body.layer2.0.bn3"].momentum = 0.05               # a non-default momentum comes back too
    clips = [_clips(i, dev) for i in range(4)]
    per = [_batch_stats(model, c) for c in clips[:3]]
    n = recompute_bn_stats(model, clips, num_batches=3)
    torch.cuda.synchronize()
    assert n == 3
    assert torch.equal(store.flat, flat0), "weights touched"
    moms = {k: m.momentum for k, m in _bns(model).items()}
    assert moms.pop("backbone.body.layer2.0.bn3") == 0.05 and set(moms.values()) == {0.1}
    assert model.training
    after = _stats(model)
    for k, (rm, rv, nbt) in after.items():
        assert nbt == 3
        want = torch.stack([p[k][0].double() for p in per]).mean(0)
        assert float((rm.double() - want).abs().max() / max(1.0, float(want.abs().max()))) <= 2e-6, k
    # an eval forward equals one from a model given the same statistics through load_state_dict
    _, twin, crit2, _ = _model(dev)
    twin.load_state_dict(model.state_dict())
    _bns(twin)["backbone.body.layer2.0.bn3"].momentum = 0.05
    model.eval()
    twin.eval()
    with torch.no_grad():
        a, b = model(clips[3]), twin(clips[3])
    for k in ("pred_logits", "pred_boxes", "pred_logits_b"):
        assert torch.equal(a[k], b[k]), k
    # and a following training step updates the statistics exactly as in that model, which never ran the pass
    model.train()
    twin.train()
    targets = synth.synthetic_targets(2, "ava", 80, seed=9, device=dev, hw=(64, 96))
    for m, c in ((model, crit), (twin, crit2)):
        train_step(m, c, build_optimizer(m, cfg), clips[3], targets, 0.1)
    torch.cuda.synchronize()
    s1, s2 = _stats(model), _stats(twin)
    for k in s1:
        assert torch.equal(s1[k][0], s2[k][0]) and torch.equal(s1[k][1], s2[k][1]) and s1[k][2] == s2[k][2] == 4, k


def test_no_grad_train_forward_updates_the_statistics_like_a_recorded_one(dev):
    _, model, _, state = _model(dev)
    clips = _clips(1, dev)
    model(clips)
    torch.cuda.synchronize()
    rec = _stats(model)
    model.load_state_dict(state)
    with torch.no_grad():
        model(clips)
    torch.cuda.synchronize()
    for k, v in _stats(model).items():
        assert torch.equal(v[0], rec[k][0]) and torch.equal(v[1], rec[k][1]) and v[2] == rec[k][2] == 1, k


def test_graphed_step_recaptures_when_a_momentum_changes(dev):
    """eager and captured sequences with a momentum change after step 1 and back after step 2: identical bit for bit; the changed step
    runs a new graph, the step back at 0.1 replays the first one"""
    frozen_layer, cum_layer = "backbone.body.layer1.1.bn1", "backbone.body.bn1"      # the depthwise-fused finalisation / tuber_bn_finalize
    results = []
    for graphed in (False, True):
        cfg, model, crit, _ = _model(dev)
        opt = build_optimizer(model, cfg)
        store, _ = model.engine()
        store.manual_seed(321)
        step = GraphedTrainStep(model, crit, opt, 0.1) if graphed else None
        bns = _bns(model)
        seq = []
        for i in range(3):
            if i == 1:
                bns[frozen_layer].momentum, bns[cum_layer].momentum = 0.0, None
            if i == 2:
                bns[frozen_layer].momentum = bns[cum_layer].momentum = 0.1
            before = _stats(model)
            targets = synth.synthetic_targets(2, "ava", 80, seed=70 + i, device=dev, hw=(64, 96))
            if graphed:
                step(_clips(i, dev), targets)
            else:
                train_step(model, crit, opt, _clips(i, dev), targets, 0.1)
            torch.cuda.synchronize()
            after = _stats(model)
            seq.append(after)
            if i == 1:
                assert torch.equal(after[frozen_layer][0], before[frozen_layer][0]), "momentum 0.0 must leave the statistics as they were"
                assert after[frozen_layer][2] == before[frozen_layer][2] + 1 and after[cum_layer][2] == before[cum_layer][2] + 1
            else:
                assert not torch.equal(after[frozen_layer][0], before[frozen_layer][0])
            if graphed:
                assert len(step.graphs) == (1 if i == 0 else 2), (i, list(step.graphs))
        if graphed:
            assert (tuple(_clips(0, dev).shape), store.trainable_signature(), True, 16, False) in step.graphs
        results.append((seq, store.flat.detach().clone()))
    (s0, f0), (s1, f1) = results
    assert torch.equal(f0, f1)
    for i in range(3):
        for k in s0[i]:
            assert torch.equal(s0[i][k][0], s1[i][k][0]) and torch.equal(s0[i][k][1], s1[i][k][1]) and s0[i][k][2] == s1[i][k][2], (i, k)


# ------------------------------------------------------------------------------------------------------------------------------
# world size 2 on ONE GPU (gloo, both ranks on cuda:0): both ranks end with the mean of their cumulative averages
# ------------------------------------------------------------------------------------------------------------------------------
_WORKER = r"""
import os, sys, numpy as np, torch, torch.distributed as dist
root, port, rank, out = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
sys.path.insert(0, root)
from tubelet_transformer_amd import synth
from tubelet_transformer_amd.bn_stats import recompute_bn_stats
from tubelet_transformer_amd.config import load_cfg
from tubelet_transformer_amd.input_pipeline import ClipBatch, FrameClip
from tubelet_transformer_amd.tuber import build_model
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
cfg = load_cfg(os.path.join(root, "configuration", "TubeR_CSN152_AVA21.yaml"))
cfg.CONFIG.MODEL.BACKBONE_NAME = "CSN-TEST"
model, crit, _ = build_model(cfg)
synth.load_name_hashed(model)
synth.zero_dropout(model)
model.to(dev).eval()
rng = np.random.default_rng(100 + rank)
items = [(ClipBatch([FrameClip(rng.integers(0, 256, (32, 64, 96, 3), dtype=np.uint8)) for _ in range(2)]), [{}, {}]) for _ in range(3)]
stats = lambda: {n: (b.detach().cpu().clone()) for n, b in model.named_buffers() if "running_" in n or "num_batches" in n}
n_local = recompute_bn_stats(model, items, num_batches=2)
local = stats()
os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", port
dist.init_process_group("gloo", rank=rank, world_size=2)
n = recompute_bn_stats(model, items, num_batches=2)
torch.save({"n": (n_local, n), "local": local, "got": stats(), "training": model.training,
            "momenta": sorted({m.momentum for m in model.modules() if isinstance(m, torch.nn.BatchNorm3d)})}, out + ".%d" % rank)
dist.barrier()
dist.destroy_process_group()
"""


def test_world2_recompute_bn_stats_averages_over_the_ranks(tmp_path, dev):
    script = str(tmp_path / "w2bn.py")
    open(script, "w").write(_WORKER)
    port = str(29650 + os.getpid() % 150)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", TUBER_SHARE_GPU="1")
    for k in ("TUBER_RCCL_IN_GRAPH", "TUBER_DDP_BF16", "TUBER_FORCE_DDP", "TUBER_NO_SPLIT_GRAPH"):
        env.pop(k, None)
    out = str(tmp_path / "res")
    procs = [subprocess.Popen([sys.executable, script, ROOT, port, str(r), out], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = [p.communicate(timeout=900)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-3000:] for l in logs)
    res = [torch.load(out + ".%d" % r) for r in range(2)]
    for r in res:
        assert r["n"] == (2, 2) and r["training"] is False and r["momenta"] == [0.1]
    for k, v0 in res[0]["got"].items():
        v1 = res[1]["got"][k]
        assert torch.equal(v0, v1), k
        if "num_batches" in k:
            assert int(v0) == 2, k
            continue
        a, b = res[0]["local"][k], res[1]["local"][k]
        assert not torch.equal(a, b), k                                # the ranks saw different clips
        want = (a.double() + b.double()) / 2
        assert float((v0.double() - want).abs().max() / max(1.0, float(want.abs().max()))) <= 1e-6, k
