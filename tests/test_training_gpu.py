"""Optimizer, frozen-parameter and captured-step semantics of the training path.

  * ``csrc/optim.hip`` (sum-of-squares, clip coefficient, AdamW) against ``torch.nn.utils.clip_grad_norm_`` +
    ``torch.optim.AdamW`` with the reference's four parameter groups (train_tuber_ava.py:41-58,
    utils/video_action_recognition.py:150-154): fp32, <= 1e-6 relative on parameters / moments / clip coefficient;
  * ``requires_grad = False`` parameters (the pretrained recipe freezes stem + layer1 + layer2: ir_CSN_152.py:251-254,301-303):
    no gradient is computed or stored for them, the trainable tensors' gradients are bit-identical to the unfrozen run,
    the clip coefficient ignores them, AdamW leaves them untouched, BatchNorm running statistics keep updating;
  * the captured hipGraph step replays with the CURRENT batch's targets / mask, the current learning rate and loss
    weights, i.e. it is bit-identical to the eager step sequence.
"""
import math
import os

import pytest
import torch

from tubelet_transformer_amd import synth
from tubelet_transformer_amd.config import load_cfg
from tubelet_transformer_amd.training import GraphedTrainStep, build_optimizer, train_step
from tubelet_transformer_amd.tuber import build_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(yaml_name, dev, body="CSN-TEST", dropout=True):
    cfg = load_cfg(os.path.join(ROOT, "configuration", yaml_name))
    if body:
        cfg.CONFIG.MODEL.BACKBONE_NAME = body
    model, crit, _ = build_model(cfg)
    synth.load_name_hashed(model)
    if not dropout:
        synth.zero_dropout(model)
    model.to(dev).train()
    crit.to(dev).train()
    return cfg, model, crit


def _freeze_like_load_csn_mat(model):
    """the requires_grad pattern ``load_csn_mat(tune_point=4)`` leaves behind: stem, layer1, layer2 frozen"""
    body = model.backbone.body
    for mod in (body.conv1, body.bn1, body.layer1, body.layer2):
        for p in mod.parameters():
            p.requires_grad = False


# ------------------------------------------------------------------------------------------------------------------------------
def test_refresh_writes_the_bf16_and_the_transposed_copy_of_every_gemm_weight(dev):
    """ParamStore.refresh(): shadow = bf16(flat) and, for every GEMM weight W [N, K] of the model (1x1x1 convs, linears, packed
    in-projections; rows of 81 classes, 4 box coordinates ... included), tshadow = W^T [K, ldt] with zero padding columns -- bit for bit
    (tuber_cast_f32_bf16 + tuber_multi_transpose_bf16, 64 x 64 tiles)."""
    from tubelet_transformer_amd.engine import ParamStore
    _, model, _ = _model("TubeR_CSN152_AVA21.yaml", dev)
    store = ParamStore(model, dev)
    with torch.no_grad():
        store.flat.copy_(torch.randn(store.total, device=dev, generator=torch.Generator(device=dev).manual_seed(3)))
    store.tshadow.fill_(7.0)                       # the kernel owns every element it is responsible for ...
    store.refresh()
    assert torch.equal(store.shadow, store.flat.to(torch.bfloat16))
    assert len(store.tinfo) > 50
    shapes = set()
    for name, (toff, N, K, ldt) in store.tinfo.items():
        o = store.offsets[name]
        want = store.flat[o:o + N * K].view(N, K).to(torch.bfloat16).t()
        got = store.tshadow[toff:toff + K * ldt].view(K, ldt)
        assert torch.equal(got[:, :N], want), name
        shapes.add((N % 64 != 0, K % 8 != 0))
        # ... and nothing else: the padding columns N .. ldt-1 inside the last row tile are written as zero, the rest keeps its value
        assert bool(((got[:, N:] == 0) | (got[:, N:] == 7)).all()), name
    assert (True, False) in shapes                 # ragged row counts (class / box heads) are part of the model


@pytest.mark.parametrize("frozen", [False, True])
def test_fused_clip_adamw_matches_torch(dev, frozen):
    cfg, model, _ = _model("TubeR_CSN152_AVA21.yaml", dev)
    if frozen:
        _freeze_like_load_csn_mat(model)
    opt = build_optimizer(model, cfg)
    store, _ = model.engine()
    # plain-torch twin: cloned fp32 parameters in the same four groups, same hyper-parameters
    named = list(model.named_parameters())
    twin = {n: torch.nn.Parameter(p.detach().clone()) for n, p in named}
    T = cfg.CONFIG.TRAIN
    groups = [
        {"params": [twin[n] for n, p in named if "backbone" not in n and "class_embed" not in n and "query_embed" not in n and p.requires_grad]},
        {"params": [twin[n] for n, p in named if "backbone" in n and p.requires_grad], "lr": T.LR_BACKBONE},
        {"params": [twin[n] for n, p in named if "class_embed" in n and p.requires_grad], "lr": T.LR},
        {"params": [twin[n] for n, p in named if "query_embed" in n and p.requires_grad], "lr": T.LR},
    ]
    ref = torch.optim.AdamW(groups, lr=T.LR, weight_decay=T.W_DECAY, foreach=False)
    trainable = [n for n, p in named if p.requires_grad]
    gen = torch.Generator(device="cpu").manual_seed(11)
    for step in range(3):
        opt.zero_grad()
        for n, p in named:
            if p.requires_grad:
                g = (torch.randn(p.shape, generator=gen) * (0.05 + 0.02 * step)).to(dev)
                p.grad.copy_(g)                       # windows of the flat gradient buffer
                twin[n].grad = g.clone()
            else:
                assert p.grad is None
        if step == 2:                                  # a scheduler step between optimizer steps must reach the kernel
            for a, b in zip(opt.param_groups, ref.param_groups):
                a["lr"] *= 0.5
                b["lr"] *= 0.5
        tot = torch.nn.utils.clip_grad_norm_([twin[n] for n in trainable], 0.1)
        ref.step()
        opt.step(max_norm=0.1)
        torch.cuda.synchronize()
        norm, coef = float(opt.norm_out[0]), float(opt.norm_out[1])
        want_coef = min(1.0, 0.1 / (float(tot) + 1e-6))
        assert abs(norm - float(tot)) <= 1e-5 * float(tot), (norm, float(tot))
        assert abs(coef - want_coef) <= 1e-5 * want_coef
        worst = 0.0
        for n, p in named:
            d = float((p.detach() - twin[n].detach()).abs().max())
            scale = max(1.0, float(twin[n].detach().abs().max()))
            worst = max(worst, d / scale)
            if not p.requires_grad:
                assert d == 0.0, n                     # frozen: bit-unchanged
        assert worst <= 1e-6, worst
        for n in trainable:
            o = store.offsets[n]
            k = twin[n].numel()
            st = ref.state[twin[n]]
            m, v = opt.exp_avg[o:o + k].view(twin[n].shape), opt.exp_avg_sq[o:o + k].view(twin[n].shape)
            assert float((m - st["exp_avg"]).abs().max()) <= 1e-6 * max(1e-3, float(st["exp_avg"].abs().max())), n
            assert float((v - st["exp_avg_sq"]).abs().max()) <= 1e-6 * max(1e-6, float(st["exp_avg_sq"].abs().max())), n
        print("step %d: |g| hip %.6f torch %.6f, clip coef %.6e, worst relative parameter difference %.2e" % (step, norm, float(tot), coef, worst))
    assert opt.t == 3
    # optimizer state round trip (moments + step count live outside Optimizer.state)
    sd = opt.state_dict()
    opt2 = build_optimizer(model, cfg)
    opt2.load_state_dict(sd)
    assert opt2.t == 3 and torch.equal(opt2.exp_avg, opt.exp_avg) and torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq)


def _surrogate(out):
    g = torch.Generator().manual_seed(5)
    tot = 0
    for o in [out] + list(out.get("aux_outputs", [])):
        for k in ("pred_logits", "pred_boxes", "pred_logits_b"):
            tot = tot + (o[k].float() * torch.randn(o[k].shape, generator=g).to(o[k].device)).sum()
    return tot


def test_frozen_backbone_prefix_gradients_and_step(dev):
    """freeze pattern of the pretrained recipe on the shallow body: (a) frozen tensors get no gradient, their windows of the flat
    buffer stay zero; (b) every trainable gradient is bit-identical to the unfrozen run (same kernels above the cut);
    (c) BatchNorm buffers of frozen layers still update; (d) one full step leaves the frozen tensors bit-unchanged and uses the
    clip coefficient of the trainable gradients only."""
    cfg, model, crit = _model("TubeR_CSN152_AVA21.yaml", dev, dropout=False)
    store, runner = model.engine()
    clips = synth.synthetic_clips(2, 32, 64, 96, seed=3, device=dev)
    bn0 = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}

    def run():
        model.load_state_dict(bn0, strict=False)
        store.zero_grad()
        _surrogate(model(clips)).backward()
        torch.cuda.synchronize()
        return store.gflat.detach().clone()

    g_full = run()
    bn_full = {k: v.clone() for k, v in model.state_dict().items() if k in bn0}
    _freeze_like_load_csn_mat(model)
    plans, stem, lowest = runner.trainable_plan()
    assert not stem["any"] and runner.blocks[lowest].stage == 3 and runner.blocks[lowest].first
    g_frozen = run()
    for k, v in model.state_dict().items():
        if k in bn0:
            assert torch.equal(v, bn_full[k]), k                     # (c) running statistics identical to the unfrozen run
            if "running_mean" in k:
                assert not torch.equal(v, bn0[k]), k
    nfrozen, gsum = 0, 0.0
    for n, p in model.named_parameters():
        o = store.offsets[n]
        w = slice(o, o + p.numel())
        if p.requires_grad:
            assert torch.equal(g_frozen[w], g_full[w]), n            # (b)
        else:
            nfrozen += 1
            assert p.grad is None and float(g_frozen[w].abs().max()) == 0.0, n      # (a)
            gsum += float(g_full[w].abs().sum())
    assert nfrozen > 20 and gsum > 0.0          # ... and the unfrozen run did produce gradients there
    # (d) one optimisation step
    opt = build_optimizer(model, cfg)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    targets = synth.synthetic_targets(2, "ava", 80, seed=5, device=dev, hw=(64, 96))
    train_step(model, crit, opt, clips, targets, 0.1)
    torch.cuda.synchronize()
    tr = torch.cat([p.grad.flatten() for p in model.parameters() if p.grad is not None]).double()
    want = math.sqrt(float((tr ** 2).sum()))
    assert abs(float(opt.norm_out[0]) - want) <= 1e-5 * want
    moved = 0
    for n, p in model.named_parameters():
        if p.requires_grad:
            moved += int(not torch.equal(p.detach(), before[n]))
        else:
            assert torch.equal(p.detach(), before[n]), n
    assert moved > 100


def test_lr_backbone_zero_skips_the_body_backward(dev):
    """LR_BACKBONE <= 0 freezes the whole CSN body (backbone_builder.py:38-40): no body gradient, transformer gradients unchanged"""
    cfg, model, _ = _model("TubeR_CSN152_AVA21.yaml", dev, dropout=False)
    store, runner = model.engine()
    clips = synth.synthetic_clips(1, 32, 64, 64, seed=4, device=dev)
    bn0 = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
    store.zero_grad()
    _surrogate(model(clips)).backward()
    g_full = store.gflat.detach().clone()
    for p in model.backbone.body.parameters():
        p.requires_grad_(False)
    assert not runner.any_trainable()
    model.load_state_dict(bn0, strict=False)
    store.zero_grad()
    _surrogate(model(clips)).backward()
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        o = store.offsets[n]
        w = slice(o, o + p.numel())
        if n.startswith("backbone.body."):
            assert float(store.gflat[w].abs().max()) == 0.0, n
        else:
            assert torch.equal(store.gflat[w], g_full[w]), n


# ------------------------------------------------------------------------------------------------------------------------------
def _ragged_batch(dev, seed, hw=(64, 96)):
    """two clips of different width padded to a common size: NestedTensor with a non-trivial mask"""
    from tubelet_transformer_amd.misc import nested_tensor_from_tensor_list
    a, b = synth.synthetic_clips(2, 32, 0, 0, seed=seed, sizes=[hw, (hw[0] - 16, hw[1] - 16)])
    return nested_tensor_from_tensor_list([a.to(dev), b.to(dev)])


@pytest.mark.parametrize("yaml_name,dataset", [("TubeR_CSN152_AVA21.yaml", "ava"), ("Tuber_CSN152_JHMDB.yaml", "jhmdb")])
def test_graph_replay_tracks_batch_state_like_eager(dev, yaml_name, dataset):
    """four steps with per-step different clips, padding masks, targets (JHMDB: key_pos and vis too), a learning-rate change after
    step 2 and the loss_ce weight switch after step 3: the captured step must reproduce the eager sequence bit for bit"""
    results = []
    for graphed in (False, True):
        cfg, model, crit = _model(yaml_name, dev)
        opt = build_optimizer(model, cfg)
        store, _ = model.engine()
        store.manual_seed(321)
        step = GraphedTrainStep(model, crit, opt, 0.1) if graphed else None
        losses = []
        for i in range(4):
            samples = _ragged_batch(dev, seed=50 + i)
            targets = synth.synthetic_targets(2, dataset, cfg.CONFIG.DATA.NUM_CLASSES, seed=70 + i, device=dev, hw=(64, 96))
            if dataset != "ava":
                for b, t in enumerate(targets):
                    t["key_pos"] = torch.tensor((5 * i + 3 * b) % 32, dtype=torch.int64, device=dev)
                    t["vis"] = torch.tensor([(i + b) % 2], dtype=torch.int64, device=dev)
            if i == 2:
                for gr in opt.param_groups:
                    gr["lr"] = gr["lr"] * 0.1
            if i == 3:
                crit.weight_dict["loss_ce"] = 3.0
            if graphed:
                loss, _ = step(samples, targets)
            else:
                loss, _ = train_step(model, crit, opt, samples, targets, 0.1)
            losses.append(float(loss))
        torch.cuda.synchronize()
        if graphed:
            assert len(step.graphs) == 1, "one clip shape -> one captured graph"
        results.append((losses, store.flat.detach().clone(), {k: v.clone() for k, v in model.state_dict().items() if "running" in k}, opt.t))
    (l0, f0, b0, t0), (l1, f1, b1, t1) = results
    print("eager losses %s\ngraph losses %s" % (l0, l1))
    assert t0 == 4 and t1 == 4, "capture warm-up passes must not count as optimisation steps"
    assert l0 == l1
    assert torch.equal(f0, f1), "%d parameters differ" % int((f0 != f1).sum())
    for k in b0:
        assert torch.equal(b0[k], b1[k]), k


def test_graph_cache_is_bounded_and_keyed_on_frozen_set(dev):
    cfg, model, crit = _model("TubeR_CSN50_AVA21.yaml", dev)
    opt = build_optimizer(model, cfg)
    step = GraphedTrainStep(model, crit, opt, 0.1, max_graphs=2)
    targets = synth.synthetic_targets(1, "ava", 80, seed=5, device=dev, hw=(64, 64))
    for hw in ((64, 64), (64, 80), (64, 96), (64, 64)):
        clips = synth.synthetic_clips(1, 32, hw[0], hw[1], seed=3, device=dev)
        loss, _ = step(clips, targets)
        assert math.isfinite(float(loss)) and len(step.graphs) <= 2
    _freeze_like_load_csn_mat(model)
    n = len(step.graphs)
    step(clips, targets)
    assert len(step.graphs) <= 2 and (tuple(clips.shape), model.engine()[0].trainable_signature(), True, 16, False) in step.graphs and n <= 2
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------------
# the N > 1 code path on ONE GPU: a one-rank RCCL communicator (csrc/collective.cpp) forced through the DDP branch
# ------------------------------------------------------------------------------------------------------------------------------
def _ddp_run(dev, mode, monkeypatch, steps=2):
    from tubelet_transformer_amd.ddp import attach_reducer
    for k in ("TUBER_RCCL_IN_GRAPH", "TUBER_DDP_BF16", "TUBER_FORCE_SPLIT_GRAPH"):
        monkeypatch.delenv(k, raising=False)
    if mode == "in_graph":
        monkeypatch.setenv("TUBER_RCCL_IN_GRAPH", "1")
    if mode == "bf16":
        monkeypatch.setenv("TUBER_DDP_BF16", "1")
    cfg, model, crit = _model("TubeR_CSN50_AVA21.yaml", dev)
    opt = build_optimizer(model, cfg)
    store, _ = model.engine()
    red = None
    if mode != "single" and mode != "single_eager":
        red = attach_reducer(store, force=True)
        assert red is not None and red.comm is not None and red.comm.version >= 20000 and red.world == 1
    store.manual_seed(99)
    clips = synth.synthetic_clips(2, 32, 64, 96, seed=3, device=dev)
    targets = synth.synthetic_targets(2, "ava", 80, seed=5, device=dev, hw=(64, 96))
    eager = mode in ("eager", "single_eager")
    step = None if eager else GraphedTrainStep(model, crit, opt, 0.1)
    for _ in range(steps):
        if eager:
            loss, _ = train_step(model, crit, opt, clips, targets, 0.1)
        else:
            loss, _ = step(clips, targets)
    torch.cuda.synchronize()
    info = {}
    if red is not None:
        info["issued"] = red.issued
        info["trainable"] = sum(b - a for a, b in store.trainable_ranges())
        if step is not None:
            g = next(iter(step.graphs.values()))
            info["split"] = g.A2 is not None
            info["in_graph"] = g.in_graph
        red.comm.close()
    return float(loss), store.flat.detach().clone(), info


def test_one_rank_rccl_communicator_drives_the_ddp_step(dev, monkeypatch):
    """RCCL init through the C ABI, ncclAllReduce on the reducer's own stream, the cut graph (A / all-reduce / A2 / all-reduce / B2),
    the in-graph capture of the collectives, the eager hook path and the bf16-compressed transport -- all on a one-rank
    communicator, so the results must equal the plain single-GPU step (bit for bit; bf16 compression within its rounding)."""
    l0, f0, _ = _ddp_run(dev, "single", monkeypatch)
    l1, f1, i1 = _ddp_run(dev, "split", monkeypatch)
    assert i1["split"] and not i1["in_graph"] and i1["issued"] == i1["trainable"], i1
    assert l1 == l0 and torch.equal(f1, f0)
    l2, f2, i2 = _ddp_run(dev, "in_graph", monkeypatch)
    assert i2["in_graph"] and not i2["split"], i2
    assert l2 == l0 and torch.equal(f2, f0)
    l3, f3, _ = _ddp_run(dev, "single_eager", monkeypatch)
    l4, f4, i4 = _ddp_run(dev, "eager", monkeypatch)
    assert i4["issued"] == i4["trainable"], i4
    assert l4 == l3 and torch.equal(f4, f3)
    l5, f5, i5 = _ddp_run(dev, "bf16", monkeypatch)
    assert i5["issued"] == i5["trainable"]
    assert abs(l5 - l0) <= 1e-2 * abs(l0) and float((f5 - f0).abs().max()) <= 1e-3


_NCCL_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from tubelet_transformer_amd import synth
from tubelet_transformer_amd.config import load_cfg
from tubelet_transformer_amd.training import GraphedTrainStep, build_optimizer, deploy_model
from tubelet_transformer_amd.tuber import build_model
dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%s" % sys.argv[2], rank=0, world_size=1)
cfg = load_cfg(os.path.join(sys.argv[1], "configuration", "TubeR_CSN50_AVA21.yaml"))
cfg.CONFIG.MODEL.BACKBONE_NAME = "CSN-TEST"
cfg.DDP_CONFIG.GPU = 0
model, crit, _ = build_model(cfg)
synth.load_name_hashed(model)
model = deploy_model(model, cfg, is_tuber=True)
crit.to("cuda:0")
model.train(); crit.train()
store, _ = model.engine()
assert (store.reducer is not None) == bool(os.environ.get("TUBER_FORCE_DDP"))
if store.reducer is not None:
    assert store.reducer.comm is not None        # own RCCL communicator next to torch's nccl process group
    t = torch.ones(4, device="cuda:0"); dist.all_reduce(t); assert float(t.sum()) == 4.0
opt = build_optimizer(model, cfg)
store.manual_seed(99)
clips = synth.synthetic_clips(2, 32, 64, 96, seed=3, device="cuda:0")
targets = synth.synthetic_targets(2, "ava", 80, seed=5, device="cuda:0", hw=(64, 96))
step = GraphedTrainStep(model, crit, opt, 0.1)
for _ in range(2):
    loss, _ = step(clips, targets)
torch.cuda.synchronize()
print("RESULT %.9e %.17e %d" % (float(loss), float(store.flat.double().sum()), int(store.reducer.issued) if store.reducer is not None else 0))
dist.destroy_process_group()
"""


def test_deploy_model_under_a_one_rank_nccl_process_group(tmp_path):
    """the reference's launch shape (init_process_group('nccl') then deploy_model(model, cfg, is_tuber=True)) in a fresh process, with
    and without the forced DDP branch: the own communicator coexists with torch's process group (one RCCL instance), results equal"""
    import subprocess
    import sys
    script = str(tmp_path / "worker.py")
    open(script, "w").write(_NCCL_WORKER)
    out = []
    for i, force in enumerate((False, True)):
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        env.pop("TUBER_FORCE_DDP", None)
        if force:
            env["TUBER_FORCE_DDP"] = "1"
        r = subprocess.run([sys.executable, script, ROOT, str(29600 + os.getpid() % 300 + i)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT")][-1].split()
        out.append(line)
    assert out[0][1] == out[1][1] and out[0][2] == out[1][2], out
    assert int(out[1][3]) > 0 and int(out[0][3]) == 0


# ------------------------------------------------------------------------------------------------------------------------------
# world size 2 on ONE GPU (gloo transport, both ranks on cuda:0): the reduced flat gradient buffer must equal the mean of the two
# ranks' single-GPU gradients -- on the hook-driven eager path (incl. the pool-decoder window of the 'decode' configs, whose deferred
# second-stage sums must land BEFORE the window is handed to the transport) and on the cut-graph path
# ------------------------------------------------------------------------------------------------------------------------------
_WORLD2_WORKER = r"""
import os, sys, torch, torch.distributed as dist
root, port, rank, mode, out = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4], sys.argv[5]
sys.path.insert(0, root)
from tubelet_transformer_amd import synth
from tubelet_transformer_amd.config import load_cfg
from tubelet_transformer_amd.ddp import attach_reducer, broadcast_parameters
from tubelet_transformer_amd.training import GraphedTrainStep, build_optimizer
from tubelet_transformer_amd.tuber import build_model
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
cfg = load_cfg(os.path.join(root, "configuration", "TubeR_CSN50_AVA21.yaml"))      # 'decode': pool decoder behind the body
cfg.CONFIG.MODEL.BACKBONE_NAME = "CSN-TEST"
model, crit, _ = build_model(cfg)
synth.load_name_hashed(model)
model.to(dev).train(); crit.to(dev).train()
store, _ = model.engine()

def grads(reduced, graph):
    store.manual_seed(99)
    clips = synth.synthetic_clips(2, 32, 64, 96, seed=3 + rank, device=dev)
    targets = synth.synthetic_targets(2, "ava", 80, seed=5 + rank, device=dev, hw=(64, 96))
    red = store.reducer if reduced else None
    keep, store.reducer = store.reducer, red
    try:
        if graph:
            opt = build_optimizer(model, cfg)
            for g in opt.param_groups:
                g["lr"] = 0.0; g["weight_decay"] = 0.0          # the captured step includes AdamW: keep the parameters where they are
            flat0 = store.flat.clone()
            step = GraphedTrainStep(model, crit, opt, 0.1)
            step(clips, targets)
            torch.cuda.synchronize()
            assert (next(iter(step.graphs.values())).A2 is not None) == reduced
            store.flat.copy_(flat0)
        else:
            out_ = model(clips)
            ld = crit(out_, targets)
            loss = crit.weighted_total(ld, crit.weight_dict)
            store.zero_grad()
            if red is not None:
                red.begin()
            loss.backward()
            if red is not None:
                red.finish()
        torch.cuda.synchronize()
        return store.gflat.detach().clone()
    finally:
        store.reducer = keep

local = grads(False, mode == "graph")
os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", port
dist.init_process_group("gloo", rank=rank, world_size=2)
broadcast_parameters(store)
red = attach_reducer(store)
assert red is not None and red.comm is None and red.world == 2
got = grads(True, mode == "graph")
both = [torch.zeros_like(local).cpu() for _ in range(2)]
dist.all_gather(both, local.cpu())
want = (both[0] + both[1]) * 0.5
torch.save({"got": got.cpu(), "want": want, "issued": red.issued, "trainable": sum(b - a for a, b in store.trainable_ranges()),
            "names": store.names, "offsets": [store.offsets[n] for n in store.names]}, out + ".%d" % rank)
dist.barrier()
dist.destroy_process_group()
"""


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_world2_reduced_gradients_equal_the_mean_of_the_ranks(tmp_path, dev, mode):
    import subprocess
    import sys
    script = str(tmp_path / "w2.py")
    open(script, "w").write(_WORLD2_WORKER)
    port = str(29700 + os.getpid() % 200 + (0 if mode == "eager" else 1))
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
        assert res["issued"] == res["trainable"], (res["issued"], res["trainable"])      # every trainable window sent exactly once
        bad = []
        for n, o, e in zip(res["names"], res["offsets"], res["offsets"][1:] + [got.numel()]):
            if not torch.equal(got[o:e], want[o:e]):
                bad.append((n, float((got[o:e] - want[o:e]).abs().max()), float(want[o:e].abs().max())))
        assert not bad, "rank %d: %d tensors differ from the mean of the ranks, e.g. %s" % (r, len(bad), bad[:6])


# ------------------------------------------------------------------------------------------------------------------------------
# every retained A/B switch is shipped code: hold each to the default path
# ------------------------------------------------------------------------------------------------------------------------------
_AB_DEFAULT = {}


def _ab_run(dev, names):
    """one training-mode forward + backward of the 2-blocks-per-stage CSN body + transformer on a 2-clip 64x96 batch (layer1's
    256/64-channel shapes that the persistent fused kernels take, identity and projection blocks, strided blocks), dropout off, and an
    eval-mode forward of the same model -> (surrogate loss, {parameter: gradient}, BatchNorm running means, eval outputs)"""
    from parity_util import surrogate
    from tubelet_transformer_amd import ab
    with ab.override(*names):
        cfg, model, crit = _model("TubeR_CSN152_AVA21.yaml", dev, dropout=False)
        store, _ = model.engine()
        clips = synth.synthetic_clips(2, 32, 64, 96, seed=21, device=dev)
        model.eval()
        with torch.no_grad():
            ev = {k: v.detach().float().clone() for k, v in model(clips).items() if k in ("pred_logits", "pred_boxes", "pred_logits_b")}
        model.train()
        store.zero_grad()
        out = model(clips)
        loss = surrogate(out)          # smooth functional of every output: the Hungarian assignment is discontinuous -- a one-ulp change of
        loss.backward()                # an activation can flip a match and move the decoder's gradients by O(1) at an unchanged loss
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None}
        bufs = {n: b.detach().float().clone() for n, b in model.named_buffers() if n.endswith("running_mean")}
        return float(loss.detach()), grads, bufs, ev


def _ab_names():
    from tubelet_transformer_amd import ab
    return sorted(k for k in ab.KNOWN if k != "eager_step")      # (eager_step: the training loop's switch, test_boundary_gpu.py)


# switches that change the FORWARD arithmetic (another kernel computes the same activation with other rounding points).  On this
# tiny batch training-mode BatchNorm amplifies a one-ulp activation change through the whole body (the default path against itself
# is bit-stable; these three measure median 4-7 % / p99 20-50 % on the gradients), so they are held tightly on the eval-mode outputs
# and to the chaos level on the training gradients; every other switch only regroups launches and measures <= 8 % on single tensors.
_AB_FORWARD = {"dw_register_tiled", "no_blockout_conv1", "no_entry_conv", "no_decoder_coop"}
# backward-only switches that change the fp32 SUMMATION ORDER of a data-gradient GEMM (other split of the reduction over waves): the bf16
# rounding of that gradient flips on a few elements and everything below it moves by a bf16 ulp -- linear, no chaos: median <= 1e-2
_AB_SUMORDER = {"no_in_proj_dx2"}
_AB_EVAL = {"eval_bf16_stream", "eval_bf16_decoder"}      # (no_eval_conv4_join is bit-identical: held at 1e-6 like the launch-structure switches)


@pytest.mark.parametrize("name", _ab_names())
def test_every_ab_switch_reproduces_the_default_path(dev, name):
    """``TUBER_AB=<name>`` routes part of the step through the separate kernels a fused / grouped form replaced.  Those paths ship in
    the library, so each is held to the default path on the same inputs: eval-mode outputs, training-mode surrogate loss, every
    parameter gradient (most are bit-identical: same arithmetic in a different launch structure), BatchNorm running statistics."""
    if not _AB_DEFAULT:
        _AB_DEFAULT["ref"] = _ab_run(dev, ())
    l0, g0, b0, e0 = _AB_DEFAULT["ref"]
    l1, g1, b1, e1 = _ab_run(dev, (name,))
    fwd = name in _AB_FORWARD
    for k in e0:
        err = float((e1[k] - e0[k]).abs().max())
        # (the eval_* switches select the eval forward's PRECISION, round 6: the eval outputs move by the bf16 path's own error, the training step not at all)
        assert err <= (4e-2 if name in _AB_EVAL else 2e-2 if fwd else 1e-6), (k, err)
    assert math.isfinite(l1) and abs(l1 - l0) <= (6e-2 if fwd else 1e-4) * max(abs(l0), 1.0), (l0, l1)
    assert set(g0) == set(g1)
    rels = []
    gmax = max(float(v.norm()) for v in g0.values())
    for n in g0:
        den = float(g0[n].norm())
        if den < 1e-12:
            continue
        # a gradient that is numerically zero (norm below 1e-4 of the largest tensor's: layer 0's self-attention in-projection -- tgt = 0, so
        # its true gradient vanishes -- is bf16 rounding noise of the attention backward) is held to that floor, not to itself
        floor = 1e-4 * gmax
        rels.append((float((g1[n] - g0[n]).norm()) / max(den, floor), n))
        if den > floor:
            assert 0.5 < float(g1[n].norm()) / den < 2.0, n
        else:
            assert float(g1[n].norm()) <= 2.0 * floor, (n, float(g1[n].norm()), floor)
    rels.sort(reverse=True)
    med = rels[len(rels) // 2][0]
    if fwd:
        assert med <= 0.15 and rels[0][0] <= 1.0, (med, rels[:3])
    else:
        assert rels[0][0] <= 0.15 and med <= (1e-2 if name in _AB_SUMORDER else 1e-3), (med, rels[:3])      # (a wrong kernel is O(1) on everything below it)
    for n in b0:
        assert torch.allclose(b0[n], b1[n], rtol=2e-2 if fwd else 1e-5, atol=2e-3 if fwd else 1e-6), n
    print("TUBER_AB=%s: loss %.6f vs %.6f, median / worst gradient relerr %.2e / %.2e (%s)" % (name, l1, l0, med, rels[0][0], rels[0][1]))


# ------------------------------------------------------------------------------------------------------------------------------
# round 5: the decoder stack as ONE cooperative launch (csrc/decoder_coop.hip) against the launch chain it replaces
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dropout", [False, True])
def test_cooperative_decoder_launch_equals_the_launch_chain(dev, dropout):
    """tuber_decoder_coop_fwd fills the tensors a DRY run of the decoder's op sequence allocated (tape.Tape.dry), so the launch chain's
    backward closures run on them unchanged.  Held against ``TUBER_AB=no_decoder_coop`` on the same model / inputs / seed:
    * eval outputs within bf16 rounding of the chain's (other accumulation order in linear2 and the self-attention, same rounding points);
    * training forward WITH dropout on: the fused kernel draws the chain's masks (same seed, salts, element indices) -- a wrong stream
      would move the outputs by O(0.1), not by bf16 noise;
    * every parameter gradient of a smooth surrogate loss: median relative difference <= 6e-2 (the chaos level of this fixture for a switch
      that moves forward rounding points: test_every_ab_switch_...), no tensor above 0.6 (query_embed: a cancellation-dominated 1e-2 gradient),
      norms within 10 % for every tensor above 1e-3 of the largest;
    * the synchronisation words are zero after every launch (no barrier timed out, the last workgroup out reset them), also on the
      second and third launch and from a captured hipGraph."""
    from parity_util import surrogate
    from tubelet_transformer_amd import ab, lib

    def run(names):
        with ab.override(*names):
            cfg, model, crit = _model("TubeR_CSN152_AVA21.yaml", dev, dropout=dropout)
            store, _ = model.engine()
            assert lib.query("tuber_decoder_coop_supported", 256, 8, 2048, 2, 15, 6) == 1
            clips = synth.synthetic_clips(2, 32, 64, 96, seed=21, device=dev)
            model.eval()
            with torch.no_grad():
                ev = {k: v.detach().float().clone() for k, v in model(clips).items() if k in ("pred_logits", "pred_boxes", "pred_logits_b")}
            model.train()
            res = []
            for rep in range(2):                                  # twice: the second launch finds the words the first one left
                store.manual_seed(1234)
                store.zero_grad()
                out = model(clips)
                tr = {k: v.detach().float().clone() for k, v in out.items() if k in ("pred_logits", "pred_boxes", "pred_logits_b")}
                loss = surrogate(out)
                loss.backward()
                torch.cuda.synchronize()
                grads = {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None}
                res.append((tr, grads))
            sync = store.coop_sync.cpu().tolist()
            assert sync == [0, 0, 0, 0], sync
            for k in res[0][0]:
                assert torch.equal(res[0][0][k], res[1][0][k]), "the same step twice must be bit-identical (%s)" % k
            g = None
            if not names:
                # the launch inside a captured graph
                g = torch.cuda.CUDAGraph()
                model.eval()
                static = clips.clone()
                with torch.no_grad():
                    ev2 = {k: v.detach().float().clone() for k, v in model(static).items() if k in ev}      # (the training passes moved the BatchNorm buffers)
                    torch.cuda.synchronize()
                    with torch.cuda.graph(g):
                        go = model(static)
                    g.replay(); g.replay()
                    torch.cuda.synchronize()
                for k in ev:
                    assert torch.equal(go[k].float(), ev2[k]), k
                assert store.coop_sync.cpu().tolist() == [0, 0, 0, 0]
            return ev, res[0][0], res[0][1]
    e1, t1, g1 = run(())
    e0, t0, g0 = run(("no_decoder_coop",))
    for k in e0:
        err, terr = float((e1[k] - e0[k]).abs().max()), float((t1[k] - t0[k]).abs().max())
        print("cooperative decoder vs launch chain, dropout %s: %-14s eval max |diff| %.3e   train max |diff| %.3e  (|value| max %.2f)" % (
            dropout, k, err, terr, float(e0[k].abs().max())))
        assert err <= 2e-2 and terr <= (6e-2 if dropout else 3e-2), (k, err, terr)
    rels = []
    gmax = max(float(v.norm()) for v in g0.values())
    for n in g0:
        den = float(g0[n].norm())
        if den < 1e-12:
            continue
        rels.append((float((g1[n] - g0[n]).norm()) / max(den, 1e-4 * gmax), n))       # (numerically-zero gradients: see test_every_ab_switch_...)
        if den > 1e-3 * gmax:
            assert 0.9 < float(g1[n].norm()) / den < 1.1, (n, float(g1[n].norm()) / den)
    rels.sort(reverse=True)
    med = rels[len(rels) // 2][0]
    print("   gradients: median relative difference %.3e, worst %.3e (%s) over %d tensors; |grad| of layer 0's self-attention in-projection %.3e of the largest tensor's" % (
        med, rels[0][0], rels[0][1], len(rels), float(g0["transformer.decoder.layers.0.self_attn.in_proj_weight"].norm()) / gmax))
    assert med <= 6e-2 and rels[0][0] <= 0.6, (med, rels[:3])


# ------------------------------------------------------------------------------------------------------------------------------
# round 6: the cooperative decoder launch fails SAFE (VERDICT r05 item 7 / ADVICE r05 medium)
# ------------------------------------------------------------------------------------------------------------------------------
def _xcd_blocker():
    """tests/helpers/xcd_blocker.hip compiled with hipcc at test time (the same toolchain the library is built with) -> ctypes handle"""
    import ctypes
    import subprocess
    import tempfile
    src = os.path.join(ROOT, "tests", "helpers", "xcd_blocker.hip")
    out = os.path.join(tempfile.gettempdir(), "tuber_xcd_blocker_%d.so" % os.getpid())
    if not os.path.exists(out):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O2", "-shared", "-fPIC", "-o", out, src],
                       check=True, cwd=tempfile.gettempdir())
    lib = ctypes.CDLL(out)
    lib.xcd_blocker_launch.argtypes = [ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
    lib.xcd_blocker_launch.restype = ctypes.c_int
    return lib


def test_cooperative_decoder_fails_safe_when_starved(dev):
    """tuber_decoder_coop_fwd needs its 16 workgroups co-resident on ONE XCD and does not ask the runtime for that (a plain launch inside a
    captured graph).  Here a helper kernel on a second stream holds 28 of the 32 CUs of every XCD (120 KB of LDS each) for 0.5 s, so at most 8 of the 16
    workgroups become resident (two fit the LDS of a free CU): their barrier times out.  What must happen then:
      * the launch ends (bounded spins), raises its error word and overwrites its output with NaN -- the actor logits are NaN;
      * a training step on such a forward is SKIPPED on the device: loss NaN, gradient norm NaN, clip coefficient -1, parameters, both
        AdamW moments and the step count bit-unchanged (the reference stops before optimizer.step() on a non-finite loss);
      * ``ParamStore.coop_failed()`` reports it once, clears the words and switches the engine to the launch chain: the next forward is
        bit-identical to ``TUBER_AB=no_decoder_coop`` and the next training step moves the parameters;
      * the validation loops' ``_forward_checked`` repeats the batch by itself."""
    from tubelet_transformer_amd import ab
    from tubelet_transformer_amd.evaluation import _forward_checked
    blk = _xcd_blocker()
    side = torch.cuda.Stream()
    started = torch.zeros(2, dtype=torch.int32, device=dev)
    KEYS = ("pred_logits", "pred_boxes", "pred_logits_b")

    def starve(ms=500.0, keep=28):
        started.zero_()
        torch.cuda.synchronize()
        assert blk.xcd_blocker_launch(keep, ms, started.data_ptr(), side.cuda_stream) == 0
        import time
        t0 = time.time()
        while int(started[0].item()) < 8 * keep:               # every blocker workgroup is resident before the model's launches are issued
            assert time.time() - t0 < 5.0, "the blocker kernel did not start"
        return

    cfg, model, crit = _model("TubeR_CSN152_AVA21.yaml", dev, dropout=False)
    store, _ = model.engine()
    clips = synth.synthetic_clips(2, 32, 64, 96, seed=21, device=dev)
    targets = synth.synthetic_targets(2, "ava", 80, seed=5, device=dev, hw=(64, 96))
    model.eval()
    with torch.no_grad():
        good = {k: v.detach().float().clone() for k, v in model(clips).items() if k in KEYS}
        with ab.override("no_decoder_coop"):
            chain = {k: v.detach().float().clone() for k, v in model(clips).items() if k in KEYS}
    assert store.coop_sync.cpu().tolist() == [0, 0, 0, 0] and not store.coop_off
    assert all(bool(torch.isfinite(v).all()) for v in good.values())

    # ---- a starved TRAINING step: skipped on the device ----
    model.train()
    opt = build_optimizer(model, cfg)
    train_step(model, crit, opt, clips, targets, 0.1)          # one clean step first: non-zero moments, step count 1
    torch.cuda.synchronize()
    flat0, m0, v0, t0 = store.flat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.t
    assert t0 == 1
    starve()
    loss, _ = train_step(model, crit, opt, clips, targets, 0.1)
    torch.cuda.synchronize()
    words = store.coop_sync.cpu().tolist()
    print("starved cooperative decoder: sync words %s, loss %s, norm_out %s" % (words, float(loss), opt.norm_out.tolist()))
    assert words[2] == 1, words
    assert not bool(torch.isfinite(loss)), float(loss)
    assert float(opt.norm_out[1]) == -1.0 and not math.isfinite(float(opt.norm_out[0]))
    assert torch.equal(store.flat, flat0) and torch.equal(opt.exp_avg, m0) and torch.equal(opt.exp_avg_sq, v0) and opt.t == 1
    # ---- the host notices once, the engine switches to the launch chain, training goes on ----
    assert store.coop_failed() is True and store.coop_off and store.coop_sync.cpu().tolist() == [0, 0, 0, 0]
    assert store.coop_failed() is False
    loss, _ = train_step(model, crit, opt, clips, targets, 0.1)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and opt.t == 2 and not torch.equal(store.flat, flat0)

    # ---- a starved EVAL forward: NaN outputs; the validation loops' wrapper repeats the batch on the launch chain ----
    with torch.no_grad():
        store.flat.copy_(flat0)
    model.eval()                                               # (the training steps moved the BatchNorm buffers: fresh chain reference below)
    store.coop_off = False
    # (the default eval forward -- the eval precision mode -- runs its decoder in fp32 and never takes the cooperative launch; the form that does is
    #  TUBER_AB=eval_bf16_stream, the training path's rounding points)
    with torch.no_grad(), ab.override("eval_bf16_stream"):
        with ab.override("no_decoder_coop", "eval_bf16_stream"):
            chain2 = {k: v.detach().float().clone() for k, v in model(clips).items() if k in KEYS}
        starve()
        bad = {k: v.detach().float().clone() for k, v in model(clips).items() if k in KEYS}
        torch.cuda.synchronize()
        # the actor logits (a linear layer on the poisoned decoder output) are NaN throughout; the box MLP's ReLU (fmaxf) and the class
        # branch's softmax swallow a NaN, so those outputs are finite GARBAGE -- which is why the validation loops read the error word
        assert bool(torch.isnan(bad["pred_logits_b"]).all()), {k: int(torch.isnan(v).sum()) for k, v in bad.items()}
        assert store.coop_sync.cpu().tolist()[2] == 1
        store.coop_sync.zero_()
        starve()
        out = {k: v.detach().float().clone() for k, v in _forward_checked(model, clips).items() if k in KEYS}
    assert store.coop_off
    for k in KEYS:
        assert torch.equal(out[k], chain2[k]), k
    torch.cuda.synchronize()


def test_stream_flag_edge_orders_two_streams_and_gives_up_when_its_signal_never_comes(dev):
    """csrc/stream_flag.hip: the software edge the gradient exchange uses at its first issue point.  (1) a consumer stream that waits for
    counter value k reads what the producer stream wrote before its k-th signal -- 50 rounds, the producer's kernel is a long one, the
    consumer would read the stale value if it ran early; (2) a wait whose signal never comes ends after ~2 s with the error word set."""
    import time
    from tubelet_transformer_amd import lib
    flags = torch.zeros(16, dtype=torch.int32, device=dev)
    prod, cons = torch.cuda.Stream(), torch.cuda.Stream()
    big = torch.zeros(32 << 20, device=dev)
    seen = torch.zeros(50, device=dev)
    torch.cuda.synchronize()
    for k in range(1, 51):
        with torch.cuda.stream(prod):
            big.add_(1.0)                                                    # ~0.1 ms of work the signal must wait for
            lib.call("tuber_flag_signal", flags.data_ptr())
        with torch.cuda.stream(cons):
            lib.call("tuber_flag_wait", flags.data_ptr(), k, flags.data_ptr() + 4 * 15)
            seen[k - 1:k].copy_(big[-1:])                                    # must see k
    torch.cuda.synchronize()
    assert seen.tolist() == [float(k) for k in range(1, 51)], seen.tolist()
    assert int(flags[0]) == 50 and int(flags[15]) == 0
    t0 = time.time()
    with torch.cuda.stream(cons):
        lib.call("tuber_flag_wait", flags.data_ptr() + 4, 1, flags.data_ptr() + 4 * 15)      # counter 1 is never bumped
    torch.cuda.synchronize()
    dt = time.time() - t0
    assert int(flags[15]) == 1 and 1.5 < dt < 4.0, (flags.tolist(), dt)
