"""Precise BatchNorm statistics: recompute every BatchNorm's running mean / variance as the plain average over many training batches.

The published recipe trains with 2 clips per GPU and unsynchronised BatchNorm, and under ``ACCUM_STEPS`` (accum.py) only micro-batch 0
of a group updates the running statistics, so the statistics used at validation are an exponential average (momentum 0.1) of about ten
2-clip batches.  ``recompute_bn_stats`` replaces them with the cumulative average over ``num_batches`` batches -- what
``torch.optim.swa_utils.update_bn`` computes (momentum=None), with a batch limit, the project's loader items, and an average over the
ranks of a process group.  The engine honours ``momentum=None`` on the device (backbone.CSNRunner: tuber_bn_finalize_ex /
tuber_bn_count_advance), so the stock ``update_bn`` gives the same statistics over a whole loader.

Frozen BatchNorm: a backbone BatchNorm whose module is in eval mode while the model trains normalises with its running statistics and leaves
them alone (backbone.CSNRunner reads every module's ``training`` flag on each training-mode forward).  ``bn.eval()`` after ``model.train()``
is all it takes; ``freeze_batchnorm`` / ``CONFIG.MODEL.FREEZE_BN`` store a policy on the model that ``DETR.train()`` re-applies, so the
layers stay frozen across the training loop's ``model.train()`` calls.
"""
import torch
from torch.nn.modules.batchnorm import _BatchNorm


def _samples(item):
    """the model input of a loader item: ``(samples, targets, ...)`` -> samples; a tensor, NestedTensor or ClipBatch as it is"""
    if isinstance(item, (list, tuple)):
        if not item:
            raise ValueError("recompute_bn_stats: empty loader item")
        return item[0]
    return item


def _average_over_ranks(bns):
    """running_mean / running_var averaged over the ranks of the default process group (one all-reduce of the float buffers); every rank
    ends with the largest local batch count in num_batches_tracked.  Nothing happens without an initialised group of > 1 ranks."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return
    world = dist.get_world_size()
    bufs = [b for m in bns for b in (m.running_mean, m.running_var)]
    dev = bufs[0].device if dist.get_backend() == "nccl" else torch.device("cpu")
    flat = torch.cat([b.detach().reshape(-1).to(dev, torch.float32) for b in bufs])
    count = torch.tensor([max(int(m.num_batches_tracked) for m in bns)], dtype=torch.int64, device=dev)
    dist.all_reduce(flat)
    dist.all_reduce(count, op=dist.ReduceOp.MAX)
    flat /= world
    with torch.no_grad():
        o = 0
        for b in bufs:
            b.copy_(flat[o:o + b.numel()].view_as(b))
            o += b.numel()
        for m in bns:
            m.num_batches_tracked.fill_(int(count))


FREEZE_POLICIES = ("none", "frozen", "all")


def _backbone_bns(model):
    """(name, module) of the BatchNorm layers a freeze policy governs: those of ``model.backbone`` (the CSN body), or of ``model`` itself"""
    root, prefix = (model.backbone, "backbone.") if hasattr(model, "backbone") else (model, "")
    return [(prefix + n, m) for n, m in root.named_modules() if isinstance(m, _BatchNorm)]


def _policy_layers(model, policy):
    if policy not in FREEZE_POLICIES:
        raise ValueError("FREEZE_BN must be one of %s, got %r" % (" | ".join(FREEZE_POLICIES), policy))
    if policy == "none":
        return []
    bns = _backbone_bns(model)
    if policy == "all":
        return bns
    return [(n, m) for n, m in bns if not any(p.requires_grad for p in (m.weight, m.bias) if p is not None)]


def apply_freeze_policy(model):
    """put the layers of the model's stored policy (``model.freeze_bn``) into eval mode, evaluated now; returns their names"""
    layers = _policy_layers(model, getattr(model, "freeze_bn", "none"))
    for _, m in layers:
        m.training = False
    return [n for n, _ in layers]


def freeze_batchnorm(model, policy):
    """Store a frozen-BatchNorm policy on a built model and apply it at once (when the model is in train mode; ``DETR.train()`` applies it at
    every later call).  ``"none"``: no layer; ``"frozen"``: every backbone BatchNorm whose weight and bias both have ``requires_grad ==
    False`` (pretrained recipe: stem + layer1 + layer2); ``"all"``: every backbone BatchNorm (``requires_grad`` is left alone).  Returns the
    names of the affected modules.  A frozen layer normalises with its running statistics, never writes them, and costs no statistics
    launch; ``"none"`` does not put layers a user froze by hand back into train mode."""
    layers = _policy_layers(model, policy)
    model.freeze_bn = policy
    if model.training:
        for _, m in layers:
            m.training = False
    return [n for n, _ in layers]


def recompute_bn_stats(model, loader, num_batches=200, device=None):
    """Reset every BatchNorm's running statistics and re-estimate them as the cumulative average (``momentum = None``) over the first
    ``num_batches`` items of ``loader`` (``None``: all of them), with train-mode forwards under ``torch.no_grad()`` -- the
    ``torch.optim.swa_utils.update_bn`` procedure.

    ``loader`` items: ``(samples, targets, ...)`` tuples (the training loader), tensors, NestedTensors or ``input_pipeline.ClipBatch``es;
    ``samples.to(device)`` moves each one like the training loop does (for a ClipBatch that is the HIP pre-pass).  ``device`` defaults to
    the model's.  When ``torch.distributed`` is initialised with more than one rank, every rank must call this; running_mean /
    running_var are then averaged over the ranks, so all ranks validate with the same statistics.

    Layers the model's frozen-BatchNorm policy (``freeze_batchnorm`` / CONFIG.MODEL.FREEZE_BN) keeps in eval mode are neither reset nor
    re-estimated: their statistics are the ones the user froze.  (Layers frozen by hand with no policy set are re-estimated like the
    others and get their flag back.  The stock ``torch.optim.swa_utils.update_bn`` knows no policy: it resets every BatchNorm.)

    Every module's ``momentum`` and train / eval flag are restored afterwards, also when a forward raises.  Weights, gradients, the
    optimizer and the flat parameter store are not touched.  Returns the number of batches used on this rank."""
    if num_batches is not None:
        if isinstance(num_batches, bool) or int(num_batches) != num_batches or num_batches < 1:
            raise ValueError("num_batches must be a positive integer or None, got %r" % (num_batches,))
        num_batches = int(num_batches)
    kept = {id(m) for _, m in _policy_layers(model, getattr(model, "freeze_bn", "none"))}
    bns = [m for m in model.modules() if isinstance(m, _BatchNorm) and m.track_running_stats and m.running_mean is not None and id(m) not in kept]
    if not bns:
        return 0
    if device is None:
        device = next(model.parameters()).device
    momenta = [m.momentum for m in bns]
    modes = [(m, m.training) for m in model.modules()]
    n = 0
    try:
        for m in bns:
            m.reset_running_stats()
            m.momentum = None
        model.train()
        for m in model.modules():           # (a model whose train() knows no policy: the stub of the tests, a wrapped model)
            if id(m) in kept:
                m.training = False
        with torch.no_grad():
            for item in loader:
                model(_samples(item).to(device))
                n += 1
                if num_batches is not None and n >= num_batches:
                    break           # (before the next item: a ClipBatch loader does not decode one more batch)
        _average_over_ranks(bns)
    finally:
        for m, mom in zip(bns, momenta):
            m.momentum = mom
        for m, mode in modes:
            m.training = mode
    return n
