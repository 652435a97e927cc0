"""Frozen BatchNorm without a GPU: the FREEZE_BN config key, ``bn_stats.freeze_batchnorm`` and the policy ``DETR.train()`` re-applies,
the graph-key helpers of the captured step, ``recompute_bn_stats`` leaving policy-frozen layers alone, and the C-ABI exports."""
import os

import pytest
import torch
from torch import nn

from tubelet_transformer_amd import lib
from tubelet_transformer_amd.bn_stats import apply_freeze_policy, freeze_batchnorm, recompute_bn_stats
from tubelet_transformer_amd.config import get_cfg_defaults, load_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "configuration", "TubeR_CSN152_AVA21.yaml")


def test_config_default_and_yaml_round_trip(tmp_path):
    cfg = get_cfg_defaults()
    assert cfg.CONFIG.MODEL.FREEZE_BN == "none"
    assert load_cfg(YAML).CONFIG.MODEL.FREEZE_BN == "none"            # the published YAMLs do not name the key
    for policy in ("frozen", "all"):
        cfg.CONFIG.MODEL.FREEZE_BN = policy
        path = tmp_path / ("%s.yaml" % policy)
        path.write_text(cfg.dump())
        assert load_cfg(str(path)).CONFIG.MODEL.FREEZE_BN == policy
    cfg.merge_from_list(["CONFIG.MODEL.FREEZE_BN", "all"])
    assert cfg.CONFIG.MODEL.FREEZE_BN == "all"


def _built(name, policy="none", pretrained_freeze=False):
    from tubelet_transformer_amd.tuber import build_model
    cfg = load_cfg(YAML)
    cfg.CONFIG.MODEL.BACKBONE_NAME = name
    cfg.CONFIG.MODEL.FREEZE_BN = policy
    model = build_model(cfg)[0]
    if pretrained_freeze:             # what load_csn_mat / bench.py --pretrained-freeze do to stem + layer1 + layer2
        for n, p in model.backbone.body.named_parameters():
            if n.startswith(("conv1.", "bn1.", "layer1.", "layer2.")):
                p.requires_grad = False
    return model


def _bn_names(model):
    return [n for n, m in model.named_modules() if isinstance(m, nn.BatchNorm3d)]


@pytest.mark.parametrize("name,blocks", [("CSN-152", (3, 8, 36, 3)), ("CSN-50", (3, 4, 6, 3))])
def test_freeze_batchnorm_names_the_layers_of_each_policy(name, blocks):
    model = _built(name, pretrained_freeze=True)
    every = _bn_names(model)
    assert len(every) == 1 + 3 * sum(blocks) + 4 and all(k + ".running_mean" in model.state_dict() for k in every)
    assert freeze_batchnorm(model, "all") == every and model.freeze_bn == "all"
    assert all(not model.get_submodule(n).training for n in every)
    low = [n for n in every if n.startswith(("backbone.body.bn1", "backbone.body.layer1.", "backbone.body.layer2."))]
    assert len(low) == 1 + 3 * (blocks[0] + blocks[1]) + 2
    model.train()
    assert freeze_batchnorm(model, "frozen") == low
    model.train()
    assert [n for n in every if not model.get_submodule(n).training] == low
    assert all(p.requires_grad for n, p in model.named_parameters() if "layer3" in n)         # requires_grad is left alone
    assert freeze_batchnorm(model, "none") == []
    model.train()
    assert all(model.get_submodule(n).training for n in every)
    with pytest.raises(ValueError):
        freeze_batchnorm(model, "some")


def test_train_reapplies_each_policy_evaluated_at_the_call():
    model = _built("CSN-TEST", "all")
    every = _bn_names(model)
    assert model.freeze_bn == "all" and model.training                 # build_model stored the policy and applied it
    assert all(not model.get_submodule(n).training for n in every)
    model.eval()
    model.train()                                                      # the training loop's call at the start of every epoch
    assert all(not model.get_submodule(n).training for n in every)
    assert model.backbone.body.layer1[0].conv1.training and model.transformer.training      # only the BatchNorm layers
    model = _built("CSN-TEST", "frozen")
    model.train()
    assert all(model.get_submodule(n).training for n in every)         # nothing has requires_grad == False yet
    for p in model.backbone.body.layer1.parameters():
        p.requires_grad = False
    model.train()                                                      # evaluated at this call
    assert [n for n in every if not model.get_submodule(n).training] == [n for n in every if ".layer1." in n]
    assert apply_freeze_policy(model) == [n for n in every if ".layer1." in n]
    model = _built("CSN-TEST")
    model.backbone.body.layer2.eval()                                  # by hand, no policy: train() is nn.Module's
    model.train()
    assert all(model.get_submodule(n).training for n in every)
    assert model.eval() is model and not model.training


def test_graph_key_helpers():
    from tubelet_transformer_amd.training import _FROZEN_TAG, _frozen, _momenta
    base = ((2, 3, 32, 64, 96), ("sig",), True, 16, False)
    assert _frozen(base) == () and _frozen(base + ("last",)) == ()                 # no frozen layer: the key keeps its five entries
    mom = ((3, None), (7, 0.0))
    f1, f2 = (_FROZEN_TAG, (0, 1, 2)), (_FROZEN_TAG, (0, 1, 3))
    assert _frozen(base + (f1,)) == f1 and _frozen(base + (mom, f1, "first")) == f1
    assert _momenta(base + (f1,)) == () and _momenta(base + (mom, f1)) == mom and _momenta(base + (mom, "last")) == mom
    assert base + (f1,) != base + (f2,) != base


def test_frozen_signature_reads_the_module_flags():
    """CSNRunner.frozen_signature / GraphedTrainStep._key on a runner without a device: () while every module trains, the indices of the eval-mode
    layers otherwise -- different sets give different keys, an empty set today's key"""
    from tubelet_transformer_amd.backbone import CSNRunner
    from tubelet_transformer_amd.training import GraphedTrainStep, _frozen
    model = _built("CSN-TEST")
    runner = CSNRunner.__new__(CSNRunner)
    runner._bn_mods = [m for m in model.backbone.body.modules() if isinstance(m, nn.BatchNorm3d)]
    assert runner.frozen_signature() == () and runner.momentum_signature() == ()
    model.backbone.body.layer1[0].bn3.eval()
    model.backbone.body.bn1.eval()
    assert runner.frozen_signature() == (0, 2)

    class _Store:
        coop_off = False

        def trainable_signature(self):
            return ("t",)

    class _Model:
        def engine(self):
            return _Store(), runner
    step = GraphedTrainStep.__new__(GraphedTrainStep)
    step.model, step.criterion = _Model(), nn.Module()
    k1 = step._key((2, 3, 32, 64, 96), 16)
    model.backbone.body.layer4[1].bn4.eval()
    k2 = step._key((2, 3, 32, 64, 96), 16)
    model.train()
    k0 = step._key((2, 3, 32, 64, 96), 16)
    assert k0 == ((2, 3, 32, 64, 96), ("t",), True, 16, False)                      # today's key
    assert len({k0, k1, k2}) == 3 and _frozen(k1)[1] == (0, 2) and k1[:5] == k0
    assert step._key((2, 3, 32, 64, 96), 16, "last") == k0 + ("last",)


class _Stub(nn.Module):
    def __init__(self):
        super().__init__()
        self.backbone = nn.Sequential(nn.Linear(3, 4), nn.BatchNorm1d(4), nn.ReLU(), nn.BatchNorm1d(4, momentum=0.3))
        self.head = nn.BatchNorm1d(4)
        self.freeze_bn = "none"

    def forward(self, x):
        return self.head(self.backbone(x))


def test_recompute_bn_stats_leaves_policy_frozen_layers_alone():
    torch.manual_seed(0)
    model = _Stub()
    batches = [torch.randn(6, 3) * (1 + i) + i for i in range(4)]
    for x in batches[:2]:
        model(x)
    for p in model.backbone[1].parameters():
        p.requires_grad = False
    assert freeze_batchnorm(model, "frozen") == ["backbone.1"]
    frozen, other, head = model.backbone[1], model.backbone[3], model.head
    keep = [b.clone() for b in (frozen.running_mean, frozen.running_var, frozen.num_batches_tracked)]
    before = other.running_mean.clone()
    assert recompute_bn_stats(model, batches, num_batches=3) == 3
    for b, k in zip((frozen.running_mean, frozen.running_var, frozen.num_batches_tracked), keep):
        assert torch.equal(b, k)                                       # neither reset nor re-estimated
    assert not frozen.training and other.training and other.momentum == 0.3
    # the others: the cumulative average over the 3 batches of what they see behind the FROZEN layer (eval-mode normalisation)
    ref = _Stub()
    ref.load_state_dict(model.state_dict())
    ref.train()
    ref.backbone[1].eval()
    for m in (ref.backbone[3], ref.head):
        m.reset_running_stats()
        m.momentum = None
    with torch.no_grad():
        for x in batches[:3]:
            ref(x)
    assert int(other.num_batches_tracked) == 3 and not torch.equal(other.running_mean, before)
    for got, want in ((other, ref.backbone[3]), (head, ref.head)):
        assert torch.allclose(got.running_mean, want.running_mean, rtol=1e-5, atol=1e-6)
        assert torch.allclose(got.running_var, want.running_var, rtol=1e-5, atol=1e-6)
    # frozen by hand with no policy: today's behaviour -- re-estimated, flag restored
    model = _Stub()
    model.backbone[1].eval()
    model(batches[0])
    recompute_bn_stats(model, batches, num_batches=2)
    assert int(model.backbone[1].num_batches_tracked) == 2 and not model.backbone[1].training


def test_new_entry_points_are_exported():
    """declared in the header with the argument counts the backbone passes, and bound from the built library (a missing library fails here,
    as in test_cpu.py::test_library_exports_every_symbol_the_header_declares)"""
    declared = {name: args for _, name, args in lib.header_prototypes()}
    lib.load()
    for name, nargs in (("tuber_bn_frozen_affine_multi", 4), ("tuber_bn_frozen_param_grads", 8), ("tuber_bn_bwd_fa_frozen", 12),
                        ("tuber_dwconv_tile_bwd_data_bn_frozen", 21), ("tuber_dwconv_tile_bwd_weight_bn_frozen", 15),
                        ("tuber_dwconv_tile_bwd_both_bn_frozen", 22)):
        assert name in declared and len(declared[name]) == nargs + 1, (name, len(declared.get(name, ())))      # (+ the stream)
        assert name in lib._sigs and len(lib._sigs[name]) == nargs + 1, (name, len(lib._sigs[name]))
