"""Weight averaging (weight_avg.py), the parts that need no GPU: the weight function against torch.optim.swa_utils on a small CPU module,
timm's warm-up ramp, the CONFIG.TRAIN.EMA keys and their validation, and the header entry of tuber_weight_average."""
import copy
import os
import re

import numpy as np
import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

from tubelet_transformer_amd.config import get_cfg_defaults, load_cfg
from tubelet_transformer_amd.lib import HEADER, header_prototypes
from tubelet_transformer_amd.weight_avg import check_settings, effective_weight, ema_settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 12
U = 2.0 ** -24


def _flat(module):
    return torch.cat([p.detach().reshape(-1) for p in module.parameters()]).clone()


def _perturb(module, gen):
    with torch.no_grad():
        for p in module.parameters():
            p.add_(torch.randn(p.shape, generator=gen) * 0.1)


def _lerp(avg, p, w):
    """the kernel's update in fp32 tensor arithmetic: avg += w * (p - avg), w == 1 copies"""
    return p.clone() if w == 1.0 else avg + np.float32(w) * (p - avg)


def _bound(k, *tensors):
    return 4 * k * U * max(float(t.abs().max()) for t in tensors)


def test_swa_weights_reproduce_torch_averaged_model():
    gen = torch.Generator().manual_seed(3)
    m = torch.nn.Linear(7, 5)
    ref = AveragedModel(m)
    avg = _flat(m)                                  # this averager starts as a copy of the parameters
    for n in range(1, K + 1):
        _perturb(m, gen)
        ref.update_parameters(m)
        w = effective_weight("swa", 0.5, False, n)
        assert w == float(np.float32(1.0 / n))
        avg = _lerp(avg, _flat(m), w)
        if n == 1:
            assert torch.equal(avg, _flat(m))       # the first update is a copy, as in AveragedModel
        err = float((avg - _flat(ref.module)).abs().max())
        assert err <= _bound(n, avg, _flat(m)), (n, err)
    assert int(ref.n_averaged) == K


def test_ema_weights_reproduce_torch_ema_multi_avg_fn_one_update_apart():
    d = 0.9
    gen = torch.Generator().manual_seed(4)
    m = torch.nn.Linear(7, 5)
    ref = AveragedModel(m, multi_avg_fn=get_ema_multi_avg_fn(d))
    _perturb(m, gen)
    ref.update_parameters(m)                        # torch's first update copies ...
    avg = _flat(m)                                  # ... which is this averager's construction
    assert torch.equal(avg, _flat(ref.module))
    for n in range(1, K + 1):                       # this averager's update n is torch's update n + 1
        _perturb(m, gen)
        ref.update_parameters(m)
        w = effective_weight("ema", d, False, n)
        assert w == float(np.float32(1.0 - float(np.float32(d))))
        avg = _lerp(avg, _flat(m), w)
        err = float((avg - _flat(ref.module)).abs().max())
        assert err <= _bound(n, avg, _flat(m)), (n, err)
    assert int(ref.n_averaged) == K + 1


@pytest.mark.parametrize("n", [1, 2, 10, 10 ** 6])
def test_warmup_ramp_is_timms(n):
    d = 0.9999
    d32 = float(np.float32(d))
    want = 1.0 - min(d32, (1.0 + n) / (10.0 + n))
    got = effective_weight("ema", d, True, n)
    assert got == float(np.float32(want))
    assert abs(got - want) <= U * want
    if n <= 10:
        assert got > effective_weight("ema", d, False, n)      # the ramp is below the decay early on
    else:
        assert got == effective_weight("ema", d, False, n)     # ... and the decay itself in the long run


def test_effective_weight_rejects_bad_arguments():
    with pytest.raises(ValueError):
        effective_weight("mean", 0.9, False, 1)
    with pytest.raises(ValueError):
        effective_weight("ema", 0.9, False, 0)


def test_config_defaults_are_present_and_off():
    for cfg in (get_cfg_defaults(), load_cfg(os.path.join(ROOT, "configuration", "TubeR_CSN152_AVA21.yaml"))):
        E = cfg.CONFIG.TRAIN.EMA
        assert dict(E) == {"ENABLE": False, "MODE": "ema", "DECAY": 0.9999, "WARMUP": False, "START": 0, "PERIOD": 1, "EVAL": True}
        s = ema_settings(cfg)
        assert s["enable"] is False and s["eval"] is True and s["mode"] == "ema" and s["decay"] == 0.9999
        assert cfg.to_dict()["CONFIG"]["TRAIN"]["EMA"]["ENABLE"] is False
    other = copy.deepcopy(cfg)
    other.merge_from_list(["CONFIG.TRAIN.EMA.ENABLE", "True", "CONFIG.TRAIN.EMA.MODE", "swa", "CONFIG.TRAIN.EMA.PERIOD", "8"])
    s = ema_settings(other)
    assert s["enable"] is True and s["mode"] == "swa" and s["period"] == 8
    assert cfg.CONFIG.TRAIN.EMA.ENABLE is False


@pytest.mark.parametrize("key,value", [("DECAY", -0.1), ("DECAY", 1.5), ("DECAY", "high"), ("PERIOD", 0), ("PERIOD", -3), ("PERIOD", 1.5),
                                       ("MODE", "mean"), ("START", -1), ("WARMUP", 2), ("ENABLE", "yes"), ("EVAL", 1)])
def test_bad_config_values_raise_and_name_the_key(key, value):
    cfg = get_cfg_defaults()
    cfg.CONFIG.TRAIN.EMA[key] = value
    with pytest.raises(ValueError, match=r"CONFIG\.TRAIN\.EMA\.%s\b" % key):
        ema_settings(cfg)


def test_check_settings_accepts_the_range_ends():
    assert check_settings("ema", 0, False, 0, 1) == ("ema", 0.0, False, 0, 1)
    assert check_settings("swa", 1.0, True, 5, 8) == ("swa", 1.0, True, 5, 8)


def test_header_declares_the_entry_point_with_a_doc():
    protos = {n: (r, a) for r, n, a in header_prototypes(HEADER)}
    assert "tuber_weight_average" in protos
    ret, args = protos["tuber_weight_average"]
    assert ret == "int"
    assert [a for _, a in args] == ["avg", "p", "n", "table", "n_avg", "step_ptr", "clip", "stream"]
    assert args[1][0].startswith("const float") and args[-1][0] == "hipStream_t"
    text = open(HEADER).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int tuber_weight_average\(", text, flags=re.S)
    assert m is not None
    doc = " ".join(l.strip(" *") for l in m.group(1).splitlines()).strip()
    assert len(doc) > 80 and "undocumented" not in doc and "avg" in doc
