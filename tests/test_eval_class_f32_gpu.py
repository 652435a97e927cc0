"""TUBER_EVAL_PRECISION=fp32_class (round 7): the class branch once per clip, in fp32 (DETR._class_branch_f32, csrc/eval_f32.hip).

* the kernels against float64 torch: the mapped fp32 attention on the t / s / cross shapes of configs 1, 3 and 5 (T' in {1, 2, 4, 8}, K / V at
  stride 0 over the decoder layer), the strided fp32 LayerNorm, and tuber_linear_f32 at the branch's row counts;
* the model on the six full-size fixtures of tests/test_fullsize_gpu.py: pred_logits within 1.0e-2 x the output's range factor of the fp32
  oracle (the oracle's selective rounding predicts 6.4e-3 / 3.3e-3 for config 3 / its spread fixture:
  profiles/r07_oracle_selective_rounding_fp32_class.txt), no top-class flip outside the oracle's own margin, pred_boxes and pred_logits_b
  bit-identical to the default fp32_stream mode (the class branch feeds neither);
* a captured hipGraph replay equals the eager forward bit for bit; a training step does not see the variable.
"""
import os

import numpy as np
import pytest
import torch

from parity_util import flat_outputs, run_oracle, surrogate
from test_fullsize_gpu import FULL, _build, _decision_flips
from tubelet_transformer_amd import lib, synth
from tubelet_transformer_amd import tape as T

pytestmark = pytest.mark.gpu
F64 = torch.float64
SCALE = 32 ** -0.5


def _rows(m, L, nb):
    """row index of token l of sequence b under the token map m = (sL, s1, s2, B2): [nb, L]"""
    sL, s1, s2, B2 = m
    b = torch.arange(nb)[:, None]
    return torch.arange(L)[None, :] * sL + (b // B2) * s1 + (b % B2) * s2


def _attn_ref(q, qm, k, km, v, vm, nb, H, Lq, Lk):
    """float64 softmax(scale q k^T) v per (sequence, head): [nb, Lq, H * 32]"""
    qr, kr = _rows(qm, Lq, nb), _rows(km, Lk, nb)
    Q = q.double()[qr].view(nb, Lq, H, 32).transpose(1, 2)
    K = k.double()[kr].view(nb, Lk, H, 32).transpose(1, 2)
    V = v.double()[_rows(vm, Lk, nb)].view(nb, Lk, H, 32).transpose(1, 2)
    P = torch.softmax(SCALE * Q @ K.transpose(-1, -2), -1)
    return (P @ V).transpose(1, 2).reshape(nb, Lq, H * 32)


def _run_mapped(q, ldq, qm, k, ldk, km, v, ldv, vm, o, ldo, om, nb, H, Lq, Lk):
    maps = [T._map(ld, *m) for ld, m in ((ldq, qm), (ldk, km), (ldv, vm), (ldo, om))]
    lib.call("tuber_attention_f32_mapped", q, maps[0].ctypes.data, k, maps[1].ctypes.data, v, maps[2].ctypes.data, o, maps[3].ctypes.data,
             nb, H, Lq, Lk, SCALE)
    torch.cuda.synchronize()


def _check(got, want, what):
    err = float((got.double() - want).abs().max()) / max(float(want.abs().max()), 1e-30)
    print("%-48s rel err %.2e" % (what, err))
    assert err <= 1e-5, (what, err)


# (B, T', hw): configs 1 / 3 / 5 (14 x 14, 16 x 22 = 352, 18 x 24 = 432 tokens per frame)
SHAPES = [(1, 4, 196), (2, 4, 352), (2, 4, 432)]


@pytest.mark.parametrize("B,Tp,hw", SHAPES + [(2, 1, 352), (2, 2, 352), (1, 8, 196)])
def test_mapped_attention_t_and_s_against_float64(dev, B, Tp, hw):
    """t-attention (sequence over hw, batch (b, t)) and s-attention (sequence over t at stride hw, batch (b, hw)) read in place from the
    packed [q | k | v] rows (b, t, hw) of one in-projection, as the class branch calls them."""
    lib.load()
    E, H = 256, 8
    R0 = B * Tp * hw
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + Tp * 100 + hw)
    qkv = torch.randn(R0, 3 * E, generator=g).mul_(2.0).to(dev)
    qkv_h = qkv.cpu()
    for nm, m, nb, L in (("t", (1, hw, 0, 1), B * Tp, hw), ("s", (hw, Tp * hw, 1, hw), B * hw, Tp)):
        o = torch.full((R0, E), float("nan"), device=dev)
        _run_mapped(qkv, 3 * E, m, qkv.data_ptr() + 4 * E, 3 * E, m, qkv.data_ptr() + 8 * E, 3 * E, m, o, E, m, nb, H, L, L)
        want = _attn_ref(qkv_h[:, :E], m, qkv_h[:, E:2 * E], m, qkv_h[:, 2 * E:], m, nb, H, L, L)
        got = o.cpu()[_rows(m, L, nb)]
        _check(got, want, "%s-attention B %d T' %d hw %d (Lq = Lk = %d)" % (nm, B, Tp, hw, L))


@pytest.mark.parametrize("B,Tp,hw,Q", [(1, 4, 196, 15), (2, 4, 352, 15), (2, 4, 432, 10), (2, 8, 196, 15), (2, 1, 352, 10)])
def test_mapped_attention_cross_with_stride_zero_kv_against_float64(dev, B, Tp, hw, Q):
    """cross-attention: queries (layer, b, q) of the decoder output, keys / values the clip's T' * hw rows at stride 0 over the layer."""
    lib.load()
    E, H, lay_n = 256, 8, 6
    L = Tp * hw
    g = torch.Generator(device="cpu").manual_seed(7 + L + Q)
    q = torch.randn(lay_n * B * Q, E, generator=g).mul_(2.0).to(dev)
    kv = torch.randn(B * L, 2 * E, generator=g).mul_(2.0).to(dev)
    qm, km = (1, Q, 0, 1), (1, 0, L, B)
    o = torch.full((lay_n * B * Q, E), float("nan"), device=dev)
    _run_mapped(q, E, qm, kv, 2 * E, km, kv.data_ptr() + 4 * E, 2 * E, km, o, E, qm, lay_n * B, H, Q, L)
    kvh = kv.cpu()
    want = _attn_ref(q.cpu(), qm, kvh[:, :E], km, kvh[:, E:], km, lay_n * B, H, Q, L).reshape(lay_n * B * Q, E)
    _check(o.cpu(), want, "cross-attention B %d Lq %d Lk %d (x%d layers)" % (B, Q, L, lay_n))
    # the stride-0 batch really is stride 0: every layer's block of the output is the same attention over the same keys
    o1 = torch.full_like(o, float("nan"))
    _run_mapped(q, E, qm, kv, 2 * E, (1, L, 0, 1), kv.data_ptr() + 4 * E, 2 * E, (1, L, 0, 1), o1, E, qm, B, H, Q, L)
    assert torch.equal(o1[:B * Q], o[:B * Q])


def test_layernorm_rows_against_float64(dev):
    """y = LayerNorm(x + res) into a column half of a wider matrix (the [t | s] concatenation), and without a residual."""
    lib.load()
    E, M = 256, 2816 + 3
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(M, 3 * E, generator=g).mul_(3.0).add_(0.5)
    r = torch.randn(M, E, generator=g)
    ga, be = torch.randn(E, generator=g), torch.randn(E, generator=g)
    xd, rd, gd, bd = x.to(dev), r.to(dev), ga.to(dev), be.to(dev)
    y = torch.full((M, 2 * E), float("nan"), device=dev)
    lib.call("tuber_layernorm_f32_rows", xd.data_ptr() + 4 * E, 3 * E, rd, E, gd, bd, y.data_ptr() + 4 * E, 2 * E, M, E, 1e-5)
    lib.call("tuber_layernorm_f32_rows", xd, 3 * E, None, 0, gd, bd, y, 2 * E, M, E, 1e-5)
    torch.cuda.synchronize()
    ln = lambda t: torch.nn.functional.layer_norm(t.double(), (E,), ga.double(), be.double(), 1e-5)
    _check(y.cpu()[:, E:], ln(x[:, E:2 * E] + r), "layernorm rows (x + res, into columns E..2E)")
    _check(y.cpu()[:, :E], ln(x[:, :E]), "layernorm rows (no residual)")


@pytest.mark.parametrize("M,N,K", [(2816, 256, 2048), (2816, 768, 256), (2816, 256, 256), (2816, 2048, 512), (2816, 512, 256),
                                   (3456, 256, 2048), (1409, 768, 256), (1409, 256, 2048), (180, 80, 256), (180, 256, 256)])
def test_linear_f32_at_the_class_branch_shapes_against_float64(dev, M, N, K):
    """tuber_linear_f32 at the branch's row counts (2 x 1 408 rows for config 3, 2 x 1 728 for config 5, a ragged 1 409) and the class_fc /
    cross-attention rows (6 x 2 x 15): error within 1e-6 of sum |x w| (an fp32 fma chain: ~3.5e-7 at K = 4096)."""
    lib.load()
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g)
    y = torch.full((M, N), float("nan"), device=dev)
    for act in (0, 1):
        lib.call("tuber_linear_f32", x.to(dev), K, None, 0, 0, w.to(dev), K, b.to(dev), y, N, M, N, K, act)
        torch.cuda.synchronize()
        want = x.double() @ w.double().T + b.double()
        if act:
            want = want.clamp_min(0)
        bound = x.double().abs() @ w.double().abs().T + b.double().abs()
        err = float(((y.cpu().double() - want).abs() / bound).max())
        print("linear_f32 M %d N %d K %d act %d: max |err| / sum|x w| %.2e" % (M, N, K, act, err))
        assert err <= 1e-6


@pytest.mark.parametrize("case", list(FULL))
def test_fp32_class_full_size_eval_vs_oracle(dev, case, monkeypatch):
    yaml_name, B, hw, dataset = FULL[case]
    spread = case.endswith("_spread")
    cfg, model, _, state = _build(yaml_name, dev, residual_gain=0.05 if spread else None, spread=spread)
    clips = synth.structured_clips(B, 32, hw[0], hw[1], seed=1234) if spread else synth.synthetic_clips(B, 32, hw[0], hw[1], seed=1234)
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    want, _ = run_oracle(cfg, state, clips, train=False)
    x = clips.to(dev)
    names = ("pred_logits", "pred_boxes", "pred_logits_b")
    with torch.no_grad():
        monkeypatch.delenv("TUBER_EVAL_PRECISION", raising=False)
        base = {k: v.float().clone() for k, v in model(x).items() if k in names}
        monkeypatch.setenv("TUBER_EVAL_PRECISION", "fp32_class")
        got = {k: v.float().clone() for k, v in model(x).items() if k in names}
    for k in ("pred_boxes", "pred_logits_b"):
        assert torch.equal(got[k], base[k]), "%s moved under fp32_class: the mode leaked beyond the class branch" % k
    scale = max(float(np.abs(v).max()) for kk, v in flat_outputs(want).items() if kk.split(".")[-1] == "pred_logits")
    rng = max(1.0, scale / 3.0)
    err = float((got["pred_logits"].cpu() - want["pred_logits"].float()).abs().max())
    err0 = float((base["pred_logits"].cpu() - want["pred_logits"].float()).abs().max())
    print("%s: pred_logits max |err| vs the fp32 oracle: fp32_class %.2e, fp32_stream %.2e (range factor %.2f)" % (case, err, err0, rng))
    assert err <= 1.0e-2 * rng, (err, rng)
    _decision_flips(case + " [fp32_class]", got, want, dataset)


def _small(dev, train=False):
    cfg, model, crit, state = _build("TubeR_CSN152_AVA21.yaml", dev, train=train)
    return model, crit, synth.synthetic_clips(2, 32, 64, 96, seed=21, device=dev)


def test_fp32_class_eval_forward_captures_into_a_hipgraph(dev, monkeypatch):
    """the mode's forward runs the mapped fp32 kernels, no bf16 class-branch attention, and a captured replay equals it bit for bit"""
    model, _, clips = _small(dev)
    names = ("pred_logits", "pred_boxes", "pred_logits_b")

    def launches():
        seen = []
        lib.set_launch_hook(lambda name, args, launch: (seen.append(name), launch(name, *args))[1])
        try:
            with torch.no_grad():
                out = {k: v.float().clone() for k, v in model(clips).items() if k in names}
        finally:
            lib.set_launch_hook(None)
        return out, seen
    monkeypatch.delenv("TUBER_EVAL_PRECISION", raising=False)
    _, seen0 = launches()
    monkeypatch.setenv("TUBER_EVAL_PRECISION", "fp32_class")
    eager, seen = launches()
    assert seen.count("tuber_attention_f32_mapped") == 3 and seen.count("tuber_layernorm_f32_rows") == 3, seen
    assert "tuber_attention_f32_mapped" not in seen0
    assert seen0.count("tuber_attn_fwd") - seen.count("tuber_attn_fwd") == 3          # the branch's t / s / cross bf16 attentions are gone
    static = clips.clone()
    g = torch.cuda.CUDAGraph()
    with torch.no_grad():
        model(static)
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            out = model(static)
        g.replay()
        torch.cuda.synchronize()
    for k in names:
        assert torch.equal(out[k].float(), eager[k]), k


def test_training_step_ignores_fp32_class(dev, monkeypatch):
    """one eager training step with TUBER_EVAL_PRECISION=fp32_class gives the same loss and gradients, bit for bit"""
    def step():
        model, _, clips = _small(dev, train=True)
        store, _ = model.engine()
        store.manual_seed(77)
        store.zero_grad()
        out = model(clips)
        loss = surrogate(out)
        loss.backward()
        torch.cuda.synchronize()
        return float(loss), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    monkeypatch.delenv("TUBER_EVAL_PRECISION", raising=False)
    l0, g0 = step()
    monkeypatch.setenv("TUBER_EVAL_PRECISION", "fp32_class")
    l1, g1 = step()
    assert l1 == l0
    assert set(g0) == set(g1) and len(g0) > 100
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
