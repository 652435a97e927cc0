"""The plane loop of the one-launch depthwise backward (tuber_dwconv_tile_bwd_both_bn and its frozen form): every address is a
workgroup-uniform base per tensor and plane plus a 32-bit per-thread byte offset, the eight column offsets of a thread derived from one
row offset.  Shapes where that arithmetic (and any reordering of the loop's loads and stores) can go wrong; construction and tolerances of
test_dwconv_tile_backward_with_bn_backward_folded_in (tests/test_kernels_gpu.py) and test_frozen_dwconv_tile_backward_forms
(tests/test_frozen_bn_kernels_gpu.py): dz / dgamma / dbeta bit-identical to the data-gradient kernel (another kernel body with its own
addressing), statistics rows and weight gradient against the two-launch form and fp32 torch math."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tubelet_transformer_amd import lib

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

SHAPES = [
    # tc = 4 -> chunks of 4, 4, 4, 4, 2 planes: a multi-iteration loop and a short last chunk; two channel blocks; W = 43 leaves a third
    # column tile with 11 valid columns, so both 8-column halves meet wo0 + j >= W
    (2, 18, 32, 43, 128, 64),
    (1, 6, 9, 21, 64, 7),        # row overhang (H = 9) and column overhang, tc = 1
    (2, 1, 16, 22, 64, 5),       # T = 1: both halo planes outside the volume, one plane step, no prefetch inside the loop
    (1, 2, 8, 16, 192, 3),       # exactly one tile, no overhang, three channel blocks: the base arithmetic over c0 alone
]


def rnd(*shape, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dev)


def bfr(x):
    return x.to(BF).float()


def close(name, got, ref, rel=2 ** -7, abs_=None):
    got, ref = got.float(), ref.float()
    tol = rel * float(ref.abs().max()) if abs_ is None else abs_
    err = float((got - ref).abs().max())
    print("%s: max err %.4e (tol %.4e)" % (name, err, tol))
    assert err <= tol, "%s: max err %.4e > tol %.4e" % (name, err, tol)


@functools.lru_cache(maxsize=None)
def _operands(dev, N, T, H, W, C, R):
    """random bf16 operands and partial rows whose column sums are the true statistics; shared by the two tests of a shape, never written"""
    M = N * T * H * W
    o = {"M": M}
    o["dz3"] = rnd(M, C, dev=dev, seed=1).to(BF)
    o["c3"] = (rnd(M, C, dev=dev, seed=2) * 1.5 + 0.3).to(BF)
    o["c1"] = rnd(M, C, dev=dev, seed=3).to(BF)
    o["w"] = rnd(C, 27, dev=dev, seed=4) / 5
    o["sc1"], o["sh1"] = 1.0 + 0.2 * rnd(C, dev=dev, seed=5), 0.3 * rnd(C, dev=dev, seed=6)
    o["gamma"] = 1.0 + 0.1 * rnd(C, dev=dev, seed=7)
    o["mean"], o["invstd"] = 0.3 + 0.1 * rnd(C, dev=dev, seed=8), 1.0 / (1.5 + 0.1 * rnd(C, dev=dev, seed=9).abs())
    o["s_dz"], o["s_dzx"] = o["dz3"].float().sum(0), (o["dz3"].float() * o["c3"].float()).sum(0)
    wts = (torch.rand(R, 1, generator=torch.Generator().manual_seed(6)) + 0.1).to(dev)
    wts = wts / wts.sum()
    o["st0"], o["st1"] = (wts * o["s_dz"]).contiguous(), (wts * o["s_dzx"]).contiguous()
    return o


def _reference(o, dc3, N, T, H, W, C):
    """fp32 torch math of the composite: (dz1, dW) of the depthwise conv behind relu(bn1(.)) for the gradient dc3"""
    a1 = bfr((o["c1"].float() * o["sc1"] + o["sh1"]).relu()).view(N, T, H, W, C).permute(0, 4, 1, 2, 3)
    a1 = a1.detach().requires_grad_(True)
    wt = o["w"].view(C, 1, 3, 3, 3).detach().requires_grad_(True)
    out = F.conv3d(a1, wt, padding=1, groups=C)
    out.backward(dc3.view(N, T, H, W, C).permute(0, 4, 1, 2, 3))
    mask = ((o["c1"].float() * o["sc1"] + o["sh1"]) > 0).view(N, T, H, W, C)
    return a1.grad.permute(0, 2, 3, 4, 1) * mask, wt.grad.view(C, 27)


def _check_one_launch(got, two, dw_ref, dz1_ref, Rb, C):
    """got = (dz, dgamma, dbeta, rows0, rows1, partial) of the one-launch kernel, two = (dz, dgamma, dbeta, rows0, rows1, dW) of the two launches"""
    dz1m, dgm, dbm, m0, m1, part2 = got
    dz1, dg, db, o0, o1, dwg = two
    assert bool(torch.isfinite(dz1.float()).all())
    close("two-launch dz vs fp32 reference", dz1.view(dz1_ref.shape), dz1_ref)
    assert torch.equal(dz1m, dz1), "dz: %d elements differ" % int((dz1m.float() != dz1.float()).sum())
    assert torch.equal(dgm, dg) and torch.equal(dbm, db)
    for g, want, what in ((m0, o0, "sum dz rows"), (m1, o1, "sum dz*x rows")):
        close("one-launch " + what, g.sum(0), want.sum(0), abs_=1e-5 * float(want.abs().sum(0).max()))
    dw_both = part2.view(Rb, 27, C).sum(0).t()
    close("one-launch weight gradient vs two-launch", dw_both, dwg, abs_=2e-4 * float(dwg.abs().max()))
    close("one-launch weight gradient vs fp32 reference", dw_both, dw_ref, rel=3e-3, abs_=3e-3 * float(dw_ref.abs().max()))


def _nan_outputs(dev, M, C, Rb):
    return (torch.full((M, C), float("nan"), device=dev, dtype=BF), torch.full((C,), 0.5, device=dev), torch.full((C,), 0.25, device=dev),
            torch.full((Rb, C), float("nan"), device=dev), torch.full((Rb, C), float("nan"), device=dev))


@pytest.mark.parametrize("N,T,H,W,C,R", SHAPES)
def test_bwd_both_loop_train(dev, N, T, H, W, C, R):
    o = _operands(dev, N, T, H, W, C, R)
    M, gamma, mean, invstd = o["M"], o["gamma"], o["mean"], o["invstd"]
    xhat_sum = (o["s_dzx"] - mean * o["s_dz"]) * invstd
    cA, cB = gamma * invstd, -gamma * invstd * invstd * (xhat_sum / M)
    cC = -cB * mean - gamma * invstd * (o["s_dz"] / M)
    dz1_ref, dw_ref = _reference(o, cA * o["dz3"].float() + cB * o["c3"].float() + cC, N, T, H, W, C)
    Rb = lib.query("tuber_dwconv_tile_blocks", N, T, H, W, C)
    dz1, dg, db, o0, o1 = _nan_outputs(dev, M, C, Rb)
    lib.call("tuber_dwconv_tile_bwd_data_bn", o["dz3"], o["c3"], o["st0"], o["st1"], R, float(M), gamma, mean, invstd, dg, db,
             o["w"], o["c1"], o["sc1"], o["sh1"], dz1, o0, o1, N, T, H, W, C)
    nb = lib.query("tuber_dwconv_tile_wgrad_blocks", N, T, H, W, C)
    part = torch.empty(nb * 27 * C, device=dev)
    dwg = torch.zeros(C, 27, device=dev)
    lib.call("tuber_dwconv_tile_bwd_weight_bn", o["dz3"], o["c3"], o["st0"], o["st1"], R, float(M), gamma, mean, invstd,
             o["c1"], o["sc1"], o["sh1"], part, dwg, 0, N, T, H, W, C)
    dz1m, dgm, dbm, m0, m1 = _nan_outputs(dev, M, C, Rb)
    part2 = torch.full((Rb * 27 * C,), float("nan"), device=dev)
    lib.call("tuber_dwconv_tile_bwd_both_bn", o["dz3"], o["c3"], o["st0"], o["st1"], R, float(M), gamma, mean, invstd, dgm, dbm,
             o["w"], o["c1"], o["sc1"], o["sh1"], dz1m, m0, m1, part2, N, T, H, W, C)
    torch.cuda.synchronize()
    _check_one_launch((dz1m, dgm, dbm, m0, m1, part2), (dz1, dg, db, o0, o1, dwg), dw_ref, dz1_ref, Rb, C)


@pytest.mark.parametrize("N,T,H,W,C,R", SHAPES)
def test_bwd_both_loop_frozen(dev, N, T, H, W, C, R):
    o = _operands(dev, N, T, H, W, C, R)
    M, gamma, mean, invstd = o["M"], o["gamma"], o["mean"], o["invstd"]
    dz1_ref, dw_ref = _reference(o, gamma * invstd * o["dz3"].float(), N, T, H, W, C)
    Rb = lib.query("tuber_dwconv_tile_blocks", N, T, H, W, C)
    dz1, dg, db, o0, o1 = _nan_outputs(dev, M, C, Rb)
    lib.call("tuber_dwconv_tile_bwd_data_bn_frozen", o["dz3"], o["st0"], o["st1"], R, gamma, mean, invstd, dg, db,
             o["w"], o["c1"], o["sc1"], o["sh1"], dz1, o0, o1, N, T, H, W, C)
    nb = lib.query("tuber_dwconv_tile_wgrad_blocks", N, T, H, W, C)
    part = torch.empty(nb * 27 * C, device=dev)
    dwg = torch.zeros(C, 27, device=dev)
    lib.call("tuber_dwconv_tile_bwd_weight_bn_frozen", o["dz3"], gamma, mean, invstd, o["c1"], o["sc1"], o["sh1"], part, dwg, 0, N, T, H, W, C)
    dz1m, dgm, dbm, m0, m1 = _nan_outputs(dev, M, C, Rb)
    part2 = torch.full((Rb * 27 * C,), float("nan"), device=dev)
    lib.call("tuber_dwconv_tile_bwd_both_bn_frozen", o["dz3"], o["st0"], o["st1"], R, gamma, mean, invstd, dgm, dbm,
             o["w"], o["c1"], o["sc1"], o["sh1"], dz1m, m0, m1, part2, N, T, H, W, C)
    torch.cuda.synchronize()
    _check_one_launch((dz1m, dgm, dbm, m0, m1, part2), (dz1, dg, db, o0, o1, dwg), dw_ref, dz1_ref, Rb, C)
    # frozen affine parameters: no dgamma / dbeta, no partial rows -- the same dz and the same partial blocks
    dz1q = torch.full((M, C), float("nan"), device=dev, dtype=BF)
    part3 = torch.full((Rb * 27 * C,), float("nan"), device=dev)
    lib.call("tuber_dwconv_tile_bwd_both_bn_frozen", o["dz3"], None, None, 0, gamma, mean, invstd, None, None,
             o["w"], o["c1"], o["sc1"], o["sh1"], dz1q, m0, m1, part3, N, T, H, W, C)
    torch.cuda.synchronize()
    assert torch.equal(dz1q, dz1) and torch.equal(part3, part2)


def test_bwd_both_rejects_planes_beyond_32_bit_offsets(dev):
    """a plane of H * W * C * 2 bytes = 4 GiB or more does not fit the kernel's 32-bit offsets: refused by the launcher, nothing runs"""
    C = 64
    t = torch.zeros(4096, C, device=dev, dtype=BF)
    v = torch.ones(C, device=dev)
    rows = torch.zeros(4, C, device=dev)
    out = torch.full((4096, C), 7.0, device=dev, dtype=BF)
    part = torch.full((27 * C,), 7.0, device=dev)
    w = torch.zeros(C, 27, device=dev)
    H = W = 1 << 13                      # 2^26 positions x 64 channels x 2 B = 2^33 B per plane
    with pytest.raises(RuntimeError, match="failed with code"):
        lib.call("tuber_dwconv_tile_bwd_both_bn", t, t, rows, rows, 4, 1.0, v, v, v, None, None, w, t, v, v, out, rows, rows, part, 1, 1, H, W, C)
    with pytest.raises(RuntimeError, match="failed with code"):
        lib.call("tuber_dwconv_tile_bwd_both_bn_frozen", t, None, None, 0, v, v, v, None, None, w, t, v, v, out, rows, rows, part, 1, 1, H, W, C)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((part == 7.0).all()) and bool((rows == 0).all())
