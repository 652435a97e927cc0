"""The frozen-BatchNorm kernels on their own (shapes of tests/test_bn_momentum_gpu.py and the layer shapes of tests/test_kernels_gpu.py):
the one-launch affine table, the frozen forms of tuber_bn_bwd_fa and of the three tuber_dwconv_tile_bwd_*_bn kernels, and dgamma / dbeta
of a frozen layer against float64 autograd of F.batch_norm(training=False)."""
import pytest
import torch
import torch.nn.functional as F

from tubelet_transformer_amd import lib

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
EPS = 1e-3


def rnd(*shape, dev, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def bfr(x):
    return x.to(BF).float()


def close(name, got, ref, rel=2 ** -7, abs_=None):
    got, ref = got.float(), ref.float()
    tol = rel * float(ref.abs().max()) if abs_ is None else abs_
    err = float((got - ref).abs().max())
    assert err <= tol, "%s: max err %.4e > tol %.4e" % (name, err, tol)


def _partial_rows(dz, x, R):
    """R row blocks of the true sums (sum dz, sum dz*x)"""
    dch, xch = dz.double().chunk(R, 0), x.double().chunk(R, 0)
    b0 = torch.stack([c.sum(0) for c in dch]).float().contiguous()
    b1 = torch.stack([(c * d).sum(0) for c, d in zip(dch, xch)]).float().contiguous()
    return b0, b1, b0.shape[0]


def _frozen_table(dev, layers):
    """device table of tuber_bn_frozen_affine_multi: one row of 12 words per layer"""
    rows = []
    for L in layers:
        rows.append([L[k].data_ptr() for k in ("gamma", "beta", "rm", "rv", "scale", "shift", "mean", "invstd", "cA", "cB", "cC")] + [L["C"]])
    return torch.tensor(rows, dtype=torch.int64).to(dev)


def _layer(dev, C, seed):
    L = {"C": C, "gamma": 1 + 0.1 * rnd(C, dev=dev, seed=seed), "beta": 0.1 * rnd(C, dev=dev, seed=seed + 1),
         "rm": 0.1 * rnd(C, dev=dev, seed=seed + 2), "rv": 0.5 + rnd(C, dev=dev, seed=seed + 3).abs()}
    for k in ("scale", "shift", "mean", "invstd", "cA", "cB", "cC"):
        L[k] = torch.full((C,), float("nan"), device=dev)
    return L


def test_frozen_affine_table_in_one_launch(dev):
    """scale / shift bit-identical to tuber_bn_eval_affine, cB = cC = 0 exactly, mean = running_mean; cA, invstd against float64 to the
    finalisation tests' 5e-6 relative; the running buffers are not written"""
    layers = [_layer(dev, C, 10 * i) for i, C in enumerate((64, 2048, 512, 256, 128, 1024, 64))]
    keep = [(L["rm"].clone(), L["rv"].clone()) for L in layers]
    table = _frozen_table(dev, layers)
    lib.call("tuber_bn_frozen_affine_multi", table, len(layers), 2048, EPS)
    torch.cuda.synchronize()
    for L, (rm, rv) in zip(layers, keep):
        C = L["C"]
        sc, sh = torch.empty(C, device=dev), torch.empty(C, device=dev)
        lib.call("tuber_bn_eval_affine", L["gamma"], L["beta"], L["rm"], L["rv"], EPS, sc, sh, C)
        assert torch.equal(L["scale"], sc) and torch.equal(L["shift"], sh), C
        assert torch.equal(L["cB"], torch.zeros_like(sc)) and torch.equal(L["cC"], torch.zeros_like(sc))
        assert torch.equal(L["mean"], L["rm"]) and torch.equal(L["rm"], rm) and torch.equal(L["rv"], rv)
        inv64 = 1.0 / torch.sqrt(L["rv"].double() + EPS)
        for got, want, what in ((L["invstd"], inv64, "invstd"), (L["cA"], L["gamma"].double() * inv64, "cA")):
            rel = float(((got.double() - want).abs() / want.abs()).max())
            assert rel <= 5e-6, (what, C, rel)
    # a table of one narrow layer; bad arguments are refused
    one = _layer(dev, 64, 99)
    lib.call("tuber_bn_frozen_affine_multi", _frozen_table(dev, [one]), 1, 64, EPS)
    assert bool(torch.isfinite(one["cA"]).all())
    with pytest.raises(Exception):
        lib.call("tuber_bn_frozen_affine_multi", table, 0, 2048, EPS)


@pytest.mark.parametrize("M,C,R", [(5632, 1024, 88), (5632, 256, 88), (2816, 2048, 44), (1408, 2048, 22), (1000, 128, 7), (2816, 512, 128)])
def test_frozen_bn_bwd_one_launch_matches_param_grads_plus_apply(dev, M, C, R):
    """tuber_bn_bwd_fa_frozen against the frozen two-launch path (tuber_bn_frozen_affine_multi's coefficients -> tuber_bn_bwd_apply, and
    tuber_bn_frozen_param_grads), held to the standard of test_bn_bwd_one_launch_matches_finalize_plus_apply: dx equal up to one bf16 ulp
    on rare elements (here cB = cC = 0, so it IS equal), dgamma / dbeta to 1e-5 rel; with NULL dgamma / dbeta the partial rows may be NULL"""
    dz = rnd(M, C, dev=dev, seed=1).to(BF)
    x = rnd(M, C, dev=dev, seed=2).to(BF)
    L = _layer(dev, C, 3)
    lib.call("tuber_bn_frozen_affine_multi", _frozen_table(dev, [L]), 1, C, EPS)
    gamma, mean, invstd = L["gamma"], L["mean"], L["invstd"]
    b0, b1, R = _partial_rows(dz, x, R)
    dg0, db0 = torch.full((C,), 0.5, device=dev), torch.full((C,), 0.25, device=dev)
    lib.call("tuber_bn_frozen_param_grads", b0, b1, R, C, mean, invstd, dg0, db0)
    dx0 = torch.empty(M, C, device=dev, dtype=BF)
    lib.call("tuber_bn_bwd_apply", dz, x, L["cA"], L["cB"], L["cC"], dx0, M, C)
    try:
        for kr in (0, 4, 8, 11):
            lib.query("tuber_bn_bwd_fa_rows_set", kr)
            dg1, db1 = torch.full((C,), 0.5, device=dev), torch.full((C,), 0.25, device=dev)
            dx1 = torch.full((M, C), float("nan"), device=dev, dtype=BF)
            lib.call("tuber_bn_bwd_fa_frozen", b0, b1, R, C, gamma, mean, invstd, dg1, db1, dz, dx1, M)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(dx1.float()).all())
            diff = (dx0.float() - dx1.float()).abs()
            assert float((diff > 0).float().mean()) < 1e-3 and float(diff.max()) <= 2 ** -7 * float(dx0.float().abs().max())
            assert torch.equal(dx1, dx0)
            close("frozen fa dgamma", dg1, dg0, rel=1e-5)
            close("frozen fa dbeta", db1, db0, rel=1e-5)
            dx2 = torch.empty(M, C, device=dev, dtype=BF)
            lib.call("tuber_bn_bwd_fa_frozen", None, None, 0, C, gamma, mean, invstd, None, None, dz, dx2, M)
            assert torch.equal(dx2, dx1)
    finally:
        lib.query("tuber_bn_bwd_fa_rows_set", 0)
    # dx is the gradient of the frozen affine map: gamma * invstd * dz
    close("frozen dx", dx0, bfr(L["cA"] * dz.float()), abs_=0.0)


@pytest.mark.parametrize("M,C,R", [(5632, 1024, 88), (1000, 128, 7), (45056, 64, 704), (3000, 2048, 300)])
def test_frozen_param_grads_match_float64_autograd(dev, M, C, R):
    """dgamma / dbeta of a frozen layer with trainable affine parameters against float64 autograd of F.batch_norm(training=False), to the
    1e-5 relative (of the largest entry) the train-mode sibling tests hold dgamma / dbeta to; accumulated (+=)"""
    dz = rnd(M, C, dev=dev, seed=1).to(BF)
    x = (rnd(M, C, dev=dev, seed=2) * 1.5 + 0.3).to(BF)
    L = _layer(dev, C, 5)
    lib.call("tuber_bn_frozen_affine_multi", _frozen_table(dev, [L]), 1, C, EPS)
    b0, b1, R = _partial_rows(dz, x, R)
    dg, db = torch.full((C,), 0.5, device=dev), torch.full((C,), 0.25, device=dev)
    lib.call("tuber_bn_frozen_param_grads", b0, b1, R, C, L["mean"], L["invstd"], dg, db)
    w = L["gamma"].double().requires_grad_(True)
    b = L["beta"].double().requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    y = F.batch_norm(x64, L["rm"].double(), L["rv"].double(), w, b, False, 0.1, EPS)
    y.backward(dz.double())
    close("frozen dgamma", (dg - 0.5).double(), w.grad, rel=1e-5)
    close("frozen dbeta", (db - 0.25).double(), b.grad, rel=1e-5)
    # and the data gradient the coefficients stand for
    dx = torch.empty(M, C, device=dev, dtype=BF)
    lib.call("tuber_bn_bwd_apply", dz, x, L["cA"], L["cB"], L["cC"], dx, M, C)
    close("frozen dx vs autograd", dx, x64.grad, rel=2 ** -8)


@pytest.mark.parametrize("N,T,H,W,C,R", [(2, 8, 16, 22, 256, 88), (2, 4, 16, 22, 512, 44), (1, 6, 9, 21, 64, 7), (2, 16, 32, 43, 128, 64)])
def test_frozen_dwconv_tile_backward_forms(dev, N, T, H, W, C, R):
    """each frozen tuber_dwconv_tile_bwd_*_bn_frozen form against the plain form fed a precomputed dc3 = cA * dz3, to the standard of
    test_dwconv_tile_backward_with_bn_backward_folded_in: fp32 torch math of the composite at `close`'s 2^-7, the weight gradient at 3e-3,
    dz1 / dgamma / dbeta of the one-launch form bit-identical to the data-gradient form, fused vs unfused dz1 to the rounding of the bf16
    dc3 (2^-6); dgamma / dbeta equal to the stand-alone frozen kernel's; NULL dgamma / dbeta take no partial rows"""
    M = N * T * H * W
    dz3 = rnd(M, C, dev=dev, seed=1).to(BF)
    c3 = (rnd(M, C, dev=dev, seed=2) * 1.5 + 0.3).to(BF)
    c1 = rnd(M, C, dev=dev, seed=3).to(BF)
    w = rnd(C, 27, dev=dev, seed=4) / 5
    sc1, sh1 = 1.0 + 0.2 * rnd(C, dev=dev, seed=5), 0.3 * rnd(C, dev=dev, seed=6)
    gamma = 1.0 + 0.1 * rnd(C, dev=dev, seed=7)
    mean, invstd = 0.3 + 0.1 * rnd(C, dev=dev, seed=8), 1.0 / (1.5 + 0.1 * rnd(C, dev=dev, seed=9).abs())
    s_dz, s_dzx = dz3.float().sum(0), (dz3.float() * c3.float()).sum(0)
    wts = (torch.rand(R, 1, generator=torch.Generator().manual_seed(6)) + 0.1).to(dev)
    wts = wts / wts.sum()
    st0, st1 = (wts * s_dz).contiguous(), (wts * s_dzx).contiguous()
    xhat_sum = (s_dzx - mean * s_dz) * invstd
    cA = gamma * invstd
    dc3 = cA * dz3.float()
    a1 = bfr((c1.float() * sc1 + sh1).relu()).view(N, T, H, W, C).permute(0, 4, 1, 2, 3)
    a1 = a1.detach().requires_grad_(True)
    wt = w.view(C, 1, 3, 3, 3).detach().requires_grad_(True)
    out = F.conv3d(a1, wt, padding=1, groups=C)
    out.backward(dc3.view(N, T, H, W, C).permute(0, 4, 1, 2, 3))
    mask = ((c1.float() * sc1 + sh1) > 0).view(N, T, H, W, C)
    dz1_ref = a1.grad.permute(0, 2, 3, 4, 1) * mask
    dw_ref = wt.grad.view(C, 27)
    # data gradient
    dg, db = torch.full((C,), 0.5, device=dev), torch.full((C,), 0.25, device=dev)
    Rb = lib.query("tuber_dwconv_tile_blocks", N, T, H, W, C)
    o0, o1 = torch.empty(Rb, C, device=dev), torch.empty(Rb, C, device=dev)
    dz1 = torch.full((M, C), float("nan"), device=dev, dtype=BF)
    lib.call("tuber_dwconv_tile_bwd_data_bn_frozen", dz3, st0, st1, R, gamma, mean, invstd, dg, db, w, c1, sc1, sh1, dz1, o0, o1, N, T, H, W, C)
    close("frozen dw bwd data", dz1.view(N, T, H, W, C), dz1_ref)
    close("frozen bn3 dgamma", dg - 0.5, xhat_sum, rel=1e-4, abs_=1e-3 * float(xhat_sum.abs().max()))
    close("frozen bn3 dbeta", db - 0.25, s_dz, rel=1e-4, abs_=1e-3 * float(s_dz.abs().max()))
    close("dz1 stats sum", o0.sum(0), dz1_ref.reshape(M, C).sum(0), abs_=2e-3 * float(dz1_ref.abs().sum(dim=(0, 1, 2, 3)).max()))
    dgs, dbs = torch.full((C,), 0.5, device=dev), torch.full((C,), 0.25, device=dev)
    lib.call("tuber_bn_frozen_param_grads", st0, st1, R, C, mean, invstd, dgs, dbs)
    close("dgamma vs the stand-alone kernel", dg, dgs, rel=1e-5)
    close("dbeta vs the stand-alone kernel", db, dbs, rel=1e-5)
    dz1n = torch.full((M, C), float("nan"), device=dev, dtype=BF)
    lib.call("tuber_dwconv_tile_bwd_data_bn_frozen", dz3, None, None, 0, gamma, mean, invstd, None, None, w, c1, sc1, sh1, dz1n, o0, o1, N, T, H, W, C)
    torch.cuda.synchronize()
    assert torch.equal(dz1n, dz1)
    # ... and NULL statistics rows of its own (a frozen bn1 with frozen affine parameters below it reads none)
    dz1z = torch.full((M, C), float("nan"), device=dev, dtype=BF)
    lib.call("tuber_dwconv_tile_bwd_data_bn_frozen", dz3, None, None, 0, gamma, mean, invstd, None, None, w, c1, sc1, sh1, dz1z, None, None, N, T, H, W, C)
    torch.cuda.synchronize()
    assert torch.equal(dz1z, dz1)
    # weight gradient
    nb = lib.query("tuber_dwconv_tile_wgrad_blocks", N, T, H, W, C)
    part = torch.empty(nb * 27 * C, device=dev)
    dwg = torch.zeros(C, 27, device=dev)
    lib.call("tuber_dwconv_tile_bwd_weight_bn_frozen", dz3, gamma, mean, invstd, c1, sc1, sh1, part, dwg, 0, N, T, H, W, C)
    close("frozen dw weight gradient", dwg, dw_ref, rel=3e-3, abs_=3e-3 * float(dw_ref.abs().max()))
    # both in one launch
    dgm, dbm = torch.full((C,), 0.5, device=dev), torch.full((C,), 0.25, device=dev)
    m0, m1 = torch.full((Rb, C), float("nan"), device=dev), torch.full((Rb, C), float("nan"), device=dev)
    dz1m = torch.full((M, C), float("nan"), device=dev, dtype=BF)
    part2 = torch.full((Rb * 27 * C,), float("nan"), device=dev)
    lib.call("tuber_dwconv_tile_bwd_both_bn_frozen", dz3, st0, st1, R, gamma, mean, invstd, dgm, dbm, w, c1, sc1, sh1, dz1m, m0, m1, part2,
             N, T, H, W, C)
    torch.cuda.synchronize()
    assert torch.equal(dz1m, dz1) and torch.equal(dgm, dg) and torch.equal(dbm, db)
    for got, want, what in ((m0, o0, "sum dz rows"), (m1, o1, "sum dz*x rows")):
        close("one-launch " + what, got.sum(0), want.sum(0), abs_=1e-5 * float(want.abs().sum(0).max()))
    dw_both = part2.view(Rb, 27, C).sum(0).t()
    close("one-launch weight gradient vs two-launch", dw_both, dwg, abs_=2e-4 * float(dwg.abs().max()))
    close("one-launch weight gradient vs fp32 reference", dw_both, dw_ref, rel=3e-3, abs_=3e-3 * float(dw_ref.abs().max()))
    dz1q = torch.full((M, C), float("nan"), device=dev, dtype=BF)
    part3 = torch.empty(Rb * 27 * C, device=dev)
    lib.call("tuber_dwconv_tile_bwd_both_bn_frozen", dz3, None, None, 0, gamma, mean, invstd, None, None, w, c1, sc1, sh1, dz1q, m0, m1, part3,
             N, T, H, W, C)
    torch.cuda.synchronize()
    assert torch.equal(dz1q, dz1) and torch.equal(part3, part2)
    # the plain forms fed the precomputed dc3 (bf16, as the unfused path stores it) agree to that rounding
    dc3_t = torch.empty(M, C, device=dev, dtype=BF)
    if C % 128 == 0:
        lib.call("tuber_bn_bwd_fa_frozen", None, None, 0, C, gamma, mean, invstd, None, None, dz3, dc3_t, M)
        assert torch.equal(dc3_t, dc3.to(BF))
    else:
        dc3_t.copy_(dc3)
    dz1_u = torch.empty(M, C, device=dev, dtype=BF)
    lib.call("tuber_dwconv_tile_bwd_data", dc3_t, w, c1, sc1, sh1, dz1_u, o0, o1, N, T, H, W, C)
    close("fused vs unfused dz1", dz1, dz1_u.float(), rel=2 ** -6)
    dwu = torch.zeros(C, 27, device=dev)
    lib.call("tuber_dwconv_tile_bwd_weight", dc3_t, c1, sc1, sh1, part, dwu, 0, N, T, H, W, C)
    close("fused vs unfused weight gradient", dwg, dwu, rel=3e-3, abs_=3e-3 * float(dw_ref.abs().max()))
