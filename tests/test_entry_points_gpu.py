"""Direct parity tests of the entry points the model-level checks only see through loose bounds: the LSTR wide-head attention, the
layer1 BatchNorm statistics chain, the depthwise weight-gradient reduction, the eval-mode BatchNorm affine table, the fp32-stream
LayerNorm, the fused criterion's edge cases and the small elementwise launchers.  References are fp64 on the bf16-rounded values the
kernel sees; outputs are prefilled with NaN (or a sentinel) so that an element the kernel never writes fails the comparison."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tubelet_transformer_amd import lib

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def rnd(*shape, dev, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def close(name, got, ref, rel=2 ** -7, abs_=None):
    got, ref = got.double(), ref.double()
    scale = float(ref.abs().max()) + 1e-12
    err = float((got - ref).abs().max())
    tol = rel * scale if abs_ is None else abs_
    print("%-52s max|err| %.3e  (scale %.3e, tol %.3e)" % (name, err, scale, tol))
    assert math.isfinite(err) and err <= tol, "%s: err %.3e > tol %.3e" % (name, err, tol)


def close_each(name, got, ref, tol):
    """element-wise bound: |got - ref| <= tol (a tensor of the same shape); NaN anywhere fails"""
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    ratio = float((err / tol).max()) if err.numel() else 0.0
    print("%-52s max|err| %.3e  max err/tol %.3f" % (name, float(err.max()) if err.numel() else 0.0, ratio))
    assert bool(torch.isfinite(got).all()), "%s: non-finite (unwritten?) elements" % name
    assert ratio <= 1.0, "%s: err/tol %.3f" % (name, ratio)


def rc(name, *args):
    """the launcher's return code, without lib.call's raise (argument-check tests)"""
    fn = getattr(lib.load(), name)
    sig = lib._sigs[name]
    if len(args) == len(sig) - 1:
        args = args + (lib.current_stream(),)
    return fn(*[lib._conv(v, t) for v, (t, _) in zip(args, sig)])


def nan(*shape, dev, dtype=torch.float32):
    return torch.full(shape, float("nan"), device=dev, dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# tuber_attn_wide_fwd / _bwd: LSTR pooling decoder, one query per pixel, 8 heads of 256 over T <= 8 temporal slots
# ---------------------------------------------------------------------------------------------------------------------------------
def _wide_rows(NQ, HW, T, dev):
    """kv row of (pixel, t): T == 1 -> pixel (self-attention), else (b*T + t)*HW + hw"""
    pix = torch.arange(NQ, device=dev)
    if T == 1:
        return pix[:, None], NQ
    b, hw = pix // HW, pix % HW
    t = torch.arange(T, device=dev)
    return (b[:, None] * T + t[None, :]) * HW + hw[:, None], (NQ // HW) * T * HW


def _wide_ref(q, kv, rows, T, keep=None):
    """softmax(q.k^T * 0.0625) (* keep) . v per 256-wide head, fp64 autograd leaves"""
    NQ = q.shape[0]
    q64 = q.double().requires_grad_(True)
    kv64 = kv.double().requires_grad_(True)
    g = kv64[rows.reshape(-1)].view(NQ, T, 4096)
    k, v = g[..., :2048].view(NQ, T, 8, 256), g[..., 2048:].view(NQ, T, 8, 256)
    s = torch.einsum("nhd,nthd->nht", q64.view(NQ, 8, 256), k) * 0.0625
    p = torch.softmax(s, -1)
    if keep is not None:
        p = p * keep
    o = torch.einsum("nht,nthd->nhd", p, v).reshape(NQ, 2048)
    return q64, kv64, o


@pytest.mark.parametrize("T", [1, 3, 4, 8])
@pytest.mark.parametrize("NQ,HW", [(704, 352), (21, 7)])
def test_attn_wide_fwd_bwd(dev, NQ, HW, T):
    """tuber_attn_wide_fwd / _bwd with pdrop = 0 against fp64 autograd of softmax(q k^T / 16) v per head, at the model's NQ = 704
    (2 clips x 16 x 22) and a small odd NQ, T = 1 (row = pixel) and T > 1 ((b*T + t)*HW + hw) addressing up to WT_MAX = 8.
    Tolerance 2^-7 of the output scale: bf16 stores of fp32 math (one rounding, 2^-8 relative) plus fp32 reduction noise."""
    rows, nrows = _wide_rows(NQ, HW, T, dev)
    q = rnd(NQ, 2048, dev=dev, seed=1).to(BF)
    kv = rnd(nrows, 4096, dev=dev, seed=2).to(BF)
    seed_t = torch.full((1,), 11, dtype=torch.int64, device=dev)
    o = nan(NQ, 2048, dev=dev, dtype=BF)
    lib.call("tuber_attn_wide_fwd", q, kv, o, NQ, HW, T, 0.0, seed_t, 5)
    q64, kv64, ref = _wide_ref(q, kv, rows, T)
    close("attn_wide fwd NQ=%d T=%d" % (NQ, T), o, ref.detach())
    dO = rnd(NQ, 2048, dev=dev, seed=3).to(BF)
    ref.backward(dO.double())
    dq, dkv = nan(NQ, 2048, dev=dev, dtype=BF), nan(nrows, 4096, dev=dev, dtype=BF)
    lib.call("tuber_attn_wide_bwd", q, kv, dO, dq, dkv, NQ, HW, T, 0.0, seed_t, 5)
    close("attn_wide bwd dq NQ=%d T=%d" % (NQ, T), dq, q64.grad)
    close("attn_wide bwd dk NQ=%d T=%d" % (NQ, T), dkv[:, :2048], kv64.grad[:, :2048])
    close("attn_wide bwd dv NQ=%d T=%d" % (NQ, T), dkv[:, 2048:], kv64.grad[:, 2048:])


@pytest.mark.parametrize("T", [1, 4, 8])
@pytest.mark.parametrize("NQ,HW", [(704, 352), (21, 7)])
def test_attn_wide_dropout_forward_and_backward_use_one_mask(dev, NQ, HW, T):
    """pdrop = 0.1: a first forward with V one-hot per slot (v[row(pix, t), head*256 + t] = 1) returns o[pix, head*256 + t] =
    p_t * keep_t, which exposes the keep mask.  The mask depends on (seed, salt, pixel, head, t) only, so a second call with the same
    seed and salt on random V must equal fp64 autograd of (softmax * keep / 0.9) . v -- and so must the backward's dq / dk / dv, which
    fails if the backward draws its mask at other indices than the forward.  Tolerances as in test_attn_wide_fwd_bwd."""
    p = 0.1
    rows, nrows = _wide_rows(NQ, HW, T, dev)
    q = rnd(NQ, 2048, dev=dev, seed=4, scale=0.5).to(BF)
    kv = rnd(nrows, 4096, dev=dev, seed=5, scale=0.5).to(BF)
    seed_t = torch.full((1,), 23, dtype=torch.int64, device=dev)
    salt = 991
    onehot = kv.clone()
    onehot[:, 2048:] = 0
    tt = torch.arange(T, device=dev)
    for h in range(8):                                  # slot t of every pixel carries a 1 in column head*256 + t of its head
        onehot[rows.reshape(-1), 2048 + h * 256 + tt.repeat(NQ)] = 1
    pd = nan(NQ, 2048, dev=dev, dtype=BF)
    lib.call("tuber_attn_wide_fwd", q, onehot, pd, NQ, HW, T, p, seed_t, salt)
    probe = pd.float().view(NQ, 8, 256)[:, :, :T]                                       # [NQ, 8, T] = p_t * keep_t
    assert bool(torch.isfinite(probe).all())
    keep = (probe > 0).double() / (1 - p)
    frac = float((probe > 0).float().mean())
    print("attn_wide dropout keep fraction %.3f (expected %.2f)" % (frac, 1 - p))
    assert 0.75 < frac < 0.99
    _, _, ref_p = _wide_ref(q, onehot, rows, T, keep)
    close("attn_wide dropout probe == p*keep", pd, ref_p.detach())

    kv2 = rnd(nrows, 4096, dev=dev, seed=6).to(BF)
    o = nan(NQ, 2048, dev=dev, dtype=BF)
    lib.call("tuber_attn_wide_fwd", q, kv2, o, NQ, HW, T, p, seed_t, salt)
    q64, kv64, ref = _wide_ref(q, kv2, rows, T, keep)
    close("attn_wide dropout fwd NQ=%d T=%d" % (NQ, T), o, ref.detach())
    dO = rnd(NQ, 2048, dev=dev, seed=7).to(BF)
    ref.backward(dO.double())
    dq, dkv = nan(NQ, 2048, dev=dev, dtype=BF), nan(nrows, 4096, dev=dev, dtype=BF)
    lib.call("tuber_attn_wide_bwd", q, kv2, dO, dq, dkv, NQ, HW, T, p, seed_t, salt)
    close("attn_wide dropout bwd dq NQ=%d T=%d" % (NQ, T), dq, q64.grad)
    close("attn_wide dropout bwd dk NQ=%d T=%d" % (NQ, T), dkv[:, :2048], kv64.grad[:, :2048])
    close("attn_wide dropout bwd dv NQ=%d T=%d" % (NQ, T), dkv[:, 2048:], kv64.grad[:, 2048:])


def test_attn_wide_rejects_bad_arguments(dev):
    """T outside [1, WT_MAX = 8] and pdrop = 1 return TUBER_EINVAL before any launch: the NaN-filled outputs stay NaN."""
    NQ, HW = 14, 7
    q = rnd(NQ, 2048, dev=dev, seed=1).to(BF)
    kv = rnd(2 * 9 * HW, 4096, dev=dev, seed=2).to(BF)
    seed_t = torch.full((1,), 1, dtype=torch.int64, device=dev)
    for T, p in ((0, 0.0), (9, 0.0), (4, 1.0)):
        o, dq, dkv = nan(NQ, 2048, dev=dev, dtype=BF), nan(NQ, 2048, dev=dev, dtype=BF), nan(2 * 9 * HW, 4096, dev=dev, dtype=BF)
        assert rc("tuber_attn_wide_fwd", q, kv, o, NQ, HW, T, p, seed_t, 3) == EINVAL, (T, p)
        assert rc("tuber_attn_wide_bwd", q, kv, q, dq, dkv, NQ, HW, T, p, seed_t, 3) == EINVAL, (T, p)
        torch.cuda.synchronize()
        assert bool(o.isnan().all() and dq.isnan().all() and dkv.isnan().all()), (T, p)


# ---------------------------------------------------------------------------------------------------------------------------------
# layer1 BatchNorm statistics: tuber_gemm_nt (stats epilogue) -> tuber_stat_rows_reduce -> tuber_bn_finalize
# ---------------------------------------------------------------------------------------------------------------------------------
def _stats_gemm(A, B):
    """tuber_gemm_nt with the statistics epilogue as the backbone calls it (_gemm_stats), partial rows NaN-prefilled"""
    dev = A.device
    M, K = A.shape
    N = B.shape[0]
    R = lib.query("tuber_gemm_nt_stat_rows", M, N)
    C = nan(M, N, dev=dev, dtype=BF)
    st0, st1 = nan(R, N, dev=dev), nan(R, N, dev=dev)
    lib.call("tuber_gemm_nt", A, K, B, K, C, N, M, N, K, 0, None, None, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, None, None, 0, 0, 0,
             st0, st1, None, 0, None, None, 1.0, 0.0, None, 0, None, 0, None)
    return C, st0, st1, R


def _moments(A, B):
    """fp64 per-channel mean and variance of the fp32 accumulator A . B^T (what the epilogue sums), through the column means and
    the covariance of A: exact to fp64 rounding, without forming the M x N product"""
    A64, B64 = A.double(), B.double()
    M = A64.shape[0]
    mu = A64.mean(0)
    cov = (A64 - mu).t() @ (A64 - mu) / M
    return B64 @ mu, ((B64 @ cov) * B64).sum(1)


def _finalize(o0, o1, R, N, M, dev, gamma, beta, rm0, rv0, mom=0.1):
    rm, rv = rm0.clone(), rv0.clone()
    nbt = torch.full((1,), 7, dtype=torch.int64, device=dev)
    outs = [nan(N, dev=dev) for _ in range(4)]
    lib.call("tuber_bn_finalize", o0, o1, R, N, float(M), gamma, beta, rm, rv, nbt, mom, 1e-5, *outs)
    return (*outs, rm, rv, nbt)


@pytest.mark.parametrize("N", [64, 256])
@pytest.mark.parametrize("M", [348160, 442368])
def test_layer1_bn_statistics_chain(dev, M, N):
    """The layer1 statistics path of a training forward (backbone._gemm_stats -> _stat_rows -> _bn_train) at the AVA (348 160) and
    JHMDB (442 368) layer1 row counts, on NON-NEGATIVE A (post-ReLU input), so every channel has a non-zero mean and E[x^2] - mean^2
    cancels.  The epilogue sums the fp32 accumulator (gemm.hip EPI_STATS), so the reference is the fp64 mean / variance of the exact
    products.  Tolerances: mean within 1e-5 of the channel's rms, variance within 1e-5 of E[x^2] (fp32 partial sums over 64 / 96-row
    tiles and row chunks: ~1e-6 relative each); scale / shift within 1e-6 relative of the fp64 formula on the kernel's own mean / invstd
    (fp32 rounding); running statistics (momentum 0.1, unbiased variance) within 1e-5 of their magnitude; num_batches_tracked + 1."""
    K = 64
    A = rnd(M, K, dev=dev, seed=1).abs().to(BF)
    B = rnd(N, K, dev=dev, seed=2, scale=K ** -0.5).to(BF)
    _, st0, st1, R = _stats_gemm(A, B)
    R2 = lib.query("tuber_stat_rows_reduced", R)
    assert R2 < R, "layer1 statistics rows must take the first-stage reduction"
    o0, o1 = nan(R2, N, dev=dev), nan(R2, N, dev=dev)
    lib.call("tuber_stat_rows_reduce", st0, st1, R, N, o0, o1)
    gamma, beta = 1.0 + 0.2 * rnd(N, dev=dev, seed=5), 0.3 * rnd(N, dev=dev, seed=6)
    rm0, rv0 = 0.5 * rnd(N, dev=dev, seed=7), 0.5 + rnd(N, dev=dev, seed=8).abs()
    scale, shift, mean, invstd, rm, rv, nbt = _finalize(o0, o1, R2, N, M, dev, gamma, beta, rm0, rv0)
    m_ref, v_ref = _moments(A, B)
    ex2 = v_ref + m_ref ** 2
    print("layer1 stats M=%d N=%d: R=%d -> %d rows, max |mean|/std %.2f" % (M, N, R, R2, float((m_ref.abs() / v_ref.sqrt()).max())))
    assert float((m_ref.abs() / v_ref.sqrt()).max()) > 1.0          # the cancellation the test is about is present
    close_each("layer1 mean", mean, m_ref, 1e-5 * ex2.sqrt())
    var_k = 1.0 / invstd.double() ** 2 - 1e-5
    close_each("layer1 variance (from invstd)", var_k, v_ref, 1e-5 * ex2)
    sc64 = gamma.double() * invstd.double()
    close_each("layer1 scale", scale, sc64, 1e-6 * sc64.abs())
    close_each("layer1 shift", shift, beta.double() - mean.double() * sc64, 1e-6 * (beta.double().abs() + (mean.double() * sc64).abs()))
    unb = v_ref * M / (M - 1)
    close_each("layer1 running_mean", rm, 0.9 * rm0.double() + 0.1 * m_ref, 1e-5 * (rm0.double().abs() + ex2.sqrt()))
    close_each("layer1 running_var", rv, 0.9 * rv0.double() + 0.1 * unb, 1e-5 * (rv0.double().abs() + ex2))
    assert int(nbt) == 8


@pytest.mark.parametrize("ratio", [10.0, 100.0])
def test_layer1_bn_variance_error_at_large_mean(dev, ratio):
    """Evidence, not a gate: the relative variance error of the same chain when mean / std = 10 and 100 (one-pass E[x^2] - mean^2
    in fp32 partial sums).  Nobody has measured how far the model's own BatchNorm inputs go, so the number is printed; only
    finiteness is asserted."""
    M, N, K = 348160, 64, 64
    A = rnd(M, K, dev=dev, seed=1)
    A[:, 0] = 1.0
    A = A.to(BF)
    B = rnd(N, K, dev=dev, seed=2, scale=(K - 1) ** -0.5)
    B[:, 0] = ratio
    B = B.to(BF)
    _, st0, st1, R = _stats_gemm(A, B)
    R2 = lib.query("tuber_stat_rows_reduced", R)
    o0, o1 = nan(R2, N, dev=dev), nan(R2, N, dev=dev)
    lib.call("tuber_stat_rows_reduce", st0, st1, R, N, o0, o1)
    ones, zeros = torch.ones(N, device=dev), torch.zeros(N, device=dev)
    _, _, mean, invstd, _, _, _ = _finalize(o0, o1, R2, N, M, dev, ones, zeros, zeros.clone(), ones.clone())
    m_ref, v_ref = _moments(A, B)
    var_k = 1.0 / invstd.double() ** 2 - 1e-5
    rel = ((var_k - v_ref).abs() / v_ref)
    print("layer1 stats at mean/std ~ %.0f: max relative variance error %.3e (median %.3e), max relative mean error %.3e" % (
        float((m_ref / v_ref.sqrt()).abs().median()), float(rel.max()), float(rel.median()),
        float(((mean.double() - m_ref).abs() / m_ref.abs()).max())))
    assert bool(torch.isfinite(var_k).all())


@pytest.mark.parametrize("C", [100, 64, 256])
@pytest.mark.parametrize("R", [513, 1000, 5440])
def test_stat_rows_reduce(dev, R, C):
    """tuber_stat_rows_reduce on its own: R = 513 (just over the 512-row threshold), 1000 (not a multiple of 64: a chunk tail) and the
    AVA layer1 5 440; C = 100 has C % 4 == 0 but a partial 32-channel block.  Output row j must be the fp64 sum of input rows
    [j*chunk, min(R, (j+1)*chunk)), chunk = ceil(R / 64) (empty chunks: 0), within 1e-5 of the chunk's sum of |x| -- a dropped or doubled
    row is off by a whole |x|."""
    R2 = lib.query("tuber_stat_rows_reduced", R)
    assert R2 == 64
    st0, st1 = rnd(R, C, dev=dev, seed=1), rnd(R, C, dev=dev, seed=2).abs()
    o0, o1 = nan(R2, C, dev=dev), nan(R2, C, dev=dev)
    lib.call("tuber_stat_rows_reduce", st0, st1, R, C, o0, o1)
    chunk = -(-R // R2)
    idx = torch.arange(R, device=dev) // chunk
    for name, src, got in (("sum", st0, o0), ("sumsq", st1, o1)):
        ref = torch.zeros(R2, C, dtype=torch.float64, device=dev).index_add_(0, idx, src.double())
        mag = torch.zeros(R2, C, dtype=torch.float64, device=dev).index_add_(0, idx, src.double().abs())
        close_each("stat_rows_reduce %s R=%d C=%d" % (name, R, C), got, ref, 1e-5 * mag + 1e-30)


def test_stat_rows_reduce_rejects_bad_arguments(dev):
    """R <= 512 (no first stage) and C % 4 != 0 return TUBER_EINVAL without writing."""
    st = rnd(1024, 104, dev=dev, seed=1)
    for R, C in ((512, 64), (100, 64), (1000, 102)):
        o0, o1 = nan(64, 104, dev=dev), nan(64, 104, dev=dev)
        assert rc("tuber_stat_rows_reduce", st, st, R, C, o0, o1) == EINVAL, (R, C)
        torch.cuda.synchronize()
        assert bool(o0.isnan().all() and o1.isnan().all())


# ---------------------------------------------------------------------------------------------------------------------------------
# tuber_dw_wgrad_reduce: second stage of the depthwise weight gradient
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(32, 64, 85, 64), (16, 32, 43, 128), (8, 16, 22, 256), (4, 8, 11, 512), (16, 32, 43, 96)])
def test_dw_wgrad_reduce(dev, shape):
    """dw[c][tap] (+)= sum_r partial[r][tap][c] with R = tuber_dwconv_tile_wgrad_blocks of the AVA layer1-4 depthwise shapes (2 clips),
    C = 64 ... 512 and C = 96 (not a multiple of 64).  accumulate = 0 must overwrite a NaN-filled dw, accumulate = 1 add onto a random
    one.  Tolerance 1e-5 of sum_r |partial| (+ |dw| when accumulating): fp32 sums of R partial rows."""
    T, H, W, C = shape
    R = lib.query("tuber_dwconv_tile_wgrad_blocks", 2, T, H, W, C)
    assert R > 0
    P = rnd(R, 27, C, dev=dev, seed=R + C)
    ref = P.double().sum(0).t()                                     # [C, 27]
    mag = P.double().abs().sum(0).t()
    dw = nan(C, 27, dev=dev)
    lib.call("tuber_dw_wgrad_reduce", P, dw, R, C, 0)
    close_each("dw_wgrad_reduce overwrite R=%d C=%d" % (R, C), dw, ref, 1e-5 * mag + 1e-30)
    dw0 = rnd(C, 27, dev=dev, seed=9)
    dw = dw0.clone()
    lib.call("tuber_dw_wgrad_reduce", P, dw, R, C, 1)
    close_each("dw_wgrad_reduce accumulate R=%d C=%d" % (R, C), dw, dw0.double() + ref, 1e-5 * (mag + dw0.double().abs()) + 1e-30)


# ---------------------------------------------------------------------------------------------------------------------------------
# tuber_bn_eval_affine_multi: every BatchNorm's eval affine map in one launch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_bn_eval_affine_multi(dev):
    """A device table of rows with C = 64 ... 2048, including C = 1000 < cmax (not a multiple of 256) and C = 100: every row's scale and
    shift must be bit-identical to tuber_bn_eval_affine on that row and within 1e-6 relative of the fp64 formula (fp32 add, sqrt,
    divide, multiply-add: a few ulp); running_var down to 1e-3 makes eps = 1e-5 visible at 5e-3 relative.  16 guard words after each
    row's scale / shift buffers must keep their sentinel."""
    Cs = [64, 2048, 256, 1000, 512, 100, 128]
    cmax, eps, G = max(Cs), 1e-5, 16
    rows, bufs = [], []
    for i, C in enumerate(Cs):
        gamma, beta = 1.0 + 0.3 * rnd(C, dev=dev, seed=10 * i), 0.2 * rnd(C, dev=dev, seed=10 * i + 1)
        rmean = rnd(C, dev=dev, seed=10 * i + 2)
        rvar = rnd(C, dev=dev, seed=10 * i + 3).abs() + 1e-3
        sc = torch.full((C + G,), 12345.0, device=dev)
        sh = torch.full((C + G,), -54321.0, device=dev)
        sc[:C], sh[:C] = float("nan"), float("nan")
        rows.append([gamma.data_ptr(), beta.data_ptr(), rmean.data_ptr(), rvar.data_ptr(), sc.data_ptr(), sh.data_ptr(), C, 0])
        bufs.append((C, gamma, beta, rmean, rvar, sc, sh))
    table = torch.tensor(rows, dtype=torch.int64).to(dev)
    lib.call("tuber_bn_eval_affine_multi", table, len(Cs), cmax, eps)
    torch.cuda.synchronize()
    for C, gamma, beta, rmean, rvar, sc, sh in bufs:
        s1, h1 = nan(C, dev=dev), nan(C, dev=dev)
        lib.call("tuber_bn_eval_affine", gamma, beta, rmean, rvar, eps, s1, h1, C)
        assert torch.equal(sc[:C], s1) and torch.equal(sh[:C], h1), "row C=%d differs from tuber_bn_eval_affine" % C
        ref_sc = gamma.double() / torch.sqrt(rvar.double() + eps)
        ref_sh = beta.double() - rmean.double() * ref_sc
        close_each("bn_eval_affine_multi scale C=%d" % C, sc[:C], ref_sc, 1e-6 * ref_sc.abs())
        close_each("bn_eval_affine_multi shift C=%d" % C, sh[:C], ref_sh, 1e-6 * (beta.double().abs() + (rmean.double() * ref_sc).abs()))
        assert bool((sc[C:] == 12345.0).all() and (sh[C:] == -54321.0).all()), "guard words after row C=%d overwritten" % C


# ---------------------------------------------------------------------------------------------------------------------------------
# tuber_layernorm_fwd_f32: the eval precision mode's LayerNorm with an fp32 residual stream
# ---------------------------------------------------------------------------------------------------------------------------------
# (x fp32 twin given, residual: None / "bf16" / "f32", y32 written, extra columns of ldy) -- the operand forms tape.py:516-518 passes
LN_FORMS = [(False, None, True, 0), (True, None, False, 0), (False, "bf16", True, 8), (True, "bf16", True, 0),
            (False, "f32", False, 64), (True, "f32", True, 128)]


@pytest.mark.parametrize("form", LN_FORMS, ids=lambda f: "x32%d-res%s-y32%d-pad%d" % (f[0], f[1], f[2], f[3]))
@pytest.mark.parametrize("M,E", [(30, 256), (704, 256), (2816, 256), (30, 2048), (704, 2048), (2816, 2048)])
def test_layernorm_fwd_f32(dev, M, E, form):
    """LayerNorm(x + res) against fp64 F.layer_norm on the values the kernel reads (x32 over x, res32 over res), a quarter of the rows
    at mean 100 / std 1 (the cancellation case).  y32 within 1e-5 of the output scale (fp32 two-pass statistics); the bf16 y within
    one bf16 rounding of the reference (2^-8 of the element) plus that fp32 error, and equal to bf16(y32) when y32 is written.  Columns
    [E, ldy) of y keep their sentinel."""
    use_x32, res_kind, want_y32, pad = form
    ldy = E + pad
    x32 = rnd(M, E, dev=dev, seed=1)
    x32[: M // 4] += 100.0
    x = x32.to(BF)
    xin = x32 if use_x32 else x.float()
    res = res32 = None
    rin = torch.zeros_like(x32)
    if res_kind == "bf16":
        res = rnd(M, E, dev=dev, seed=2).to(BF)
        rin = res.float()
    elif res_kind == "f32":
        res32 = rnd(M, E, dev=dev, seed=2)
        res = res32.to(BF)                      # the bf16 twin travels along; the fp32 stream takes precedence
        rin = res32
    gamma, beta = 1.0 + 0.2 * rnd(E, dev=dev, seed=3), 0.3 * rnd(E, dev=dev, seed=4)
    y = torch.full((M, ldy), -3.0, device=dev, dtype=BF)
    y[:, :E] = float("nan")
    y32 = nan(M, E, dev=dev) if want_y32 else None
    lib.call("tuber_layernorm_fwd_f32", x, x32 if use_x32 else None, res, res32, gamma, beta, y, ldy, y32, M, E, 1e-5)
    ref = F.layer_norm(xin.double() + rin.double(), (E,), gamma.double(), beta.double(), eps=1e-5)
    scale = float(ref.abs().max())
    tag = "M=%d E=%d x32=%d res=%s" % (M, E, use_x32, res_kind)
    if want_y32:
        close("layernorm_fwd_f32 y32 " + tag, y32, ref, rel=1e-5)
        assert torch.equal(y[:, :E], y32.to(BF)), "bf16 output is not the rounded fp32 output"
    close_each("layernorm_fwd_f32 y " + tag, y[:, :E], ref, 2 ** -8 * ref.abs() + 1e-5 * scale)
    if pad:
        assert bool((y[:, E:] == -3.0).all()), "columns beyond E of the ldy-strided output were written"


# ---------------------------------------------------------------------------------------------------------------------------------
# the fused criterion at its edges, against the fp64 oracle: tuber_criterion_cost (matching cost), tuber_criterion_loss (loss table and
# stored gradients), tuber_criterion_scale (its backward) and tuber_weighted_sum (the weighted total), all through SetCriterion
# ---------------------------------------------------------------------------------------------------------------------------------
def _crit_setup(yaml_name):
    from tubelet_transformer_amd.config import load_cfg
    from tubelet_transformer_amd.tuber import build_model
    cfg = load_cfg(os.path.join(ROOT, "configuration", yaml_name))
    _, crit, _ = build_model(cfg)
    return cfg, crit


def _outputs(g, ava, nq, nc, box_fn=None, logit_fn=None):
    Q = nq if ava else nq * 32

    def mk():
        lg = torch.randn(3, Q, nc if ava else nc + 1, generator=g, dtype=torch.float64)
        if logit_fn is not None:
            lg = logit_fn(lg)
        bx = torch.rand(3, Q, 4, generator=g, dtype=torch.float64) * 0.5 + 0.25 if box_fn is None else box_fn(Q)
        lb = torch.randn(3, Q, 3, generator=g, dtype=torch.float64) if ava else torch.randn(3, 2, generator=g, dtype=torch.float64)
        return {"pred_logits": lg, "pred_boxes": bx, "pred_logits_b": lb}
    o = mk()
    o["aux_outputs"] = [mk() for _ in range(5)]
    return o


def _leaves(outs, dev, dtype):
    leaves = {}

    def conv(o, pfx):
        r = {}
        for k, v in o.items():
            r[k] = v.to(dev, dtype).requires_grad_(True)
            leaves[pfx + k] = r[k]
        return r
    out = conv({k: v for k, v in outs.items() if k != "aux_outputs"}, "")
    out["aux_outputs"] = [conv(a, "aux%d." % i) for i, a in enumerate(outs["aux_outputs"])]
    return out, leaves


def _check_criterion(dev, cfg, crit, outs, targets, name, gscale=1.7):
    """HIP criterion (float32 outputs on the GPU) against oracle.set_criterion run in fp64 with autograd on the same values; the
    weighted total is back-propagated with an incoming gradient of ``gscale``"""
    from oracle import tuber_oracle as O
    crit.to(dev)
    outs = {k: (v.float().double() if torch.is_tensor(v) else [{kk: vv.float().double() for kk, vv in a.items()} for a in v])
            for k, v in outs.items()}                                    # the fp32 values the kernels see
    o_hip, l_hip = _leaves(outs, dev, torch.float32)
    ld = crit(o_hip, targets)
    total = crit.weighted_total(ld)
    (total * gscale).backward()

    def cpu64(t):
        r = {}
        for k, v in t.items():
            r[k] = v.detach().cpu()
            if k == "boxes" or (k == "labels" and v.is_floating_point()):
                r[k] = r[k].double()
        return r
    t_ref = [cpu64(t) for t in targets]
    o_ref, l_ref = _leaves(outs, "cpu", torch.float64)
    ld_r, idx_r = O.set_criterion(cfg, o_ref, t_ref)
    total_r = O.total_loss(cfg, ld_r)
    (total_r * gscale).backward()
    for li, per in enumerate(crit.last_indices):
        for b, (i, j) in enumerate(per):
            ri, rj = idx_r[li][b]
            assert np.array_equal(i.numpy(), ri.numpy()) and np.array_equal(j.numpy(), rj.numpy()), (name, li, b)
    worst = 0.0
    for k, r in ld_r.items():
        worst = max(worst, abs(float(ld[k]) - float(r)) / max(1.0, abs(float(r))))
    tw = abs(float(total) - float(total_r)) / abs(float(total_r))
    gw = 0.0
    for k, t in l_hip.items():
        ref = l_ref[k].grad if l_ref[k].grad is not None else torch.zeros_like(l_ref[k])
        got = t.grad.detach().cpu().double() if t.grad is not None else torch.zeros_like(ref)
        gw = max(gw, float((got - ref).abs().max()))
    print("%s: worst relative loss error %.2e (total %.2e), worst abs gradient error %.2e" % (name, worst, tw, gw))
    assert worst <= 1e-4 and tw <= 1e-4
    assert gw <= 2e-5


@pytest.mark.parametrize("bpc", [[0, 3, 1], [2, 0, 0], [5, 1, 0]])
def test_criterion_ava_with_empty_clips(dev, bpc):
    """AVA batches with empty clips mixed in: losses within 1e-4 relative, gradients w.r.t. every output within 2e-5 abs and identical
    assignments (the bounds of test_criterion_matches_reference), continuous random costs so the optimum is unique."""
    from tubelet_transformer_amd import synth
    cfg, crit = _crit_setup("TubeR_CSN152_AVA21.yaml")
    g = torch.Generator().manual_seed(31 + sum(bpc))
    outs = _outputs(g, True, cfg.CONFIG.MODEL.QUERY_NUM, cfg.CONFIG.DATA.NUM_CLASSES)
    targets = synth.synthetic_targets(3, "ava", cfg.CONFIG.DATA.NUM_CLASSES, seed=41, device=dev, boxes_per_clip=bpc)
    _check_criterion(dev, cfg, crit, outs, targets, "ava empty clips %s" % bpc)


def test_criterion_ava_saturated_logits(dev):
    """Class logits of magnitude 20 ... 27 (softplus_clamped's linear branch; up to 27 the fp64 oracle's BCE backward is not yet
    bent by torch's 1e-12 clamp of p(1-p)) and two columns at +-120, where BCE's log clamp at -100 holds the loss at 100 and its
    gradient at 0.  Bounds as in test_criterion_ava_with_empty_clips."""
    from tubelet_transformer_amd import synth
    cfg, crit = _crit_setup("TubeR_CSN152_AVA21.yaml")
    g = torch.Generator().manual_seed(5)

    def sat(lg):
        mag = 20.0 + 7.0 * torch.rand(lg.shape, generator=g, dtype=torch.float64)
        out = torch.where(lg >= 0, mag, -mag)
        out[..., 11] = torch.where(lg[..., 11] >= 0, 120.0, -120.0)
        out[..., 3] = torch.where(lg[..., 3] >= 0, 120.0, -120.0)
        return out
    outs = _outputs(g, True, cfg.CONFIG.MODEL.QUERY_NUM, cfg.CONFIG.DATA.NUM_CLASSES, logit_fn=sat)
    targets = synth.synthetic_targets(3, "ava", cfg.CONFIG.DATA.NUM_CLASSES, seed=42, device=dev, boxes_per_clip=[2, 3, 1])
    _check_criterion(dev, cfg, crit, outs, targets, "ava saturated logits")


GEOMETRIES = ["disjoint_x", "disjoint_y", "nested_pred_in_target", "nested_target_in_pred", "partial"]


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_criterion_ava_box_geometry(dev, geometry):
    """Every predicted box disjoint from every target (in x, or in y), nested in it, containing it, or partly overlapping, so that each
    sub-gradient branch of giou_loss (intersection clamped at 0, enclosing box = one of the two) carries the matched pairs.  Bounds as in
    test_criterion_ava_with_empty_clips."""
    from tubelet_transformer_amd import synth
    cfg, crit = _crit_setup("TubeR_CSN152_AVA21.yaml")
    g = torch.Generator().manual_seed(100 + GEOMETRIES.index(geometry))
    nq = cfg.CONFIG.MODEL.QUERY_NUM

    def u(lo, hi, *shape):
        return lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=torch.float64)

    # targets (cx, cy, w, h) and predictions drawn so that every (query, target) pair has the wanted relation
    if geometry == "disjoint_x":
        tb = lambda n: torch.stack([u(0.15, 0.3, n), u(0.3, 0.7, n), u(0.1, 0.2, n), u(0.2, 0.4, n)], 1)
        pb = lambda Q: torch.stack([u(0.7, 0.85, 3, Q), u(0.3, 0.7, 3, Q), u(0.1, 0.2, 3, Q), u(0.2, 0.4, 3, Q)], -1)
    elif geometry == "disjoint_y":
        tb = lambda n: torch.stack([u(0.3, 0.7, n), u(0.15, 0.3, n), u(0.2, 0.4, n), u(0.1, 0.2, n)], 1)
        pb = lambda Q: torch.stack([u(0.3, 0.7, 3, Q), u(0.7, 0.85, 3, Q), u(0.2, 0.4, 3, Q), u(0.1, 0.2, 3, Q)], -1)
    elif geometry == "nested_pred_in_target":
        tb = lambda n: torch.stack([u(0.48, 0.52, n), u(0.48, 0.52, n), u(0.7, 0.8, n), u(0.7, 0.8, n)], 1)
        pb = lambda Q: torch.stack([u(0.4, 0.6, 3, Q), u(0.4, 0.6, 3, Q), u(0.05, 0.2, 3, Q), u(0.05, 0.2, 3, Q)], -1)
    elif geometry == "nested_target_in_pred":
        tb = lambda n: torch.stack([u(0.4, 0.6, n), u(0.4, 0.6, n), u(0.05, 0.2, n), u(0.05, 0.2, n)], 1)
        pb = lambda Q: torch.stack([u(0.48, 0.52, 3, Q), u(0.48, 0.52, 3, Q), u(0.7, 0.8, 3, Q), u(0.7, 0.8, 3, Q)], -1)
    else:
        tb = lambda n: torch.stack([u(0.35, 0.65, n), u(0.35, 0.65, n), u(0.2, 0.3, n), u(0.2, 0.3, n)], 1)
        pb = lambda Q: torch.stack([u(0.35, 0.65, 3, Q), u(0.35, 0.65, 3, Q), u(0.2, 0.3, 3, Q), u(0.2, 0.3, 3, Q)], -1)
    outs = _outputs(g, True, nq, cfg.CONFIG.DATA.NUM_CLASSES, box_fn=pb)
    targets = synth.synthetic_targets(3, "ava", cfg.CONFIG.DATA.NUM_CLASSES, seed=43, device=dev, boxes_per_clip=[2, 3, 1])
    for t in targets:
        n = t["boxes"].shape[0]
        t["boxes"] = torch.cat([torch.full((n, 1), 16.0), tb(n)], 1).float().to(dev)
    _check_criterion(dev, cfg, crit, outs, targets, "ava boxes %s" % geometry)


@pytest.mark.parametrize("key_pos", [[0, 31, 16], [31, 0, 0]])
def test_criterion_jhmdb_key_frame_at_the_ends(dev, key_pos):
    """JHMDB with the key frame at 0 and at the last of the 32 frames (the gather of the key-frame queries, key_pos * nq + j).  Bounds
    as in test_criterion_ava_with_empty_clips."""
    from tubelet_transformer_amd import synth
    cfg, crit = _crit_setup("Tuber_CSN152_JHMDB.yaml")
    g = torch.Generator().manual_seed(7 + key_pos[0])
    outs = _outputs(g, False, cfg.CONFIG.MODEL.QUERY_NUM, cfg.CONFIG.DATA.NUM_CLASSES)
    targets = synth.synthetic_targets(3, "jhmdb", cfg.CONFIG.DATA.NUM_CLASSES, seed=44, device=dev)
    for t, k in zip(targets, key_pos):
        t["key_pos"] = torch.tensor(k, dtype=torch.int64, device=dev)
    _check_criterion(dev, cfg, crit, outs, targets, "jhmdb key_pos %s" % key_pos)


# ---------------------------------------------------------------------------------------------------------------------------------
# small launchers: exact or within one ulp
# ---------------------------------------------------------------------------------------------------------------------------------
def _ulp_close(name, got, ref32, ulps=1):
    """|got - ref32| <= ulps * 2^-23 * |ref32| element-wise (ref32: the same fp32 expression evaluated by torch)"""
    err = (got.double() - ref32.double()).abs()
    tol = ulps * 2.0 ** -23 * ref32.double().abs() + 1e-38
    print("%-52s max|err| %.3e  max err/ulp %.2f" % (name, float(err.max()), float((err / tol).max()) * ulps))
    assert bool(torch.isfinite(got).all()) and bool((err <= tol).all()), name


def test_sigmoid_bwd(dev):
    """dx = dy * y * (1 - y) over an odd n: within 1 ulp of the same fp32 expression, within 2 ulp of fp64; the sentinel after n
    stays."""
    n = 1000003
    dy, y = rnd(n, dev=dev, seed=1), torch.sigmoid(rnd(n, dev=dev, seed=2, scale=3.0))
    dx = torch.full((n + 5,), 777.0, device=dev)
    dx[:n] = float("nan")
    lib.call("tuber_sigmoid_bwd", dy, y, dx, n)
    _ulp_close("sigmoid_bwd vs fp32", dx[:n], dy * y * (1 - y))
    _ulp_close("sigmoid_bwd vs fp64", dx[:n], dy.double() * y.double() * (1 - y.double()), ulps=2)
    assert bool((dx[n:] == 777.0).all())


@pytest.mark.parametrize("R,C,ldd", [(64, 441, 448), (1000, 100, 104), (3, 5, 5)])
def test_cast_pad_rows(dev, R, C, ldd):
    """fp32 [R, C] -> bf16 [R, ldd] with zero pad columns (64 x 441 -> 448 is the stem's weight-gradient operand): bit-exact to
    .to(bfloat16), pad columns zero over a NaN prefill."""
    src = rnd(R, C, dev=dev, seed=R)
    dst = nan(R, ldd, dev=dev, dtype=BF)
    lib.call("tuber_cast_pad_rows", src, dst, R, C, ldd)
    assert torch.equal(dst[:, :C], src.to(BF))
    assert bool((dst[:, C:] == 0).all())
    assert rc("tuber_cast_pad_rows", src, dst, R, C, C - 1) == EINVAL


@pytest.mark.parametrize("n", [3, 8 * 1000 + 5, 704 * 256])
@pytest.mark.parametrize("scale", [1.0, 0.37])
def test_cast_bf16_f32_scale(dev, n, scale):
    """float(bf16) * scale with the vectorised body and the scalar tail: bit-exact to torch's fp32 product; the sentinel after n stays."""
    src = rnd(n, dev=dev, seed=n).to(BF)
    dst = torch.full((n + 8,), 555.0, device=dev)
    dst[:n] = float("nan")
    lib.call("tuber_cast_bf16_f32_scale", src, dst, n, scale)
    assert torch.equal(dst[:n], src.float() * torch.tensor(scale, dtype=torch.float32, device=dev))
    assert bool((dst[n:] == 555.0).all())


def test_scale_f32(dev):
    """x[a, a + n) *= c on a window of a larger buffer as ddp.py passes it (odd base offset, n not a multiple of the vector width):
    scalar coefficient, device coefficient max(coef_dev[1], 0) * coef, and the negative coef_dev[1] a non-finite gradient norm leaves
    (scale 0).  Bit-exact to torch's fp32 product; everything outside the window untouched."""
    buf0 = rnd(300001, dev=dev, seed=1)
    a, n = 1001, 123457
    for coef_dev, coef in ((None, 0.125), (None, 1.0 / 3.0), (torch.tensor([5.0, 0.3], device=dev), 0.5),
                           (torch.tensor([float("inf"), -1.0], device=dev), 0.5)):
        buf = buf0.clone()
        lib.call("tuber_scale_f32", buf.data_ptr() + 4 * a, n, coef_dev, coef)
        c = torch.tensor(coef, dtype=torch.float32, device=dev)
        if coef_dev is not None:
            c = coef_dev[1].clamp(min=0) * c
        assert torch.equal(buf[a:a + n], buf0[a:a + n] * c), (coef_dev, coef)
        assert torch.equal(buf[:a], buf0[:a]) and torch.equal(buf[a + n:], buf0[a + n:])


@pytest.mark.parametrize("n", [24, 300, 4096])
def test_weighted_sum(dev, n):
    """sum_i a[i] w[i] against fp64 within 1e-6 of sum |a w| (fp32 sums), and its backward gout * w bit-exact to torch's fp32
    product; both bit-identical across two calls (fixed summation order)."""
    a, w = rnd(n, dev=dev, seed=1), rnd(n, dev=dev, seed=2).abs()
    outs = []
    for _ in range(2):
        out = nan(1, dev=dev)
        lib.call("tuber_weighted_sum", a, w, n, out, None, None)
        outs.append(out)
    ref = (a.double() * w.double()).sum()
    close("weighted_sum n=%d" % n, outs[0], ref.view(1), abs_=1e-6 * float((a.double() * w.double()).abs().sum()))
    assert torch.equal(outs[0], outs[1])
    gout = torch.tensor([1.7], device=dev)
    gs = []
    for _ in range(2):
        g = nan(n, dev=dev)
        lib.call("tuber_weighted_sum", None, w, n, None, gout, g)
        gs.append(g)
    assert torch.equal(gs[0], gout * w) and torch.equal(gs[0], gs[1])
    assert rc("tuber_weighted_sum", a, w, 4097, outs[0], None, None) == EINVAL


def test_bn_stats_copy_round_trip(dev):
    """Save -> perturb -> restore of BatchNorm buffers of different lengths (1, 64, 300, 2048, 17 000 words -- more than the 64 x 256
    grid stride -- and an int64 counter), bit-exact; arena words between the rows keep their sentinel."""
    lens = [64, 2048, 1, 300, 17000]
    bufs = [rnd(L, dev=dev, seed=L) for L in lens]
    nbt = torch.tensor([123456789012], dtype=torch.int64, device=dev)
    views = [(b.data_ptr(), b.numel()) for b in bufs] + [(nbt.data_ptr(), 2)]
    gap, off, rows = 4, 0, []
    for ptr, words in views:
        rows.append([ptr, off, words])
        off += words + gap
    arena = torch.full((off,), -999.0, device=dev)
    table = torch.tensor(rows, dtype=torch.int64).to(dev)
    orig = [b.clone() for b in bufs] + [nbt.clone()]
    lib.call("tuber_bn_stats_copy", table, len(rows), arena, max(w for _, w in views), 0)
    for (ptr, o, words), b in zip(rows, bufs):
        assert torch.equal(arena[o:o + words], b)
    for (_, o, words) in rows:
        assert bool((arena[o + words:o + words + gap] == -999.0).all())
    for b in bufs:
        b.mul_(-2.0).add_(1.0)
    nbt.add_(5)
    lib.call("tuber_bn_stats_copy", table, len(rows), arena, max(w for _, w in views), 1)
    for b, o in zip(bufs + [nbt], orig):
        assert torch.equal(b, o)
