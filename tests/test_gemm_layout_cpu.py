"""The checker of the GEMM layout tests, tested itself -- no GPU.

A tiny emulation of C = A . B^T that addresses its operands the way a kernel does (base + row * ld + k into the flat parent), rounds nothing
but its inputs (bf16) and its output (bf16), accumulates in fp32 in 64-wide k-tiles and writes into a guarded output.
  * the honest emulation passes the footprint check and the derived elementwise bound at every (M, N, K) of test_gemm_layout_gpu.py, in
    three summation orders: the reference and `tol` are not too tight;
  * seven deliberate defects are each reported: the checker bites.  Each notes whether test_kernels_gpu.close() on contiguous tensors with
    a torch.empty output -- what the kernel tests did before -- would have let it through."""
import numpy as np
import pytest
import torch

import gemm_layout_util as U

BF = U.BF


def emulate(Av, Bv, out, M, N, K, order="fwd", defect=None, at=None):
    base = lambda t: t if t._base is None else t._base
    fa, fb = base(Av).float().reshape(-1), base(Bv).float().reshape(-1)
    oa, ob, lda, ldb = Av.storage_offset(), Bv.storage_offset(), Av.stride(0), Bv.stride(0)
    if defect == "ld_is_K":
        lda = K
    m, n = torch.arange(M)[:, None], torch.arange(N)[:, None]
    nkt = K // 64
    tiles = list(range(nkt))
    if defect == "skip_last_ktile":
        tiles = tiles[:-1]
    if order == "rev":
        tiles = tiles[::-1]
    parts = [torch.zeros(M, N) for _ in range(4 if order == "split4" else 1)]
    for kt in tiles:
        k = kt * 64 + torch.arange(64)[None, :]
        ka = k.clone()
        if defect == "col_past" and kt == nkt - 1:
            ka[0, -1] += 1                  # the last column of the window read one element further on
        parts[kt % len(parts)] += fa[oa + m * lda + ka] @ fb[ob + n * ldb + k].t()
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    c = acc.to(BF)
    if defect == "perturb":
        bits = c.view(torch.int16)
        bits[at] += 2                       # two bf16 ulps up in magnitude
    flat = out.parent.view(-1)
    o0, ldc = out.v.storage_offset(), out.v.stride(0)
    rows = M - 1 if defect == "skip_last_row" else M
    idx = o0 + torch.arange(rows)[:, None] * ldc + torch.arange(N)[None, :]
    flat[idx.reshape(-1)] = c[:rows].reshape(-1)
    if defect == "write_col_N":
        flat[o0 + (M - 1) * ldc + N] = c[M - 1, N - 1]
    if defect == "write_row_M":
        flat[o0 + M * ldc + torch.arange(N)] = c[M - 1]


_cache = {}


def problem(M, N, K):
    if (M, N, K) not in _cache:
        A, B = U.rand((M, K), 1), U.rand((N, K), 2, K ** -0.5)
        _cache[(M, N, K)] = (A, B) + U.ref64(A, B)
    return _cache[(M, N, K)]


def verdict(out, ref, S, K):
    """what the GPU file asserts: (a) footprint, (b) every element within tol"""
    errs = U.footprint_errors(out)
    r, idx, fin = U.worst(out.v, ref, U.tol(ref, S, K, True))
    if not fin or r > 1.0:
        errs.append("worst err/tol %.3f at %s" % (r, idx))
    return errs, r


LAYOUTS = [dict(lda=8, a0=0, ldb=8, b0=0, ldc=8), dict(lda=None, a0=None, ldb=None, b0=None, ldc=136), dict(lda=8, a0=0, ldb=None, b0=None, ldc=1)]


def views(A, B, M, N, K, lay):
    """lda / ldb: K + pad, or (None) 3 K with the window at column K -- the packed 768 / 256 in-projection; ldc: N + pad"""
    Av = U.embed(A, 3 * K if lay["lda"] is None else K + lay["lda"], K if lay["a0"] is None else lay["a0"])
    Bv = U.embed(B, 3 * K if lay["ldb"] is None else K + lay["ldb"], K if lay["b0"] is None else lay["b0"])
    return Av, Bv, U.guarded_out(M, N, N + lay["ldc"], BF)


@pytest.mark.parametrize("order", ["fwd", "rev", "split4"])
@pytest.mark.parametrize("M,N,K", U.SHAPES)
def test_honest_emulation_passes_the_checker(M, N, K, order):
    A, B, ref, S = problem(M, N, K)
    lay = LAYOUTS[(M + N + K) // 2 % 3]
    Av, Bv, out = views(A, B, M, N, K, lay)
    emulate(Av, Bv, out, M, N, K, order)
    errs, r = verdict(out, ref, S, K)
    print("honest %s %dx%dx%d ldc N+%d: worst err/tol %.3f" % (order, M, N, K, lay["ldc"], r))
    assert not errs, errs
    # the three orders differ in fp32 rounding only: had tol been tuned to one of them, another would not fit
    tight = U.guarded_out(M, N, N, BF)
    emulate(A, B, tight, M, N, K, order)                 # contiguous operands are their own parents
    if order == "fwd":
        assert torch.equal(tight.v, out.v), "same k order, other layout: same bits"


def small_element(ref):
    """an element at the 10th percentile of |ref|: small against the matrix maximum, not so small that cancellation decides its error"""
    a = np.abs(ref)
    idx = np.unravel_index(int(np.argmin(np.abs(a - np.quantile(a, 0.10)))), a.shape)
    return tuple(int(i) for i in idx)


#   defect             (M, N, K)      did the old way pass it: close() at 2^-7 max|ref| on tight tensors (ld = width), the output a recycled
#                                     torch.empty block that still holds an earlier launch's correct result, nothing inspected around it
DEFECTS = [
    ("ld_is_K", (130, 64, 64), True),             # lda = K there, so the wrong index is the right one
    ("col_past", (200, 64, 1088), False),         # reads the next row's first element for one k: a typical output is off by ~0.04 sigma, under the
                                                  # old bound, but the largest of 12 800 is not: seen through the matrix maximum only
    ("skip_last_ktile", (200, 64, 1088), False),  # sixty-four terms of 1088 missing, ~0.24 sigma: the old bound sees that too
    ("skip_last_row", (130, 80, 192), True),      # the recycled block still holds the first launch's row
    ("write_col_N", (130, 80, 192), True),        # behind the last row's end: outside the tensor, where no assertion looked
    ("write_row_M", (130, 80, 192), True),        # likewise
    ("perturb", (200, 192, 192), True),           # 2 ulps of an element at a tenth of the typical magnitude is ~2^-10 max|ref|
]


@pytest.mark.parametrize("defect,shape,old_passes", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_checker_reports_each_defect(defect, shape, old_passes):
    M, N, K = shape
    A, B, ref, S = problem(M, N, K)
    Av, Bv, out = views(A, B, M, N, K, LAYOUTS[0])
    at = small_element(ref) if defect == "perturb" else None
    emulate(Av, Bv, out, M, N, K, defect=defect, at=at)
    errs, r = verdict(out, ref, S, K)
    print("%s: %s" % (defect, errs))
    assert errs, "the checker let the defect '%s' through (worst err/tol %.3f)" % (defect, r)
    kind = {"ld_is_K": "not finite", "col_past": "not finite", "skip_last_ktile": "err/tol", "skip_last_row": "not finite",
            "write_col_N": "outside the window", "write_row_M": "outside the window", "perturb": "err/tol"}[defect]
    assert any(kind in e for e in errs), (defect, errs)
    if defect in ("write_col_N", "write_row_M"):
        assert len(errs) == 1, errs                     # the window itself is right: only the footprint check sees these
    if defect == "perturb":
        assert 1.0 < r < 6.0, r                         # a small excess
    # the old way: tight operands (finite memory behind them), an output that already holds the correct result
    old = U.guarded_out(M, N, N, BF)
    At, Bt = U.embed(A, K, fill=1.0), U.embed(B, K, fill=1.0)
    emulate(At, Bt, old, M, N, K)
    emulate(At, Bt, old, M, N, K, defect=defect, at=at)
    passed = U.loose_close(old.v, ref)
    print("%s: the old check %s it" % (defect, "PASSES" if passed else "fails"))
    assert passed == old_passes


def test_one_dropped_term_of_a_small_element_passes_the_old_bound_and_fails_the_new_one():
    """what a matrix-wide bound is blind to: one k-term of 1088 missing from an output that is small against the matrix maximum"""
    M, N, K = 200, 64, 1088
    A, B, ref, S = problem(M, N, K)
    got = (A.float() @ B.float().t()).to(BF)
    term = np.abs(U.f64(A)[:, K - 1:K] * U.f64(B)[:, K - 1][None, :])
    cand = (np.abs(ref) < 0.25) & (term >= np.median(term)) & (term <= 2 * np.median(term))
    m, n = [int(i[0]) for i in np.nonzero(cand)]
    got[m, n] = float(ref[m, n] - U.f64(A)[m, K - 1] * U.f64(B)[n, K - 1])
    assert U.loose_close(got, ref)
    r, idx, _ = U.worst(got, ref, U.tol(ref, S, K, True))
    assert r > 1.0 and idx == (m, n), (r, idx)


def test_guard_geometry():
    g = U.guarded_out(130, 80, 80 + 136, BF)
    assert g.guard >= 128 and g.ld - g.cols >= 128 and g.parent.shape == (130 + 256, 216)
    assert any("not finite" in e for e in U.footprint_errors(g))            # the window starts as NaN: an unwritten element is reported
    assert U.untouched(g)
    g.v.zero_()
    assert U.footprint_errors(g) == [] and not U.untouched(g)
    f = U.guarded_out(3, 64, None, torch.float32, guard=4)
    f.v.zero_()
    f.parent[0, 0] = f.parent[0, 0] * 1.0000002                             # one fp32 ulp: the sentinel is compared as bits
    assert any("outside" in e for e in U.footprint_errors(f))
    v = U.embed(U.rand((5, 16), 3), 48, 16)
    assert v.stride(0) == 48 and bool(torch.isnan(v._base.float()).sum() == 9 * 48 - 5 * 16) and v.data_ptr() % 16 == 0
