"""The GEMM family at the operand layouts the model hands it -- windows inside wider matrices, leading dimensions that are not the width,
padded and odd ones -- with every output guarded.  test_kernels_gpu.py gives the kernels one layout (everything contiguous, ld = width).

Each case runs the kernel twice: the LAYOUT run (operands are windows inside NaN-filled parents: a read outside a window that is not masked
poisons the result; outputs and statistics buffers sit inside sentinel bits with 128 guard rows around and ld - cols columns beside them) and
the TIGHT run (the same values, ld = width, outputs NaN-prefilled and guarded as well).  Asserted per case:
  (a) footprint: the sentinel around every output / statistics buffer is intact bit for bit, every element inside is finite;
  (b) every element within the DERIVED bound (gemm_layout_util.tol) of a float64 CPU reference formed from the bf16-rounded operands;
  (c) layout run == tight run bit for bit wherever both launch the same kernel: tuber_gemm_nt_plan names the same form and tile (the plan
      is asserted per case, so a case cannot silently test another kernel); for gemm_tn the same kernel and slab count.  The bounds-checked
      epilogue (an odd leading dimension) computes the same expressions in the same order as the FULL one, so (c) holds across the two.
Statistics rows: (a), (c), and their column sums against the reference at the tolerances of test_gemm_nt_bn_prologue_stats.
Shapes are the smallest at which each path can go wrong: M 130 / 200 (ragged last tile of 64- and 96-row tiles), N 64 / 192 / 80 (full,
full at 64 and ragged at 128, ragged), K 64 / 192 / 1088 (one k-tile, an odd count, 17 = wave split-K), and 1100 x 1024 x 1088, which takes
96-row wave split-K by itself.  The run log prints the plan and the worst err / tol of every comparison."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import gemm_layout_util as U
from tubelet_transformer_amd import lib

pytestmark = pytest.mark.gpu
BF, F32 = U.BF, torch.float32
EINVAL = -1
A_PLAIN, A_BN_RELU, A_ADD = 0, 1, 3
EPI = dict(plain=0, stats=1, bwd=2, join=3, join_sr=4, join_ds=5, eval=6, join_m=7, join_sr_m=8, join_ds_m=9)

# ---- layouts: name of an operand -> (width -> (ld, col0)); operands a layout does not name are tight ----
pad = lambda p, c0=0: (lambda w: (c0 + w + p, c0))
win3 = lambda at: (lambda w: (3 * w, at * w))                # a window inside a matrix three times as wide: the packed 768 / 256 in-projection
LAYOUTS = {
    # every leading dimension a multiple of 8, all different
    "pad8": dict(A=pad(8), B=pad(8), C=pad(8), R=pad(16), Cm=pad(24), Y=pad(40), Cd=pad(48), A2=pad(16), src=pad(8)),
    # the packed weight: windows at column K / 2 K of 3 K-wide parents, the output with 136 columns beside it and a window offset
    "packed": dict(A=win3(1), B=win3(2), C=pad(136, 8), R=pad(8, 8), Cm=win3(1), Y=pad(8), Cd=pad(16, 16), A2=pad(72, 8), src=win3(1)),
    # an odd ldc: the bounds-checked instantiation with scalar stores, also at N % 64 == 0; the side operands stay 16-byte addressable
    "oddc": dict(A=pad(8), B=win3(1), C=pad(1), R=pad(8), Cm=pad(8), Y=pad(8), Cd=pad(8), A2=pad(24), src=pad(8)),
    # ldc aligned, one odd side operand each: every term of nt_full() on its own (Cd is the one it did not look at)
    "oddR": dict(A=pad(8), B=pad(8), C=pad(8), R=pad(3)),
    "oddCm": dict(A=pad(8), B=pad(8), C=pad(8), R=pad(8), Cm=pad(5), Y=pad(8), Cd=pad(8)),
    "oddY": dict(A=pad(8), B=pad(8), C=pad(8), R=pad(8), Cm=pad(8), Y=pad(7), Cd=pad(8)),
    "oddCd": dict(A=pad(8), B=pad(8), C=pad(8), R=pad(8), Cm=pad(8), Y=pad(8), Cd=pad(9)),
}


def ld(t):
    return t.stride(0)


class Run:
    """one launch's operands and outputs under a layout (None: tight)"""
    def __init__(self, dev, lay):
        self.dev, self.lay, self.outs, self.epi_lds = dev, LAYOUTS[lay] if lay else {}, {}, []

    def i(self, name, x, epi=False):
        f = self.lay.get(name)
        ldx, c0 = f(x.shape[1]) if f else (x.shape[1], 0)
        v = U.embed(x, ldx, c0, device=self.dev)
        if epi:
            self.epi_lds.append(ldx)
        return v

    def vec(self, x):
        return x.to(self.dev)

    def o(self, name, rows, cols, dtype=BF, fill=None, epi=True):
        f = self.lay.get(name)
        ldx, c0 = f(cols) if f else (cols, 0)
        g = U.guarded_out(rows, cols, ldx, dtype, self.dev, c0)
        if fill is not None:
            g.v.fill_(fill)
        if epi and name == "C":
            self.epi_lds.append(ldx)
        self.outs[name] = g
        return g

    def aligned(self):
        return int(all(l % 8 == 0 for l in self.epi_lds))

    def footprints(self, tag):
        torch.cuda.synchronize()
        for name, g in self.outs.items():
            U.assert_footprint(g, "%s %s" % (tag, name))


class forced:
    def __init__(self, cfg):
        self.cfg = cfg

    def __enter__(self):
        if self.cfg >= 0:
            assert lib.query("tuber_gemm_nt_has_cfg", self.cfg)
            lib.call("tuber_gemm_nt_set_cfg", self.cfg)

    def __exit__(self, *a):
        lib.call("tuber_gemm_nt_set_cfg", -1)


def plan(M, N, K, amode, epi, gather, out_f32, aligned):
    v = lib.query("tuber_gemm_nt_plan", M, N, K, amode, epi, gather, out_f32, aligned)
    return None if v < 0 else (v // 1000000, v // 1000 % 1000, v % 1000)


def expected_plan(M, N, K, cfg, amode, epi, gather, out_f32, aligned):
    """the rules of gemm.hip's nt_plan, written out again for shapes with M < 2048 and M * N < 2^25 (every shape here): the automatic
    choice is 64 x 64; wave split-K from 16 k-tiles on, on 96-row tiles where 64-row tiles outnumber the 256 CUs and 96-row ones do not"""
    assert M < 2048 and M * N < 2 ** 25
    mask = epi >= 7
    full64 = N % 64 == 0 and aligned and not out_f32
    can96 = amode == A_PLAIN and full64 and epi in (0, 1, 2)
    if cfg == 0:
        return (0, 128, 128)
    if cfg == 7:
        return (0, 64, 128)
    if cfg == 23:
        return (2, 96, 64) if can96 else (0, 64, 64)
    t64, t96 = -(-M // 64) * -(-N // 64), -(-M // 96) * -(-N // 64)
    if cfg < 0 and not mask and amode == A_PLAIN and not gather and not out_f32 and K // 64 >= 16 and t64 <= 512:
        return (1, 96 if (t64 > 256 and t96 <= 256 and can96) else 64, 64)
    return (0, 64, 64)


@functools.lru_cache(maxsize=None)
def data(M, N, K):
    """operands (CPU, rounded to what the kernels read) and the float64 product shared by every case of a shape -- never modified"""
    d = dict(A=U.rand((M, K), 1), B=U.rand((N, K), 2, K ** -0.5), bias=U.rand((N,), 3, 1.0, F32), R=U.rand((M, N), 4), Cm=U.rand((M, N), 7),
             Y=U.rand((M, N), 8).relu(), Cd=U.rand((M, N), 9), A2=U.rand((M, K), 10),
             sc=1.0 + 0.2 * U.rand((K,), 5, 1.0, F32), sh=0.3 * U.rand((K,), 6, 1.0, F32),
             msc=1.0 + 0.2 * U.rand((N,), 11, 1.0, F32), msh=0.3 * U.rand((N,), 12, 1.0, F32))
    d["P"], d["S"] = U.ref64(d["A"], d["B"])
    return d


@functools.lru_cache(maxsize=None)
def data_bn(M, N, K):
    d = data(M, N, K)
    a = U.bn_relu_bf16(d["A"], d["sc"], d["sh"])
    return (a,) + U.ref64(a, d["B"])


def check_cols(name, st, ref_cols, scale, rel=2e-3):
    """column sums of the partial statistics rows at the tolerance test_gemm_nt_bn_prologue_stats uses: rel * the largest column's scale"""
    got = U.f64(st).sum(0)
    err = float(np.abs(got - ref_cols).max())
    print("%-58s max|err| %.3e (tol %.3e)" % (name, err, rel * scale))
    assert math.isfinite(err) and err <= rel * scale, name


def same_bits(tag, a, b):
    for name in a.outs:
        assert torch.equal(a.outs[name].v, b.outs[name].v), "%s: %s differs between the layout run and the tight run" % (tag, name)


# =====================================================================================================================================
# tuber_gemm_nt: plain (bias, residual, ReLU), fp32 out with alpha, statistics, masked backward (BatchNorm mask / alpha as the mask value)
# =====================================================================================================================================
def nt_launch(r, d, M, N, K, kind):
    A, B = r.i("A", d["A"]), r.i("B", d["B"])
    C = r.o("C", M, N, F32 if kind == "f32" else BF)
    rows = lib.query("tuber_gemm_nt_stat_rows", M, N)
    stats = lambda: dict(stat0=r.o("st0", rows, N, F32).v, stat1=r.o("st1", rows, N, F32).v)
    if kind == "plain":
        R = r.i("R", d["R"], epi=True)
        kw = dict(bias=r.vec(d["bias"]), R=R, ldr=ld(R), relu=1)
    elif kind == "f32":
        kw = dict(bias=r.vec(d["bias"]), relu=1, out_f32=1, alpha=0.5)
    elif kind == "stats":
        kw = dict(epi=1, **stats())
    elif kind == "bn_stats":
        kw = dict(amode=1, a_scale=r.vec(d["sc"]), a_shift=r.vec(d["sh"]), epi=1, **stats())
    elif kind == "bwd":
        Cm = r.i("Cm", d["Cm"], epi=True)
        kw = dict(epi=2, Cm=Cm, ldcm=ld(Cm), m_scale=r.vec(d["msc"]), m_shift=r.vec(d["msh"]), **stats())
    else:                                    # bwd_alpha: the ReLU + Dropout backward mask of tape.py -- no affine, no statistics rows, alpha = 1 / keep
        Cm = r.i("Cm", d["Cm"], epi=True)
        kw = dict(epi=2, Cm=Cm, ldcm=ld(Cm), alpha=1.25)
    lib.gemm_nt(A, ld(A), B, ld(B), C.v, ld(C.v), M, N, K, **kw)
    return kw.get("amode", 0), kw.get("epi", 0), kw.get("out_f32", 0)


def nt_check(tag, r, d, M, N, K, kind):
    P, S = d["P"], d["S"]
    C = r.outs["C"].v
    if kind == "plain":
        ref, S = P + U.f64(d["bias"]) + U.f64(d["R"]), S + np.abs(U.f64(d["bias"])) + np.abs(U.f64(d["R"]))
        U.check(tag, C, np.maximum(ref, 0), U.tol(ref, S, K, True))
    elif kind == "f32":
        ref, S = 0.5 * P + U.f64(d["bias"]), 0.5 * S + np.abs(U.f64(d["bias"]))
        U.check(tag, C, np.maximum(ref, 0), U.tol(ref, S, K, False))
    elif kind in ("stats", "bn_stats"):
        if kind == "bn_stats":
            _, P, S = data_bn(M, N, K)
        U.check(tag, C, P, U.tol(P, S, K, True))
        check_cols(tag + " sum", r.outs["st0"].v, P.sum(0), float(np.abs(P).sum(0).max()))
        check_cols(tag + " sumsq", r.outs["st1"].v, (P * P).sum(0), float((P * P).sum(0).max()))
    else:
        cm = U.f64(d["Cm"])
        if kind == "bwd":
            m = U.f64(U.fma32(d["Cm"], d["msc"], d["msh"])) > 0
            ref = P * m
            check_cols(tag + " sum dz", r.outs["st0"].v, ref.sum(0), float(np.abs(ref).sum(0).max()))
            check_cols(tag + " sum dz*c", r.outs["st1"].v, (ref * cm).sum(0), float(np.abs(ref * cm).sum(0).max()))
        else:
            ref, S = 1.25 * P * (cm > 0), 1.25 * S
        U.check(tag, C, ref, U.tol(ref, S, K, True))


NT_CASES = [
    # M, N, K, forced cfg, layout, kinds
    (130, 64, 64, -1, "pad8", ("plain", "f32", "stats", "bwd", "bn_stats")),
    (130, 64, 64, -1, "oddc", ("plain", "stats", "bwd")),            # N % 64 == 0 and not FULL: the instantiation gemm_plan.json pins, unchecked so far
    (200, 192, 192, 13, "packed", ("plain", "stats", "bwd_alpha", "bn_stats")),
    (200, 192, 192, 7, "oddc", ("plain", "bwd")),
    (200, 192, 64, 7, "packed", ("plain", "f32", "stats", "bwd", "bn_stats")),
    (130, 80, 192, 0, "pad8", ("plain", "stats", "bwd")),
    (130, 80, 192, 13, "oddc", ("plain", "f32", "bwd_alpha", "bn_stats")),
    (200, 192, 192, 23, "pad8", ("plain", "stats", "bwd")),          # regular 96 x 64
    (200, 192, 192, 23, "oddR", ("plain",)),                         # an odd ldr alone: 64 x 64, scalar residual reads
    (200, 64, 1088, -1, "packed", ("plain", "stats", "bwd")),        # wave split-K 64, 17 k-tiles
    (130, 192, 1088, -1, "oddc", ("plain", "stats", "bwd_alpha")),
    (200, 80, 1088, -1, "pad8", ("plain", "bwd")),
    (200, 192, 192, 13, "oddCm", ("bwd", "bwd_alpha")),
    (1100, 1024, 1088, -1, "pad8", ("plain", "stats")),              # wave split-K on 96-row tiles by itself
    (1100, 1024, 1088, -1, "oddc", ("bwd",)),                        # ... and the 64-row form it falls back to without 16-byte stores
]


@pytest.mark.parametrize("M,N,K,cfg,lay,kinds", NT_CASES, ids=["%dx%dx%d-cfg%d-%s" % c[:5] for c in NT_CASES])
def test_gemm_nt_layouts(dev, M, N, K, cfg, lay, kinds):
    d = data(M, N, K)
    with forced(cfg):
        for kind in kinds:
            runs = []
            for layout in (lay, None):
                r = Run(dev, layout)
                amode, epi, f32 = nt_launch(r, d, M, N, K, kind)
                r.plan = plan(M, N, K, amode, epi, 0, f32, r.aligned())
                assert r.plan == expected_plan(M, N, K, cfg, amode, epi, 0, f32, r.aligned()), (kind, layout, r.plan)
                runs.append(r)
            tag = "nt %s %dx%dx%d cfg %d %s plan %s" % (kind, M, N, K, cfg, lay, runs[0].plan)
            for r in runs:
                r.footprints(tag)
            nt_check(tag, runs[0], d, M, N, K, kind)
            if runs[0].plan == runs[1].plan:
                same_bits(tag, *runs)
            else:
                print(tag, "-- tight run plan", runs[1].plan, ": no bit comparison")
                nt_check(tag + " (tight)", runs[1], d, M, N, K, kind)


def test_gemm_nt_strided_row_gather_from_an_embedded_source(dev):
    """the down_sample conv's row gather reads (n, t*st, h*ss, w*ss) of a source that is itself a window: the rows in between are never read
    (they are NaN here, like everything around the window)"""
    n, Ti, Hi, Wi, st, ss, N, K = 2, 1, 9, 25, 2, 2, 192, 192
    To, Ho, Wo = (Ti - 1) // st + 1, (Hi - 1) // ss + 1, (Wi - 1) // ss + 1
    M = n * To * Ho * Wo
    assert M == 130
    X = U.rand((n * Ti * Hi * Wi, K), 21)
    sampled = torch.zeros(n, Ti, Hi, Wi, dtype=torch.bool)
    sampled[:, ::st, ::ss, ::ss] = True
    Xs = X[sampled.view(-1)]
    X = torch.where(sampled.view(-1, 1), X, torch.full_like(X, float("nan")))
    B, bias = data(M, N, K)["B"], data(M, N, K)["bias"]
    ref, S = U.ref64(Xs, B, 1.0, (bias,))
    gather = (To, Ho, Wo, Ti, Hi, Wi, st, ss)
    runs = []
    for layout in ("packed", None):
        r = Run(dev, layout)
        src, Bv = r.i("src", X), r.i("B", B)
        C = r.o("C", M, N)
        lib.gemm_nt(src, ld(src), Bv, ld(Bv), C.v, ld(C.v), M, N, K, gather=gather, bias=r.vec(bias))
        r.plan = plan(M, N, K, 0, 0, 1, 0, r.aligned())
        assert r.plan == (0, 64, 64), r.plan
        r.footprints("nt gather")
        runs.append(r)
    U.check("nt gather 130x192x192 packed plan %s" % (runs[0].plan,), runs[0].outs["C"].v, ref, U.tol(ref, S, K, True))
    same_bits("nt gather", *runs)


@pytest.mark.parametrize("M,N,K,cfg,lay", [(200, 192, 192, 13, "packed"), (200, 192, 64, 7, "pad8"), (130, 192, 1088, -1, "oddc")])
def test_gemm_nt_addproj_layouts(dev, M, N, K, cfg, lay):
    """the packed in-projection with the positional embedding folded in: output columns [0, 128) see bf16(A + A2), the rest A; lda != lda2"""
    d = data(M, N, K)
    add = 128
    Pa, Sa = U.ref64(U.add_bf16(d["A"], d["A2"]), d["B"][:add], 1.0, (d["bias"][:add],))
    Pp, Sp = U.ref64(d["A"], d["B"][add:], 1.0, (d["bias"][add:],))
    ref, S = np.concatenate([Pa, Pp], 1), np.concatenate([Sa, Sp], 1)
    runs = []
    with forced(cfg):
        for layout in (lay, None):
            r = Run(dev, layout)
            A, A2, B = r.i("A", d["A"]), r.i("A2", d["A2"]), r.i("B", d["B"])
            C = r.o("C", M, N)
            assert layout is None or ld(A) != ld(A2)
            lib.call("tuber_gemm_nt_addproj", A, ld(A), A2, ld(A2), add, B, ld(B), C.v, ld(C.v), M, N, K, r.vec(d["bias"]))
            r.plan = plan(M, N, K, A_ADD, 0, 0, 0, r.aligned())
            assert r.plan == expected_plan(M, N, K, cfg, A_ADD, 0, 0, 0, r.aligned()), r.plan
            r.footprints("addproj")
            runs.append(r)
    U.check("addproj %dx%dx%d cfg %d %s plan %s" % (M, N, K, cfg, lay, runs[0].plan), runs[0].outs["C"].v, ref, U.tol(ref, S, K, True))
    assert runs[0].plan == runs[1].plan
    same_bits("addproj", *runs)


# =====================================================================================================================================
# the join entry points
# =====================================================================================================================================
def bits_of(y):
    """the [M][N / 8] bit field of y > 0, tight as its contract says"""
    M, N = y.shape
    b = (y.float() > 0).view(M, N // 8, 8).to(torch.int32)
    return (b << torch.arange(8, dtype=torch.int32)).sum(-1).to(torch.uint8).contiguous()


GRIDS = {200: (2, 4, 5, 5, 2, 2), 130: (1, 2, 5, 13, 2, 2), 1100: (1, 2, 22, 25, 2, 2)}          # (n, Ti, Hi, Wi, st, ss) with n Ti Hi Wi = M


def join_launch(r, d, M, N, K, form):
    A, B = r.i("A", d["A"]), r.i("B", d["B"])
    dz = r.o("C", M, N)
    Cm = r.i("Cm", d["Cm"], epi=True)
    rows = lib.query("tuber_gemm_nt_stat_rows", M, N)
    s0, s1 = r.o("st0", rows, N, F32).v, r.o("st1", rows, N, F32).v
    masked = form.endswith("_m")
    Y = r.vec(bits_of(d["Y"])) if masked else r.i("Y", d["Y"], epi=True)
    head = (A, ld(A), B, ld(B), dz.v, ld(dz.v), M, N, K)
    ytail = (Y,) if masked else (Y, ld(Y))
    if form.startswith("join_sr"):
        n, Ti, Hi, Wi, st, ss = GRIDS[M]
        To, Ho, Wo = (Ti - 1) // st + 1, (Hi - 1) // ss + 1, (Wi - 1) // ss + 1
        Rs = r.i("R", d["R"][:n * To * Ho * Wo], epi=True)
        lib.call("tuber_gemm_nt_join_strided_mask" if masked else "tuber_gemm_nt_join_strided", *head, Rs, ld(Rs), To, Ho, Wo, Ti, Hi, Wi, st, ss,
                 *ytail, Cm, ld(Cm), s0, s1)
    elif form.startswith("join_ds"):
        R, Cd = r.i("R", d["R"], epi=True), r.i("Cd", d["Cd"], epi=True)
        s2 = r.o("st2", rows, N, F32).v
        lib.call("tuber_gemm_nt_join_ds_mask" if masked else "tuber_gemm_nt_join_ds", *head, R, ld(R), *ytail, Cm, ld(Cm), Cd, ld(Cd), s0, s1, s2)
    else:
        R = r.i("R", d["R"], epi=True)
        lib.call("tuber_gemm_nt_join_mask" if masked else "tuber_gemm_nt_join", *head, R, ld(R), *ytail, Cm, ld(Cm), s0, s1)


def join_ref(d, M, N, K, form):
    Rfull = d["R"]
    if form.startswith("join_sr"):
        n, Ti, Hi, Wi, st, ss = GRIDS[M]
        To, Ho, Wo = (Ti - 1) // st + 1, (Hi - 1) // ss + 1, (Wi - 1) // ss + 1
        full = torch.zeros(n, Ti, Hi, Wi, N, dtype=BF)
        full[:, ::st, ::ss, ::ss] = d["R"][:n * To * Ho * Wo].view(n, To, Ho, Wo, N)
        Rfull = full.view(M, N)
    ref, S = d["P"] + U.f64(Rfull), d["S"] + np.abs(U.f64(Rfull))
    m = U.f64(d["Y"]) > 0
    return ref * m, S


JOIN_CASES = [
    # M, N, K, cfg, layout, forms
    (200, 192, 192, 13, "pad8", ("join", "join_ds", "join_sr", "join_m", "join_ds_m", "join_sr_m")),
    (130, 64, 64, -1, "packed", ("join", "join_ds", "join_sr", "join_m", "join_ds_m", "join_sr_m")),
    (200, 192, 64, 7, "packed", ("join", "join_ds", "join_sr")),
    (130, 80, 192, 13, "oddc", ("join", "join_ds", "join_sr")),
    (200, 64, 1088, -1, "pad8", ("join", "join_ds", "join_sr")),                 # wave split-K
    (200, 192, 192, 13, "oddR", ("join", "join_sr")),
    (200, 192, 192, 13, "oddCm", ("join", "join_ds")),
    (200, 192, 192, 13, "oddY", ("join", "join_ds", "join_sr")),
    (200, 192, 192, 13, "oddCd", ("join_ds",)),                                    # the leading dimension nt_full() did not look at
    (200, 64, 1088, -1, "oddCd", ("join_ds",)),
    (1100, 1024, 1088, 7, "pad8", ("join_m", "join_sr_m")),                      # the bit-field forms on 64 x 128 tiles
]


@pytest.mark.parametrize("M,N,K,cfg,lay,forms", JOIN_CASES, ids=["%dx%dx%d-cfg%d-%s" % c[:5] for c in JOIN_CASES])
def test_gemm_nt_join_layouts(dev, M, N, K, cfg, lay, forms):
    """dz = (A . B^T + R) * [y > 0] with the statistics rows sum dz, sum dz * Cm (, sum dz * Cd): the y-reading and the bit-field forms, the
    strided-shortcut residual and the first-block form.  `oddCd`: with an odd ldcd the FULL instantiation read Cd in 16-byte pieces at
    2-byte-aligned addresses (nt_full() looked at every other leading dimension); it now takes the bounds-checked one like the other odd
    leading dimensions do -- same expressions, same order, bit-identical to the aligned run."""
    d = data(M, N, K)
    with forced(cfg):
        for form in forms:
            runs = []
            for layout in (lay, None):
                r = Run(dev, layout)
                join_launch(r, d, M, N, K, form)
                r.plan = plan(M, N, K, A_PLAIN, EPI[form], 0, 0, r.aligned())
                assert r.plan == expected_plan(M, N, K, cfg, A_PLAIN, EPI[form], 0, 0, r.aligned()), (form, layout, r.plan)
                runs.append(r)
            tag = "%s %dx%dx%d cfg %d %s plan %s" % (form, M, N, K, cfg, lay, runs[0].plan)
            for r in runs:
                r.footprints(tag)
            ref, S = join_ref(d, M, N, K, form)
            U.check(tag, runs[0].outs["C"].v, ref, U.tol(ref, S, K, True))
            cm, cd = U.f64(d["Cm"]), U.f64(d["Cd"])
            check_cols(tag + " sum dz", runs[0].outs["st0"].v, ref.sum(0), float(np.abs(ref).sum(0).max()))
            check_cols(tag + " sum dz*cm", runs[0].outs["st1"].v, (ref * cm).sum(0), float(np.abs(ref * cm).sum(0).max()))
            if "st2" in runs[0].outs:
                check_cols(tag + " sum dz*cd", runs[0].outs["st2"].v, (ref * cd).sum(0), float(np.abs(ref * cd).sum(0).max()))
            assert runs[0].plan == runs[1].plan
            same_bits(tag, *runs)


@pytest.mark.parametrize("M,N,K,cfg", [(200, 192, 192, -1), (130, 64, 1088, 13), (1100, 1024, 1088, 7)])
def test_gemm_nt_bn_out_layouts(dev, M, N, K, cfg):
    """the eval tail y = relu(bf16(relu(bn3(A)) . B^T) * s4 + h4 + R32) with ldr32, ldy32 and ldy each their own; both outputs guarded.
    Bound: the bf16 rounding of the product (tol16 of it) scaled by |s4|, plus the epilogue's fp32 operations; y is that value rounded once more."""
    d = data(M, N, K)
    _, P, S = data_bn(M, N, K)
    s4, h4 = d["msc"].abs() + 0.5, d["msh"]
    R32 = U.rand((M, N), 13, 1.0, F32).abs()
    pre = P * U.f64(s4) + U.f64(h4) + U.f64(R32)
    ref = np.maximum(pre, 0)
    t32 = np.abs(U.f64(s4)) * U.tol(P, S, K, True) + 8 * U.U32 * (np.abs(P * U.f64(s4)) + np.abs(U.f64(h4)) + np.abs(U.f64(R32)))
    lays = dict(B=pad(8), A=win3(1), R32=pad(4), y32=pad(12), C=pad(8, 8))
    runs = []
    with forced(cfg):
        for layout in (lays, {}):
            r = Run(dev, None)
            r.lay = layout
            A, B, Rv = r.i("A", d["A"]), r.i("B", d["B"]), r.i("R32", R32)
            y, y32 = r.o("C", M, N), r.o("y32", M, N, F32)
            lib.call("tuber_gemm_nt_bn_out", A, ld(A), r.vec(d["sc"]), r.vec(d["sh"]), B, ld(B), r.vec(s4), r.vec(h4), Rv, ld(Rv), y.v, ld(y.v),
                     y32.v, ld(y32.v), M, N, K)
            r.plan = plan(M, N, K, A_BN_RELU, EPI["eval"], 0, 0, 1)
            assert r.plan == expected_plan(M, N, K, cfg, A_BN_RELU, EPI["eval"], 0, 0, 1), r.plan
            r.footprints("bn_out")
            runs.append(r)
    tag = "bn_out %dx%dx%d cfg %d plan %s" % (M, N, K, cfg, runs[0].plan)
    U.check(tag + " y32", runs[0].outs["y32"].v, ref, t32)
    U.check(tag + " y", runs[0].outs["C"].v, ref, U.U16 * (np.abs(ref) + t32) + t32)
    assert torch.equal(runs[0].outs["C"].v, runs[0].outs["y32"].v.to(BF))
    same_bits(tag, *runs)


# =====================================================================================================================================
# tuber_gemm_tn / tuber_gemm_tn_group: dW[N, K] = G^T . f(A), reduction over the M rows; outputs are dense fp32 (row guards only)
# =====================================================================================================================================
def first_multi_slab_M(N, K):
    """the smallest M at which tuber_gemm_tn cuts the rows into several slabs"""
    for M in range(64, 4096):
        if lib.query("tuber_gemm_tn_slabs", M, N, K) > 1:
            return M
    raise AssertionError("no multi-slab M below 4096")


def tn_launch(r, G, A, M, N, K, accumulate, amode=0, sc=None, sh=None, bias=False, prev=0.25):
    S = lib.query("tuber_gemm_tn_slabs", M, N, K)
    out = r.o("out", N, K, F32, fill=prev)
    part = r.o("part", S * N, K, F32) if S > 1 else None
    bg = None
    if bias:
        bg = r.o("bias", S if S > 1 else 1, N, F32, fill=None if S > 1 else prev)
    lib.call("tuber_gemm_tn", G, ld(G), A, ld(A), part.v if part else None, out.v, accumulate, M, N, K, amode, sc, sh,
             0, 0, 0, 0, 0, 0, 0, 0, 0, None, 0, None, None, None, bg.v if bg else None)
    return S


def tn_checks(tag, r, Gc, Ac, M, N, K, accumulate, S, bias=False, prev=0.25):
    """(a) and (b) of one tuber_gemm_tn run: out / the slabs / the bias gradient against float64"""
    torch.cuda.synchronize()
    add = (np.full((N, K), prev),) if accumulate == 1 or (accumulate == 2 and S == 1) else ()
    ref, Sm = U.ref64_tn(Gc, Ac, add)
    if accumulate == 2 and S > 1:
        assert U.untouched_window(r.outs["out"], prev), "accumulate = 2 leaves the slabs to the caller: out is not written"
        U.assert_footprint(r.outs["part"], tag + " part")
        got = r.outs["part"].v.view(S, N, K).double().sum(0)
        U.check(tag + " sum of slabs", got.float(), *U_ref_plain(Gc, Ac, M))
    else:
        for name in ("out", "part"):
            if name in r.outs:
                U.assert_footprint(r.outs[name], "%s %s" % (tag, name))
        U.check(tag, r.outs["out"].v, ref, U.tol(ref, Sm, M, False))
    if bias:
        U.assert_footprint(r.outs["bias"], tag + " bias")
        g = U.f64(Gc)
        bsum = r.outs["bias"].v.double().sum(0).float() if S > 1 else r.outs["bias"].v[0]
        padd = 0.0 if S > 1 else prev
        U.check(tag + " dbias", bsum, g.sum(0) + padd, U.tol(g.sum(0), np.abs(g).sum(0) + padd, M, False))


def U_ref_plain(Gc, Ac, M):
    ref, Sm = U.ref64_tn(Gc, Ac)
    return ref, U.tol(ref, Sm, M, False)


TN_CASES = [
    # N, K, M (None: the smallest multi-slab M), layout of (G, A) as (ld, col0) functions, amode, bias, what runs
    ("tr-pad", 192, 64, 130, (pad(8), pad(16)), 0, False),                   # transpose read, ldg > N, lda > K
    ("tr-window", 64, 192, 200, (win3(1), win3(2)), 0, True),                # G a column window of a 3 N-wide gradient, + bias gradient (one slab)
    ("tr-bn", 80, 64, 130, (pad(24, 8), pad(8)), 1, False),                  # BatchNorm + ReLU prologue, ragged 64-wide tiles (N = 80)
    ("tr-slabs", 192, 64, None, (win3(1), pad(8)), 0, True),                 # several slabs: bias gradient rows per slab
    ("reg-ld4", 64, 192, 200, (pad(4, 8), pad(12, 8)), 0, False),            # ld % 8 == 4 (76, 212), N and K % 8 == 0: the in-register transpose on 64-wide tiles
    ("reg-odd84", 81, 100, 130, (pad(3), pad(4)), 0, False),                 # odd N / K: ldg = 84 = ceil4(N), lda = 104 = ceil4(K): NaN pads inside what may be read
    ("reg-odd88", 81, 100, 200, (pad(7), pad(12)), 1, False),                # ldg = 88, lda = 112, BatchNorm + ReLU prologue
    ("reg-slabs", 81, 100, None, (pad(3, 8), pad(4, 8)), 0, False),            # ldg = 92, lda = 112, windows 8 columns in
]


@pytest.mark.parametrize("name,N,K,M,lays,amode,bias", TN_CASES, ids=[c[0] for c in TN_CASES])
def test_gemm_tn_layouts(dev, name, N, K, M, lays, amode, bias):
    """accumulate 0, 1 and 2 of every case into guarded out / partial.  The tight run: ld = width where the launcher takes that (multiples
    of 4), ceil4(width) for the odd shapes; bit-identical where both runs take the same kernel (transpose-read: N, K, ld all multiples of 8)."""
    M = M or first_multi_slab_M(N, K)
    Gc, A0 = U.rand((M, N), 31), U.rand((M, K), 32)
    sc, sh = 1.0 + 0.2 * U.rand((K,), 5, 1.0, F32), 0.3 * U.rand((K,), 6, 1.0, F32)
    Ac = U.bn_relu_bf16(A0, sc, sh) if amode else A0
    S = lib.query("tuber_gemm_tn_slabs", M, N, K)
    assert (S > 1) == name.endswith("slabs")
    tr = lambda G, A: not ((N | K | ld(G) | ld(A)) & 7)
    c4 = lambda w: (w + 3) // 4 * 4
    if bias:
        assert lib.query("tuber_gemm_tn_fuses_bias", M, N, K, lays[0](N)[0], lays[1](K)[0]) == (2 if S > 1 else 1)
    for accumulate in (0, 1, 2):
        runs = []
        for tight in (False, True):
            r = Run(dev, None)
            fg, fa = (pad(c4(N) - N), pad(c4(K) - K)) if tight else lays
            G = U.embed(Gc, *fg(N), device=dev)
            A = U.embed(A0, *fa(K), device=dev)
            assert tr(G, A) == name.startswith("tr") or tight
            r.tr = tr(G, A)
            tn_launch(r, G, A, M, N, K, accumulate, amode, r.vec(sc) if amode else None, r.vec(sh) if amode else None, bias)
            tn_checks("tn %s M %d acc %d %s slabs %d %s" % (name, M, accumulate, "tight" if tight else "layout", S,
                                                             "transpose-read" if r.tr else "in-register"), r, Gc, Ac, M, N, K, accumulate, S, bias)
            runs.append(r)
        if runs[0].tr == runs[1].tr:
            same_bits("tn %s acc %d" % (name, accumulate), *runs)


def test_gemm_tn_group_on_column_windows_of_the_gradient(dev):
    """the entries in_proj.bwd builds: G = g + c0 with ldg = the full width and N = c1 - c0, the first block against bf16(x + addend) formed
    on load (A2 with its own lda2), bias gradients and dW as row blocks of the full tensors; one single-slab pair and one multi-slab pair
    (accumulate 2).  == single tuber_gemm_tn launches bit for bit (those get the sum x + addend as a finished operand), and within the bound."""
    from tubelet_transformer_amd.engine import TnArgs
    assert lib.query("tuber_gemm_tn_args_bytes") == ctypes.sizeof(TnArgs)
    Nt, add, K = 192, 128, 64
    entries, singles, keep = [], [], []
    for M in (130, first_multi_slab_M(64, K)):
        gc, xc, pc = U.rand((M, Nt), 41), U.rand((M, K), 42), U.rand((M, K), 43)
        g = U.embed(gc, Nt + 8, 0, device=dev)
        x, pos = U.embed(xc, 3 * K, K, device=dev), U.embed(pc, K + 16, 8, device=dev)
        xsum = U.add_bf16(xc, pc)
        xs = U.embed(xsum, K + 8, 0, device=dev)
        keep += [g, x, pos, xs]
        for c0, c1, a2 in ((0, add, pos), (add, Nt, None)):
            N = c1 - c0
            S = lib.query("tuber_gemm_tn_slabs", M, N, K)
            acc = 2 if S > 1 else 1
            res = []
            for grouped in (False, True):
                r = Run(dev, None)
                out = r.o("out", N, K, F32, fill=0.25)
                part = r.o("part", S * N, K, F32) if S > 1 else None
                bg = r.o("bias", S if S > 1 else 1, N, F32, fill=None if S > 1 else 0.25)
                G = g[:, c0:c1]
                if grouped:
                    entries.append(TnArgs(G=G.data_ptr(), ldg=ld(G), A=x.data_ptr(), lda=ld(x), partial=part.v.data_ptr() if part else None,
                                          out=out.v.data_ptr(), accumulate=acc, M=M, N=N, K=K, amode=0, gather=0, bias_grad=bg.v.data_ptr(),
                                          A2=a2.data_ptr() if a2 is not None else None, lda2=ld(a2) if a2 is not None else 0))
                else:
                    Aop = xs if a2 is not None else x
                    lib.call("tuber_gemm_tn", G, ld(G), Aop, ld(Aop), part.v if part else None, out.v, acc, M, N, K, 0, None, None,
                             0, 0, 0, 0, 0, 0, 0, 0, 0, None, 0, None, None, None, bg.v)
                res.append(r)
            singles.append((M, N, S, acc, gc[:, c0:c1], xsum if a2 is not None else xc, res))
    arr = (TnArgs * len(entries))(*entries)
    lib.call("tuber_gemm_tn_group", arr, len(entries))
    for M, N, S, acc, Gc, Ac, (single, grouped) in singles:
        tag = "tn_group M %d N %d slabs %d" % (M, N, S)
        tn_checks(tag, grouped, Gc, Ac, M, N, K, acc, S, bias=True)
        same_bits(tag, single, grouped)


@pytest.mark.parametrize("M,N,Nq,Kin,with_res", [(30, 768, 512, 64, True), (77, 768, 768, 48, False), (33, 1280, 512, 64, True)])
def test_rows_dx2_layouts(dev, M, N, Nq, Kin, with_res):
    """ldg > N, W^T as a column window (offset 256) of a wider matrix as in_proj.bwd passes it; dx and dpos guarded"""
    gc, wc = U.rand((M, N), 51), U.rand((Kin, N), 52, N ** -0.5)
    res = U.rand((M, Kin), 53) if with_res else None
    ref, S = U.ref64(gc, wc, 1.0, (res,) if with_res else ())
    refq, Sq = U.ref64(gc[:, :Nq], wc[:, :Nq])
    runs = []
    for layout in (True, False):
        r = Run(dev, None)
        g = U.embed(gc, N + 8 if layout else N, 0, device=dev)
        wt = U.embed(wc, N + 512 if layout else N, 256 if layout else 0, device=dev)
        dx, dpos = r.o("dx", M, Kin), r.o("dpos", M, Kin)
        lib.call("tuber_rows_dx2", g, ld(g), M, N, Nq, wt, ld(wt), Kin, dx.v, r.vec(res) if with_res else None, dpos.v)
        r.footprints("rows_dx2")
        runs.append(r)
    tag = "rows_dx2 %dx%d Nq %d Kin %d" % (M, N, Nq, Kin)
    U.check(tag + " dx", runs[0].outs["dx"].v, ref, U.tol(ref, S, N, True))
    U.check(tag + " dpos", runs[0].outs["dpos"].v, refq, U.tol(refq, Sq, Nq, True))
    same_bits(tag, *runs)


# =====================================================================================================================================
# contract: what the launchers document as refused is refused (TUBER_EINVAL) and nothing is written
# =====================================================================================================================================
def _nt_args(dev, M=130, N=64, K=64, lda=None, ldb=None, ldc=None, Kcall=None):
    r = Run(dev, None)
    A = U.embed(U.rand((M, K), 1), lda or K, 0, row_guard=4, device=dev)
    B = U.embed(U.rand((N, K), 2), ldb or K, 0, row_guard=4, device=dev)
    C = U.guarded_out(M, N, ldc or N, BF, dev)
    r.outs["C"] = C
    return r, A, B, C, (A, ld(A), B, ld(B), C.v, ld(C.v), M, N, Kcall or K)


def _side(dev, M, N, ldx=None, seed=4):
    return U.embed(U.rand((M, N), seed), ldx or N, 0, row_guard=4, device=dev)


def _refuse_nt(dev, what):
    kw = dict(lda_odd=dict(lda=68), ldb_odd=dict(ldb=68), k_not_64=dict(K=128, Kcall=96))[what]
    r, A, B, C, head = _nt_args(dev, **kw)
    return r, lib.call_rc("tuber_gemm_nt", *head, 0, None, None, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, None, None, 0, 0, 0, None, None, None, 0, None, None,
                          1.0, 0.0, None, 0, None, 0, None)


def _refuse_addproj(dev, what):
    M, N, K = 130, 192, 64
    r, A, B, C, head = _nt_args(dev, M, N, K)
    A2 = _side(dev, M, K, 68 if what == "lda2_odd" else K)
    return r, lib.call_rc("tuber_gemm_nt_addproj", A, ld(A), A2, ld(A2), 64 if what == "add_ncols_not_128" else 128, B, ld(B), C.v, ld(C.v), M, N, K, None)


def _refuse_join(dev, form, what):
    M, K = 200, 64
    N = 80 if what == "n_not_64" else 64
    kw = dict(lda=68) if what == "lda_odd" else dict(ldc=N + 1) if what == "ldc_odd" else {}
    r, A, B, C, head = _nt_args(dev, M, N, K, **kw)
    R, Cm, Cd = _side(dev, M, N), _side(dev, M, N, seed=7), _side(dev, M, N, N + 9 if what == "ldcd_odd" else None, seed=9)
    Yc = U.rand((M, N), 8).relu()
    masked = form.endswith("_mask")
    ytail = (bits_of(Yc).to(dev) if N % 8 == 0 else None,) if masked else (Yc.to(dev), N)
    rows = lib.query("tuber_gemm_nt_stat_rows", M, N)
    st = [r.o("st%d" % i, rows, N, F32).v for i in range(3)]
    if "strided" in form:
        n, Ti, Hi, Wi, s_t, s_s = GRIDS[200]
        if what == "rows_not_grid":
            Ti = 3
        To, Ho, Wo = (Ti - 1) // s_t + 1, (Hi - 1) // s_s + 1, (Wi - 1) // s_s + 1
        return r, lib.call_rc("tuber_gemm_nt_" + form, *head, R, ld(R), To, Ho, Wo, Ti, Hi, Wi, s_t, s_s, *ytail, Cm, ld(Cm), st[0], st[1])
    if "_ds" in form:
        return r, lib.call_rc("tuber_gemm_nt_" + form, *head, R, ld(R), *ytail, Cm, ld(Cm), Cd, ld(Cd), st[0], st[1], st[2])
    return r, lib.call_rc("tuber_gemm_nt_" + form, *head, R, ld(R), *ytail, Cm, ld(Cm), st[0], st[1])


def _refuse_bn_out(dev, what):
    M, K = 130, 64
    N = 80 if what == "n_not_64" else 64
    r, A, B, C, _ = _nt_args(dev, M, N, K, ldc=N + 4 if what == "ldy_odd" else N + 8)
    R32 = U.embed(U.rand((M, N), 13, 1.0, F32), N + (2 if what == "ldr32_not_4" else 4), 0, row_guard=4, device=dev)
    y32 = U.guarded_out(M, N, N + (6 if what == "ldy32_not_4" else 8), F32, dev)
    r.outs["y32"] = y32
    v = lambda n, s: U.rand((n,), s, 1.0, F32).to(dev)
    return r, lib.call_rc("tuber_gemm_nt_bn_out", A, ld(A), v(K, 5), v(K, 6), B, ld(B), v(N, 11), v(N, 12), R32, ld(R32), C.v, ld(C.v), y32.v, ld(y32.v), M, N, K)


def _refuse_tn(dev, what):
    M, N, K = 130, 64, 64
    ldg, lda, bias = N, K, False
    if what == "ldg_not_4":
        ldg = N + 2
    elif what == "lda_not_4":
        lda = K + 6
    elif what == "ld_below_ceil4":
        N, ldg = 81, 84                      # the tensor has 84 columns; the call claims ldg = 80 < ceil4(81)
    elif what == "bias_off_transpose_read":
        ldg, bias = N + 4, True
    r = Run(dev, None)
    G = U.embed(U.rand((M, N), 31), ldg, 0, row_guard=4, device=dev)
    A = U.embed(U.rand((M, K), 32), lda, 0, row_guard=4, device=dev)
    out, bg = r.o("out", N, K, F32), r.o("bias", 1, N, F32)
    return r, lib.call_rc("tuber_gemm_tn", G, 80 if what == "ld_below_ceil4" else ld(G), A, ld(A), None, out.v, 0, M, N, K, 0, None, None,
                          0, 0, 0, 0, 0, 0, 0, 0, 0, None, 0, None, None, None, bg.v if bias else None)


def _refuse_tn_group(dev, what):
    from tubelet_transformer_amd.engine import TnArgs
    N, K = 64, 64
    M = first_multi_slab_M(N, K) if what == "slabs_without_accumulate_2" else 130
    S = lib.query("tuber_gemm_tn_slabs", M, N, K)
    r = Run(dev, None)
    G = U.embed(U.rand((M, N), 31), N + 4 if what == "ldg_not_8" else N + 8, 0, row_guard=4, device=dev)
    A = U.embed(U.rand((M, K), 32), K + 8, 0, row_guard=4, device=dev)
    A2 = U.embed(U.rand((M, K), 33), K + 4 if what == "lda2_not_8" else K + 8, 0, row_guard=4, device=dev)
    out, part = r.o("out", N, K, F32), r.o("part", S * N, K, F32)
    e = TnArgs(G=G.data_ptr(), ldg=ld(G), A=A.data_ptr(), lda=ld(A), partial=part.v.data_ptr(), out=out.v.data_ptr(), accumulate=0, M=M, N=N, K=K,
               amode=0, gather=0, A2=A2.data_ptr(), lda2=ld(A2))
    arr = (TnArgs * 1)(e)
    return r, lib.call_rc("tuber_gemm_tn_group", arr, 1)


def _refuse_rows_dx2(dev, what):
    M, N, Nq, Kin = 30, 768, 512, 64
    ldg, ldt = N + 8, N + 8
    if what == "ldg_odd":
        ldg = N + 4
    elif what == "kin_not_16":
        Kin = 72
    elif what == "nq_not_span":
        Nq = 384
    r = Run(dev, None)
    g = U.embed(U.rand((M, N), 51), ldg, 0, row_guard=4, device=dev)
    wt = U.embed(U.rand((Kin, N), 52), ldt, 0, row_guard=4, device=dev)
    dx, dpos = r.o("dx", M, Kin), r.o("dpos", M, Kin)
    return r, lib.call_rc("tuber_rows_dx2", g, ld(g), M, N, Nq, wt, N - 8 if what == "ldt_below_n" else ld(wt), Kin, dx.v, None, dpos.v)


REFUSED = [("nt", _refuse_nt, w) for w in ("lda_odd", "ldb_odd", "k_not_64")] + \
          [("addproj", _refuse_addproj, w) for w in ("lda2_odd", "add_ncols_not_128")] + \
          [("join", lambda dev, w: _refuse_join(dev, "join", w), "lda_odd"), ("join_ds", lambda dev, w: _refuse_join(dev, "join_ds", w), "lda_odd")] + \
          [("join_mask", lambda dev, w: _refuse_join(dev, "join_mask", w), w) for w in ("n_not_64", "ldc_odd", "lda_odd")] + \
          [("join_ds_mask", lambda dev, w: _refuse_join(dev, "join_ds_mask", w), w) for w in ("n_not_64", "ldc_odd", "ldcd_odd")] + \
          [("join_strided_mask", lambda dev, w: _refuse_join(dev, "join_strided_mask", w), w) for w in ("n_not_64", "ldc_odd", "rows_not_grid")] + \
          [("join_strided", lambda dev, w: _refuse_join(dev, "join_strided", w), "rows_not_grid")] + \
          [("bn_out", _refuse_bn_out, w) for w in ("ldy_odd", "ldr32_not_4", "ldy32_not_4", "n_not_64")] + \
          [("tn", _refuse_tn, w) for w in ("ldg_not_4", "lda_not_4", "ld_below_ceil4", "bias_off_transpose_read")] + \
          [("tn_group", _refuse_tn_group, w) for w in ("ldg_not_8", "lda2_not_8", "slabs_without_accumulate_2")] + \
          [("rows_dx2", _refuse_rows_dx2, w) for w in ("ldg_odd", "ldt_below_n", "kin_not_16", "nq_not_span")]


@pytest.mark.parametrize("entry,fn,what", REFUSED, ids=["%s-%s" % (e, w) for e, _, w in REFUSED])
def test_refused_layouts_return_einval_and_write_nothing(dev, entry, fn, what):
    """every operand really has the geometry the call names (so even an accepted launch would stay inside memory the test owns); the launcher
    must answer TUBER_EINVAL before anything is launched, and every guarded output keeps its sentinel AND its NaN window.
    Base pointers are not part of this test: the loads are 16 bytes wide (8 in the in-register gemm_tn), the launchers take the caller's word
    that A / B / G and every 16-byte addressable epilogue tensor start on a 16-byte boundary (include/tuber_hip.h states it), and a
    misaligned pointer is not launched to see what happens."""
    r, rc = fn(dev, what)
    torch.cuda.synchronize()
    assert rc == EINVAL, (entry, what, rc)
    for name, g in r.outs.items():
        assert U.untouched(g), "%s %s: the refused call wrote to %s" % (entry, what, name)
