"""Digest of the raw output bytes of every entry point of csrc/norm.hip and of the depthwise tile kernels that finalise a BatchNorm or fold
its backward in (tuber_dwconv_tile_fwd_bn*, tuber_dwconv_tile_bwd_*_bn and their _frozen forms), on seeded inputs at the small shapes of the
kernel tests.  Run it from the root of two trees (it loads the library of the tree it is started in) and compare the lists: a change that
claims to leave these kernels' arithmetic alone must leave every line equal.
usage: python scripts/bn_bytes_digest.py --out FILE         (one line per output: <entry point> <case> <output> <sha256>)
       python scripts/bn_bytes_digest.py --compare A B      (exit status 1 when a line differs or is missing)"""
import argparse
import hashlib
import os
import re
import sys

sys.path.insert(0, os.getcwd())


def compare(a, b):
    A, B = ([l.rstrip("\n") for l in open(p)] for p in (a, b))
    keys = lambda ls: [l.rsplit(" ", 1)[0] for l in ls]
    diff = [(x, y) for x, y in zip(A, B) if x != y]
    print("%d and %d digests, %d differ" % (len(A), len(B), len(diff) + abs(len(A) - len(B))))
    for x, y in diff:
        print("  DIFFERS: %s | %s" % (x, y))
    return 0 if not diff and keys(A) == keys(B) and A else 1


ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--compare", nargs=2)
opt = ap.parse_args()
if opt.compare:
    sys.exit(compare(*opt.compare))

import numpy as np
import torch
from tubelet_transformer_amd import lib

dev = torch.device("cuda:0")
BF = torch.bfloat16
lines, called = [], set()


def rnd(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dev)


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device=dev, dtype=dtype)


def call(name, *args):
    called.add(name)
    return lib.call(name, *args)


def query(name, *args):
    called.add(name)
    return lib.query(name, *args)


def rec(name, case, **outs):
    torch.cuda.synchronize()
    for k, v in outs.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().contiguous().cpu()
            raw = (v.view(torch.int16) if v.dtype == BF else v).numpy().tobytes()
        else:
            raw = repr(v).encode()
        lines.append("%s %s %s %s" % (name, case, k, hashlib.sha256(raw).hexdigest()))


def stat_rows(R, C, seed, positive=False):
    a, b = rnd(R, C, seed=seed), rnd(R, C, seed=seed + 1)
    return a, (b.abs() + 1.0 if positive else b)


# ---- the finalize kernels: both instantiations (R <= 128: 256 threads), a partial 32-channel block (C = 100) ----
for R, C in ((7, 256), (97, 100), (300, 100), (517, 256)):
    case = "R%d_C%d" % (R, C)
    st0, st1 = stat_rows(R, C, 10, positive=True)
    st1 = st1 * 40.0
    gamma, beta = 1 + 0.1 * rnd(C, seed=2), 0.1 * rnd(C, seed=3)
    for name, mom, n0 in (("tuber_bn_finalize", 0.1, 41), ("tuber_bn_finalize_ex", 0.03, 41), ("tuber_bn_finalize_ex", -1.0, 41)):
        rm, rv = 0.1 * rnd(C, seed=4), 1 + 0.1 * rnd(C, seed=5).abs()
        nbt = torch.full((1,), n0, dtype=torch.int64, device=dev)
        o = [nan(C) for _ in range(4)]
        call(name, st0, st1, R, C, 37.0 * R, gamma, beta, rm, rv, nbt, mom, 1e-3, *o)
        rec(name, "%s_mom%g" % (case, mom), scale=o[0], shift=o[1], mean=o[2], invstd=o[3], rmean=rm, rvar=rv, nbt=nbt)
    o = [nan(C) for _ in range(4)]
    call("tuber_bn_finalize_ex", st0, st1, R, C, 1.0, gamma, beta, None, None, None, 0.1, 1e-3, *o)      # count = 1, no running statistics
    rec("tuber_bn_finalize_ex", case + "_norunning", scale=o[0], shift=o[1], mean=o[2], invstd=o[3])
    mean, invstd = 0.3 + 0.1 * rnd(C, seed=8), 1.0 / (1.5 + 0.1 * rnd(C, seed=9).abs())
    b0, b1 = stat_rows(R, C, 20)
    for acc in (0, 1):
        k = [nan(C) for _ in range(3)]
        dg, db = rnd(C, seed=30), rnd(C, seed=31)
        call("tuber_bn_bwd_finalize", b0, b1, R, C, 37.0 * R, gamma, mean, invstd, *k, dg, db, acc)
        rec("tuber_bn_bwd_finalize", "%s_acc%d" % (case, acc), cA=k[0], cB=k[1], cC=k[2], dgamma=dg, dbeta=db)
    k = [nan(C) for _ in range(3)]
    call("tuber_bn_bwd_finalize", b0, b1, R, C, 37.0 * R, gamma, mean, invstd, *k, None, None, 0)
    rec("tuber_bn_bwd_finalize", case + "_nograds", cA=k[0], cB=k[1], cC=k[2])
    dg, db = rnd(C, seed=30), rnd(C, seed=31)
    call("tuber_bn_frozen_param_grads", b0, b1, R, C, mean, invstd, dg, db)
    rec("tuber_bn_frozen_param_grads", case, dgamma=dg, dbeta=db)

nbt = torch.tensor([5, 9], dtype=torch.int64, device=dev)
table = torch.tensor([nbt.data_ptr(), nbt.data_ptr() + 8], dtype=torch.int64).to(dev)
call("tuber_bn_count_advance", table, 2)
rec("tuber_bn_count_advance", "two", nbt=nbt)

rec("tuber_stat_rows_reduced", "values", v=[query("tuber_stat_rows_reduced", R) for R in (1, 512, 513, 5440)])
st0, st1 = stat_rows(1000, 100, 40)
o0, o1 = nan(64, 100), nan(64, 100)
call("tuber_stat_rows_reduce", st0, st1, 1000, 100, o0, o1)
rec("tuber_stat_rows_reduce", "R1000_C100", o0=o0, o1=o1)

# ---- eval / frozen affine maps ----
Cs = [64, 1000, 100]
layers = []
for i, C in enumerate(Cs):
    L = dict(C=C, gamma=1 + 0.3 * rnd(C, seed=10 * i), beta=0.2 * rnd(C, seed=10 * i + 1), rm=rnd(C, seed=10 * i + 2), rv=rnd(C, seed=10 * i + 3).abs() + 1e-3)
    for k in ("scale", "shift", "mean", "invstd", "cA", "cB", "cC", "scale1", "shift1", "scale2", "shift2"):
        L[k] = nan(C)
    layers.append(L)
    call("tuber_bn_eval_affine", L["gamma"], L["beta"], L["rm"], L["rv"], 1e-5, L["scale1"], L["shift1"], C)
    rec("tuber_bn_eval_affine", "C%d" % C, scale=L["scale1"], shift=L["shift1"])
t8 = torch.tensor([[L[k].data_ptr() for k in ("gamma", "beta", "rm", "rv", "scale2", "shift2")] + [L["C"], 0] for L in layers], dtype=torch.int64).to(dev)
call("tuber_bn_eval_affine_multi", t8, len(Cs), max(Cs), 1e-5)
t12 = torch.tensor([[L[k].data_ptr() for k in ("gamma", "beta", "rm", "rv", "scale", "shift", "mean", "invstd", "cA", "cB", "cC")] + [L["C"]] for L in layers],
                   dtype=torch.int64).to(dev)
call("tuber_bn_frozen_affine_multi", t12, len(Cs), max(Cs), 1e-3)
for L in layers:
    rec("tuber_bn_eval_affine_multi", "C%d" % L["C"], scale=L["scale2"], shift=L["shift2"])
    rec("tuber_bn_frozen_affine_multi", "C%d" % L["C"], **{k: L[k] for k in ("scale", "shift", "mean", "invstd", "cA", "cB", "cC")})

# ---- the residual join and the BatchNorm backward apply ----
for M, C, ds in ((3000, 256, False), (700, 2048, True), (37, 64, True)):
    case = "M%d_C%d_ds%d" % (M, C, ds)
    c4, res = rnd(M, C, seed=1).to(BF), rnd(M, C, seed=2).to(BF)
    s4, h4 = 1 + 0.1 * rnd(C, seed=3), 0.1 * rnd(C, seed=4)
    rs, rh = (1 + 0.1 * rnd(C, seed=5), 0.1 * rnd(C, seed=6)) if ds else (None, None)
    y = nan(M, C, dtype=BF)
    call("tuber_block_out_fwd", c4, s4, h4, res, rs, rh, y, M, C)
    rec("tuber_block_out_fwd", case, y=y)
    y2, mk = nan(M, C, dtype=BF), torch.full((M, C // 8), 0xAA, dtype=torch.uint8, device=dev)
    call("tuber_block_out_fwd_mask", c4, s4, h4, res, rs, rh, y2, mk, M, C)
    rec("tuber_block_out_fwd_mask", case, y=y2, mask=mk)
    res32 = rnd(M, C, seed=7)
    for form, r32 in (("bf16res", None), ("res32", res32)):
        y3, y32 = nan(M, C, dtype=BF), nan(M, C)
        call("tuber_block_out_fwd_f32", c4, s4, h4, res, rs, rh, r32, y3, y32, M, C)
        rec("tuber_block_out_fwd_f32", case + "_" + form, y=y3, y32=y32)
    dy, dz = rnd(M, C, seed=8).to(BF), nan(M, C, dtype=BF)
    Rb = query("tuber_rowblock_count", M, C)
    a, b, c = (nan(Rb, C) for _ in range(3))
    call("tuber_block_out_bwd", dy, y, c4, res if ds else None, dz, a, b, c if ds else None, M, C)
    rec("tuber_block_out_bwd", case, rows=Rb, dz=dz, st_dz=a, st_c4=b, **({"st_ds": c} if ds else {}))
    dx = nan(M, C, dtype=BF)
    call("tuber_bn_bwd_apply", dz, c4, s4, h4, 0.01 * s4, dx, M, C)
    rec("tuber_bn_bwd_apply", case, dx=dx)

# ---- BatchNorm backward in one launch: every rows-per-thread instantiation, train-mode and frozen ----
rec("tuber_bn_bwd_fa_max_rows", "value", v=query("tuber_bn_bwd_fa_max_rows"))
for M, C, R in ((1000, 128, 7), (2816, 512, 128), (5632, 256, 88)):
    dz, x = rnd(M, C, seed=1).to(BF), (rnd(M, C, seed=2) * 1.5 + 0.3).to(BF)
    gamma = 1.0 + 0.1 * rnd(C, seed=7)
    mean, invstd = 0.3 + 0.1 * rnd(C, seed=8), 1.0 / (1.5 + 0.1 * rnd(C, seed=9).abs())
    b0, b1 = stat_rows(R, C, 20)
    rec("tuber_bn_bwd_fa_rows", "M%d_C%d" % (M, C), v=query("tuber_bn_bwd_fa_rows", M, C))
    for kr in (0, 4, 8, 11):
        case = "M%d_C%d_R%d_kr%d" % (M, C, R, kr)
        query("tuber_bn_bwd_fa_rows_set", kr)
        dg, db, dx = rnd(C, seed=30), rnd(C, seed=31), nan(M, C, dtype=BF)
        call("tuber_bn_bwd_fa", b0, b1, R, C, float(M), gamma, mean, invstd, dg, db, dz, x, dx, M)
        rec("tuber_bn_bwd_fa", case, dgamma=dg, dbeta=db, dx=dx)
        dg, db, dx = rnd(C, seed=30), rnd(C, seed=31), nan(M, C, dtype=BF)
        call("tuber_bn_bwd_fa_frozen", b0, b1, R, C, gamma, mean, invstd, dg, db, dz, dx, M)
        rec("tuber_bn_bwd_fa_frozen", case, dgamma=dg, dbeta=db, dx=dx)
        dx = nan(M, C, dtype=BF)
        call("tuber_bn_bwd_fa_frozen", None, None, 0, C, gamma, mean, invstd, None, None, dz, dx, M)
        rec("tuber_bn_bwd_fa_frozen", case + "_nograds", dx=dx)
    query("tuber_bn_bwd_fa_rows_set", 0)

# ---- LayerNorm ----
seed = torch.tensor([1234], dtype=torch.int64, device=dev)
for M, E in ((704, 256), (30, 256), (77, 2048)):
    x, r = rnd(M, E, seed=1).to(BF), rnd(M, E, seed=2).to(BF)
    x32, r32 = rnd(M, E, seed=3) + 100.0, rnd(M, E, seed=4)
    g, b = 1 + 0.1 * rnd(E, seed=5), 0.1 * rnd(E, seed=6)
    nb = query("tuber_layernorm_bwd_blocks", M)
    dy = rnd(M, E + 8, seed=7).to(BF)
    for p in (0.0, 0.1):
        case = "M%d_E%d_p%g" % (M, E, p)
        y, xh, rstd = nan(M, E + 8, dtype=BF), nan(M, E, dtype=BF), nan(M)
        call("tuber_layernorm_fwd", x, r, g, b, y, E + 8, xh, rstd, M, E, 1e-5, p, seed, 7)
        rec("tuber_layernorm_fwd", case, y=y[:, :E], xhat=xh, rstd=rstd)
        part, dx, dxd, dgb = nan(2 * nb * E), nan(M, E, dtype=BF), nan(M, E, dtype=BF), nan(2 * E)
        call("tuber_layernorm_bwd", dy, E + 8, xh, rstd, g, dx, dxd, part, dgb, dgb.data_ptr() + 4 * E, 0, M, E, p, seed, 7)
        rec("tuber_layernorm_bwd", case, blocks=nb, dx=dx, dxd=dxd, dgamma_dbeta=dgb)
        dg, db = rnd(E, seed=8), rnd(E, seed=9)
        call("tuber_layernorm_bwd", dy, E + 8, xh, rstd, g, dx, None, part, dg, db, 1, M, E, p, seed, 7)
        rec("tuber_layernorm_bwd", case + "_separate", dx=dx, dgamma=dg, dbeta=db)
    y = nan(M, E, dtype=BF)
    call("tuber_layernorm_fwd", x, None, g, b, y, E, None, None, M, E, 1e-5, 0.0, None, 0)
    rec("tuber_layernorm_fwd", "M%d_E%d_plain" % (M, E), y=y)
    for form, a32, rb, rf, want32 in (("x", None, None, None, True), ("x32", x32, None, None, False), ("x_res", None, r, None, True),
                                      ("x32_res32", x32, r, r32, True), ("x_res32", None, r, r32, False)):
        y, y32 = nan(M, E + 8, dtype=BF), nan(M, E) if want32 else None
        call("tuber_layernorm_fwd_f32", x, a32, rb, rf, g, b, y, E + 8, y32, M, E, 1e-5)
        rec("tuber_layernorm_fwd_f32", "M%d_E%d_%s" % (M, E, form), y=y[:, :E], **({"y32": y32} if want32 else {}))

# ---- column reductions ----
P = rnd(70, 100, seed=1)
for acc in (0, 1):
    out = rnd(100, seed=2)
    call("tuber_reduce_rows", P, out, 70, 100, acc)
    rec("tuber_reduce_rows", "R70_C100_acc%d" % acc, out=out)
for M, C, ld in ((704, 256, 256), (180, 3, 64), (16896, 512, 512)):
    gq = rnd(M, ld, seed=1).to(BF)
    nbc = query("tuber_colsum_blocks", M)
    part, out = nan(nbc * C), rnd(C, seed=2)
    call("tuber_colsum", gq, part, out, 1, M, C, ld)
    rec("tuber_colsum", "M%d_C%d" % (M, C), blocks=nbc, out=out)
ENTRY = np.dtype([("P", "<u8"), ("out", "<u8"), ("n", "<i8"), ("stride", "<i8"), ("S", "<i4"), ("mode", "<i4"), ("C", "<i4"), ("next", "<i4")])
assert query("tuber_multi_reduce_entry_bytes") == ENTRY.itemsize
rec("tuber_multi_reduce_entry_bytes", "value", v=ENTRY.itemsize)
Ps = [rnd(3, 1000, seed=1), rnd(5, 8192, seed=2), rnd(70, 100, seed=3), rnd(40, 100, seed=4), rnd(9, 27, 64, seed=5)]
outs = [rnd(1000, seed=6), nan(8192), rnd(100, seed=7), rnd(64, 27, seed=8)]
ent = np.zeros(5, dtype=ENTRY)
for i, (Pi, oi, n, S, mode, C, nxt) in enumerate(((0, 0, 1000, 3, 0, 0, -1), (1, 1, 8192, 5, 2 | 8, 0, -1), (2, 2, 100, 70, 1, 0, 3), (3, 2, 100, 40, 1, 0, -1),
                                                (4, 3, 27 * 64, 9, 1, 64, -1))):
    ent[i] = (Ps[Pi].data_ptr(), outs[oi].data_ptr(), n, n, S, mode, C, nxt)
blk = [(0, 0)] + [(1, j) for j in range(2)] + [(2, j) for j in range(4)] + [(4, j) for j in range(54)]
call("tuber_multi_reduce", torch.from_numpy(ent.view(np.uint8)).to(dev), torch.tensor(blk, dtype=torch.int32).to(dev), len(blk))
rec("tuber_multi_reduce", "modes", **{"out%d" % i: o for i, o in enumerate(outs)})

# ---- the depthwise tile kernels with a BatchNorm finalised in front or its backward folded in ----
for N, T, H, W, C, R in ((1, 6, 9, 21, 64, 7), (2, 8, 16, 22, 256, 88), (1, 4, 16, 22, 128, 128)):
    case = "N%d_%dx%dx%d_C%d_R%d" % (N, T, H, W, C, R)
    M = N * T * H * W
    Rb = query("tuber_dwconv_tile_blocks", N, T, H, W, C)
    nbw = query("tuber_dwconv_tile_wgrad_blocks", N, T, H, W, C)
    x = rnd(N, T, H, W, C, seed=1, scale=1.5).to(BF)
    w = rnd(C, 27, seed=2, scale=27 ** -0.5)
    gamma, beta = 1 + 0.1 * rnd(C, seed=3), 0.1 * rnd(C, seed=4)
    for Rf in (R, 150):                                                    # 150: the loop for lists longer than the early-issued rows
        p0, p1 = stat_rows(Rf, C, 10, positive=True)
        p1 = p1 * 40.0
        for name, mom in (("tuber_dwconv_tile_fwd_bn", 0.1), ("tuber_dwconv_tile_fwd_bn_ex", 0.03), ("tuber_dwconv_tile_fwd_bn_ex", -1.0)):
            rm, rv = 0.1 * rnd(C, seed=5), 1 + 0.1 * rnd(C, seed=6).abs()
            nbt = torch.full((1,), 41, dtype=torch.int64, device=dev)
            o = [nan(C) for _ in range(4)]
            out, s0, s1 = nan(N, T, H, W, C, dtype=BF), nan(Rb, C), nan(Rb, C)
            call(name, x, p0, p1, Rf, 37.0 * Rf, gamma, beta, rm, rv, nbt, mom, 1e-3, *o, w, out, s0, s1, N, T, H, W, C)
            rec(name, "%s_Rf%d_mom%g" % (case, Rf, mom), scale=o[0], shift=o[1], mean=o[2], invstd=o[3], rmean=rm, rvar=rv, nbt=nbt, out=out, st0=s0, st1=s1)
    dz3, c3, c1 = rnd(M, C, seed=1).to(BF), (rnd(M, C, seed=2) * 1.5 + 0.3).to(BF), rnd(M, C, seed=3).to(BF)
    sc1, sh1 = 1.0 + 0.2 * rnd(C, seed=5), 0.3 * rnd(C, seed=6)
    mean, invstd = 0.3 + 0.1 * rnd(C, seed=8), 1.0 / (1.5 + 0.1 * rnd(C, seed=9).abs())
    b0, b1 = stat_rows(R, C, 20)
    for frozen in (False, True):
        sfx = "_frozen" if frozen else ""
        head = (dz3,) if frozen else (dz3, c3)
        cnt = () if frozen else (float(M),)
        for grads in ((True, False) if frozen else (True,)):
            cs = case + ("" if grads else "_nograds")
            rows = (b0, b1, R) if grads else (None, None, 0)
            dg, db = (rnd(C, seed=30), rnd(C, seed=31)) if grads else (None, None)
            dz1, o0, o1 = nan(M, C, dtype=BF), nan(Rb, C), nan(Rb, C)
            call("tuber_dwconv_tile_bwd_data_bn" + sfx, *head, *rows, *cnt, gamma, mean, invstd, dg, db, w, c1, sc1, sh1, dz1, o0, o1, N, T, H, W, C)
            rec("tuber_dwconv_tile_bwd_data_bn" + sfx, cs, dz=dz1, st0=o0, st1=o1, **({"dgamma": dg, "dbeta": db} if grads else {}))
            dg, db = (rnd(C, seed=30), rnd(C, seed=31)) if grads else (None, None)
            dz1, o0, o1, part = nan(M, C, dtype=BF), nan(Rb, C), nan(Rb, C), nan(Rb * 27 * C)
            call("tuber_dwconv_tile_bwd_both_bn" + sfx, *head, *rows, *cnt, gamma, mean, invstd, dg, db, w, c1, sc1, sh1, dz1, o0, o1, part, N, T, H, W, C)
            rec("tuber_dwconv_tile_bwd_both_bn" + sfx, cs, dz=dz1, st0=o0, st1=o1, partial=part, **({"dgamma": dg, "dbeta": db} if grads else {}))
        part, dwg = nan(nbw * 27 * C), nan(C, 27)
        wrows = () if frozen else (b0, b1, R)
        call("tuber_dwconv_tile_bwd_weight_bn" + sfx, *head, *wrows, *cnt, gamma, mean, invstd, c1, sc1, sh1, part, dwg, 0, N, T, H, W, C)
        rec("tuber_dwconv_tile_bwd_weight_bn" + sfx, case, dw=dwg)

src = open(os.path.join("tubelet_transformer_amd", "csrc", "norm.hip")).read()
missing = sorted(set(re.findall(r"^int (tuber_\w+)\(", src, re.M)) - called)
assert not missing, "entry points of norm.hip without a digest: %s" % missing
with open(opt.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("%d digests of %d entry points -> %s" % (len(lines), len(called), opt.out))
