"""Plain helpers for the GEMM layout tests (test_gemm_layout_gpu.py / test_gemm_layout_cpu.py): no fixtures, no GPU needed.

  embed        an operand as a window inside a larger parent whose every other element is NaN (a read outside the window poisons the result)
  guarded_out  an output window (NaN) inside a parent of sentinel bits, `guard` rows before and after and ld - cols columns beside it
  assert_footprint   the sentinel survives bit for bit, the window is finite
  ref64 / tol / check   a float64 CPU reference from the bf16-rounded operands and an elementwise bound DERIVED from the number formats

The bound.  u32 = 2^-24, u16 = 2^-8 (unit roundoffs of fp32 / bf16), S = sum_k |a_k b_k| + sum |epilogue addends| (float64):
    tol32 = 2 (K + 8) u32 S             tol16 = u16 (|ref| + tol32) + tol32
Products of two bf16 values are exact in fp32; any summation order of K terms errs by at most (K - 1) u32 S to first order; + 8 covers the
epilogue's few fp32 operations; the factor 2 covers the accumulation order inside an MFMA.  Every element must pass."""
import numpy as np
import torch

BF = torch.bfloat16
U32, U16 = 2.0 ** -24, 2.0 ** -8
SENT16 = 0x5A3C              # bf16 bits: a finite value (1.3e16) no kernel under test produces
SENT32 = 0x5A3C1E0F          # fp32 bits: finite as well
GUARD = 128                  # rows before and behind an output: a whole tile of overrun lands in memory the test owns


def rand(shape, seed, scale=1.0, dtype=BF):
    """N(0, scale^2) on the CPU, rounded to `dtype` (the values a kernel actually sees)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def embed(x, ld, col0=0, row_guard=2, fill=float("nan"), device=None):
    """x [rows, cols] placed in a parent [row_guard + rows + row_guard][ld] of `fill`, starting row_guard rows down and col0 columns in;
    returns the VIEW (stride(0) == ld).  col0 a multiple of 8 elements keeps the 16-byte alignment of the window's rows."""
    rows, cols = x.shape
    assert ld >= col0 + cols and col0 % 8 == 0, (ld, col0, cols)
    parent = torch.full((rows + 2 * row_guard, ld), fill, dtype=x.dtype, device=device if device is not None else x.device)
    view = parent[row_guard:row_guard + rows, col0:col0 + cols]
    view.copy_(x)
    assert view.stride(0) == ld and view.stride(1) == 1
    return view


class Guarded:
    """an output window `v` [rows, cols] (leading dimension ld) inside `parent` [guard + rows + guard][ld]"""
    def __init__(self, rows, cols, ld, dtype, device, col0=0, guard=GUARD):
        assert dtype in (BF, torch.float32) and ld >= col0 + cols
        self.rows, self.cols, self.ld, self.col0, self.guard, self.dtype = rows, cols, ld, col0, guard, dtype
        bits = torch.full((rows + 2 * guard, ld), SENT16 if dtype == BF else SENT32, dtype=torch.int16 if dtype == BF else torch.int32)
        self.parent = bits.view(dtype).to(device)
        self.v = self.parent[guard:guard + rows, col0:col0 + cols]
        self.v.fill_(float("nan"))

    def bits(self):
        return self.parent.cpu().view(torch.int16 if self.dtype == BF else torch.int32)

    def outside(self):
        m = torch.ones(self.rows + 2 * self.guard, self.ld, dtype=torch.bool)
        m[self.guard:self.guard + self.rows, self.col0:self.col0 + self.cols] = False
        return m


def guarded_out(rows, cols, ld=None, dtype=BF, device="cpu", col0=0, guard=GUARD):
    return Guarded(rows, cols, cols if ld is None else ld, dtype, device, col0, guard)


def footprint_errors(g):
    """[] when every element outside the window still holds the sentinel bit for bit and every element inside is finite"""
    errs = []
    b, out = g.bits(), g.outside()
    sent = SENT16 if g.dtype == BF else SENT32
    bad = (b != sent) & out
    if bool(bad.any()):
        r, c = [int(t[0]) for t in torch.nonzero(bad, as_tuple=True)]
        errs.append("%d elements outside the window were written, first at parent row %d (window rows %d..%d) column %d (window columns %d..%d)"
                    % (int(bad.sum()), r, g.guard, g.guard + g.rows - 1, c, g.col0, g.col0 + g.cols - 1))
    fin = torch.isfinite(g.v.float().cpu())
    if not bool(fin.all()):
        r, c = [int(t[0]) for t in torch.nonzero(~fin, as_tuple=True)]
        errs.append("%d elements of the window are not finite (unwritten, or poisoned by a read outside an operand's window), first at (%d, %d)"
                    % (int((~fin).sum()), r, c))
    return errs


def assert_footprint(g, name=""):
    errs = footprint_errors(g)
    assert not errs, "%s: %s" % (name, "; ".join(errs))


def untouched(g):
    """a refused launch: the sentinel is intact and the window still holds nothing but the NaN guarded_out put there"""
    return bool(((g.bits() == (SENT16 if g.dtype == BF else SENT32)) | ~g.outside()).all()) and bool(torch.isnan(g.v.float()).all())


def untouched_window(g, value):
    """an output a launch must leave alone: the sentinel is intact and the window still holds the value it was filled with"""
    return bool(((g.bits() == (SENT16 if g.dtype == BF else SENT32)) | ~g.outside()).all()) and bool((g.v.float() == value).all())


def f64(x):
    return x.detach().cpu().double().numpy()


def ref64(A, B, alpha=1.0, addends=()):
    """(ref, S): ref = alpha * A . B^T + sum(addends) in float64 from the operands as given (already rounded to what the kernel reads),
    S = |alpha| * |A| . |B|^T + sum |addends|, the magnitude the rounding-error bound scales with.  Addends broadcast against [M, N]."""
    a, b = f64(A), f64(B)
    ref = alpha * (a @ b.T)
    S = abs(alpha) * (np.abs(a) @ np.abs(b).T)
    for t in addends:
        t = f64(t) if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)
        ref = ref + t
        S = S + np.abs(t)
    return ref, S


def ref64_tn(G, A, addends=()):
    """the weight-gradient form: ref = G^T . A (reduction over the rows), S likewise"""
    return ref64(G.t(), A.t(), 1.0, addends)


def fma32(x, a, b):
    """fp32 fma(x, a, b) as the kernels' prologues compute it (bf16 x, fp32 a and b): the product is exact in float64, one rounding to 53 bits and
    one to 24 (a double rounding differs from the fused result with probability ~2^-29 per element)"""
    return (x.detach().cpu().double() * a.detach().cpu().double() + b.detach().cpu().double()).float()


def bn_relu_bf16(A, sc, sh):
    """relu(A * sc + sh) in fp32, rounded to bf16: the operand the BatchNorm + ReLU prologue forms (an INPUT of the product, not its result)"""
    return fma32(A, sc, sh).relu().to(BF)


def add_bf16(A, A2):
    """bf16(A + A2), the sum formed in fp32: the operand of the addproj / A2 prologues"""
    return (A.detach().cpu().float() + A2.detach().cpu().float()).to(BF)


def tol(ref, S, K, out_bf16):
    t32 = 2.0 * (K + 8) * U32 * S
    return U16 * (np.abs(ref) + t32) + t32 if out_bf16 else t32


def worst(got, ref, tolv):
    """(worst err / tol, its index, all finite)"""
    got = f64(got) if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    err = np.abs(got - ref)
    fin = bool(np.isfinite(got).all())
    ratio = np.where(np.isfinite(err), err / np.maximum(tolv, 1e-300), np.inf)
    ratio = np.where((err == 0) & np.isfinite(err), 0.0, ratio)
    idx = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[idx]), tuple(int(i) for i in idx), fin


def check(name, got, ref, tolv, note=""):
    """|got - ref| <= tol for EVERY element; prints the worst err / tol and where"""
    r, idx, fin = worst(got, ref, tolv)
    print("%-58s worst err/tol %.3f at %s %s" % (name, r, idx, note))
    assert fin and r <= 1.0, "%s: worst err/tol %.3f at %s (got %r, ref %r, tol %.3e) %s" % (
        name, r, idx, float(f64(got)[idx]) if isinstance(got, torch.Tensor) else float(np.asarray(got)[idx]), float(ref[idx]), float(np.broadcast_to(tolv, ref.shape)[idx]), note)
    return r


def loose_close(got, ref, rel=2.0 ** -7):
    """what test_kernels_gpu.close() accepts: max |err| <= rel * max |ref| over the whole matrix (kept to show what it lets through)"""
    got = f64(got) if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    err = np.abs(got - ref).max()
    return bool(np.isfinite(err)) and err <= rel * (np.abs(ref).max() + 1e-12)


# the (M, N, K) of the GPU file: ragged last tiles for 64- and 96-row tiles, FULL / ragged widths, 1 / 3 / 17 k-tiles, and the shape that
# takes 96-row wave split-K by itself
SHAPES = [(130, 64, 64), (130, 80, 192), (200, 192, 64), (200, 192, 192), (130, 192, 1088), (200, 80, 1088), (200, 64, 1088), (1100, 1024, 1088)]
