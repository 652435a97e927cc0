"""The step monitor on the device (csrc/tensor_stats.hip, monitor.py): the kernel against an fp64 restatement on a synthetic flat layout,
where a row goes (cadence, ring, the keep-first bad slot), the argument checks, the launch inside the eager and the captured training step,
that it only reads, a non-finite step, and the training loop.  Small shapes (2 x 32 x 64 x 96 clips, the CSN-TEST body), dropout off.

Error bound of a sum of squares against the fp64 restatement (which takes the fp32 betas and eps of the device table and fp64 everywhere
else): ``|err| <= (k + c) * 2^-24 * S64`` with S64 the fp64 sum and k the longest chain of fp32 additions from an element to the result.  For
this kernel's reduction shape (CH = tuber_tensor_stats_chunk(), 256 threads per chunk):
    a thread adds at most CH / 256 elements of its float4 trips plus one tail element        CH / 256 + 1
    wave_sum: 6 exchange levels; the four wave results: 3 additions                          9
    a tensor's chunks: 8 lane groups take every eighth chunk in order, then 3 exchange levels  ceil(chunks / 8) + 3
so k = CH / 256 + 13 + ceil(chunks(tensor) / 8) (the issue's CH / 256 + 8 + chunks(tensor) describes a serial second stage).  c = 2 for the
gradient and parameter columns (the rounding of the square, fused or not, and slack), c = 16 for column 7: u is five rounded fp32 operations on
two rounded bias corrections, squared.  Counts and maxima are exact."""
import math
import os

import numpy as np
import pytest
import torch

from tubelet_transformer_amd import lib, monitor, synth
from tubelet_transformer_amd.config import load_cfg
from tubelet_transformer_amd.monitor import StepMonitor, monitor_of
from tubelet_transformer_amd.training import GraphedTrainStep, build_optimizer, train_step, train_tuber_detection
from tubelet_transformer_amd.tuber import build_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
U = 2.0 ** -24
EXACT, SUMS = (1, 2, 3, 5, 6), ((0, 2), (4, 2), (7, 16))
GROUP_A, GROUP_B, NO_GROUP = (0.9, 0.999, 1e-8), (0.8, 0.99, 1e-6), (0.0, 0.0, 0.0)


def _model(dev):
    cfg = load_cfg(os.path.join(ROOT, "configuration", "TubeR_CSN152_AVA21.yaml"))
    cfg.CONFIG.MODEL.BACKBONE_NAME = "CSN-TEST"
    model, crit, post = build_model(cfg)
    synth.load_name_hashed(model)
    synth.zero_dropout(model)
    model.to(dev).train()
    crit.to(dev).train()
    return cfg, model, crit


def _batch(i, dev):
    return (synth.synthetic_clips(2, 32, 64, 96, seed=40 + i, device=dev),
            synth.synthetic_targets(2, "ava", 80, seed=60 + i, device=dev, hw=(64, 96)))


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def rc(name, *args):
    """the launcher's return code, without lib.call's raise"""
    fn = getattr(lib.load(), name)
    sig = lib._sigs[name]
    if len(args) == len(sig) - 1:
        args = args + (lib.current_stream(),)
    return fn(*[lib._conv(v, t) for v, (t, _) in zip(args, sig)])


# ------------------------------------------------------------------------------------------------------------------------------
# the fp64 restatement and the bound
# ------------------------------------------------------------------------------------------------------------------------------
def _restate(g, p, m, v, offsets, numels, hyper, t):
    """[T, 8] fp64 table of the flat buffers; hyper [T, 3] = (beta1, beta2, eps) as the device table holds them (fp32); t = the AdamW step
    count of the bias corrections (0: none).  Everything outside the tensors' own elements falls into a bucket that is dropped."""
    dev, T = g.device, len(numels)
    seg = torch.full((g.numel(),), T, dtype=torch.int64, device=dev)
    for ti, (o, n) in enumerate(zip(offsets, numels)):
        seg[o:o + n] = ti

    def sums(x):
        return torch.zeros(T + 1, dtype=torch.float64, device=dev).index_add_(0, seg, x.double())[:T]

    def maxs(x):
        return torch.zeros(T + 1, dtype=torch.float64, device=dev).scatter_reduce_(0, seg, x, "amax")[:T]

    out = torch.zeros(T, 8, dtype=torch.float64, device=dev)
    for base, x in ((0, g), (4, p)):
        fin = torch.isfinite(x)
        a = torch.where(fin, x.double().abs(), torch.zeros((), dtype=torch.float64, device=dev))
        out[:, base] = sums(a * a)
        out[:, base + 1] = maxs(a)
        out[:, base + 2] = sums(~fin)
        if base == 0:
            out[:, 3] = sums(x == 0)
    if m is not None and v is not None:
        h = torch.cat([torch.as_tensor(np.asarray(hyper, dtype=np.float32)).double(), torch.zeros(1, 3, dtype=torch.float64)]).to(dev)[seg]
        bc1 = 1.0 - h[:, 0] ** t if t >= 1 else torch.ones_like(h[:, 0])
        bc2 = 1.0 - h[:, 1] ** t if t >= 1 else torch.ones_like(h[:, 1])
        u = (m.double() / bc1) / (v.double().sqrt() / bc2.sqrt() + h[:, 2])
        u = torch.where(m == 0, torch.zeros((), dtype=torch.float64, device=dev), u)
        out[:, 7] = sums(u * u)
    return out


def _check_table(name, got, ref, nchunks, chunk, moments=True):
    """exact columns bit for bit, sums of squares within (k + c) * 2^-24 * S64; prints every figure before it asserts"""
    got, ref = got.detach().double().cpu(), ref.cpu()
    k = chunk // 256 + 13 + torch.as_tensor(np.asarray(nchunks)).double().div(8).ceil()
    worst = {}
    for col, c in SUMS:
        tol = (k + c) * U * ref[:, col]
        err = (got[:, col] - ref[:, col]).abs()
        worst[col] = float(torch.where(err > 0, err / tol.clamp_min(1e-300), torch.zeros_like(err)).max())
    exact = {col: bool(torch.equal(got[:, col], ref[:, col])) for col in EXACT}
    print("%-40s err/tol col0 %.3f col4 %.3f col7 %.3f   exact %s" % (name, worst[0], worst[4], worst[7], exact))
    assert bool(torch.isfinite(got[:, [0, 1, 2, 3, 4, 5, 6]]).all())
    assert all(exact.values()), "%s: columns %s differ" % (name, [c for c, ok in exact.items() if not ok])
    assert worst[0] <= 1.0 and worst[4] <= 1.0 and worst[7] <= 1.0, "%s: err/tol %s" % (name, worst)
    if not moments:
        assert bool((got[:, 7] == 0).all())


# ------------------------------------------------------------------------------------------------------------------------------
# a synthetic flat layout driven through the C entry point
# ------------------------------------------------------------------------------------------------------------------------------
PAD = 8


class _Raw:
    """tables and output buffers of tuber_tensor_stats for a flat layout, each output with PAD sentinel floats behind it"""

    def __init__(self, dev, numels, hyper, every=1, history=1):
        self.chunk = lib.query("tuber_tensor_stats_chunk")
        assert lib.query("tuber_tensor_stats_tensor_bytes") == monitor.TENSOR.itemsize
        assert lib.query("tuber_tensor_stats_chunk_bytes") == monitor.CHUNK.itemsize
        self.numels, self.hyper, self.history = list(numels), list(hyper), history
        self.offsets, off = [], 0
        for n in numels:
            self.offsets.append(off)
            off += (n + 63) // 64 * 64
        self.total, self.T = off, len(numels)
        chunks = monitor.chunk_table(self.offsets, numels, self.chunk)
        tens = np.zeros(self.T, dtype=monitor.TENSOR)
        count = np.bincount(chunks["tensor"], minlength=self.T)
        tens["nchunks"], tens["chunk0"] = count, np.cumsum(count) - count
        tens["beta1"], tens["beta2"], tens["eps"] = zip(*hyper)
        self.nchunks, self.n_chunks = count, len(chunks)
        self.chunks = torch.from_numpy(chunks.view(np.uint8).copy()).to(dev)
        self.tensors = torch.from_numpy(tens.view(np.uint8).copy()).to(dev)
        self.state = torch.tensor([every, history, 0, 0], dtype=torch.int32, device=dev)
        self.row_step = torch.full((history,), -1, dtype=torch.int32, device=dev)
        mk = lambda n: torch.full((n + PAD,), 777.0, device=dev)
        self._bufs = {"partial": mk(self.n_chunks * 8), "row_norm": mk(2 * history), "ring": mk(history * self.T * 8), "bad": mk(self.T * 8)}
        self.partial, self.row_norm = self._bufs["partial"][:-PAD], self._bufs["row_norm"][:-PAD]
        self.ring, self.bad = self._bufs["ring"][:-PAD], self._bufs["bad"][:-PAD]

    def args(self, g, p, m, v, t, clip):
        return (g, p, m, v, self.tensors, self.T, self.chunks, self.n_chunks, self.partial, self.state, self.history, self.row_step,
                self.row_norm, self.ring, self.bad, t, clip)

    def launch(self, g, p, m, v, t=None, clip=None):
        lib.call("tuber_tensor_stats", *self.args(g, p, m, v, t, clip))
        torch.cuda.synchronize()

    def row(self, slot=0):
        return self.ring.view(self.history, self.T, 8)[slot].clone()

    def sentinels_intact(self):
        return all(bool((b[-PAD:] == 777.0).all()) for b in self._bufs.values())


def _values(n, gen, dev):
    """n values in +-[1e-3, 1e3], log-uniform"""
    mag = torch.pow(10.0, torch.rand(n, device=dev, generator=gen) * 6.0 - 3.0)
    return torch.where(torch.rand(n, device=dev, generator=gen) < 0.5, -mag, mag)


def _synthetic(dev):
    CH = lib.query("tuber_tensor_stats_chunk")
    numels = [1, 3, 63, 64, 65, CH - 1, CH, CH + 1, 3 * CH + 5]
    hyper = [GROUP_A, GROUP_B, NO_GROUP, GROUP_A, GROUP_B, GROUP_A, GROUP_B, GROUP_A, GROUP_B]
    raw = _Raw(dev, numels, hyper)
    gen = torch.Generator(device=dev).manual_seed(11)
    nan, inf = float("nan"), float("inf")
    size = raw.total + 64                                   # a sentinel region behind each buffer
    g, m = torch.full((size,), nan, device=dev), torch.full((size,), nan, device=dev)      # padding and sentinel: NaN / 1e30
    p, v = torch.full((size,), 1e30, device=dev), torch.full((size,), 1e30, device=dev)
    for ti, (o, n) in enumerate(zip(raw.offsets, numels)):
        g[o:o + n], p[o:o + n] = _values(n, gen, dev), _values(n, gen, dev)
        m[o:o + n], v[o:o + n] = _values(n, gen, dev), _values(n, gen, dev) ** 2
        if hyper[ti] == NO_GROUP:
            m[o:o + n], v[o:o + n] = 0.0, 0.0
    o = raw.offsets
    g[o[0]] = inf                                           # a one-element tensor that is all non-finite
    g[o[1]], p[o[1] + 2] = nan, -inf                        # first / last element
    g[o[3] + 5], g[o[3] + 6] = 0.0, -0.0                    # exact zeros of both signs
    g[o[4] + 64] = inf                                      # the scalar tail behind a full float4 run
    g[o[6] + CH - 1] = 0.0
    g[o[7] + CH - 1], p[o[7]], p[o[7] + CH] = nan, -inf, nan            # left of a chunk boundary; first; last = a one-element chunk
    g[o[8] + CH - 1], g[o[8] + CH], g[o[8] + 3 * CH + 4] = -inf, nan, nan            # both sides of a chunk boundary, the last element
    p[o[8]], p[o[8] + 2 * CH - 1], p[o[8] + 2 * CH] = inf, nan, inf
    g[o[8] + 100:o[8] + 110] = 0.0
    return raw, g, p, m, v


def test_kernel_matches_the_fp64_restatement(dev):
    raw, g, p, m, v = _synthetic(dev)
    CH, T = raw.chunk, raw.T
    before = [x.clone() for x in (g, p, m, v)]
    t = torch.tensor([3], dtype=torch.int32, device=dev)
    raw.launch(g, p, m, v, t, None)                         # a good step at t = 3, every 1, history 1 -> slot 0
    first = raw.row()
    ref = _restate(g, p, m, v, raw.offsets, raw.numels, raw.hyper, 3)
    _check_table("synthetic t=3", first, ref, raw.nchunks, CH)
    assert first[0].tolist() == [0.0, 0.0, 1.0, 0.0] + first[0, 4:].tolist()          # every element non-finite: sum and maximum 0
    assert first[3, 3] == 2 and first[8, 2] == 3 and first[8, 6] == 3 and first[8, 3] == 10 and first[7, 6] == 2
    assert bool((first[2, 7] == 0)) and bool((first[[0, 1, 3], 7] > 0).all())        # no group, zero moments: 0, not 0 / 0
    assert int(raw.row_step[0]) == 3 and raw.row_norm.tolist() == [0.0, 1.0]
    # the same input twice: bit-identical
    raw.ring.zero_()
    raw.launch(g, p, m, v, t, None)
    assert _same_bits(raw.row(), first)
    # without moments (either pointer NULL): column 7 is 0, the others keep their bits
    for mm, vv in ((None, None), (m, None), (None, v)):
        raw.ring.fill_(5.0)
        raw.launch(g, p, mm, vv, t, None)
        got = raw.row()
        assert _same_bits(got[:, :7], first[:, :7]) and bool((got[:, 7] == 0).all())
    # both pointers NULL: unconditional, slot 0, no bias correction
    raw.launch(g, p, m, v, None, None)
    _check_table("synthetic unconditional", raw.row(), _restate(g, p, m, v, raw.offsets, raw.numels, raw.hyper, 0), raw.nchunks, CH)
    assert int(raw.row_step[0]) == 0 and raw.state.tolist() == [1, 1, 0, 0]
    # padding and sentinels neither influenced a row (the restatement drops them) nor changed
    assert all(_same_bits(a, b) for a, b in zip((g, p, m, v), before)) and raw.sentinels_intact()
    assert bool((raw.bad == 777.0).all())


def test_argument_checks(dev):
    raw = _Raw(dev, [5, 70], [GROUP_A, GROUP_B])
    n = raw.total + 4
    g, p, m, v = (torch.ones(n, device=dev) for _ in range(4))
    t, clip = torch.tensor([1], dtype=torch.int32, device=dev), torch.tensor([1.0, 1.0], device=dev)
    good = raw.args(g[:raw.total], p[:raw.total], m[:raw.total], v[:raw.total], t, clip)
    bad = []
    for i in (0, 1, 4, 6, 8, 9, 11, 12, 13, 14):           # g, p, tensors, chunks, partial, state, row_step, row_norm, ring, bad: NULL
        bad.append(good[:i] + (None,) + good[i + 1:])
    for i, x in ((0, g), (1, p), (2, m), (3, v)):           # 4 bytes off a 16-byte boundary
        bad.append(good[:i] + (x[1:raw.total + 1],) + good[i + 1:])
    bad.append(good[:5] + (0,) + good[6:])                  # n_tensors = 0
    bad.append(good[:5] + (-2,) + good[6:])
    bad.append(good[:7] + (0,) + good[8:])                  # n_chunks = 0
    bad.append(good[:10] + (0,) + good[11:])                # history = 0
    for args in bad:
        assert rc("tuber_tensor_stats", *args) == EINVAL
    torch.cuda.synchronize()
    assert bool((raw.ring == 777.0).all()) and raw.state.tolist() == [1, 1, 0, 0] and int(raw.row_step[0]) == -1
    assert rc("tuber_tensor_stats", *good) == 0
    torch.cuda.synchronize()
    assert raw.row()[:, 0].tolist() == [5.0, 70.0] and raw.sentinels_intact()


# ------------------------------------------------------------------------------------------------------------------------------
# placement: cadence, ring, the keep-first bad slot
# ------------------------------------------------------------------------------------------------------------------------------
def _model_restate(mon, opt, t):
    st = mon.store
    h = np.stack([mon._tensors_host["beta1"], mon._tensors_host["beta2"], mon._tensors_host["eps"]], axis=1)
    offsets = [st.offsets[n] for n in mon.names]
    if opt is None:
        return _restate(st.gflat, st.flat, None, None, offsets, mon.numels, h, t)
    return _restate(st.gflat, st.flat, opt.exp_avg, opt.exp_avg_sq, offsets, mon.numels, h, t)


def _nchunks(mon):
    return mon._tensors_host["nchunks"]


def test_placement_cadence_ring_and_bad_slot(dev):
    cfg, model, crit = _model(dev)
    store = model.engine()[0]
    mon = StepMonitor(model, every=3, history=2)
    assert mon.rows() == [] and mon.bad() is None
    gen = torch.Generator(device=dev).manual_seed(3)
    t = torch.zeros(1, dtype=torch.int32, device=dev)
    clip = torch.zeros(2, device=dev)
    tables = {}

    def launch(step, coef=0.25):
        t.fill_(step)
        clip.copy_(torch.tensor([0.5 * step if coef >= 0 else float("nan"), coef]))
        mon._launch(None, None, t, clip)
        torch.cuda.synchronize()

    for step in (1, 3, 4, 6, 9):
        store.gflat.copy_(torch.randn(store.total, device=dev, generator=gen))
        before = mon.mem.clone()
        launch(step)
        if step % 3:
            assert _same_bits(mon.mem, before), "a non-recording launch wrote something (t = %d)" % step
            continue
        rows = mon.rows()
        assert rows[0][:3] == (step, 0.5 * step, 0.25)
        tables[step] = rows[0][3]
        _check_table("placement t=%d" % step, torch.from_numpy(rows[0][3]), _model_restate(mon, None, step), _nchunks(mon), mon.chunk, moments=False)
        slot = (step // 3) % 2
        assert int(mon.row_step[slot]) == step and mon.row_norm[2 * slot:2 * slot + 2].tolist() == [0.5 * step, 0.25]
        assert np.array_equal(mon.ring.view(2, -1, 8)[slot].cpu().numpy().view(np.int32), rows[0][3].view(np.int32))
    rows = mon.rows()
    assert [r[0] for r in rows] == [9, 6]                    # newest first; t = 3 was overwritten by t = 9 (slot 1)
    assert np.array_equal(rows[1][3].view(np.int32), tables[6].view(np.int32))
    assert not np.array_equal(tables[9], tables[6]) and mon.bad() is None
    # a skipped step: the bad slot, once; the ring is not touched
    a, b = mon.names.index("bbox_embed.layers.0.weight"), mon.names.index("query_embed.weight")
    ring = mon.mem[:mon._o_bad].clone()
    store.gflat[store.offsets[mon.names[a]] + 1] = float("nan")
    launch(9, coef=-1.0)
    step, count, table = mon.bad()
    assert (step, count) == (9, 1) and mon.nonfinite_names(table) == [mon.names[a]] and table[a, 2] == 1
    assert _same_bits(mon.mem[mon._o_step:mon._o_bad], ring[mon._o_step:])
    first = table.copy()
    # a second one, another tensor poisoned: only counted
    store.gflat[store.offsets[mon.names[a]] + 1] = 0.5
    store.gflat[store.offsets[mon.names[b]]] = float("inf")
    t.fill_(10)
    launch(10, coef=-1.0)
    step, count, table = mon.bad()
    assert (step, count) == (9, 2) and np.array_equal(table.view(np.int32), first.view(np.int32))
    assert [r[0] for r in mon.rows()] == [9, 6]
    mon.clear_bad()
    assert mon.bad() is None and [r[0] for r in mon.rows()] == [9, 6]
    launch(10, coef=-1.0)
    step, count, table = mon.bad()
    assert (step, count) == (10, 1) and mon.nonfinite_names(table, "grad") == [mon.names[b]] and mon.nonfinite_names(table, "param") == []
    mon.reset()
    assert mon.rows() == [] and mon.bad() is None


# ------------------------------------------------------------------------------------------------------------------------------
# in the step: eager and captured
# ------------------------------------------------------------------------------------------------------------------------------
def test_eager_step_records_the_row_of_its_own_buffers(dev):
    cfg, model, crit = _model(dev)
    opt = build_optimizer(model, cfg)
    mon = StepMonitor(model, every=1, history=2).attach(opt)
    assert opt.monitor is mon and monitor_of(model) is mon and set(mon.groups) == {0, 1, 2, 3}
    train_step(model, crit, opt, *_batch(0, dev), 0.1)
    torch.cuda.synchronize()
    rows = mon.rows()
    assert len(rows) == 1 and rows[0][0] == 1 and mon.bad() is None
    t, norm, coef, table = rows[0]
    assert (norm, coef) == (float(opt.norm_out[0]), float(opt.norm_out[1])) and 0 < coef <= 1
    _check_table("eager step t=1", torch.from_numpy(table), _model_restate(mon, opt, 1), _nchunks(mon), mon.chunk)
    total = math.sqrt(float(table[:, 0].astype(np.float64).sum()))
    print("sqrt(sum col 0) %.9g   norm_out[0] %.9g" % (total, norm))
    assert abs(total - norm) <= 1e-5 * norm                # both are sums of the same squares
    s = mon.summary(rows[0])
    assert list(s) == ["transformer", "backbone", "class_embed", "query_embed", "all"]
    assert abs(s["all"]["grad_norm"] - norm) <= 1e-5 * norm and s["all"]["nonfinite_grads"] == 0
    assert s["backbone"]["update_ratio"] > 0 and s["transformer"]["update_ratio"] > 0
    assert len(mon.worst(rows[0], 3, "update_ratio")) == 3 and mon.worst(rows[0], 1, "grad_absmax")[0][1] == float(table[:, 1].max())


def test_captured_step_records_and_follows_configure_without_a_new_capture(dev):
    cfg, model, crit = _model(dev)
    opt = build_optimizer(model, cfg)
    mon = StepMonitor(model, every=1, history=8).attach(opt)
    step = GraphedTrainStep(model, crit, opt, 0.1)
    for i in range(3):
        step(*_batch(i, dev))
        torch.cuda.synchronize()
        rows = mon.rows()
        # (i == 0: the capture's warm-up passes recorded nothing -- the only row is that of the call itself)
        assert [r[0] for r in rows] == list(range(i + 1, 0, -1)) and mon.bad() is None and opt.t == i + 1
        assert rows[0][1] == float(opt.norm_out[0])
        _check_table("captured step t=%d" % (i + 1), torch.from_numpy(rows[0][3]), _model_restate(mon, opt, i + 1), _nchunks(mon), mon.chunk)
    assert len(step.graphs) == 1
    mon.configure(every=2)
    for i in (3, 4):
        step(*_batch(i, dev))
    torch.cuda.synchronize()
    assert len(step.graphs) == 1 and opt.t == 5
    rows = mon.rows()
    assert [r[0] for r in rows] == [4, 3, 1]                 # t = 4 took slot (4 / 2) % 8 = 2 from t = 2; t = 5 was not recorded
    assert mon.state.tolist() == [2, 8, 0, 0]


def _three_steps(dev, monitored):
    cfg, model, crit = _model(dev)
    opt = build_optimizer(model, cfg)
    step = GraphedTrainStep(model, crit, opt, 0.1)
    plain = step._key((2, 3, 32, 64, 96), 16)
    if monitored:
        mon = StepMonitor(model, every=1, history=2).attach(opt)
        key = step._key((2, 3, 32, 64, 96), 16)
        assert key[:len(plain)] == plain and key[len(plain):] == (("step_monitor", mon.serial),)
    losses = []
    for i in range(3):
        loss, terms = step(*_batch(i, dev))
        losses += [loss.detach().clone()] + [terms[k].detach().clone() for k in sorted(terms) if torch.is_tensor(terms[k])]
    torch.cuda.synchronize()
    store = model.engine()[0]
    out = [store.flat.detach().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.t_dev.clone()] + losses
    if monitored:
        assert len(mon.rows()) == 2
        mon.detach()
        assert step._key((2, 3, 32, 64, 96), 16) == plain and opt.monitor is None
    return out


def test_the_monitor_only_reads(dev):
    a, b = _three_steps(dev, False), _three_steps(dev, True)
    assert len(a) == len(b) and len(a) > 10
    assert all(_same_bits(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------------------
# a non-finite step
# ------------------------------------------------------------------------------------------------------------------------------
def test_non_finite_step_fills_the_bad_slot(dev):
    cfg, model, crit = _model(dev)
    opt = build_optimizer(model, cfg)
    store = model.engine()[0]
    mon = StepMonitor(model, every=1, history=2).attach(opt)
    train_step(model, crit, opt, *_batch(0, dev), 0.1)
    c, t = _batch(1, dev)
    loss = crit.weighted_total(crit(model(c), t), crit.weight_dict)
    store.zero_grad()
    loss.backward()
    a, b = "class_embed_b.weight", "query_embed.weight"
    store.gflat[store.offsets[a] + 3] = float("nan")        # values planted in memory: the optimizer's existing skip path
    store.gflat[store.offsets[b] + 7] = float("inf")
    torch.cuda.synchronize()
    flat = store.flat.detach().clone()
    opt.step(max_norm=0.1)
    torch.cuda.synchronize()
    assert float(opt.norm_out[1]) == -1.0 and _same_bits(store.flat, flat) and opt.t == 1
    step, count, table = mon.bad()
    assert (step, count) == (opt.t, 1)
    assert sorted(mon.nonfinite_names(table)) == sorted([a, b]) and mon.nonfinite_names(table, "param") == []
    assert table[mon.names.index(a), 2] == 1 and table[mon.names.index(b), 2] == 1
    assert [r[0] for r in mon.rows()] == [1]                 # the ring still holds the good step only


# ------------------------------------------------------------------------------------------------------------------------------
# the training loop
# ------------------------------------------------------------------------------------------------------------------------------
class _Writer:
    def __init__(self):
        self.scalars = []

    def add_scalar(self, tag, value, it):
        self.scalars.append((tag, float(value), it))


TRAIN_TAGS = ["train/class_error", "train/totall_loss", "train/loss_bbox", "train/loss_giou", "train/loss_ce", "train/loss_ce_b"]


def test_training_loop_writes_the_monitor_tags_and_names_a_nan_parameter(dev, tmp_path):
    cfg, model, crit = _model(dev)
    M = cfg.CONFIG.TRAIN.MONITOR
    M.ENABLE, M.EVERY = True, 1
    cfg.DDP_CONFIG.GPU_WORLD_RANK = 0
    opt = build_optimizer(model, cfg)
    loader = [_batch(i, dev) for i in range(3)]
    w = _Writer()
    assert monitor_of(model) is None
    train_tuber_detection(cfg, model, crit, loader, opt, 0, 0.1, writer=w, print_freq=1)
    torch.cuda.synchronize()
    mon = monitor_of(model)
    assert mon is not None and opt.monitor is mon and mon.settings() == dict(every=1, history=8) and mon.bad() is None
    keys = [key for step in model.__dict__["_tuber_graphed"].values() for key in step.graphs]
    assert len(keys) == 1 and ("step_monitor", mon.serial) in keys[0][5:]          # the loop ran the captured step, the monitor inside it
    tags = {}
    for tag, value, it in w.scalars:
        tags.setdefault(tag, []).append(value)
    for kind in ("grad_norm", "param_norm", "update_ratio"):
        for group in ("transformer", "backbone", "class_embed", "query_embed"):
            vals = tags["monitor/%s/%s" % (kind, group)]
            assert len(vals) == 3 and all(math.isfinite(x) and x > 0 for x in vals), (kind, group, vals)
    assert len(tags["monitor/zero_grad_fraction"]) == 3 and all(0 <= x < 1 for x in tags["monitor/zero_grad_fraction"])
    assert sorted(t for t in tags if t.startswith("train/")) == sorted(TRAIN_TAGS)
    assert len(tags) == len(TRAIN_TAGS) + 13
    # the same loop with a NaN planted in one bbox_embed bias before the epoch
    name = "bbox_embed.layers.2.bias"
    assert name in mon.names
    with torch.no_grad():
        dict(model.named_parameters())[name][1] = float("nan")
    with pytest.raises(FloatingPointError) as info:
        train_tuber_detection(cfg, model, crit, loader, opt, 0, 0.1, writer=_Writer(), print_freq=1)
    text = str(info.value)
    print(text)
    assert "non-finite parameter" in text and name in text.split("non-finite parameter")[1].split("]")[0]


def test_training_loop_without_the_monitor_writes_todays_six_tags(dev):
    cfg, model, crit = _model(dev)
    assert cfg.CONFIG.TRAIN.MONITOR.ENABLE is False
    cfg.DDP_CONFIG.GPU_WORLD_RANK = 0
    opt = build_optimizer(model, cfg)
    w = _Writer()
    train_tuber_detection(cfg, model, crit, [_batch(i, dev) for i in range(3)], opt, 0, 0.1, writer=w, print_freq=1)
    torch.cuda.synchronize()
    assert monitor_of(model) is None and opt.monitor is None
    assert [t for t, _, _ in w.scalars] == TRAIN_TAGS * 3
    keys = [key for step in model.__dict__["_tuber_graphed"].values() for key in step.graphs]
    assert len(keys) == 1 and not any(isinstance(e, tuple) and e[:1] == ("step_monitor",) for e in keys[0][5:])
