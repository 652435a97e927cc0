"""BatchNorm momentum and the precise-BN pass without a GPU: ``bn_stats.recompute_bn_stats`` on a stub model (stock nn.BatchNorm1d on the
CPU: argument handling, loader item forms, the batch limit, momentum / train-mode restore, the average over two gloo ranks), the graph-key
helper of the captured step, and the C-ABI exports of the momentum kernels."""
import importlib.util
import os
import subprocess
import sys

import pytest
import torch
from torch import nn

from tubelet_transformer_amd import lib
from tubelet_transformer_amd.bn_stats import recompute_bn_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Stub(nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(3, 4)
        self.bn = nn.BatchNorm1d(4, momentum=0.3)
        self.head = nn.Sequential(nn.ReLU(), nn.BatchNorm1d(4))
        self.seen = []
        self.fail_at = None

    def forward(self, x):
        if self.fail_at is not None and len(self.seen) == self.fail_at:
            raise RuntimeError("boom")
        self.seen.append(x)
        return self.head(self.bn(self.lin(x)))


class _Moved:
    """a loader item with ``.to(device)`` (what input_pipeline.ClipBatch offers)"""

    def __init__(self, x, log):
        self.x, self.log = x, log

    def to(self, device):
        self.log.append(torch.device(device))
        return self.x


def _batches(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(6, 3, generator=g) * (1 + i) + i for i in range(n)]


def _cumulative(model, batches):
    """per layer: the arithmetic mean of the per-batch (mean, unbiased var), from the stock modules at momentum 1.0"""
    ref = _Stub()
    ref.load_state_dict(model.state_dict())
    ref.train()
    stats = {"bn": [], "head.1": []}
    with torch.no_grad():
        for x in batches:
            for name in stats:
                ref.get_submodule(name).momentum = 1.0
            ref(x)
            for name in stats:
                m = ref.get_submodule(name)
                stats[name].append((m.running_mean.clone(), m.running_var.clone()))
    return {k: (torch.stack([a for a, _ in v]).mean(0), torch.stack([b for _, b in v]).mean(0)) for k, v in stats.items()}


def test_cumulative_average_over_the_first_batches_and_state_restored():
    torch.manual_seed(0)
    model = _Stub().eval()
    model.head.train()                                        # a mixed train / eval state comes back as it was
    batches = _batches(5)
    want = _cumulative(model, batches[:3])
    w0 = {k: v.clone() for k, v in model.named_parameters()}
    pulled = []

    def loader():
        for i, x in enumerate(batches):
            pulled.append(i)
            yield (x, {"boxes": None}, "extra")               # (samples, targets, ...) of the training loader
    n = recompute_bn_stats(model, loader(), num_batches=3)
    assert n == 3 and pulled == [0, 1, 2]                     # stops after num_batches without drawing another item
    assert len(model.seen) == 3
    for name, (mean, var) in want.items():
        m = model.get_submodule(name)
        assert torch.allclose(m.running_mean, mean, rtol=1e-5, atol=1e-6)
        assert torch.allclose(m.running_var, var, rtol=1e-5, atol=1e-6)
        assert int(m.num_batches_tracked) == 3
    assert model.bn.momentum == 0.3 and model.head[1].momentum == 0.1
    assert not model.training and not model.bn.training and model.head.training and model.head[1].training
    for k, v in model.named_parameters():
        assert torch.equal(v, w0[k]) and v.grad is None


def test_item_forms_and_the_whole_loader():
    model = _Stub()
    batches = _batches(4, seed=1)
    log = []
    items = [batches[0], _Moved(batches[1], log), [batches[2], None], (batches[3],)]
    assert recompute_bn_stats(model, items, num_batches=None, device="cpu") == 4
    assert log == [torch.device("cpu")]                       # moved with .to(device), like the training loop does
    assert all(torch.equal(a, b) for a, b in zip(model.seen, batches))
    want = _cumulative(model, batches)
    assert torch.allclose(model.bn.running_mean, want["bn"][0], rtol=1e-5, atol=1e-6)
    assert recompute_bn_stats(model, batches, num_batches=200) == 4          # a short loader ends the pass


@pytest.mark.parametrize("bad", [0, -1, 2.5, True, "3"])
def test_num_batches_is_validated(bad):
    with pytest.raises((ValueError, TypeError)):
        recompute_bn_stats(_Stub(), _batches(2), num_batches=bad)


def test_restores_momentum_and_mode_when_a_forward_raises():
    model = _Stub().eval()
    model.fail_at = 1
    with pytest.raises(RuntimeError, match="boom"):
        recompute_bn_stats(model, _batches(3))
    assert model.bn.momentum == 0.3 and model.head[1].momentum == 0.1
    assert not any(m.training for m in model.modules())


def test_model_without_batchnorm_is_left_alone():
    model = nn.Linear(3, 3)
    pulled = []

    def loader():
        pulled.append(1)
        yield torch.zeros(2, 3)
    assert recompute_bn_stats(model, loader()) == 0 and pulled == []


_WORKER = r"""
import os, sys, torch, torch.distributed as dist
root, port, rank, out = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
sys.path.insert(0, root)
from tubelet_transformer_amd.bn_stats import recompute_bn_stats
torch.manual_seed(0)
model = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.BatchNorm1d(4))
g = torch.Generator().manual_seed(10 + rank)
batches = [torch.randn(5, 3, generator=g) * (1 + rank) for _ in range(2 + rank)]    # rank 1 has one batch more
local = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.BatchNorm1d(4))
local.load_state_dict(model.state_dict())
recompute_bn_stats(local, batches)
os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", port
dist.init_process_group("gloo", rank=rank, world_size=2)
n = recompute_bn_stats(model, batches)
bn, lb = model[1], local[1]
torch.save({"n": n, "mean": bn.running_mean, "var": bn.running_var, "nbt": int(bn.num_batches_tracked),
            "local_mean": lb.running_mean, "local_var": lb.running_var, "momentum": bn.momentum}, out + ".%d" % rank)
dist.barrier()
dist.destroy_process_group()
"""


def test_world2_gloo_ranks_end_with_the_mean_of_their_averages(tmp_path):
    script = str(tmp_path / "w2.py")
    open(script, "w").write(_WORKER)
    port = str(29700 + os.getpid() % 150)
    out = str(tmp_path / "res")
    procs = [subprocess.Popen([sys.executable, script, ROOT, port, str(r), out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    logs = [p.communicate(timeout=300)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-3000:] for l in logs)
    res = [torch.load(out + ".%d" % r) for r in range(2)]
    want_mean = (res[0]["local_mean"] + res[1]["local_mean"]) / 2
    want_var = (res[0]["local_var"] + res[1]["local_var"]) / 2
    for r in res:
        assert torch.equal(r["mean"], res[0]["mean"]) and torch.equal(r["var"], res[0]["var"])
        assert torch.allclose(r["mean"], want_mean, rtol=1e-6, atol=1e-7) and torch.allclose(r["var"], want_var, rtol=1e-6, atol=1e-7)
        assert r["nbt"] == 3 and r["momentum"] == 0.1          # the same integer count on every rank (the larger local one)
    assert [r["n"] for r in res] == [2, 3]


def test_graph_key_momentum_part():
    from tubelet_transformer_amd.training import _momenta
    base = ((2, 3, 32, 64, 96), (), True, 16, False)
    assert _momenta(base) == () and _momenta(base + ("last",)) == ()            # default momenta: the key keeps its five entries
    sig = ((0, None), (7, 0.3))
    assert _momenta(base + (sig,)) == sig and _momenta(base + (sig, "first")) == sig


def test_header_declares_the_momentum_exports():
    protos = {name: args for _, name, args in lib.header_prototypes()}
    for old in ("tuber_bn_finalize", "tuber_dwconv_tile_fwd_bn"):
        # the new form takes the old argument list (momentum < 0: cumulative); the old export keeps its signature
        assert [t for t, _ in protos[old + "_ex"]] == [t for t, _ in protos[old]]
        assert protos[old][10] == ("float", "momentum") and protos[old][9] == ("long long*", "num_batches_tracked" if old == "tuber_bn_finalize" else "nbt")
    assert [t for t, _ in protos["tuber_bn_count_advance"]] == ["const long*", "int", "hipStream_t"]
    spec = importlib.util.spec_from_file_location("gen_header", os.path.join(ROOT, "tubelet_transformer_amd", "csrc", "gen_header.py"))
    gh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gh)
    defined = {n: f for f, _, n, _ in gh.prototypes()}
    assert defined["tuber_bn_finalize_ex"] == defined["tuber_bn_count_advance"] == "norm.hip"
    assert defined["tuber_dwconv_tile_fwd_bn_ex"] == "dwconv_tile.hip"
    for name in ("tuber_bn_finalize_ex", "tuber_dwconv_tile_fwd_bn_ex"):
        assert "ir_CSN_152.py" in gh.DOC[name]                                 # the reference op it replaces
    assert "_BatchNorm.forward" in gh.DOC["tuber_bn_count_advance"]
