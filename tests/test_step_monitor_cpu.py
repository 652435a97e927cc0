"""Host side of the step monitor (monitor.py): the chunk table against a brute-force loop, settings and config validation, and the readers
``summarize`` / ``worst_tensors`` / ``nonfinite_tensors`` on a hand-made table with known answers.  No GPU."""
import os

import numpy as np
import pytest

from tubelet_transformer_amd import monitor
from tubelet_transformer_amd.config import load_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg():
    return load_cfg(os.path.join(ROOT, "configuration", "TubeR_CSN152_AVA21.yaml"))


@pytest.mark.parametrize("chunk", [64, 256, 8192])
def test_chunk_table_tiles_every_tensor_exactly_once(chunk):
    numels = [1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 3 * chunk + 5]
    offsets, off = [], 0
    for n in numels:
        offsets.append(off)
        off += (n + 63) // 64 * 64
    table = monitor.chunk_table(offsets, numels, chunk)
    assert table.dtype == monitor.CHUNK and table.dtype.itemsize == 16
    # brute force: mark every element of the flat layout with the chunk that covers it
    owner = np.full(off, -1, dtype=np.int64)
    for c, (o, n, ti) in enumerate(table.tolist()):
        assert 1 <= n <= chunk
        assert offsets[ti] <= o and o + n <= offsets[ti] + numels[ti], "chunk %d crosses tensor %d" % (c, ti)
        assert (o - offsets[ti]) % chunk == 0
        assert (owner[o:o + n] == -1).all(), "chunk %d overlaps another" % c
        owner[o:o + n] = c
    for ti, (o, n) in enumerate(zip(offsets, numels)):
        assert (owner[o:o + n] >= 0).all(), "tensor %d is not covered" % ti
        assert (owner[o + n:o + (n + 63) // 64 * 64] == -1).all(), "the padding behind tensor %d is covered" % ti
        mine = [c for c, row in enumerate(table.tolist()) if row[2] == ti]
        assert len(mine) == -(-n // chunk) and mine == list(range(mine[0], mine[0] + len(mine)))      # ceil(n / chunk), contiguous, in order
    assert table["tensor"].tolist() == sorted(table["tensor"].tolist())


def test_chunk_table_edge_cases():
    assert len(monitor.chunk_table([], [], 64)) == 0
    assert len(monitor.chunk_table([0, 64], [0, 5], 64)) == 1          # an empty tensor gets no chunk
    with pytest.raises(ValueError):
        monitor.chunk_table([0], [5], 0)


@pytest.mark.parametrize("every, history, key", [(0, 8, "EVERY"), (-3, 8, "EVERY"), (2.5, 8, "EVERY"), (True, 8, "EVERY"), ("4", 8, "EVERY"),
                                                 (50, 0, "HISTORY"), (50, -1, "HISTORY"), (50, 1.0, "HISTORY"), (50, False, "HISTORY")])
def test_settings_validation_names_the_key(every, history, key):
    with pytest.raises(ValueError, match=key):
        monitor.check_settings(every, history)
    cfg = _cfg()
    cfg.CONFIG.TRAIN.MONITOR.EVERY, cfg.CONFIG.TRAIN.MONITOR.HISTORY = every, history
    with pytest.raises(ValueError, match=r"CONFIG\.TRAIN\.MONITOR\.%s" % key):
        monitor.monitor_settings(cfg)


def test_config_defaults_and_enable_validation():
    cfg = _cfg()
    M = cfg.CONFIG.TRAIN.MONITOR
    assert (M.ENABLE, M.EVERY, M.HISTORY) == (False, 50, 8)
    assert monitor.monitor_settings(cfg) == dict(enable=False, every=50, history=8)
    assert monitor.check_settings(1, 1) == (1, 1)
    assert monitor.monitor_for(cfg, object(), object()) is None          # off: nothing is built, the model is not touched
    M.ENABLE = 1
    with pytest.raises(ValueError, match=r"CONFIG\.TRAIN\.MONITOR\.ENABLE"):
        monitor.monitor_settings(cfg)


def test_group_names():
    assert monitor.group_names(4) == ["transformer", "backbone", "class_embed", "query_embed"]
    assert monitor.group_names(2) == ["group0", "group1"]


# a hand-made table: 5 tensors, groups 0 0 1 1 none
NAMES = ["a.weight", "a.bias", "b.weight", "b.bias", "frozen.weight"]
NUMELS = [10, 2, 20, 4, 8]
GROUPS = [0, 0, 1, 1, -1]
LRS = [0.5, 0.25]
#         sum g^2  max|g|  nf g  zero g  sum p^2  max|p|  nf p  sum u^2
TABLE = [[9.0,     2.0,    0,    1,      16.0,    3.0,    0,    4.0],
         [16.0,    4.0,    0,    0,      9.0,     2.5,    0,    12.0],
         [144.0,   7.0,    2,    5,      64.0,    6.0,    0,    1.0],
         [0.0,     0.0,    0,    4,      36.0,    5.0,    1,    0.0],
         [0.0,     0.0,    0,    8,      25.0,    4.0,    0,    0.0]]


def test_summary_on_a_hand_made_table():
    s = monitor.summarize(TABLE, NUMELS, GROUPS, LRS, names=["g0", "g1"])
    assert list(s) == ["g0", "g1", "all"]
    assert s["g0"] == {"grad_norm": 5.0, "param_norm": 5.0, "update_ratio": 0.5 * 4.0 / 5.0, "nonfinite_grads": 0, "nonfinite_params": 0,
                       "zero_grad_fraction": 1 / 12}
    assert s["g1"] == {"grad_norm": 12.0, "param_norm": 10.0, "update_ratio": 0.25 * 1.0 / 10.0, "nonfinite_grads": 2, "nonfinite_params": 1,
                       "zero_grad_fraction": 9 / 24}
    a = s["all"]
    assert a["grad_norm"] == 13.0 and a["param_norm"] == np.sqrt(150.0)
    assert a["update_ratio"] == pytest.approx(np.sqrt((0.5 * 4.0) ** 2 + (0.25 * 1.0) ** 2) / np.sqrt(150.0), rel=1e-15)
    assert (a["nonfinite_grads"], a["nonfinite_params"], a["zero_grad_fraction"]) == (2, 1, 18 / 44)
    assert list(monitor.summarize(TABLE, NUMELS, GROUPS, LRS)) == ["group0", "group1", "all"]
    zero = monitor.summarize(np.zeros((5, 8)), NUMELS, GROUPS, LRS)["all"]
    assert zero["update_ratio"] == 0.0 and zero["grad_norm"] == 0.0      # no parameters yet: no division by zero


def test_worst_on_a_hand_made_table():
    assert monitor.worst_tensors(TABLE, NAMES, 2, "grad_sumsq") == [("b.weight", 144.0), ("a.bias", 16.0)]
    assert monitor.worst_tensors(TABLE, NAMES, 1, 5) == [("b.weight", 6.0)]
    assert monitor.worst_tensors(TABLE, NAMES, 9, "grad_zeros")[0] == ("frozen.weight", 8.0)
    got = monitor.worst_tensors(TABLE, NAMES, 3, "update_ratio", GROUPS, LRS)
    want = [("a.bias", 0.5 * np.sqrt(12.0) / 3.0), ("a.weight", 0.5 * 2.0 / 4.0), ("b.weight", 0.25 * 1.0 / 8.0)]
    assert [n for n, _ in got] == [n for n, _ in want]
    assert [v for _, v in got] == pytest.approx([v for _, v in want], rel=1e-15)
    assert monitor.worst_tensors(TABLE, NAMES, 0, "grad_sumsq") == []


def test_nonfinite_names_on_a_hand_made_table():
    assert monitor.nonfinite_tensors(TABLE, NAMES) == ["b.weight", "b.bias"]
    assert monitor.nonfinite_tensors(TABLE, NAMES, "grad") == ["b.weight"]
    assert monitor.nonfinite_tensors(TABLE, NAMES, "param") == ["b.bias"]
    assert monitor.nonfinite_tensors(np.zeros((5, 8)), NAMES) == []
