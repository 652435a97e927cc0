"""Host-side decisions of the GEMM launchers (no GPU): the library reproduces tests/golden/gemm_plan.json, recorded by
scripts/gemm_plan_golden.py through the older queries, and tuber_gemm_nt_plan -- the decision the launchers themselves take --
agrees with those queries and with the forms the comments in gemm.hip promise for the model's shapes."""
import itertools
import json
import os

import pytest

from tubelet_transformer_amd import lib

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plan.json")))
GRID = GOLDEN["grid"]
SHAPES = [list(s) for s in itertools.product(GRID["M"], GRID["N"], GRID["K"])] + GRID["extra"]
ROWS_SHAPES = list(dict.fromkeys((M, N) for M, N, _ in SHAPES))
STATES = {"default": None, "nt96_off": ("tuber_gemm_nt_96_set", 0, 1), "wsk96_off": ("tuber_gemm_nt_wsk96_set", 0, 1),
          "cfg0": ("tuber_gemm_nt_set_cfg", 0, -1), "cfg7": ("tuber_gemm_nt_set_cfg", 7, -1), "cfg13": ("tuber_gemm_nt_set_cfg", 13, -1),
          "cfg23": ("tuber_gemm_nt_set_cfg", 23, -1)}
TILE, WSK, R96 = 0, 1, 2            # forms of tuber_gemm_nt_plan
PLAIN, STATS, JOIN_DS, EVAL, JOIN_DS_M = 0, 1, 5, 6, 9


class hook:
    """one of the tile hooks held for a block, then put back to its default"""
    def __init__(self, state):
        self.h = STATES[state]

    def __enter__(self):
        if self.h:
            lib.query(self.h[0], self.h[1])

    def __exit__(self, *a):
        if self.h:
            lib.query(self.h[0], self.h[2])


def plan(M, N, K, amode=0, epi=0, gather=0, out_f32=0, aligned=1):
    """(form, tile rows, tile columns), or None where the launchers refuse"""
    v = lib.query("tuber_gemm_nt_plan", M, N, K, amode, epi, gather, out_f32, aligned)
    return None if v < 0 else (v // 1000000, v // 1000 % 1000, v % 1000)


def test_golden_grid_is_the_recorded_one():
    assert set(GOLDEN["nt"]) == set(STATES) and len(SHAPES) == len(GOLDEN["tn"]["tile"]) >= 936
    assert len(GRID["M"]) == 13 and len(GRID["N"]) == 9 and len(GRID["K"]) == 8


@pytest.mark.parametrize("state", list(STATES))
def test_gemm_nt_queries_reproduce_the_golden_file(state):
    want = GOLDEN["nt"][state]
    with hook(state):
        got = {"cfg": [lib.query("tuber_gemm_nt_cfg", *s) for s in SHAPES],
               "stat_rows": [lib.query("tuber_gemm_nt_stat_rows", M, N) for M, N in ROWS_SHAPES],
               "wsk_tile_rows": [lib.query("tuber_gemm_nt_wsk_tile_rows", *s) for s in SHAPES]}
    for key in want:
        bad = [(s, g, w) for s, g, w in zip(ROWS_SHAPES if key == "stat_rows" else SHAPES, got[key], want[key]) if g != w]
        assert len(got[key]) == len(want[key]) and not bad, "%s under %s: (shape, got, recorded) %s" % (key, state, bad[:5])


def test_gemm_tn_queries_reproduce_the_golden_file():
    up8 = lambda v: (v + 7) // 8 * 8
    got = {"tile": [lib.query("tuber_gemm_tn_tile", *s) for s in SHAPES],
           "slabs": [lib.query("tuber_gemm_tn_slabs", *s) for s in SHAPES],
           "fuses_bias": [lib.query("tuber_gemm_tn_fuses_bias", M, N, K, N, K) for M, N, K in SHAPES],
           "fuses_bias_ld8": [lib.query("tuber_gemm_tn_fuses_bias", M, N, K, up8(N), up8(K)) for M, N, K in SHAPES]}
    for key, want in GOLDEN["tn"].items():
        bad = [(s, g, w) for s, g, w in zip(SHAPES, got[key], want) if g != w]
        assert len(got[key]) == len(want) and not bad, "%s: (shape, got, recorded) %s" % (key, bad[:5])


@pytest.mark.parametrize("state", list(STATES))
def test_plan_agrees_with_the_statistics_and_split_k_queries(state):
    """the statistics epilogue on plain A: the rows tuber_gemm_nt_stat_rows sizes are one per 64 output rows whenever the plan's tiles are
    64 or 96 rows tall (the 96-row forms write that layout) and one per 128 under a forced cfg 0; the plan is the wave-split-K form, at 64
    or 96 rows, exactly where tuber_gemm_nt_wsk_tile_rows says so"""
    with hook(state):
        for M, N, K in SHAPES:
            form, bm, bn = plan(M, N, K, epi=STATS)
            assert bm == 128 if state == "cfg0" else bm in (64, 96), (M, N, K, form, bm, bn)
            assert lib.query("tuber_gemm_nt_stat_rows", M, N) == -(-M // (128 if bm == 128 else 64)), (M, N, K, bm)
            assert lib.query("tuber_gemm_nt_wsk_tile_rows", M, N, K) == (bm if form == WSK else 0), (M, N, K, form, bm)
            assert form != WSK or bn == 64


def test_plan_of_the_named_model_shapes():
    # layer3 / layer4 long-K convs: wave split-K on 96-row tiles, with every epilogue those convs use
    for epi in (PLAIN, STATS, 2):
        assert plan(5632, 256, 1024, epi=epi) == (WSK, 96, 64)
        assert plan(2816, 512, 2048, epi=epi) == (WSK, 96, 64)
    # layer2's conv1 forward / conv4 data gradient: 96 x 64 on the regular pipeline
    assert plan(44032, 128, 512) == (R96, 96, 64)
    # the class-branch FFN (16 896 x 2048 x 512): 128 x 128 is the shared-tile choice for the plain epilogue, 64 x 128 with statistics
    # rows (one per 64 output rows) -- what is launched whenever the 96-row kernel cannot take the problem (BatchNorm prologue, an output
    # no 16-byte store can address) or is switched off; the aligned plain-A problem itself runs on 96 x 64 tiles since round 6
    assert plan(16896, 2048, 512, amode=1) == (TILE, 128, 128) and plan(16896, 2048, 512, amode=1, epi=STATS) == (TILE, 64, 128)
    assert plan(16896, 2048, 512, aligned=0) == (TILE, 128, 128) and plan(16896, 2048, 512, epi=STATS, aligned=0) == (TILE, 64, 128)
    assert plan(16896, 2048, 512) == (R96, 96, 64) and plan(16896, 2048, 512, epi=STATS) == (R96, 96, 64)
    with hook("nt96_off"):
        assert plan(16896, 2048, 512) == (TILE, 128, 128) and plan(16896, 2048, 512, epi=STATS) == (TILE, 64, 128)
        assert plan(44032, 128, 512) == (TILE, 64, 64)
    # three side operands spill the 64 x 128 tile: the DS joins of a cfg-7 shape run on 64 x 64
    assert lib.query("tuber_gemm_nt_cfg", 5632, 1024, 256) == 7
    assert plan(5632, 1024, 256, epi=3) == (TILE, 64, 128)
    assert plan(5632, 1024, 256, epi=JOIN_DS) == (TILE, 64, 64) and plan(5632, 1024, 256, epi=JOIN_DS_M) == (TILE, 64, 64)
    # the eval output epilogue: BatchNorm + ReLU prologue and full tiles only
    assert plan(5632, 1024, 256, amode=1, epi=EVAL) == (TILE, 64, 128)
    assert plan(5632, 1024, 256, amode=1, epi=EVAL, aligned=0) is None and plan(5632, 1024, 256, amode=0, epi=EVAL) is None
    # a forced cfg 23 is the regular 96-row form where that is built (plain A, full tiles) and cfg 13 elsewhere
    with hook("cfg23"):
        assert plan(700, 128, 192) == (R96, 96, 64) and plan(700, 130, 192) == (TILE, 64, 64) and plan(700, 128, 192, amode=1) == (TILE, 64, 64)
    assert plan(700, 128, 192) == (TILE, 64, 64)
