"""Record the host-side decisions of the GEMM launchers into tests/golden/gemm_plan.json.

The file pins what tuber_gemm_nt / tuber_gemm_tn DECIDE (tile configuration, statistics rows, wave-split-K tile rows under every
tile hook; weight-gradient tile edge, slab count, bias fusion) for a grid of shapes, through the host-only queries of the library.
tests/test_gemm_plan_cpu.py compares a build with it, so a change of the launchers' host code that moves a decision shows without a
GPU.  Re-record only when a decision is MEANT to change:  python scripts/gemm_plan_golden.py
"""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "gemm_plan.json")

# the grid (M x N x K) and, behind it, the GEMM shapes tests/test_cpu.py and tests/test_kernels_gpu.py name that the grid does not hold
GRID = {
    "M": [30, 64, 130, 700, 704, 1100, 2048, 2816, 5632, 8192, 16896, 44032, 348160],
    "N": [4, 64, 80, 128, 130, 256, 512, 1024, 2048],
    "K": [64, 128, 192, 256, 512, 1024, 1088, 2048],
    "extra": [[70000, 64, 64], [40000, 128, 256], [704, 768, 256], [300, 80, 256], [1000, 2048, 512], [44032, 512, 128], [70000, 64, 256],
              [40000, 128, 512], [5000, 256, 64], [3000, 64, 128], [704, 256, 2048], [30, 256, 2048], [700, 130, 1088], [64, 64, 1024],
              [20000, 64, 256], [5000, 256, 1024], [900, 2048, 256], [70000, 256, 64], [5000, 64, 448], [999, 80, 256], [348160, 64, 256],
              [348160, 256, 64], [16896, 256, 256], [87040, 128, 512], [1100, 1024, 1024], [8192, 64, 64]],
}
# hook states the three gemm_nt queries are recorded under: (name, setter, value, value that restores the default)
STATES = [("default", None, None, None), ("nt96_off", "tuber_gemm_nt_96_set", 0, 1), ("wsk96_off", "tuber_gemm_nt_wsk96_set", 0, 1)] + \
         [("cfg%d" % c, "tuber_gemm_nt_set_cfg", c, -1) for c in (0, 7, 13, 23)]


def shapes(grid):
    return [list(s) for s in itertools.product(grid["M"], grid["N"], grid["K"])] + [list(s) for s in grid["extra"]]


def rows_shapes(grid):
    """the (M, N) pairs of shapes(), each once, in order of first appearance (tuber_gemm_nt_stat_rows takes no K)"""
    return list(dict.fromkeys((M, N) for M, N, _ in shapes(grid)))


def record(query, grid):
    sh, mn = shapes(grid), rows_shapes(grid)
    nt = {}
    for name, setter, value, restore in STATES:
        if setter:
            query(setter, value)
        try:
            nt[name] = {"cfg": [query("tuber_gemm_nt_cfg", *s) for s in sh],
                        "stat_rows": [query("tuber_gemm_nt_stat_rows", M, N) for M, N in mn],
                        "wsk_tile_rows": [query("tuber_gemm_nt_wsk_tile_rows", *s) for s in sh]}
        finally:
            if setter:
                query(setter, restore)
    up8 = lambda v: (v + 7) // 8 * 8
    tn = {"tile": [query("tuber_gemm_tn_tile", *s) for s in sh],
          "slabs": [query("tuber_gemm_tn_slabs", *s) for s in sh],
          "fuses_bias": [query("tuber_gemm_tn_fuses_bias", M, N, K, N, K) for M, N, K in sh],
          "fuses_bias_ld8": [query("tuber_gemm_tn_fuses_bias", M, N, K, up8(N), up8(K)) for M, N, K in sh]}
    return {"grid": grid, "nt": nt, "tn": tn}


if __name__ == "__main__":
    from tubelet_transformer_amd import lib
    for env in ("TUBER_NT_WSK96", "TUBER_NT_96"):
        assert not os.environ.get(env), "%s is set: the default state would not be the default" % env
    doc = record(lib.query, GRID)
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s: %d shapes, %d bytes" % (OUT, len(shapes(GRID)), os.path.getsize(OUT)))
