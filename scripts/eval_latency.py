"""Eval forward latency of the three eval forms (round 6), BASELINE config 3 at its stated size (TubeR_CSN152_AVA21, 2 clips of 3x32x256x340),
eager launches and a captured hipGraph replay:
    default                      eval precision mode: fp32 residual streams + fp32 decoder / box / actor heads (csrc/eval_f32.hip)
    TUBER_EVAL_PRECISION=fp32_class   the same + the class branch once per clip in fp32 (round 7)
    TUBER_AB=eval_bf16_decoder   fp32 residual streams only
    TUBER_AB=eval_bf16_stream    the training path's rounding points (bf16-stored streams, bf16 MFMA decoder, cooperative decoder launch)
EVAL_ROUNDS=n (default 1) repeats the modes n times, alternating them, with one captured graph per mode: same-box interleaved pairs.
usage: python scripts/eval_latency.py [config.yaml H W]"""
import contextlib
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tubelet_transformer_amd import ab, synth                      # noqa: E402
from tubelet_transformer_amd.config import load_cfg               # noqa: E402
from tubelet_transformer_amd.tuber import build_model             # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "TubeR_CSN152_AVA21.yaml"
H, W = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (256, 340)
dev = torch.device("cuda:0")
cfg = load_cfg(os.path.join(ROOT, "configuration", name))
model, _, _ = build_model(cfg)
synth.load_name_hashed(model)
model.to(dev).eval()
clips = synth.synthetic_clips(2, 32, H, W, seed=1, device=dev)


def timed(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


MODES = (("eval precision mode (default)", (), None), ("fp32 streams only (eval_bf16_decoder)", ("eval_bf16_decoder",), None),
         ("bf16 streams (eval_bf16_stream)", ("eval_bf16_stream",), None), ("class branch in fp32 (fp32_class)", (), "fp32_class"))
if os.environ.get("EVAL_MODES"):                                    # e.g. EVAL_MODES=0 under rocprofv3: the default mode only
    MODES = tuple(MODES[int(i)] for i in os.environ["EVAL_MODES"].split(","))


@contextlib.contextmanager
def mode(sw, precision):
    old = os.environ.pop("TUBER_EVAL_PRECISION", None)
    if precision:
        os.environ["TUBER_EVAL_PRECISION"] = precision
    try:
        with ab.override(*sw), torch.no_grad():
            yield
    finally:
        os.environ.pop("TUBER_EVAL_PRECISION", None)
        if old is not None:
            os.environ["TUBER_EVAL_PRECISION"] = old


graphs = {}
for rnd in range(int(os.environ.get("EVAL_ROUNDS", "1"))):
    for label, sw, precision in MODES:
        with mode(sw, precision):
            eager = timed(lambda: model(clips))
            if label not in graphs:
                g = torch.cuda.CUDAGraph()
                model(clips)
                torch.cuda.synchronize()
                with torch.cuda.graph(g):
                    model(clips)
                graphs[label] = g
            graph = timed(graphs[label].replay)
        print("%-44s eager %7.3f ms   hipGraph replay %7.3f ms per 2-clip batch = %.3f ms per clip, %.1f clips/s" % (label, eager, graph, graph / 2, 2e3 / graph), flush=True)
