"""tuber_linear_f32 (csrc/eval_f32.hip) at the class branch's shapes under TUBER_EVAL_PRECISION=fp32_class (round 7): rows R0 = B * T' * hw of
config 3 (2 x 1 408) and config 5 (2 x 1 728), plus the cross-attention / class_fc rows (6 x 2 x 15).  Times each launch with HIP events over
n back-to-back launches and prints the achieved fp32 rate against the 157 TF peak of v_mfma_f32_*_f32 (MI355X_MICROARCH.md).
usage: python scripts/linear_f32_microbench.py [n]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tubelet_transformer_amd import lib                               # noqa: E402

PEAK_TF = 157.0
SHAPES = [("class_proj", 2048, 256), ("t/s in_proj", 256, 768), ("t/s out_proj", 256, 256), ("linear1 (ReLU)", 512, 2048),
          ("linear2", 2048, 256), ("cross K/V", 256, 512)]
n = int(sys.argv[1]) if len(sys.argv) > 1 else 50
dev = torch.device("cuda:0")
lib.load()
rows = [(name, M, K, N) for M in (2816, 3456) for name, K, N in SHAPES] + [("cross q / out_proj", 180, 256, 256), ("class_fc", 180, 256, 80)]
tot = {}
for name, M, K, N in rows:
    x, w, b = torch.randn(M, K, device=dev), torch.randn(N, K, device=dev), torch.randn(N, device=dev)
    y = torch.empty(M, N, device=dev)
    act = 1 if name.startswith("linear1") else 0
    call = lambda: lib.call("tuber_linear_f32", x, K, None, 0, 0, w, K, b, y, N, M, N, K, act)
    for _ in range(5):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        call()
    e1.record()
    torch.cuda.synchronize()
    us = 1e3 * e0.elapsed_time(e1) / n
    tf = 2.0 * M * N * K / us * 1e-6
    tot[M] = tot.get(M, 0.0) + us
    print("%-20s M %5d N %5d K %5d   %8.1f us   %6.1f TF/s = %4.1f %% of the fp32 matrix peak" % (name, M, N, K, us, tf, 100 * tf / PEAK_TF), flush=True)
