#!/usr/bin/env python
"""One GEMM shape, N launches of the persistent 256x256 kernel, for rocprofv3 --pmc runs: python tools/pp_probe.py M N K kind [launches]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from panst3r_amd import hip
from tools.gemm_cases import case
M, N, K, kind = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
n = int(sys.argv[5]) if len(sys.argv) > 5 else 10
hip.lib()
a, w, out, kw = case(M, N, K, kind)
for _ in range(n):
    hip.gemm(a, w, out, kernel=256, **kw)
torch.cuda.synchronize()
