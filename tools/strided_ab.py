#!/usr/bin/env python3
"""One process of the A/B timing of the strided fallback's backward (strided_backward: `ACTIVE` a run-time argument since DESIGN
3.28): policy 1 forces the fallback; the library is the in-tree one or SHIFTND_HIP_LIB.  Prints one JSON line of ms per call
(device events, `--iters` calls per figure).  Alternate two builds process by process and compare the ranges:
    SHIFTND_HIP_LIB=<parent build> python3 tools/strided_ab.py ; python3 tools/strided_ab.py ; ..."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "activesparseshifts-pytorch_amd"))

import torch  # noqa: E402
from torchshifts import abi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
a = ap.parse_args()

LINES = [((8, 64, 4096), "float32"), ((16, 64, 56, 56), "float32"), ((16, 64, 56, 56), "float16"), ((4, 32, 8, 28, 28), "bfloat16"),
         ((8, 32, 56, 56), "float64")]
abi.set_path_policy(1)
res = {}
for shape, dt in LINES:
    tdt = getattr(torch, dt)
    torch.manual_seed(1)
    x, go = torch.rand(shape, device="cuda").to(tdt), torch.rand(shape, device="cuda").to(tdt)
    w = (torch.rand(shape[1], len(shape) - 2, device="cuda") * 5 - 2.5).to(tdt)
    for active in (0, 1):
        ws = abi.backward_workspace(x, 0, active)
        gx, gw = torch.empty_like(x), torch.empty_like(w)
        for _ in range(3):
            abi.backward(go, w, x, 0, active, grad_x=gx, grad_w=gw, workspace=ws)
        assert abi.last_kernel() == "strided_backward", abi.last_kernel()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            abi.backward(go, w, x, 0, active, grad_x=gx, grad_w=gw, workspace=ws)
        e1.record()
        e1.synchronize()
        res["%s %s %s" % ("x".join(map(str, shape)), dt, "active" if active else "sparse")] = e0.elapsed_time(e1) / a.iters
print(json.dumps({"lib": "parent" if os.environ.get("SHIFTND_HIP_LIB") else "tree", "ms": res}))
