#!/usr/bin/env python3
"""The grad_x-only backward of the sparse shift (shiftnd_backward with x == NULL, csrc/shiftnd_gradx.hip) against the full sparse
backward and the sparse forward of the same geometry, through the C ABI, device-event times (GPU box):
    python3 tools/fixed_bench.py [--seconds 0.5] [--repeats 3] [--only c2,c2cut]
Per line: (a) abi.backward (reads x, forms grad_w), (b) abi.backward_input, (c) abi.forward -- each figure the mean of `repeats`
blocks that together run at least `seconds`, the three forms alternated block by block in one process; min..max of the blocks is
the run-to-run spread.  TB/s = 2 x tensor bytes (grad_out read + grad_x written, the bytes the result needs) over (b)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "activesparseshifts-pytorch_amd"))
from torchshifts import abi  # noqa: E402


def block(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--only", default=None)
ap.add_argument("--pad", type=int, default=0)
a = ap.parse_args()

LINES = [("c2", (64, 256, 224, 224), torch.float32, None), ("c2cut", (64, 256, 224, 224), torch.float32, [[1, 1], [1, 1]]),
         ("c1dcut", (256, 512, 4096), torch.float32, [[1, 1]]), ("c3", (8, 128, 16, 112, 112), torch.bfloat16, None),
         ("c3cut", (8, 128, 16, 112, 112), torch.bfloat16, [[1, 1], [1, 1], [1, 1]])]
print("%-7s %-22s %-22s %-26s  (a) full bwd ms [min..max]   (b) grad_x only ms [min..max]   (c) forward ms [min..max]   b/a    b/c    TB/s(b)"
      % ("line", "kernel (a)", "kernel (b)", "kernel (c)"))
for name, shape, tdt, cut in LINES:
    if a.only and name not in a.only.split(","):
        continue
    nd = len(shape) - 2
    b, new = abi.check_borders(list(shape), cut, nd) if cut else (None, list(shape))
    x = torch.rand(shape, device="cuda").to(tdt)
    go = torch.rand(new, device="cuda").to(tdt)
    w = torch.randint(-3, 4, (shape[1], nd), device="cuda").to(tdt)
    out, gx, gw = torch.empty_like(go), torch.empty_like(x), torch.empty_like(w)
    ws = abi.backward_workspace(x, a.pad, 0, b)
    forms = [lambda: abi.backward(go, w, x, a.pad, False, b, grad_x=gx, grad_w=gw, workspace=ws),
             lambda: abi.backward_input(go, w, shape, a.pad, b, grad_x=gx, workspace=ws),
             lambda: abi.forward(x, w, a.pad, False, b, out=out)]
    kernels, iters = [], []
    for fn in forms:   # warm-up, the kernel's name, the block length
        for _ in range(3):
            fn()
        kernels.append(abi.last_kernel())
        iters.append(max(3, int(a.seconds / a.repeats / (block(fn, 5) * 1e-3)) + 1))
    times = [[], [], []]
    for _ in range(a.repeats):
        for k, fn in enumerate(forms):
            times[k].append(block(fn, iters[k]))
    mean = [sum(t) / len(t) for t in times]
    cells = ["%.4f [%.4f..%.4f]" % (mean[k], min(times[k]), max(times[k])) for k in range(3)]
    tbs = 2.0 * x.numel() * x.element_size() / (mean[1] * 1e-3) / 1e12
    print("%-7s %-22s %-22s %-26s  %-28s %-31s %-26s %.3f  %.3f  %.2f"
          % (name, kernels[0][:22], kernels[1][:22], kernels[2][:26], cells[0], cells[1], cells[2], mean[1] / mean[0], mean[1] / mean[2], tbs))
    del x, go, out, gx
    torch.cuda.empty_cache()
