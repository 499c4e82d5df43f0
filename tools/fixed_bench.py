#!/usr/bin/env python3
"""The grad_x-only backward of the sparse shift (shiftnd_backward with x == NULL, csrc/shiftnd_gradx.hip) against the full sparse
backward and the sparse forward of the same geometry, through the C ABI, device-event times (GPU box):
    python3 tools/fixed_bench.py [--seconds 0.5] [--repeats 3] [--only c2,c2cut]
Per line: (a) abi.backward (reads x, forms grad_w), (b) abi.backward_input, (c) abi.forward -- each figure the mean of `repeats`
blocks that together run at least `seconds`, the three forms alternated block by block in one process; min..max of the blocks is
the run-to-run spread.  TB/s = 2 x tensor bytes (grad_out read + grad_x written, the bytes the result needs) over (b).

Strided lines (names s_*): the fused op torch.ops.torchshifts.shift{N}d_fixed_pool against the composed sequence shift{N}d_fixed +
ATen's average pool (what a strided GroupedShift module ran before the fused op), through the dispatcher, same rule: forward (no
graph), backward (the backward ops alone: _shift{N}d_fixed_pool_backward against avg_pool backward + _shift{N}d_fixed_backward) and
step (forward + autograd backward), fused and composed alternated block by block."""
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
         ("c3cut", (8, 128, 16, 112, 112), torch.bfloat16, [[1, 1], [1, 1], [1, 1]]),
         ("r62cut", (64, 256, 62, 62), torch.float32, [[1, 1], [1, 1]])]   # ragged grad_x rows: gradx_gather
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

OPS = torch.ops.torchshifts
AT = torch.ops.aten
C2, C3 = (64, 256, 224, 224), (8, 128, 16, 112, 112)
STRIDED = [("s_c2cut", C2, torch.float32, [[1, 1], [1, 1]], 2), ("s_c3cut", C3, torch.bfloat16, [[1, 1], [1, 1], [1, 1]], 2),
           ("s_c1dcut", (256, 512, 4096), torch.float32, [[1, 1]], 2), ("s_c2", C2, torch.float32, None, 2),
           ("s_r62cut", (64, 256, 62, 62), torch.float32, [[1, 1], [1, 1]], 2)]   # ragged grad_x rows: gradx_gather_pool
print()
print("%-9s %-24s %-18s  forward ms fused / composed [min..max]            backward ms fused / composed [min..max]           step ms fused / composed [min..max]               c/f fwd  bwd   step"
      % ("line", "kernel fwd (fused)", "kernel bwd (fused)"))
for name, shape, tdt, cut, pool in STRIDED:
    if a.only and name not in a.only.split(","):
        continue
    nd = len(shape) - 2
    k = [pool] * nd
    b, new = abi.check_borders(list(shape), cut, nd)
    bt = torch.Tensor() if cut is None else torch.tensor(cut, dtype=torch.long)
    b6 = torch.tensor(b, dtype=torch.int32)
    x = torch.rand(shape, device="cuda").to(tdt).requires_grad_(True)
    s = torch.randint(-3, 4, (shape[1], nd), device="cuda")
    gp = torch.rand(abi.pooled_shape(x, k, b), device="cuda").to(tdt)
    fixed, fused = getattr(OPS, "shift%dd_fixed" % nd), getattr(OPS, "shift%dd_fixed_pool" % nd)
    fixed_bwd, fused_bwd = getattr(OPS, "_shift%dd_fixed_backward" % nd), getattr(OPS, "_shift%dd_fixed_pool_backward" % nd)
    y_like = torch.empty(new, device="cuda", dtype=tdt)   # (the pool's backward only looks at its shape)

    def pool_fwd(y):
        return (torch.nn.functional.avg_pool1d, torch.nn.functional.avg_pool2d, torch.nn.functional.avg_pool3d)[nd - 1](y, k, k, ceil_mode=True)

    def pool_bwd(g):
        if nd == 1:
            return AT.avg_pool2d_backward(g.unsqueeze(2), y_like.unsqueeze(2), [1] + k, [1] + k, [0, 0], True, True, None).squeeze(2)
        if nd == 2:
            return AT.avg_pool2d_backward(g, y_like, k, k, [0, 0], True, True, None)
        return AT.avg_pool3d_backward(g, y_like, k, k, [0, 0, 0], True, True, None)

    def step(f):
        x.grad = None
        f().backward(gp)

    xd = x.detach()
    forms = [lambda: fused(xd, s, bt, k, a.pad), lambda: pool_fwd(fixed(xd, s, bt, a.pad)),
             lambda: fused_bwd(gp, s, b6, list(shape), k, a.pad), lambda: fixed_bwd(pool_bwd(gp), s, b6, list(shape), a.pad),
             lambda: step(lambda: fused(x, s, bt, k, a.pad)), lambda: step(lambda: pool_fwd(fixed(x, s, bt, a.pad)))]
    kernels, iters = [], []
    for fn in forms:
        for _ in range(3):
            fn()
        kernels.append(abi.last_kernel())
        iters.append(max(3, int(a.seconds / a.repeats / (block(fn, 5) * 1e-3)) + 1))
    times = [[] for _ in forms]
    for _ in range(a.repeats):
        for i, fn in enumerate(forms):
            times[i].append(block(fn, iters[i]))
    mean = [sum(t) / len(t) for t in times]
    cell = lambda i: "%.4f [%.4f..%.4f]" % (mean[i], min(times[i]), max(times[i]))
    print("%-9s %-24s %-18s  %-26s / %-26s %-26s / %-26s %-26s / %-26s %.2f  %.2f  %.2f"
          % (name, kernels[0][:24], kernels[2][:18], cell(0), cell(1), cell(2), cell(3), cell(4), cell(5),
             mean[1] / mean[0], mean[3] / mean[2], mean[5] / mean[4]))
    del x, xd, gp, y_like
    torch.cuda.empty_cache()
