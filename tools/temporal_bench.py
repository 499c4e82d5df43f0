#!/usr/bin/env python3
"""The temporal shift (TSM) of [N*T, C, H, W] tensors: the op against every way there was to get the same tensor before it,
forward and backward, device-event times (GPU box):
    SHIFTND_HIP_LIB=<a build of the parent commit's libshiftnd_hip.so> python3 tools/temporal_bench.py [--seconds 0.5] [--repeats 3]
Routes, alternated block by block in one process (each figure the mean of `repeats` blocks that together run at least `seconds`;
min..max of the blocks is the run-to-run spread):
  (a) torch.ops.torchshifts.temporal_shift / _temporal_shift_backward (csrc/shiftnd_segment.hip)
  (b) permute, .contiguous(), shift2d_fixed / _shift2d_fixed_backward on [N, C, T, M], permute back, .contiguous()
  (c) the PyTorch slicing idiom of the published module (zeros + three slice copies) and its autograd backward
  (d) the C ABI on the permuted views, no layout change, through torchshifts.abi -- which loads SHIFTND_HIP_LIB: with the parent
      commit's library this is what that stride pattern cost before (strided_gather_forward); the ops of (a) and (b) always use
      the in-tree library.  The line names the kernel (d) ran.
Every tensor is one of several sets that are rotated call by call, so that no route finds its operands in the 256 MB last-level
cache.  GB/s = the bytes the result needs -- one read of every plane that is not filled, one write of every plane -- over (a);
"of copy" = that rate over the same box's plain 1-read-1-write stream (tools/stream_probe on tensors of the largest line's size, a
child process that has exited before this one touches the GPU)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "activesparseshifts-pytorch_amd"))

LINES = [("56x56 fp16", (256, 256, 56, 56), "float16", 8), ("14x14 bf16", (256, 1024, 14, 14), "bfloat16", 8),
         ("7x7 fp16 (ragged)", (512, 2048, 7, 7), "float16", 8), ("56x56 fp32", (128, 256, 56, 56), "float32", 16)]
ES = {"float16": 2, "bfloat16": 2, "float32": 4}

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--only", default=None, help="comma-separated line numbers (0-based)")
ap.add_argument("--rotate-bytes", type=float, default=1.0e9, help="operand sets are added until they hold this many bytes")
a = ap.parse_args()


def probe(nbytes):
    try:
        out = subprocess.run([os.path.join(ROOT, "tools", "stream_probe"), "--bytes", str(int(nbytes))], capture_output=True,
                             text=True, timeout=300)
        return float(json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])["1R1W_GBps"])
    except Exception as e:  # noqa: BLE001
        print("stream_probe unavailable: %r" % (e,))
        return float("nan")


def numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


# one probe, at the largest tensor of the list: the 100 MB tensors alone would stream from the last-level cache in the probe, while
# the routes below never find theirs there
PROBE_BYTES = max(numel(shape) * ES[dt] for _, shape, dt, _ in LINES)
COPY = probe(PROBE_BYTES)

import torch  # noqa: E402
from torchshifts import abi  # noqa: E402

OPS = torch.ops.torchshifts


def block(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


# (the file's name only: the lines below name the kernel (d) ran, which is what tells the builds apart)
print("library of (d):", "SHIFTND_HIP_LIB (%s)" % os.path.basename(os.environ["SHIFTND_HIP_LIB"]) if os.environ.get("SHIFTND_HIP_LIB") else "in-tree")
print("copy stream of this box (1R1W, tensors of %d bytes): %.0f GB/s" % (PROBE_BYTES, COPY))
for li, (name, shape, dt, T) in enumerate(LINES):
    if a.only and str(li) not in a.only.split(","):
        continue
    tdt = getattr(torch, dt)
    NT, C, H, W = shape
    N, M = NT // T, H * W
    nbytes = numel(shape) * ES[dt]
    sets = max(2, int(a.rotate_bytes / (2 * nbytes)) + 1)
    f = C // 8
    s = torch.tensor([-1] * f + [1] * f + [0] * (C - 2 * f), device="cuda")
    table = torch.stack([s, torch.zeros_like(s)], 1)
    w = table.to(tdt)
    b6 = torch.tensor([0, T, 0, M, 0, 1], dtype=torch.int32)
    xs = [torch.rand(shape, device="cuda").to(tdt) for _ in range(sets)]
    outs = [torch.empty_like(xs[0]) for _ in range(sets)]
    xr = [x.clone().requires_grad_(True) for x in xs[:2]]
    turn = [0]

    def pick(lst):
        turn[0] += 1
        return lst[turn[0] % len(lst)]

    def seg(t):   # [N*T, C, H, W] -> the [N, C, T, M] view
        return t.view(N, T, C, M).permute(0, 2, 1, 3)

    def idiom(x):
        v = x.view(N, T, C, H, W)
        out = torch.zeros_like(v)
        out[:, :-1, :f] = v[:, 1:, :f]
        out[:, 1:, f:2 * f] = v[:, :-1, f:2 * f]
        out[:, :, 2 * f:] = v[:, :, 2 * f:]
        return out.view(NT, C, H, W)

    graphs = [idiom(x) for x in xr]   # (c) backward: the autograd graph of the idiom, kept

    def c_backward():
        i = turn[0] = turn[0] + 1
        return torch.autograd.grad(graphs[i % 2], xr[i % 2], xs[i % sets], retain_graph=True)

    def d_forward():
        i = turn[0] = turn[0] + 1
        return abi.forward(seg(xs[i % sets]), w, 0, 0, out=seg(outs[i % sets]))

    def d_backward():
        i = turn[0] = turn[0] + 1
        return abi.backward_input(seg(xs[i % sets]), w, (N, C, T, M), 0, grad_x=seg(outs[i % sets]))

    forms = [
        ("a fwd", lambda: OPS.temporal_shift(pick(xs), s, T, 0)),
        ("b fwd", lambda: OPS.shift2d_fixed(seg(pick(xs)).contiguous(), table, torch.Tensor(), 0).permute(0, 2, 1, 3).contiguous()),
        ("c fwd", lambda: idiom(pick(xs))),
        ("d fwd", d_forward),
        ("a bwd", lambda: OPS._temporal_shift_backward(pick(xs), s, T, 0)),
        ("b bwd", lambda: OPS._shift2d_fixed_backward(seg(pick(xs)).contiguous(), table, b6, [N, C, T, M], 0).permute(0, 2, 1, 3).contiguous()),
        ("c bwd", c_backward),
        ("d bwd", d_backward),
    ]
    ref = OPS.temporal_shift(xs[0], s, T, 0)   # the four routes return the same tensor
    assert torch.equal(ref, idiom(xs[0]))
    assert torch.equal(ref, OPS.shift2d_fixed(seg(xs[0]).contiguous(), table, torch.Tensor(), 0).permute(0, 2, 1, 3).reshape(shape))
    assert torch.equal(ref, abi.forward(seg(xs[0]), w, 0, 0, out=seg(outs[0])).permute(0, 2, 1, 3).reshape(shape))
    kernels, iters = {}, []
    for tag, fn in forms:
        for _ in range(2):
            fn()
        kernels[tag] = abi.last_kernel()
        iters.append(max(3, int(a.seconds / a.repeats / (block(fn, 3) * 1e-3)) + 1))
    times = [[] for _ in forms]
    for _ in range(a.repeats):
        for k, (tag, fn) in enumerate(forms):
            times[k].append(block(fn, iters[k]))
    mean = [sum(t) / len(t) for t in times]
    # planes that are read: every (t, c) whose source frame exists (zeros padding)
    read_planes = sum(T - min(abs(int(v)), T) for v in s.tolist())
    algo = N * M * ES[dt] * (read_planes + T * C)
    print("%s  %s %s T=%d  (%d operand sets; (d) ran %s / %s)" % (name, shape, dt, T, sets, kernels["d fwd"], kernels["d bwd"]))
    for base, word in ((0, "forward "), (4, "backward")):
        cells = "   ".join("(%s) %.4f [%.4f..%.4f]" % (forms[base + k][0][0], mean[base + k], min(times[base + k]), max(times[base + k]))
                           for k in range(4))
        best = min(range(1, 4), key=lambda k: mean[base + k])
        spread = max(max(times[base + k]) - min(times[base + k]) for k in (0, best))
        gbs = algo / (mean[base] * 1e-3) / 1e9
        print("  %s ms  %s   fastest other (%s) / (a) = %.2f, margin %.4f ms against a spread of %.4f   (a): %.0f GB/s, %.2f of copy"
              % (word, cells, forms[base + best][0][0], mean[base + best] / mean[base], mean[base + best] - mean[base], spread, gbs,
                 gbs / COPY))
    del xs, outs, xr, graphs, ref
    torch.cuda.empty_cache()
