#!/usr/bin/env python3
"""The temporal shift (TSM) of CHANNELS-LAST [N*T, C, H, W] tensors: the preserve-format op against every way there was to get the
same channels-last tensor before it, forward and backward, device-event times (GPU box):
    SHIFTND_HIP_LIB=<a build of the parent commit's libshiftnd_hip.so> python3 tools/temporal_cl_bench.py [--seconds 0.5] [--repeats 3]
Routes, alternated block by block in one process (each figure the mean of `repeats` blocks that together run at least `seconds`;
min..max of the blocks is the run-to-run spread):
  (a) torch.ops.torchshifts.temporal_shift_cl / _temporal_shift_cl_backward on the channels-last tensor (csrc/shiftnd_frames.hip)
  (b) torch.ops.torchshifts.temporal_shift / _temporal_shift_backward on the channels-last tensor (ATen's layout copy, the segment
      kernels, a contiguous result) + .contiguous(memory_format=channels_last) on the result, which the next convolution pays
  (c) the PyTorch slicing idiom of the published module on the channels-last tensor and its autograd backward
  (d) the UNFLAGGED C-ABI call of the same memory -- the NHWC 2-D problem [N, C, T, M] under the table (s, 0) -- through
      torchshifts.abi, which loads SHIFTND_HIP_LIB: with the parent commit's library this is what the layout cost at the C ABI
      before.  The line names the kernel (d) ran.
  (e) torch.ops.torchshifts.temporal_shift / _temporal_shift_backward on a CONTIGUOUS tensor of the same bytes: the segment-major
      kernel, the yardstick of what a copy-rate temporal shift costs on this box.
The quantized line is forward only: (a) temporal_shift_quantized_cl, (b) temporal_shift_quantized + the layout change back,
(c) the idiom on the int_repr, (d) unflagged shiftnd_forward_quantized, (e) temporal_shift_quantized on a contiguous tensor.
Every tensor is one of several sets that are rotated call by call, so that no route finds its operands in the 256 MB last-level
cache.  GB/s = the bytes the result needs -- one read of every channel that is not filled, one write of every channel -- over the
time; "of copy" = that rate over the same box's plain 1-read-1-write stream (tools/stream_probe on tensors of the largest line's
size, a child process that has exited before this one touches the GPU)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "activesparseshifts-pytorch_amd"))

LINES = [("56x56 fp16", (256, 256, 56, 56), "float16", 8), ("56x56 fp32", (128, 256, 56, 56), "float32", 16),
         ("14x14 bf16", (256, 1024, 14, 14), "bfloat16", 8), ("7x7 fp16", (512, 2048, 7, 7), "float16", 8),
         ("56x56 quint8", (256, 256, 56, 56), "quint8", 8)]
ES = {"float16": 2, "bfloat16": 2, "float32": 4, "quint8": 1}

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


PROBE_BYTES = max(numel(shape) * ES[dt] for _, shape, dt, _ in LINES)
COPY = probe(PROBE_BYTES)

import torch  # noqa: E402
from torchshifts import abi  # noqa: E402

OPS = torch.ops.torchshifts
CL = torch.channels_last
ZP, SCALE = 77, 0.05


def block(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


print("library of (d):", "SHIFTND_HIP_LIB (%s)" % os.path.basename(os.environ["SHIFTND_HIP_LIB"]) if os.environ.get("SHIFTND_HIP_LIB") else "in-tree")
print("copy stream of this box (1R1W, tensors of %d bytes): %.0f GB/s" % (PROBE_BYTES, COPY))
for li, (name, shape, dt, T) in enumerate(LINES):
    if a.only and str(li) not in a.only.split(","):
        continue
    quantized = dt == "quint8"
    NT, C, H, W = shape
    N, M = NT // T, H * W
    nbytes = numel(shape) * ES[dt]
    sets = max(2, int(a.rotate_bytes / (2 * nbytes)) + 1)
    f = C // 8
    s = torch.tensor([-1] * f + [1] * f + [0] * (C - 2 * f), device="cuda")
    table = torch.stack([s, torch.zeros_like(s)], 1)

    def nhwc(t):   # channels-last [N*T, C, H, W] -> the [N, C, T, M] view of the same memory
        return t.permute(0, 2, 3, 1).view(N, T, M, C).permute(0, 3, 1, 2)

    def idiom(x):
        v = x.view(N, T, C, H, W)
        out = torch.full_like(v, ZP) if quantized else torch.zeros_like(v)
        out[:, :-1, :f] = v[:, 1:, :f]
        out[:, 1:, f:2 * f] = v[:, :-1, f:2 * f]
        out[:, :, 2 * f:] = v[:, :, 2 * f:]
        return out.view(NT, C, H, W)

    turn = [0]

    def pick(lst):
        turn[0] += 1
        return lst[turn[0] % len(lst)]

    if quantized:
        reprs = [torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda").contiguous(memory_format=CL) for _ in range(sets)]
        xs = [torch._make_per_tensor_quantized_tensor(r.permute(0, 2, 3, 1), SCALE, ZP).permute(0, 3, 1, 2) for r in reprs]
        xcs = [torch._make_per_tensor_quantized_tensor(r.contiguous(), SCALE, ZP) for r in reprs]
        outs = [torch.empty_like(r) for r in reprs]
        wq = table.to(torch.int32)
        assert xs[0].stride() == reprs[0].stride()

        def d_forward():
            i = turn[0] = turn[0] + 1
            return abi.forward_quantized(nhwc(reprs[i % sets]), wq, 0, ZP, 0, out=nhwc(outs[i % sets]))

        def b_forward():
            out = OPS.temporal_shift_quantized(pick(xs), s, T, 0)
            return torch._make_per_tensor_quantized_tensor(out.int_repr().contiguous(memory_format=CL).permute(0, 2, 3, 1), SCALE, ZP)

        forms = [("a fwd", lambda: OPS.temporal_shift_quantized_cl(pick(xs), s, T, 0)), ("b fwd", b_forward),
                 ("c fwd", lambda: idiom(pick(reprs))), ("d fwd", d_forward),
                 ("e fwd", lambda: OPS.temporal_shift_quantized(pick(xcs), s, T, 0))]
        ref = OPS.temporal_shift_quantized_cl(xs[0], s, T, 0)
        assert ref.stride() == xs[0].stride() and torch.equal(ref.int_repr(), idiom(reprs[0]))
        assert torch.equal(ref.int_repr(), OPS.temporal_shift_quantized(xcs[0], s, T, 0).int_repr())
        turn[0] = -1
        d_forward()
        assert torch.equal(ref.int_repr(), outs[0])
        directions = ((0, "forward "),)
    else:
        tdt = getattr(torch, dt)
        w = table.to(tdt)
        xs = [torch.rand(shape, device="cuda").to(tdt).contiguous(memory_format=CL) for _ in range(sets)]
        xcs = [x.contiguous() for x in xs]
        outs = [torch.empty_like(xs[0]) for _ in range(sets)]
        xr = [x.clone(memory_format=torch.preserve_format).requires_grad_(True) for x in xs[:2]]
        graphs = [idiom(x) for x in xr]   # (c) backward: the autograd graph of the idiom, kept

        def c_backward():
            i = turn[0] = turn[0] + 1
            return torch.autograd.grad(graphs[i % 2], xr[i % 2], xs[i % sets], retain_graph=True)

        def d_forward():
            i = turn[0] = turn[0] + 1
            return abi.forward(nhwc(xs[i % sets]), w, 0, 0, out=nhwc(outs[i % sets]))

        def d_backward():
            i = turn[0] = turn[0] + 1
            return abi.backward_input(nhwc(xs[i % sets]), w, (N, C, T, M), 0, grad_x=nhwc(outs[i % sets]))

        forms = [
            ("a fwd", lambda: OPS.temporal_shift_cl(pick(xs), s, T, 0)),
            ("b fwd", lambda: OPS.temporal_shift(pick(xs), s, T, 0).contiguous(memory_format=CL)),
            ("c fwd", lambda: idiom(pick(xs))),
            ("d fwd", d_forward),
            ("e fwd", lambda: OPS.temporal_shift(pick(xcs), s, T, 0)),
            ("a bwd", lambda: OPS._temporal_shift_cl_backward(pick(xs), s, T, 0)),
            ("b bwd", lambda: OPS._temporal_shift_backward(pick(xs), s, T, 0).contiguous(memory_format=CL)),
            ("c bwd", c_backward),
            ("d bwd", d_backward),
            ("e bwd", lambda: OPS._temporal_shift_backward(pick(xcs), s, T, 0)),
        ]
        ref = OPS.temporal_shift_cl(xs[0], s, T, 0)   # the routes return the same tensor
        assert ref.stride() == xs[0].stride() and torch.equal(ref, idiom(xs[0])) and torch.equal(ref, OPS.temporal_shift(xcs[0], s, T, 0))
        turn[0] = -1
        d_forward()
        assert torch.equal(ref, outs[0])
        directions = ((0, "forward "), (5, "backward"))
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
    # channels that are read: every (t, c) whose source frame exists (zeros padding)
    read = sum(T - min(abs(int(v)), T) for v in s.tolist())
    algo = N * M * ES[dt] * (read + T * C)
    print("%s  %s %s T=%d channels-last  (%d operand sets; (d) ran %s%s)"
          % (name, shape, dt, T, sets, kernels["d fwd"], "" if quantized else " / " + kernels["d bwd"]))
    for base, word in directions:
        cells = "   ".join("(%s) %.4f [%.4f..%.4f]" % (forms[base + k][0][0], mean[base + k], min(times[base + k]), max(times[base + k]))
                           for k in range(5))
        best = min(range(1, 4), key=lambda k: mean[base + k])
        spread = max(max(times[base + k]) - min(times[base + k]) for k in (0, best))
        rate = [algo / (mean[base + k] * 1e-3) / 1e9 for k in (0, 4)]
        e_spread = sum(max(times[base + k]) - min(times[base + k]) for k in (0, 4))
        print("  %s ms  %s\n            fastest of b, c, d (%s) / (a) = %.2f, margin %.4f ms against a spread of %.4f;   (a): %.0f GB/s, %.2f of copy;"
              "   (e): %.0f GB/s, %.2f of copy;   (e) - (a) = %+.4f ms against spreads of %.4f"
              % (word, cells, forms[base + best][0][0], mean[base + best] / mean[base], mean[base + best] - mean[base], spread, rate[0],
                 rate[0] / COPY, rate[1], rate[1] / COPY, mean[base + 4] - mean[base], e_spread))
    del xs, xcs, outs, ref, forms
    if quantized:
        del reprs
    else:
        del xr, graphs
    torch.cuda.empty_cache()
