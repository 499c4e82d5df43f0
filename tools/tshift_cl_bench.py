#!/usr/bin/env python3
"""The LEARNABLE temporal shift of CHANNELS-LAST [N*T, C, H, W] tensors: the preserve-format op against what a channels-last model
paid before it, forward and backward, sparse and interpolating, device-event times (GPU box):
    python3 tools/tshift_cl_bench.py [--seconds 0.5] [--repeats 3] [--only 0,1]
Routes, alternated block by block in one process (each figure the mean of `repeats` blocks that together run at least `seconds`;
min..max of the blocks is the run-to-run spread):
  (a) torch.ops.torchshifts._temporal_shift_learnable_cl_forward / _backward on the channels-last tensors (a channels-last
      gradient): csrc/shiftnd_frames_learn.hip, csrc/shiftnd_frames.hip for the sparse forward
  (b) torch.ops.torchshifts._temporal_shift_learnable_forward / _backward on the same channels-last tensors (ATen's layout copies
      of the input -- and, backward, of the gradient --, the segment-major kernels, contiguous results) + .contiguous(memory_format=
      channels_last) on the result / on grad_x, which the next convolution pays: what the op did before the option existed
  (e) the same ops on CONTIGUOUS tensors of the same bytes: the segment-major kernels alone, the yardstick
The ops below the autograd key are called directly: no graph is built inside the timed region.  Weights are uniform in [-1.5, 1.5]
(every 16-byte piece of a pixel row mixes source frames), zeros padding.  Every tensor is one of several sets that are rotated call
by call, so that no route finds its operands in the 256 MB last-level cache.  GB/s = the bytes the pass needs (forward: one read and
one write of the tensor; backward: two reads and one write) over the time; "of copy" = that rate over the same box's plain
1-read-1-write stream (tools/stream_probe, a child process that has exited before this one touches the GPU)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "activesparseshifts-pytorch_amd"))

LINES = [("56x56 fp16", (256, 256, 56, 56), "float16", 8), ("56x56 fp32", (128, 256, 56, 56), "float32", 16),
         ("14x14 bf16", (256, 1024, 14, 14), "bfloat16", 8)]
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


PROBE_BYTES = max(numel(shape) * ES[dt] for _, shape, dt, _ in LINES)
COPY = probe(PROBE_BYTES)

import torch  # noqa: E402
from torchshifts import abi  # noqa: E402

OPS = torch.ops.torchshifts
CL = torch.channels_last


def block(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


print("copy stream of this box (1R1W, tensors of %d bytes): %.0f GB/s" % (PROBE_BYTES, COPY))
for li, (name, shape, dt, T) in enumerate(LINES):
    if a.only and str(li) not in a.only.split(","):
        continue
    NT, C, H, W = shape
    nbytes = numel(shape) * ES[dt]
    sets = max(2, int(a.rotate_bytes / (2 * nbytes)) + 1)
    tdt = getattr(torch, dt)
    gen = torch.Generator(device="cuda").manual_seed(li)
    w = (torch.rand(C, device="cuda", generator=gen) * 3 - 1.5).to(tdt)
    xs = [torch.rand(shape, device="cuda", generator=gen).to(tdt).contiguous(memory_format=CL) for _ in range(sets)]
    xcs = [x.contiguous() for x in xs]
    turn = [0]

    def pair(lst):   # (gradient, input): two different sets
        i = turn[0] = turn[0] + 1
        return lst[i % len(lst)], lst[(i + 1) % len(lst)]

    for active in (False, True):
        def a_backward():
            g, x = pair(xs)
            return OPS._temporal_shift_learnable_cl_backward(g, w, x, T, 0, active)

        def b_backward():
            g, x = pair(xs)
            gx, gw = OPS._temporal_shift_learnable_backward(g, w, x, T, 0, active)
            return gx.contiguous(memory_format=CL), gw

        def e_backward():
            g, x = pair(xcs)
            return OPS._temporal_shift_learnable_backward(g, w, x, T, 0, active)

        forms = [
            ("a fwd", lambda: OPS._temporal_shift_learnable_cl_forward(pair(xs)[0], w, T, 0, active)),
            ("b fwd", lambda: OPS._temporal_shift_learnable_forward(pair(xs)[0], w, T, 0, active).contiguous(memory_format=CL)),
            ("e fwd", lambda: OPS._temporal_shift_learnable_forward(pair(xcs)[0], w, T, 0, active)),
            ("a bwd", a_backward), ("b bwd", b_backward), ("e bwd", e_backward),
        ]
        # the routes return the same tensors
        ref = OPS._temporal_shift_learnable_cl_forward(xs[0], w, T, 0, active)
        assert ref.stride() == xs[0].stride() and torch.equal(ref, OPS._temporal_shift_learnable_forward(xcs[0], w, T, 0, active))
        gx, gw = OPS._temporal_shift_learnable_cl_backward(xs[1], w, xs[0], T, 0, active)
        gx_e, gw_e = OPS._temporal_shift_learnable_backward(xcs[1], w, xcs[0], T, 0, active)
        assert gx.stride() == xs[0].stride() and torch.equal(gx, gx_e)
        assert torch.allclose(gw.float(), gw_e.float(), rtol=2e-2, atol=1e-2 * float(gw_e.float().abs().max()))
        del ref, gx, gx_e
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
        print("%s  %s %s T=%d channels-last, %s  (%d operand sets; (a) ran %s / %s, (e) %s / %s)"
              % (name, shape, dt, T, "interpolating" if active else "sparse", sets, kernels["a fwd"], kernels["a bwd"], kernels["e fwd"],
                 kernels["e bwd"]))
        for base, word, passes in ((0, "forward ", 2), (3, "backward", 3)):
            cells = "   ".join("(%s) %.4f [%.4f..%.4f]" % (forms[base + k][0][0], mean[base + k], min(times[base + k]), max(times[base + k]))
                               for k in range(3))
            spread = sum(max(times[base + k]) - min(times[base + k]) for k in (0, 1))
            rate = [passes * nbytes / (mean[base + k] * 1e-3) / 1e9 for k in (0, 2)]
            margin = mean[base + 1] - mean[base]
            print("  %s ms  %s\n            (b) / (a) = %.2f, (b) - (a) = %+.4f ms against spreads of %.4f: %s;   (a): %.0f GB/s, %.2f of copy;"
                  "   (e): %.0f GB/s, %.2f of copy"
                  % (word, cells, mean[base + 1] / mean[base], margin, spread, "faster" if margin > spread else "NOT faster", rate[0],
                     rate[0] / COPY, rate[1], rate[1] / COPY))
    del xs, xcs, forms
    torch.cuda.empty_cache()
