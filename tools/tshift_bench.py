#!/usr/bin/env python3
"""The learnable temporal shift of [N*T, C, H, W] tensors against every other way to the same tensors, forward and backward,
device-event times (GPU box):
    python3 tools/tshift_bench.py [--seconds 0.5] [--repeats 3]
Routes, alternated block by block in one process (each figure the mean of `repeats` blocks that together run at least `seconds`;
min..max of the blocks is the run-to-run spread):
  (a) torch.ops.torchshifts.temporal_shift_learnable (csrc/shiftnd_tshift.hip); backward: autograd's (torch.autograd.grad on a graph
      built outside the timed region)
  (b) permute + .contiguous() + shift1d on [N*M, C, T] + permute back + .contiguous(); backward: autograd's, in the same way -- the
      shift1d node reuses the permuted input its forward saved (the only other route through public ops with the right weight
      gradient)
  (c) torch.ops.torchshifts.temporal_shift (fixed, under rint(w)) on the same tensor: the copy-rate yardstick of the forward; no
      backward figure (its backward reads no input and forms no weight gradient)
  (d) the UNFLAGGED C-ABI call on the strided view [N, C, M, T] with weights (0, w): same out and grad_x, the strided fallback
Both modes, zeros padding, weights uniform in [-1.5, 1.5].  Every tensor is one of several sets rotated call by call, more than 1 GB
in all, so that no route finds its operands in the last-level cache.  GB/s = the bytes the result needs over (a) -- forward: one
read of every plane that is not filled + one write; backward: one read each of x and grad_out + one write -- and "of copy" that
rate over the same box's plain 1-read-1-write stream (tools/stream_probe, a child process that has exited before this one touches
the GPU)."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "activesparseshifts-pytorch_amd"))

LINES = [("56x56 fp16", (256, 256, 56, 56), "float16", 8), ("56x56 fp32", (128, 256, 56, 56), "float32", 16),
         ("14x14 bf16 (ragged)", (256, 1024, 14, 14), "bfloat16", 8)]
ES = {"float16": 2, "bfloat16": 2, "float32": 4}

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--only", default=None, help="comma-separated line numbers (0-based)")
ap.add_argument("--rotate-bytes", type=float, default=1.0e9, help="operand sets are added until they hold this many bytes")
a = ap.parse_args()


def numel(shape):
    return math.prod(shape)


def probe(nbytes):
    try:
        out = subprocess.run([os.path.join(ROOT, "tools", "stream_probe"), "--bytes", str(int(nbytes))], capture_output=True,
                             text=True, timeout=300)
        return float(json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])["1R1W_GBps"])
    except Exception as e:  # noqa: BLE001
        print("stream_probe unavailable: %r" % (e,))
        return float("nan")


COPY = probe(max(numel(shape) * ES[dt] for _, shape, dt, _ in LINES))

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


print("copy stream of this box (1R1W): %.0f GB/s" % COPY)
for li, (name, shape, dt, T) in enumerate(LINES):
    if a.only and str(li) not in a.only.split(","):
        continue
    tdt = getattr(torch, dt)
    NT, C, H, W = shape
    N, M = NT // T, H * W
    nbytes = numel(shape) * ES[dt]
    sets = max(2, int(a.rotate_bytes / (2 * nbytes)) + 1)
    torch.manual_seed(li)
    w = (torch.rand(C, 1, device="cuda") * 3 - 1.5).to(tdt)
    w2 = torch.cat([torch.zeros_like(w), w], 1).contiguous()   # (0, w) for the [N, C, M, T] view
    b6 = torch.tensor([0, T, 0, 1, 0, 1], dtype=torch.int32)
    xs = [torch.rand(shape, device="cuda").to(tdt) for _ in range(sets)]
    outs = [torch.empty_like(xs[0]) for _ in range(sets)]
    ws = torch.empty(abi.backward_workspace(torch.empty((N, C, M, T), dtype=tdt, device="meta"), 0, 1).numel(), dtype=torch.uint8, device="cuda")
    turn = [0]

    def nxt():
        turn[0] += 1
        return turn[0]

    def lines_of(t):   # [N*T, C, H, W] -> [N*M, C, T], a contiguous copy
        return t.view(N, T, C, M).permute(0, 3, 2, 1).reshape(N * M, C, T)

    def frames_of(l):
        return l.view(N, M, C, T).permute(0, 3, 2, 1).reshape(shape)

    def strided(t):    # [N*T, C, H, W] -> the [N, C, M, T] view, no copy
        return t.view(N, T, C, M).permute(0, 2, 3, 1)

    for active in (False, True):
        s = torch.round(w.float()).reshape(C).to(torch.int64)

        def b_forward():
            return frames_of(OPS._shift1d_forward(lines_of(xs[nxt() % sets]), w, b6, [N * M, C, T], 0, active))

        # the backward of (a) and (b): autograd's, through graphs built once outside the timed region (the node of (b) holds the
        # permuted copy of the input its forward made; the timed call permutes the gradient, runs shift1d's backward and permutes
        # grad_x back)
        xr = [x.clone().requires_grad_(True) for x in xs[:2]]
        wr = w.clone().requires_grad_(True)
        graph_a = [OPS.temporal_shift_learnable(x, wr, T, 0, active) for x in xr]
        graph_b = [frames_of(OPS.shift1d(lines_of(x), wr, torch.Tensor(), 0, active)) for x in xr]

        def b_backward():
            i = nxt()
            return torch.autograd.grad(graph_b[i % 2], (xr[i % 2], wr), xs[i % sets], retain_graph=True)

        def a_backward():
            i = nxt()
            return torch.autograd.grad(graph_a[i % 2], (xr[i % 2], wr), xs[i % sets], retain_graph=True)

        def d_forward():
            i = nxt()
            return abi.forward(strided(xs[i % sets]), w2, 0, active, out=strided(outs[i % sets]))

        def d_backward():
            i = nxt()
            return abi.backward(strided(xs[i % sets]), w2, strided(xs[(i + 1) % sets]), 0, active, grad_x=strided(outs[i % sets]),
                                workspace=ws)

        forms = [("a fwd", lambda: OPS._temporal_shift_learnable_forward(xs[nxt() % sets], w, T, 0, active)),
                 ("b fwd", b_forward),
                 ("c fwd", lambda: OPS.temporal_shift(xs[nxt() % sets], s, T, 0)),
                 ("d fwd", d_forward),
                 ("a bwd", a_backward), ("b bwd", b_backward), ("d bwd", d_backward)]
        # the routes return the same tensors
        ref = OPS._temporal_shift_learnable_forward(xs[0], w, T, 0, active)
        assert torch.equal(ref, frames_of(OPS._shift1d_forward(lines_of(xs[0]), w, b6, [N * M, C, T], 0, active)))
        # (d) is the 2-D rule with a zero fraction in the first dim: the same tensor up to the last place of a 16-bit result
        d_out = abi.forward(strided(xs[0]), w2, 0, active, out=strided(outs[0])).permute(0, 3, 1, 2).reshape(shape)
        d_same = torch.equal(ref, d_out)
        assert float((ref.float() - d_out.float()).abs().max()) <= 2.0 ** -7
        gx_a, gw_a = torch.autograd.grad(graph_a[0], (xr[0], wr), xs[1], retain_graph=True)
        gx_b, gw_b = torch.autograd.grad(graph_b[0], (xr[0], wr), xs[1], retain_graph=True)
        # fp32: the same bits; 16-bit interpolation: each route within one ulp of the oracle (the suite's bar), so within two of the other
        assert torch.equal(gx_a, gx_b) or (ES[dt] == 2 and active and float((gx_a.float() - gx_b.float()).abs().max()) <= 2.0 ** -7)
        assert float((gw_a.float() - gw_b.float()).abs().max()) <= 1e-2 * float(gw_b.float().abs().max())
        kernels, iters = {}, []
        for tag, fn in forms:
            for _ in range(2):
                fn()
            kernels[tag] = abi.last_kernel()
        # (autograd's backward runs on another thread, and the names are per thread: one direct call names (a)'s kernel)
        OPS._temporal_shift_learnable_backward(xs[0], w, xs[1], T, 0, active)
        kernels["a bwd"] = abi.last_kernel()
        for tag, fn in forms:
            iters.append(max(3, int(a.seconds / a.repeats / (block(fn, 3) * 1e-3)) + 1))
        times = [[] for _ in forms]
        for _ in range(a.repeats):
            for k, (tag, fn) in enumerate(forms):
                times[k].append(block(fn, iters[k]))
        mean = [sum(t) / len(t) for t in times]
        # planes the forward reads (zeros padding): the frames pad(t - iw) and, interpolating, pad(t - iw + 1) that exist
        wl = w.float().reshape(C).tolist()
        read = 0
        for v in wl:
            iw = math.floor(v) if active else round(v)
            frames = set()
            for t in range(T):
                frames.update(p for p in ((t - iw, t - iw + 1) if active and v != iw else (t - iw,)) if 0 <= p < T)
            read += len(frames)
        algo_f = N * M * ES[dt] * (read + T * C)
        algo_b = 3 * nbytes
        print("%s  %s %s T=%d  %s  (%d operand sets; (a) ran %s / %s, (d) ran %s / %s, its out %s (a)'s)"
              % (name, shape, dt, T, "active" if active else "sparse", sets, kernels["a fwd"], kernels["a bwd"], kernels["d fwd"],
                 kernels["d bwd"], "bit for bit" if d_same else "within one 16-bit ulp of"))
        for word, idx, algo in (("forward ", (0, 1, 2, 3), algo_f), ("backward", (4, 5, 6), algo_b)):
            cells = "   ".join("(%s) %.4f [%.4f..%.4f]" % (forms[k][0][0], mean[k], min(times[k]), max(times[k])) for k in idx)
            ia, ib = idx[0], idx[1]
            spread = max(max(times[k]) - min(times[k]) for k in (ia, ib))
            gbs = algo / (mean[ia] * 1e-3) / 1e9
            print("  %s ms  %s   (b) / (a) = %.2f, margin %.4f ms against a spread of %.4f: %s   (a): %.0f GB/s, %.2f of copy"
                  % (word, cells, mean[ib] / mean[ia], mean[ib] - mean[ia], spread,
                     "holds" if mean[ib] - mean[ia] > spread else "DOES NOT HOLD", gbs, gbs / COPY))
        del xr, wr, graph_a, graph_b
    del xs, outs
    torch.cuda.empty_cache()
