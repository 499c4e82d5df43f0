#!/usr/bin/env python3
"""Temporal interlacing of CHANNELS-LAST [N*T, C, H, W] tensors (memory_format=torch.preserve_format), forward and backward,
device-event times and the peak memory of one training step (GPU box):
    python3 tools/interlace_cl_bench.py [--processes 3] [--seconds 0.3] [--repeats 4]
Routes, alternated block by block in one process (each figure the mean of `repeats` blocks that together run at least `seconds`);
the whole table is taken in `processes` fresh processes one after the other, and what is printed is the median over the processes
with min..max of the per-process figures, the run-to-run spread:
  (n) torch.ops.torchshifts_interlace_cl.temporal_interlace_cl on the channels-last tensor as it lies, the new route; backward:
      autograd's (torch.autograd.grad on a graph built outside the timed region), the gradient channels-last
  (a) the route before it on the same tensor: the default op (contiguous copy, tinterlace_*, contiguous result) and the layout
      change back to channels-last, with autograd
  (b) the composition on the channels-last per-clip op: temporal_shift_learnable_per_clip_cl(x, offsets) * scales, with autograd
  (c) the channels-last per-clip op alone: the floor
  (d) the contiguous interlace op on contiguous copies of the same values, for orientation
Tables: "layer" -- TemporalInterlace's own with shift_div = 1: four channel groups of C // 4 channels under (o, -o) and (w, w), so
every 16-byte piece of a pixel's channel row is uniform -- and "full" -- every (n, c) offset drawn on its own: every piece mixed.
The bar, under the layer's tables: (n) faster than (a) and than (b) in every line by more than the run's own spread, and a peak
below (b)'s.  The full-table lines are reported, not gated: mixed pieces move element by element.
Byte model: forward (n) = one read + one write of the tensor = (c); (a) adds a read and a write per layout change, (b) a second
read and write.  Backward (n) = frames_backward's traffic (grad_out twice -- the second read a cache hit --, x once, grad_x once)
plus the records: one double per (workgroup, t, c), 26 MB on the first line against 1.2 GB.
Peak memory: torch.cuda.max_memory_allocated over one forward + backward from a graph-free start, minus what was allocated before.
Zeros padding, both modes, offsets in [-1.5, 1.5], scales in [0, 2] (TIN's range).  Every tensor is one of several sets rotated call
by call, so that no route finds its operands in the last-level cache."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "activesparseshifts-pytorch_amd"))

LINES = [("56x56 fp16", (256, 256, 56, 56), "float16", 8), ("56x56 fp32", (128, 256, 56, 56), "float32", 16),
         ("14x14 bf16", (256, 1024, 14, 14), "bfloat16", 8)]
ES = {"float16": 2, "bfloat16": 2, "float32": 4}
TAGS = "nabcd"
ROUTES = [t + " " + word for word in ("fwd", "bwd") for t in TAGS]

ap = argparse.ArgumentParser()
ap.add_argument("--processes", type=int, default=3)
ap.add_argument("--seconds", type=float, default=0.3)
ap.add_argument("--repeats", type=int, default=4)
ap.add_argument("--only", default=None, help="comma-separated line numbers (0-based)")
ap.add_argument("--tables", default="layer,full")
ap.add_argument("--rotate-bytes", type=float, default=1.0e9, help="operand sets are added until they hold this many bytes")
ap.add_argument("--child", action="store_true", help="(internal) one process's table as JSON lines")
a = ap.parse_args()


def child():
    import torch
    from torchshifts import abi

    TIN, TINCL, PCCL = torch.ops.torchshifts_interlace, torch.ops.torchshifts_interlace_cl, torch.ops.torchshifts_per_clip_cl
    CL = torch.channels_last

    def block(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    for li, (name, shape, dt, T) in enumerate(LINES):
        if a.only and str(li) not in a.only.split(","):
            continue
        tdt = getattr(torch, dt)
        NT, C, H, W = shape
        N = NT // T
        nbytes = math.prod(shape) * ES[dt]
        sets = max(2, int(a.rotate_bytes / (2 * nbytes)) + 1)
        torch.manual_seed(li)
        xs = [torch.rand(shape, device="cuda").to(tdt).contiguous(memory_format=CL) for _ in range(sets)]
        xc = [x.contiguous() for x in xs[:2]]                      # (d): contiguous copies
        turn = [0]

        def nxt():
            turn[0] += 1
            return turn[0]

        def new(x, w_, s_, active):
            return TINCL.temporal_interlace_cl(x, w_, s_, T, 0, active)

        def today(x, w_, s_, active):
            return TIN.temporal_interlace(x, w_, s_, T, 0, active).contiguous(memory_format=CL)

        def composed(x, w_, s_, active):
            return PCCL.temporal_shift_learnable_per_clip_cl(x, w_, T, 0, active) * s_.reshape(NT, C, 1, 1)

        def alone(x, w_, s_, active):
            return PCCL.temporal_shift_learnable_per_clip_cl(x, w_, T, 0, active)

        def contiguous(x, w_, s_, active):
            return TIN.temporal_interlace(x, w_, s_, T, 0, active)

        routes = {"n": new, "a": today, "b": composed, "c": alone, "d": contiguous}
        for table in a.tables.split(","):
            if table == "layer":
                o, g = torch.rand(N, 2, device="cuda") * 3 - 1.5, torch.rand(N, T, 2, device="cuda") * 2
                w = torch.cat((o, -o), 1).repeat_interleave(C // 4, dim=1).to(tdt)
                s = torch.cat((g, g), 2).repeat_interleave(C // 4, dim=2).to(tdt)
            else:
                w = (torch.rand(N, C, device="cuda") * 3 - 1.5).to(tdt)
                s = (torch.rand(N, T, C, device="cuda") * 2).to(tdt)
            for active in (False, True):
                # one training step from a graph-free start: the peak above what is allocated already
                peak = {}
                for tag in "nab":
                    xr, wr, sr = xs[0].clone(memory_format=torch.preserve_format).requires_grad_(True), w.clone().requires_grad_(True), s.clone().requires_grad_(True)
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    routes[tag](xr, wr, sr, active).backward(xs[1])
                    torch.cuda.synchronize()
                    peak[tag] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
                    del xr, wr, sr
                xr = [x.clone(memory_format=torch.preserve_format).requires_grad_(True) for x in xs[:2]]
                xcr = [x.clone().requires_grad_(True) for x in xc]
                wr, sr = w.clone().requires_grad_(True), s.clone().requires_grad_(True)
                graphs = {tag: [routes[tag](x, wr, sr, active) for x in (xcr if tag == "d" else xr)] for tag in TAGS}
                assert graphs["n"][0].dtype == tdt and graphs["n"][0].stride() == xs[0].stride() and graphs["a"][0].stride() == xs[0].stride()
                assert torch.equal(graphs["n"][0], graphs["a"][0]) and torch.equal(graphs["n"][0], graphs["d"][0])   # the contiguous kernels' bits
                gn = torch.autograd.grad(graphs["n"][0], (xr[0], wr, sr), xs[1], retain_graph=True)
                ga = torch.autograd.grad(graphs["a"][0], (xr[0], wr, sr), xs[1], retain_graph=True)
                assert gn[0].stride() == xs[1].stride() and torch.equal(gn[0], ga[0])
                del gn, ga

                def backward_of(tag):
                    wrt = (wr,) if tag == "c" else (wr, sr)
                    leaves, grads = (xcr, xc) if tag == "d" else (xr, xs)

                    def fn():
                        i = nxt()
                        return torch.autograd.grad(graphs[tag][i % 2], (leaves[i % 2],) + wrt, grads[i % len(grads)], retain_graph=True)
                    return fn

                def forward_of(tag):
                    pool = xc if tag == "d" else xs

                    def fn():
                        with torch.no_grad():
                            return routes[tag](pool[nxt() % len(pool)], w, s, active)
                    return fn

                forms = [(t + " fwd", forward_of(t)) for t in TAGS] + [(t + " bwd", backward_of(t)) for t in TAGS]
                iters = {}
                for tag, fn in forms:
                    for _ in range(2):
                        fn()
                    iters[tag] = max(3, int(a.seconds / a.repeats / (block(fn, 3) * 1e-3)) + 1)
                # (autograd's backward runs on another thread, and the names are per thread: direct calls name the kernels)
                TINCL._temporal_interlace_cl_forward(xs[0], w, s, T, 0, active)
                kernels = abi.last_kernel()
                TINCL._temporal_interlace_cl_backward(xs[0], w, s, xs[1], T, 0, active)
                kernels += " / " + abi.last_kernel()
                times = {}
                for r in range(a.repeats):
                    for tag, fn in (forms if r % 2 == 0 else forms[::-1]):
                        times.setdefault(tag, []).append(block(fn, iters[tag]))
                print(json.dumps({"line": li, "name": name, "shape": shape, "dtype": dt, "T": T, "table": table, "active": active, "sets": sets,
                                  "kernel": kernels, "ms": {tag: sum(t) / len(t) for tag, t in times.items()}, "peak": peak,
                                  "tensor_mib": nbytes / 2 ** 20}), flush=True)
                del xr, xcr, wr, sr, graphs, forms
        del xs, xc
        torch.cuda.empty_cache()


def parent():
    print("%d processes, each %d blocks of >= %.2f s per route; ms, median [min..max over the processes]" % (a.processes, a.repeats, a.seconds / a.repeats))
    runs = {}
    for p in range(a.processes):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--seconds", str(a.seconds), "--repeats", str(a.repeats),
               "--rotate-bytes", str(a.rotate_bytes), "--tables", a.tables] + (["--only", a.only] if a.only else [])
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            print(out.stdout[-2000:], out.stderr[-4000:])
            sys.exit("process %d failed (%d)" % (p, out.returncode))
        for l in out.stdout.splitlines():
            if l.startswith("{"):
                r = json.loads(l)
                runs.setdefault((r["line"], r["table"] != "layer", r["active"]), []).append(r)
    misses = 0
    for (li, full, active), rs in sorted(runs.items()):
        r0 = rs[0]
        print("%s  %s %s T=%d  %s table, %s  (%d operand sets; (n) ran %s)"
              % (r0["name"], tuple(r0["shape"]), r0["dtype"], r0["T"], r0["table"], "active" if active else "sparse", r0["sets"], r0["kernel"]))
        stat = {}
        for tag in ROUTES:
            v = [r["ms"][tag] for r in rs]
            stat[tag] = (statistics.median(v), min(v), max(v))
        for word in ("fwd", "bwd"):
            print("  %s ms  " % word + "   ".join("(%s) %.4f [%.4f..%.4f]" % ((t,) + stat[t + " " + word]) for t in TAGS))
            sn = stat["n " + word]
            for other in "ab":
                so = stat[other + " " + word]
                spread = (sn[2] - sn[1]) + (so[2] - so[1])
                gain = so[0] - sn[0]
                holds = gain > spread
                misses += (not holds) and not full
                print("    %s: (%s) - (n) = %+.4f ms against spreads of %.4f: %s; (n) / (%s) = %.3f"
                      % ("reported, not gated" if full else "the bar", other, gain, spread, "holds" if holds else "DOES NOT HOLD", other, sn[0] / so[0]))
            print("    (n) / (c) = %.3f, (n) / (d) = %.3f" % (sn[0] / stat["c " + word][0], sn[0] / stat["d " + word][0]))
        pn, pa, pb = (statistics.median([r["peak"][t] for r in rs]) for t in "nab")
        misses += (not pn < pb) and not full
        print("  peak memory of one training step above its inputs, MiB: (n) %.0f  (a) %.0f  (b) %.0f  (the tensor: %.0f): %s"
              % (pn, pa, pb, r0["tensor_mib"], "below (b)" if pn < pb else "NOT BELOW (b)"))
    print("the bar under the layer's tables: %s" % ("met in every line" if misses == 0 else "%d misses" % misses))


if __name__ == "__main__":
    child() if a.child else parent()
