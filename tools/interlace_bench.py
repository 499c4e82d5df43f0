#!/usr/bin/env python3
"""Temporal interlacing (the per-clip shift times a [N, T, C] scale) of [N*T, C, H, W] tensors, forward and backward, device-event
times and the peak memory of one training step (GPU box):
    python3 tools/interlace_bench.py [--processes 3] [--seconds 0.3] [--repeats 4]
Routes, alternated block by block in one process (each figure the mean of `repeats` blocks that together run at least `seconds`);
the whole table is taken in `processes` fresh processes one after the other, and what is printed is the median over the processes
with min..max of the per-process figures, the run-to-run spread:
  (f) torch.ops.torchshifts_interlace.temporal_interlace, the fused op; backward: autograd's (torch.autograd.grad on a graph built
      outside the timed region)
  (a) the composition through the public ops: temporal_shift_learnable_per_clip(x, offsets) * scales.reshape(N*T, C, 1, 1), backward
      autograd's through the multiply and the per-clip node -- what a user pays today
  (b) the per-clip op alone on the same tensors, backward in the same way: the floor
The bar: (f) faster than (a) in every line by more than the run's own spread, and a lower peak.  Byte model: forward (f) / (a) = 1/2
(one read and one write against two of each), backward (f) / (b) = 1.
Peak memory: torch.cuda.max_memory_allocated over one forward + backward from a graph-free start, minus what was allocated before.
Both modes, zeros padding, offsets uniform in [-1.5, 1.5], scales in [0, 2] (TIN's range), every row drawn on its own.  Every tensor is
one of several sets rotated call by call, so that no route finds its operands in the last-level cache."""
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
         ("14x14 bf16 (ragged)", (256, 1024, 14, 14), "bfloat16", 8)]
ES = {"float16": 2, "bfloat16": 2, "float32": 4}
ROUTES = ["f fwd", "a fwd", "b fwd", "f bwd", "a bwd", "b bwd"]

ap = argparse.ArgumentParser()
ap.add_argument("--processes", type=int, default=3)
ap.add_argument("--seconds", type=float, default=0.3)
ap.add_argument("--repeats", type=int, default=4)
ap.add_argument("--only", default=None, help="comma-separated line numbers (0-based)")
ap.add_argument("--rotate-bytes", type=float, default=1.0e9, help="operand sets are added until they hold this many bytes")
ap.add_argument("--child", action="store_true", help="(internal) one process's table as JSON lines")
a = ap.parse_args()


def child():
    import torch
    from torchshifts import abi

    TIN, PC = torch.ops.torchshifts_interlace, torch.ops.torchshifts_per_clip

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
        w = (torch.rand(N, C, device="cuda") * 3 - 1.5).to(tdt)
        s = (torch.rand(N, T, C, device="cuda") * 2).to(tdt)
        xs = [torch.rand(shape, device="cuda").to(tdt) for _ in range(sets)]
        turn = [0]

        def nxt():
            turn[0] += 1
            return turn[0]

        def fused(x, w_, s_, active):
            return TIN.temporal_interlace(x, w_, s_, T, 0, active)

        def composed(x, w_, s_, active):
            return PC.temporal_shift_learnable_per_clip(x, w_, T, 0, active) * s_.reshape(NT, C, 1, 1)

        def alone(x, w_, s_, active):
            return PC.temporal_shift_learnable_per_clip(x, w_, T, 0, active)

        for active in (False, True):
            # one training step from a graph-free start: the peak above what is allocated already
            peak = {}
            for tag, fn in (("f", fused), ("a", composed)):
                xr, wr, sr = xs[0].clone().requires_grad_(True), w.clone().requires_grad_(True), s.clone().requires_grad_(True)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                fn(xr, wr, sr, active).backward(xs[1])
                torch.cuda.synchronize()
                peak[tag] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
                del xr, wr, sr
            xr = [x.clone().requires_grad_(True) for x in xs[:2]]
            wr, sr = w.clone().requires_grad_(True), s.clone().requires_grad_(True)
            graphs = {"f": [fused(x, wr, sr, active) for x in xr], "a": [composed(x, wr, sr, active) for x in xr],
                      "b": [alone(x, wr, sr, active) for x in xr]}
            assert graphs["f"][0].dtype == tdt
            if dt == "float32":   # the fused op returns the composition's bits
                assert torch.equal(graphs["f"][0], graphs["a"][0])
                gf = torch.autograd.grad(graphs["f"][0], (xr[0], wr, sr), xs[1], retain_graph=True)
                ga = torch.autograd.grad(graphs["a"][0], (xr[0], wr, sr), xs[1], retain_graph=True)
                assert torch.equal(gf[0], ga[0])
                del gf, ga

            def backward_of(tag):
                wrt = (wr,) if tag == "b" else (wr, sr)

                def fn():
                    i = nxt()
                    return torch.autograd.grad(graphs[tag][i % 2], (xr[i % 2],) + wrt, xs[i % sets], retain_graph=True)
                return fn

            def forward_of(route):
                def fn():
                    with torch.no_grad():
                        return route(xs[nxt() % sets], w, s, active)
                return fn

            forms = [("f fwd", forward_of(fused)), ("a fwd", forward_of(composed)), ("b fwd", forward_of(alone)),
                     ("f bwd", backward_of("f")), ("a bwd", backward_of("a")), ("b bwd", backward_of("b"))]
            iters = {}
            for tag, fn in forms:
                for _ in range(2):
                    fn()
                iters[tag] = max(3, int(a.seconds / a.repeats / (block(fn, 3) * 1e-3)) + 1)
            # (autograd's backward runs on another thread, and the names are per thread: direct calls name the kernels)
            TIN._temporal_interlace_forward(xs[0], w, s, T, 0, active)
            kernels = abi.last_kernel()
            TIN._temporal_interlace_backward(xs[0], w, s, xs[1], T, 0, active)
            kernels += " / " + abi.last_kernel()
            times = {}
            for r in range(a.repeats):
                for tag, fn in (forms if r % 2 == 0 else forms[::-1]):
                    times.setdefault(tag, []).append(block(fn, iters[tag]))
            print(json.dumps({"line": li, "name": name, "shape": shape, "dtype": dt, "T": T, "active": active, "sets": sets, "kernel": kernels,
                              "ms": {tag: sum(t) / len(t) for tag, t in times.items()}, "peak": peak, "tensor_mib": nbytes / 2 ** 20}), flush=True)
            del xr, wr, sr, graphs, forms
        del xs
        torch.cuda.empty_cache()


def parent():
    print("%d processes, each %d blocks of >= %.2f s per route; ms, median [min..max over the processes]" % (a.processes, a.repeats, a.seconds / a.repeats))
    runs = {}
    for p in range(a.processes):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--seconds", str(a.seconds), "--repeats", str(a.repeats),
               "--rotate-bytes", str(a.rotate_bytes)] + (["--only", a.only] if a.only else [])
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            print(out.stdout[-2000:], out.stderr[-4000:])
            sys.exit("process %d failed (%d)" % (p, out.returncode))
        for l in out.stdout.splitlines():
            if l.startswith("{"):
                r = json.loads(l)
                runs.setdefault((r["line"], r["active"]), []).append(r)
    for (li, active), rs in sorted(runs.items()):
        r0 = rs[0]
        print("%s  %s %s T=%d  %s  (%d operand sets; (f) ran %s)" % (r0["name"], tuple(r0["shape"]), r0["dtype"], r0["T"],
                                                                           "active" if active else "sparse", r0["sets"], r0["kernel"]))
        stat = {}
        for tag in ROUTES:
            v = [r["ms"][tag] for r in rs]
            stat[tag] = (statistics.median(v), min(v), max(v))
        for word in ("fwd", "bwd"):
            tags = [t for t in ROUTES if t.endswith(word)]
            print("  %s ms  " % word + "   ".join("(%s) %.4f [%.4f..%.4f]" % ((t[0],) + stat[t]) for t in tags))
            sf, sa, sb = stat["f " + word], stat["a " + word], stat["b " + word]
            spread = (sf[2] - sf[1]) + (sa[2] - sa[1])
            gain = sa[0] - sf[0]
            print("    the bar: (a) - (f) = %+.4f ms against spreads of %.4f: %s (%.1f x the spread)"
                  % (gain, spread, "holds" if gain > spread else "DOES NOT HOLD", gain / max(spread, 1e-9)))
            model = "1/2 of (a)" if word == "fwd" else "equal to (b)"
            print("    (f) / (a) = %.3f, (f) / (b) = %.3f  (byte model: %s)" % (sf[0] / sa[0], sf[0] / sb[0], model))
        pf, pa = (statistics.median([r["peak"][t] for r in rs]) for t in ("f", "a"))
        print("  peak memory of one training step above its inputs, MiB: (f) %.0f  (a) %.0f  (the tensor: %.0f): %s"
              % (pf, pa, r0["tensor_mib"], "lower" if pf < pa else "NOT LOWER"))


if __name__ == "__main__":
    child() if a.child else parent()
