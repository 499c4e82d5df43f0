#!/usr/bin/env python3
"""The per-clip temporal shift ([N, C] table) of [N*T, C, H, W] tensors, forward and backward, device-event times (GPU box):
    python3 tools/per_clip_bench.py [--processes 3] [--seconds 0.3] [--repeats 4] [--parent-lib variants/parent.so]
Routes, alternated block by block in one process (each figure the mean of `repeats` blocks that together run at least `seconds`);
the whole table is taken in `processes` fresh processes one after the other, and what is printed is the mean over the processes with
min..max of the per-process figures, the run-to-run spread:
  (p) torch.ops.torchshifts_per_clip._temporal_shift_learnable_per_clip_forward under a [N, C] table; backward: autograd's
      (torch.autograd.grad on a graph built outside the timed region)
  (c) torch.ops.torchshifts._temporal_shift_learnable_forward under a [C] table on the same tensors, backward in the same way: the
      same kernels moving the same bytes -- measurement 1, (p) / (c)
  (l) today's idiom for a per-clip table: the loop over the N clips of temporal_shift_learnable on slices + cat, backward autograd's
      through the N nodes and the cat -- measurement 2, (l) / (p)
  (n) / (o) with --parent-lib: the PER-CHANNEL flagged C-ABI call (SHIFTND_SHIFT_DIM0, [C] table) through this tree's library and
      through the parent commit's, same tensors, same process, the order of the two swapped from block to block (n o, o n, ...) so
      that neither always runs behind the other -- measurement 3, (n) / (o)
Both modes, zeros padding, weights uniform in [-1.5, 1.5] (every row of the per-clip table drawn on its own).  Every tensor is one of
several sets rotated call by call, so that no route finds its operands in the last-level cache."""
import argparse
import ctypes
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
ROUTES = ["p fwd", "c fwd", "l fwd", "n fwd", "o fwd", "p bwd", "c bwd", "l bwd", "n bwd", "o bwd"]

ap = argparse.ArgumentParser()
ap.add_argument("--processes", type=int, default=3)
ap.add_argument("--seconds", type=float, default=0.3)
ap.add_argument("--repeats", type=int, default=4)
ap.add_argument("--only", default=None, help="comma-separated line numbers (0-based)")
ap.add_argument("--rotate-bytes", type=float, default=1.0e9, help="operand sets are added until they hold this many bytes")
ap.add_argument("--parent-lib", default="", help="the parent commit's libshiftnd_hip.so: adds routes (n) and (o)")
ap.add_argument("--ab-only", action="store_true", help="measurement 3 alone: routes (n) and (o)")
ap.add_argument("--child", action="store_true", help="(internal) one process's table as JSON lines")
a = ap.parse_args()


def child():
    import torch
    from torchshifts import abi

    OPS, PC = torch.ops.torchshifts, torch.ops.torchshifts_per_clip
    libs = {"n": abi.lib()}
    if a.parent_lib:
        abi._LIB_PATH, abi._lib = os.path.abspath(a.parent_lib), None
        libs["o"] = abi.lib()
        assert libs["o"]._name != libs["n"]._name
        abi._lib = libs["n"]

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
        N, M = NT // T, H * W
        nbytes = math.prod(shape) * ES[dt]
        sets = max(2, int(a.rotate_bytes / (2 * nbytes)) + 1)
        torch.manual_seed(li)
        wc = (torch.rand(C, device="cuda") * 3 - 1.5).to(tdt)
        wp = (torch.rand(N, C, device="cuda") * 3 - 1.5).to(tdt)
        xs = [torch.rand(shape, device="cuda").to(tdt) for _ in range(sets)]
        outs = [torch.empty_like(xs[0]) for _ in range(sets)]
        gw = torch.empty_like(wc)
        turn = [0]

        def nxt():
            turn[0] += 1
            return turn[0]

        def seg(t):   # [N*T, C, H, W] -> the [N, C, T, M] problem the library sees, no copy
            return t.view(N, T, C, M).transpose(1, 2)

        ws = abi.backward_workspace(seg(xs[0]), 0, 1, shift_dim0=True)

        def loop(x, w, active):
            return torch.cat([OPS.temporal_shift_learnable(x[n * T:(n + 1) * T], w[n], T, 0, active) for n in range(N)], 0)

        for active in (False, True):
            xr = [x.clone().requires_grad_(True) for x in xs[:0 if a.ab_only else 2]]
            wpr, wcr = wp.clone().requires_grad_(True), wc.clone().requires_grad_(True)
            graphs = {"p": [PC.temporal_shift_learnable_per_clip(x, wpr, T, 0, active) for x in xr],
                      "c": [OPS.temporal_shift_learnable(x, wcr, T, 0, active) for x in xr],
                      "l": [loop(x, wpr, active) for x in xr]}
            if not a.ab_only:   # the per-clip op returns the loop's tensors, bit for bit
                assert torch.equal(graphs["p"][0], graphs["l"][0])
                gp = torch.autograd.grad(graphs["p"][0], (xr[0], wpr), xs[1], retain_graph=True)
                gl = torch.autograd.grad(graphs["l"][0], (xr[0], wpr), xs[1], retain_graph=True)
                assert torch.equal(gp[0], gl[0])
                assert float((gp[1].float() - gl[1].float()).abs().max()) <= 1e-2 * float(gl[1].float().abs().max())
                del gp, gl

            def backward_of(tag, w):
                def fn():
                    i = nxt()
                    return torch.autograd.grad(graphs[tag][i % 2], (xr[i % 2], w), xs[i % sets], retain_graph=True)
                return fn

            def abi_forward(tag):
                def fn():
                    abi._lib = libs[tag]
                    i = nxt()
                    return abi.forward(seg(xs[i % sets]), wc, 0, active, out=seg(outs[i % sets]), shift_dim0=True)
                return fn

            def abi_backward(tag):
                def fn():
                    abi._lib = libs[tag]
                    i = nxt()
                    return abi.backward(seg(xs[i % sets]), wc, seg(xs[(i + 1) % sets]), 0, active, grad_x=seg(outs[i % sets]), grad_w=gw,
                                        workspace=ws, shift_dim0=True)
                return fn

            forms = [("p fwd", lambda: PC._temporal_shift_learnable_per_clip_forward(xs[nxt() % sets], wp, T, 0, active)),
                     ("c fwd", lambda: OPS._temporal_shift_learnable_forward(xs[nxt() % sets], wc, T, 0, active)),
                     ("l fwd", lambda: loop(xs[nxt() % sets], wp, active)),
                     ("p bwd", backward_of("p", wpr)), ("c bwd", backward_of("c", wcr)), ("l bwd", backward_of("l", wpr))]
            if a.ab_only:
                forms = []
            pairs = []
            if a.parent_lib:
                pairs = [[("n fwd", abi_forward("n")), ("o fwd", abi_forward("o"))], [("n bwd", abi_backward("n")), ("o bwd", abi_backward("o"))]]
                # the two libraries return the same bits on the per-channel call
                res = {}
                for tag in ("n", "o"):
                    abi._lib = libs[tag]
                    abi.forward(seg(xs[0]), wc, 0, active, out=seg(outs[0]), shift_dim0=True)
                    abi.backward(seg(xs[0]), wc, seg(xs[1]), 0, active, grad_x=seg(outs[1]), grad_w=gw, workspace=ws, shift_dim0=True)
                    res[tag] = (outs[0].clone(), outs[1].clone(), gw.clone())
                assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(res["n"], res["o"])), "parent and tree differ"
                del res
                abi._lib = libs["n"]
            kernels, iters = {}, {}
            for tag, fn in forms + [f for pair in pairs for f in pair]:
                for _ in range(2):
                    fn()
                kernels[tag] = abi.last_kernel()
                iters[tag] = max(3, int(a.seconds / a.repeats / (block(fn, 3) * 1e-3)) + 1)
            abi._lib = libs["n"]
            # (autograd's backward runs on another thread, and the names are per thread: one direct call names (p)'s kernel)
            PC._temporal_shift_learnable_per_clip_backward(xs[0], wp, xs[1], T, 0, active)
            kernels["p bwd"] = abi.last_kernel()
            times = {}
            for r in range(a.repeats):
                for tag, fn in forms:
                    times.setdefault(tag, []).append(block(fn, iters[tag]))
                for pair in pairs:
                    for tag, fn in (pair if r % 2 == 0 else pair[::-1]):
                        times.setdefault(tag, []).append(block(fn, iters[tag]))
            abi._lib = libs["n"]
            print(json.dumps({"line": li, "name": name, "shape": shape, "dtype": dt, "T": T, "active": active, "sets": sets,
                              "kernel": kernels.get("p fwd", kernels.get("n fwd")) + " / " + kernels["p bwd"], "ms": {tag: sum(t) / len(t) for tag, t in times.items()}}), flush=True)
            del xr, wpr, wcr, graphs, forms
        del xs, outs
        torch.cuda.empty_cache()


def parent():
    print("%d processes, each %d blocks of >= %.2f s per route; ms, mean [min..max over the processes]" % (a.processes, a.repeats, a.seconds / a.repeats))
    runs = {}
    for p in range(a.processes):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--seconds", str(a.seconds), "--repeats", str(a.repeats),
               "--rotate-bytes", str(a.rotate_bytes)] + (["--only", a.only] if a.only else []) + (["--parent-lib", a.parent_lib] if a.parent_lib else []) + (["--ab-only"] if a.ab_only else [])
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
        print("%s  %s %s T=%d  %s  (%d operand sets; (p) ran %s)" % (r0["name"], tuple(r0["shape"]), r0["dtype"], r0["T"],
                                                                           "active" if active else "sparse", r0["sets"], r0["kernel"]))
        stat = {}
        for tag in ROUTES:
            if tag in r0["ms"]:
                v = [r["ms"][tag] for r in rs]
                stat[tag] = (sum(v) / len(v), min(v), max(v))
        for word in ("fwd", "bwd"):
            tags = [t for t in ROUTES if t.endswith(word) and t in stat]
            print("  %s ms  " % word + "   ".join("(%s) %.4f [%.4f..%.4f]" % ((t[0],) + stat[t]) for t in tags))

            def versus(x, y, text, want_faster):
                sx, sy = stat[x + " " + word], stat[y + " " + word]
                spread = (sx[2] - sx[1]) + (sy[2] - sy[1])
                diff = sx[0] - sy[0]
                verdict = ("within the spread" if abs(diff) <= spread else "(%s) slower BEYOND the spread" % x[0] if diff > 0
                           else "(%s) faster beyond the spread" % x[0])
                if want_faster:
                    verdict = "holds" if -diff > spread else "DOES NOT HOLD"
                print("    %s: (%s) / (%s) = %.3f, (%s) - (%s) = %+.4f ms against spreads of %.4f: %s"
                      % (text, x, y, sx[0] / sy[0], x, y, diff, spread, verdict))

            if "p " + word in stat:
                versus("p", "c", "1. per-clip against per-channel", False)
                versus("p", "l", "2. per-clip against the loop + cat", True)
            if "n " + word in stat:
                versus("n", "o", "3. per-channel call, this tree against the parent", False)


if __name__ == "__main__":
    child() if a.child else parent()
