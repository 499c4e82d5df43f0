#!/usr/bin/env python3
"""Mixed precision (fp32 shift weights with fp16 / bf16 tensors) through the public op, on the GPU box.

    python tools/amp_bench.py [--out profiles/amp_bench.txt] [--iters 20] [--rounds 9] [--small]

One training step (forward + backward through autograd) of BASELINE config 3's tensor (bf16, interpolating) and of config 5's
per-GPU tensor (fp16, sparse), in two forms -- the plain op, and the cropped + pooled form a Shift{N}d(emulate_dw = {kernel 3,
stride 2, padding 0}) runs (cut 1 / 1 per dim, average pool 2) -- each with three kinds of weights:

    w16         16-bit weights: the yardstick (what every 16-bit workload of this project measured so far)
    w32         fp32 weights (SHIFTND_WEIGHTS_F32): the same kernels, the table read as fp32, grad_w stored as fp32
    w32.to(dt)  fp32 parameter cast to the tensors' type inside the step: the workaround that was needed before -- a cast kernel in
                the forward, one more in the backward, shifts and gradient rounded to 16 bits

The variants run interleaved in one process (round r times every variant once, `iters` steps between two device events), so that
whatever else the host does meets all of them alike.  Reported: the median and the range of the rounds per variant, the ratio of
each median to w16's, w16's own spread (max / min of its rounds: a ratio inside it is no difference), and the kernels one step
launches (torch.profiler; "not measured" when the profiler is not available).
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "activesparseshifts-pytorch_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import torchshifts  # noqa: E402,F401  (registers the ops)

OPS = torch.ops.torchshifts
DEV = "cuda:0"

# name -> (shape, dtype, active): bench.py's WORKLOADS c3 and c5
TENSORS = {"c3": ((8, 128, 16, 112, 112), torch.bfloat16, True), "c5": ((64, 512, 224, 224), torch.float16, False)}
SMALL = {"c3": ((2, 16, 8, 56, 56), torch.bfloat16, True), "c5": ((2, 16, 112, 112), torch.float16, False)}   # --small: a rehearsal


def make_steps(shape, tdt, active, pooled, kinds):
    """-> {kind: step}.  The variants share the input and the incoming gradient -- one allocation each, so that the placement of a
    6 GB tensor in memory is the same for all of them -- and differ in the weights alone."""
    nd = len(shape) - 2
    torch.manual_seed(0)
    x = torch.rand(shape, device=DEV).to(tdt).requires_grad_(True)
    w32 = ((torch.rand(shape[1], nd, device=DEV) * 2 - 1) * 2.5)
    if pooled:
        op, cut = getattr(OPS, "shift%dd_pool" % nd), torch.tensor([[1, 1]] * nd, dtype=torch.long)
        call = lambda wt: op(x, wt, cut, [2] * nd, 0, active)   # noqa: E731
    else:
        op, cut = getattr(OPS, "shift%dd" % nd), torch.Tensor()
        call = lambda wt: op(x, wt, cut, 0, active)   # noqa: E731
    with torch.no_grad():
        go = torch.rand_like(call(w32.to(tdt)))

    def make(kind):
        w = (w32.to(tdt) if kind == "w16" else w32.clone()).requires_grad_(True)

        def step():
            x.grad = w.grad = None
            out = call(w.to(tdt) if kind == "w32.to(dt)" else w)
            out.backward(go)
            return w.grad

        return step

    return {k: make(k) for k in kinds}


def ev_time(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def kernels_of(step):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name]
        return len(names)
    except Exception as e:   # noqa: BLE001
        return "not measured (%s)" % type(e).__name__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--small", action="store_true", help="small tensors (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/amp_bench.py measures on the GPU"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("# tools/amp_bench.py: %s, torch %s, %d rounds x %d steps per variant, interleaved%s"
        % (torch.cuda.get_device_name(0), torch.__version__, a.rounds, a.iters, " (SMALL tensors: a rehearsal)" if a.small else ""))
    kinds = ("w16", "w32", "w32.to(dt)")
    for name, (shape, tdt, active) in (SMALL if a.small else TENSORS).items():
        for pooled in (False, True):
            steps = make_steps(shape, tdt, active, pooled, kinds)
            grads = {}
            for k, fn in steps.items():   # warm-up: code objects, the allocator's pool
                for _ in range(3):
                    grads[k] = fn()
            torch.cuda.synchronize()
            times = {k: [] for k in kinds}
            for _ in range(a.rounds):
                for k, fn in steps.items():
                    times[k].append(ev_time(fn, a.iters))
            launches = {k: kernels_of(fn) for k, fn in steps.items()}
            say()
            say("%s %s %s %s, %s" % (name, "x".join(map(str, shape)), str(tdt).replace("torch.", ""), "interpolating" if active else "sparse",
                                     "cut 1/1 + avg pool 2 (emulate_dw k3 s2 p0)" if pooled else "plain op"))
            base = statistics.median(times["w16"])
            say("  w16's own spread over the rounds: max / min = %.3f" % (max(times["w16"]) / min(times["w16"])))
            for k in kinds:
                t = times[k]
                say("  %-11s median %8.4f ms  (min %8.4f, max %8.4f)  ratio to w16 %.3f  kernels per step: %s  weight.grad %s"
                    % (k, statistics.median(t), min(t), max(t), statistics.median(t) / base, launches[k], str(grads[k].dtype).replace("torch.", "")))
            del steps, grads
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
