#!/usr/bin/env python3
"""The quantized interpolating temporal shift of CHANNELS-LAST [N*T, C, H, W] tensors (torchshifts.quantized.functional.
temporal_shift_learnable_quantized(..., memory_format=torch.preserve_format), csrc/shiftnd_frames_quant.hip) against the other ways
to such a tensor, zeros padding, device-event times (GPU box):
    python3 tools/qtshift_cl_bench.py [--seconds 0.3] [--repeats 3] [--processes 3] [--out profiles/qtshift_cl_bench.txt]
Routes, alternated block by block inside each of `processes` fresh child processes (this process never opens the GPU); a figure is
the median over all blocks of all processes, min..max of the blocks is the run's own spread:
  (k) the new route on the channels-last tensor as it lies (one kernel, frames_forward_quantized), channels-last out
  (a) the route before it plus the layout change back: the default op on the channels-last tensor (a tile transpose of the int_repr,
      then tshift_forward_quantized, a contiguous result), then .contiguous(memory_format=torch.channels_last) on the result
  (b) temporal_shift_quantized(..., memory_format=torch.preserve_format) under the rounded table: the channels-last copy floor
  (c) the default op on contiguous copies (tshift_forward_quantized alone, contiguous in and out)
Tables: `group` -- uniform in [-1.5, 1.5], constant over 16 channels (uniform pieces); `[-1,1]` -- the module's initialisation (few
frames); `[-1.5,1.5]` -- DESIGN 3.40's table; `[-T,T]` (many frames).  The share of (piece, frame) pairs on each of the kernel's three
paths is printed per table: the path rule of csrc/shiftnd_frames_quant.hip (K = 6 slots) restated on the CPU.
Every tensor is one of several sets rotated call by call (more than 1 GB together), so that no route finds its operands in the
last-level cache.  Peak memory: torch.cuda.max_memory_allocated over one call, above what was allocated before it.  "of copy": one
read and one write of the tensor's bytes over (k), over the same box's plain 1-read-1-write stream (tools/stream_probe, a child
process that has exited before any other touches the GPU).  The bar: on the two 56 x 56 tensors under the first three tables (k) is
faster than (a) by more than the run's own spread (max - min of the blocks of either route), and the peak of (k) is the output alone;
everything else is reported as it comes."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "activesparseshifts-pytorch_amd"))

LINES = [("56x56 quint8 T=8", (256, 256, 56, 56), "quint8", 8, True),
         ("56x56 qint8 T=16", (128, 256, 56, 56), "qint8", 16, True),
         ("14x14 quint8", (256, 1024, 14, 14), "quint8", 8, False),
         ("7x7 quint8", (512, 2048, 7, 7), "quint8", 8, False)]
TABLES = ["group", "[-1,1]", "[-1.5,1.5]", "[-T,T]"]
BARRED = TABLES[:3]
FORMS = ["k", "a", "b", "c"]
SCALE, ZP = 0.0625, {"quint8": 7, "qint8": -3}
SLOTS = 6

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=0.3)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--processes", type=int, default=3)
ap.add_argument("--rotate-bytes", type=float, default=1.0e9, help="operand sets are added until they hold this many bytes")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qtshift_cl_bench.txt"))
ap.add_argument("--child", action="store_true", help="(internal) one measuring process: prints one JSON line")
a = ap.parse_args()


def table(kind, C, T, seed):
    rs = np.random.RandomState(seed)
    if kind == "group":
        return np.repeat(rs.uniform(-1.5, 1.5, size=C // 16), 16).astype(np.float32)
    r = {"[-1,1]": 1.0, "[-1.5,1.5]": 1.5, "[-T,T]": float(T)}[kind]
    return rs.uniform(-r, r, size=C).astype(np.float32)


def path_shares(w, T, E=16):
    """share of (piece, frame) pairs on the uniform / few-frames / many-frames path, zeros padding"""
    floor = np.floor(w).astype(np.int64)
    whole = w == np.floor(w)
    count = {"uniform": 0, "few": 0, "many": 0}
    for k in range(len(w) // E):
        f, wh = floor[k * E:(k + 1) * E], whole[k * E:(k + 1) * E]
        for t in range(T):
            s0, s1 = t - f, t + 1 - f
            s0, s1 = np.where((s0 < 0) | (s0 >= T), -1, s0), np.where((s1 < 0) | (s1 >= T), -1, s1)
            if T == 1:
                s0, s1 = np.zeros_like(s0), np.zeros_like(s1)
            if (s0 == s0[0]).all() and (s1 == s1[0]).all():
                count["uniform"] += 1
            else:
                slots = set(s0.tolist()) | set(np.where(wh, s0, s1).tolist())
                count["few" if len(slots) <= SLOTS else "many"] += 1
    total = float(sum(count.values()))
    return {k: v / total for k, v in count.items()}


def child():
    import torch
    from torchshifts import abi
    from torchshifts.quantized.functional import temporal_shift_learnable_quantized, temporal_shift_quantized

    def block(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    def peak(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    direct = [True]   # .contiguous(memory_format=) of a quantized HIP tensor; where ATen refuses it, the same copy of the int_repr

    def back_to_channels_last(y):
        if direct[0]:
            try:
                return y.contiguous(memory_format=torch.channels_last)
            except RuntimeError:
                direct[0] = False
        return torch._make_per_tensor_quantized_tensor(y.int_repr().contiguous(memory_format=torch.channels_last), y.q_scale(), y.q_zero_point())

    result = []
    for li, (name, shape, qname, T, barred) in enumerate(LINES):
        qdt, idt = getattr(torch, qname), {"quint8": torch.uint8, "qint8": torch.int8}[qname]
        nbytes = math.prod(shape)
        sets = max(2, int(a.rotate_bytes / (2 * nbytes)) + 1)
        torch.manual_seed(li)
        NT, C, H, W = shape
        lo = 0 if qname == "quint8" else -128
        # memory order (N*T, H, W, C), seen as [N*T, C, H, W]; and contiguous copies of the same values for (c)
        xs = [torch._make_per_tensor_quantized_tensor(torch.randint(lo, lo + 256, (NT, H, W, C), device="cuda", dtype=torch.int16).to(idt),
                                                      SCALE, ZP[qname]).permute(0, 3, 1, 2) for _ in range(sets)]
        cs = [torch._make_per_tensor_quantized_tensor(x.int_repr().contiguous(), SCALE, ZP[qname]) for x in xs]
        assert all(x.stride(1) == 1 and not x.is_contiguous() for x in xs) and all(c.is_contiguous() for c in cs)
        turn = [0]

        def pick(lst):
            turn[0] += 1
            return lst[turn[0] % len(lst)]

        for ti, kind in enumerate(TABLES):
            w = torch.from_numpy(table(kind, C, T, 100 * li + ti)).cuda().view(C, 1)
            forms = {"k": lambda: temporal_shift_learnable_quantized(pick(xs), w, T, 0, True, memory_format=torch.preserve_format),
                     "a": lambda: back_to_channels_last(temporal_shift_learnable_quantized(pick(xs), w, T, 0, True)),
                     "b": lambda: temporal_shift_quantized(pick(xs), w, T, 0, memory_format=torch.preserve_format),
                     "c": lambda: temporal_shift_learnable_quantized(pick(cs), w, T, 0, True)}
            got = temporal_shift_learnable_quantized(xs[0], w, T, 0, True, memory_format=torch.preserve_format)
            kernel = abi.last_kernel()
            via = back_to_channels_last(temporal_shift_learnable_quantized(xs[0], w, T, 0, True))
            assert got.stride() == xs[0].stride() == via.stride(), (got.stride(), via.stride())
            assert torch.equal(got.int_repr(), via.int_repr())   # (k) and (a): the same tensor
            assert torch.equal(got.int_repr(), temporal_shift_learnable_quantized(cs[0], w, T, 0, True).int_repr())   # ... and (c)'s values
            del got, via
            peaks = {f: peak(forms[f]) for f in ("k", "a")}
            iters = {}
            for f in FORMS:
                for _ in range(2):
                    forms[f]()
                iters[f] = max(3, int(a.seconds / a.repeats / (block(forms[f], 3) * 1e-3)) + 1)
            times = {f: [] for f in FORMS}
            for _ in range(a.repeats):
                for f in FORMS:
                    times[f].append(block(forms[f], iters[f]))
            result.append({"line": li, "table": kind, "kernel": kernel, "sets": sets, "times": times, "peaks": peaks, "direct": direct[0]})
        del xs, cs
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(result))


def probe(nbytes):
    try:
        out = subprocess.run([os.path.join(ROOT, "tools", "stream_probe"), "--bytes", str(int(nbytes))], capture_output=True,
                             text=True, timeout=300)
        return float(json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])["1R1W_GBps"])
    except Exception as e:  # noqa: BLE001
        print("stream_probe unavailable: %r" % (e,))
        return float("nan")


def main():
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    copy = probe(max(math.prod(shape) for _, shape, _, _, _ in LINES))
    say("copy stream of this box (1R1W): %.0f GB/s" % copy)
    runs = []
    for _ in range(a.processes):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--seconds", str(a.seconds), "--repeats", str(a.repeats),
                              "--rotate-bytes", str(a.rotate_bytes)], capture_output=True, text=True, timeout=1100)
        if out.returncode != 0:
            sys.exit("a measuring process failed (%d):\n%s\n%s" % (out.returncode, out.stdout[-2000:], out.stderr[-4000:]))
        runs.append(json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
    missed = []
    for li, (name, shape, qname, T, barred) in enumerate(LINES):
        nbytes = math.prod(shape)
        for ti, kind in enumerate(TABLES):
            recs = [[r for r in run if r["line"] == li and r["table"] == kind][0] for run in runs]
            share = path_shares(table(kind, shape[1], T, 100 * li + ti), T)
            t = {f: [v for r in recs for v in r["times"][f]] for f in FORMS}
            med = {f: statistics.median(t[f]) for f in FORMS}
            say("%s %s, table %s  (%d processes x %d blocks, %d operand sets; (k) ran %s; pieces: %.0f %% uniform, %.0f %% few frames, "
                "%.0f %% many frames)" % (name, shape, kind, len(recs), a.repeats, recs[0]["sets"], recs[0]["kernel"],
                                          100 * share["uniform"], 100 * share["few"], 100 * share["many"]))
            say("  forward ms  " + "   ".join("(%s) %.4f [%.4f..%.4f]" % (f, med[f], min(t[f]), max(t[f])) for f in FORMS))
            spread = max(max(t[f]) - min(t[f]) for f in ("k", "a"))
            margin = med["a"] - med["k"]
            has_bar = barred and kind in BARRED
            verdict = "holds" if margin > spread else ("DOES NOT HOLD" if has_bar else "loses" if margin <= 0 else "within the spread")
            if has_bar and margin <= spread:
                missed.append("%s, table %s" % (name, kind))
            say("  (a) / (k) = %.2f, margin %.4f ms against a spread of %.4f: %s%s" % (med["a"] / med["k"], margin, spread, verdict,
                                                                                       "" if has_bar else " (no bar)"))
            gbs = 2 * nbytes / (med["k"] * 1e-3) / 1e9
            say("  (k) / (b) = %.2f   (k) / (c) = %.2f   (k) 1R1W: %.0f GB/s, %.2f of copy" % (med["k"] / med["b"], med["k"] / med["c"], gbs, gbs / copy))
            pk, pa = max(r["peaks"]["k"] for r in recs), max(r["peaks"]["a"] for r in recs)
            say("  peak memory above the operands: (k) %.0f MiB   (a) %.0f MiB   (the tensor: %.0f MiB): (k) is %s"
                % (pk / 2 ** 20, pa / 2 ** 20, nbytes / 2 ** 20, "the output alone" if pk <= nbytes + 2 ** 20 else "MORE THAN THE OUTPUT"))
    if not all(r["direct"] for run in runs for r in run):
        say("(a)'s layout change ran on the int_repr: ATen refused .contiguous(memory_format=) on the quantized HIP tensor")
    say("bars missed: %s" % ("; ".join(missed) if missed else "none"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    child() if a.child else main()
