#!/usr/bin/env python3
"""Quantized temporal interlacing of [N*T, C, H, W] tensors (torchshifts.quantized.functional.temporal_interlace_quantized,
csrc/shiftnd_interlace_quant.hip) against the other ways to such a tensor, zeros padding, under the TIN layer's own tables
(torchshifts.quantized.TemporalInterlace.tables of a freshly initialised layer, shift_div 1 and 4), device-event times (GPU box):
    python3 tools/qinterlace_bench.py [--seconds 0.3] [--repeats 3] [--processes 3]
Routes, alternated block by block inside each of `processes` fresh child processes (this process never opens the GPU); a figure is
the median over all blocks of all processes, min..max of the blocks is the run's own spread:
  (k) the new op (one kernel, tinterlace_forward_quantized, and the cat of the two small tables)
  (a) dequantize -> temporal_interlace_func (fp32) -> quantize_per_tensor: three kernels, two fp32 temporaries
  (b) temporal_shift_learnable_quantized under row 0 of the offsets: the floor (one table row, no scales; reported only)
Every tensor is one of several sets rotated call by call, so that no route finds its operands in the last-level cache; the tables
are formed once per line (every route needs them).  Peak memory: torch.cuda.max_memory_allocated over one call, above what was
allocated before it.  "1R1W" = one read and one write of the tensor's bytes over (k), and "of copy" that rate over the same box's
plain 1-read-1-write stream (tools/stream_probe, a child process that has exited before any other touches the GPU).  The bar: (k)
faster than (a) by more than the run's own spread on the 56 x 56 shapes, and a lower peak than (a); the ragged shapes are reported
as they come."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "activesparseshifts-pytorch_amd"))

SHAPES = [("56x56 quint8 T=8 (whole pieces)", (256, 256, 56, 56), "quint8", 8, True),
          ("56x56 qint8 T=16 (whole pieces)", (128, 256, 56, 56), "qint8", 16, True),
          ("14x14 quint8 (196-byte planes, 4-byte units)", (256, 1024, 14, 14), "quint8", 8, False),
          ("7x7 quint8 (49-byte planes, 1-byte units)", (512, 2048, 7, 7), "quint8", 8, False)]
LINES = [(name + ", shift_div=%d" % div, shape, qname, T, div, whole) for name, shape, qname, T, whole in SHAPES for div in (1, 4)]
FORMS = ["k", "a", "b"]
SCALE, ZP = 0.0625, {"quint8": 7, "qint8": -3}

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=0.3)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--processes", type=int, default=3)
ap.add_argument("--rotate-bytes", type=float, default=1.0e9, help="operand sets are added until they hold this many bytes")
ap.add_argument("--child", action="store_true", help="(internal) one measuring process: prints one JSON line")
a = ap.parse_args()


def child():
    import torch
    import torchshifts
    from torchshifts import abi
    from torchshifts.functional import temporal_interlace_func
    from torchshifts.quantized.functional import temporal_interlace_quantized, temporal_shift_learnable_quantized

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

    result = []
    for li, (name, shape, qname, T, div, whole) in enumerate(LINES):
        qdt, idt = getattr(torch, qname), {"quint8": torch.uint8, "qint8": torch.int8}[qname]
        nbytes = math.prod(shape)
        sets = max(2, int(a.rotate_bytes / (2 * nbytes)) + 1)
        torch.manual_seed(li)
        C = shape[1]
        lo = 0 if qname == "quint8" else -128
        xs = [torch._make_per_tensor_quantized_tensor(torch.randint(lo, lo + 256, shape, device="cuda", dtype=torch.int16).to(idt), SCALE, ZP[qname])
              for _ in range(sets)]
        # the layer's own tables: a freshly initialised TIN layer looking at the data (fractional offsets, a row of its own per clip;
        # a strongly perturbed layer saturates its sigmoids on this data: offsets of exactly +-2, which flatters the kernel)
        layer = torchshifts.TemporalInterlace(T, C, shift_div=div).eval()
        offsets, scales = torchshifts.quantized.TemporalInterlace.from_float(layer).cuda().tables(xs[0])
        row0 = offsets[0].contiguous()
        turn = [0]

        def pick(lst):
            turn[0] += 1
            return lst[turn[0] % len(lst)]

        def composite(x):
            return torch.quantize_per_tensor(temporal_interlace_func(x.dequantize(), offsets, scales, T, 0, True), SCALE, ZP[qname], qdt)

        forms = {"k": lambda: temporal_interlace_quantized(pick(xs), offsets, scales, T, 0, True),
                 "a": lambda: composite(pick(xs)),
                 "b": lambda: temporal_shift_learnable_quantized(pick(xs), row0, T, 0, True)}
        # a power-of-two scale: (k) and (a) round the same numbers up to the products' rounding (at most one level)
        got = temporal_interlace_quantized(xs[0], offsets, scales, T, 0, True)
        kernel = abi.last_kernel()
        diff = (got.int_repr().to(torch.int16) - composite(xs[0]).int_repr().to(torch.int16)).abs()
        assert int(diff.max()) <= 1, int(diff.max())
        differ = float((diff != 0).float().mean())
        del got, diff
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
        result.append({"line": li, "kernel": kernel, "sets": sets, "times": times, "peaks": peaks, "differ": differ,
                       "offsets": [float(offsets.min()), float(offsets.max())], "scales": [float(scales.min()), float(scales.max())]})
        del xs
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
    copy = probe(max(math.prod(line[1]) for line in LINES))
    print("copy stream of this box (1R1W): %.0f GB/s" % copy)
    runs = []
    for _ in range(a.processes):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--seconds", str(a.seconds), "--repeats", str(a.repeats),
                              "--rotate-bytes", str(a.rotate_bytes)], capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            sys.exit("a measuring process failed (%d):\n%s\n%s" % (out.returncode, out.stdout[-2000:], out.stderr[-4000:]))
        runs.append(json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
    for li, (name, shape, qname, T, div, whole) in enumerate(LINES):
        recs = [r[li] for r in runs]
        t = {f: [v for r in recs for v in r["times"][f]] for f in FORMS}
        med = {f: statistics.median(t[f]) for f in FORMS}
        nbytes = math.prod(shape)
        print("%s  %s T=%d  (%d processes x %d blocks, %d operand sets; (k) ran %s; offsets in [%.2f, %.2f], scales in [%.2f, %.2f]; "
              "%.2g of the elements differ from (a), by one level)"
              % (name, shape, T, len(recs), a.repeats, recs[0]["sets"], recs[0]["kernel"], recs[0]["offsets"][0], recs[0]["offsets"][1],
                 recs[0]["scales"][0], recs[0]["scales"][1], max(r["differ"] for r in recs)))
        print("  forward ms  " + "   ".join("(%s) %.4f [%.4f..%.4f]" % (f, med[f], min(t[f]), max(t[f])) for f in FORMS))
        spread = max(max(t[f]) - min(t[f]) for f in ("k", "a"))
        margin = med["a"] - med["k"]
        verdict = "holds" if margin > spread else ("DOES NOT HOLD" if whole else "loses" if margin <= 0 else "within the spread")
        print("  (a) / (k) = %.2f, margin %.4f ms against a spread of %.4f: %s%s" % (med["a"] / med["k"], margin, spread, verdict,
                                                                                   "" if whole else " (ragged: no bar)"))
        gbs = 2 * nbytes / (med["k"] * 1e-3) / 1e9
        print("  (k) / (b) = %.2f   (k) 1R1W: %.0f GB/s, %.2f of copy" % (med["k"] / med["b"], gbs, gbs / copy))
        pk, pa = max(r["peaks"]["k"] for r in recs), max(r["peaks"]["a"] for r in recs)
        print("  peak memory above the operands: (k) %.0f MiB   (a) %.0f MiB   (the tensor: %.0f MiB): %s"
              % (pk / 2 ** 20, pa / 2 ** 20, nbytes / 2 ** 20, "lower" if pk < pa else "NOT LOWER"))


if __name__ == "__main__":
    child() if a.child else main()
