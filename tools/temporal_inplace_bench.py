#!/usr/bin/env python3
"""The IN-PLACE temporal shift (TSM) against the out-of-place op of the same layout, forward, device-event times (GPU box):
    python3 tools/temporal_inplace_bench.py [--processes 3] [--seconds 0.3] [--repeats 3]
Every line of the README's temporal shapes, zeros padding, in the contiguous and in the channels-last layout.  Routes, alternated
block by block inside one process (a figure is the mean of `repeats` blocks that together run at least `seconds`, after two warm-up
calls per route); the whole table is taken in `processes` fresh processes one after the other, and what is printed is the mean over
the processes with min..max of the per-process figures, the run-to-run spread:
  (i)  temporal_shift_func_ / temporal_shift_quantized_ under the published table (fold_div 8): csrc/shiftnd_inplace.hip
  (o)  the out-of-place op of the same layout under the same table: temporal_shift on the contiguous tensor (shiftnd_segment.hip),
       temporal_shift_cl on the channels-last one (shiftnd_frames.hip); the quantized pair for quint8
  (c)  the PyTorch slicing idiom of the published module, on a clone of the same layout
  (ir) the in-place op under a dense random table in [-2, 2]: four fifths of the channels move, channels-last pieces are mixed
  (or) the out-of-place op under that table
Every tensor is one of several sets that are rotated call by call, so that no route finds its operands in the 256 MB last-level
cache.  The byte model of (i): one read of every (frame, channel) that moves and is not filled, one write of every one that moves
-- about 2 * (shifted channels / C) of the tensor -- against what (o) moves, one read of every channel that is not filled and one
write of every channel.  GB/s = the model's bytes over the time; "of copy" = that rate over this box's plain 1-read-1-write stream
(tools/stream_probe on tensors of the largest line's size, a child process that has exited before any other touches the GPU)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "activesparseshifts-pytorch_amd"))

LINES = [("56x56 fp16", (256, 256, 56, 56), "float16", 8), ("56x56 fp16", (256, 256, 56, 56), "float16", 16),
         ("56x56 fp32", (128, 256, 56, 56), "float32", 16),
         ("14x14 bf16", (256, 1024, 14, 14), "bfloat16", 8), ("14x14 bf16", (256, 1024, 14, 14), "bfloat16", 16),
         ("7x7 fp16", (512, 2048, 7, 7), "float16", 8), ("7x7 fp16", (512, 2048, 7, 7), "float16", 16),
         ("56x56 quint8", (256, 256, 56, 56), "quint8", 8), ("56x56 quint8", (256, 256, 56, 56), "quint8", 16)]
ES = {"float16": 2, "bfloat16": 2, "float32": 4, "quint8": 1}
ROUTES = ("i", "o", "c", "ir", "or")

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=0.3)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--processes", type=int, default=3)
ap.add_argument("--only", default=None, help="comma-separated line numbers (0-based)")
ap.add_argument("--rotate-bytes", type=float, default=1.0e9, help="operand sets are added until they hold this many bytes")
ap.add_argument("--child", action="store_true", help="(internal) one process's table as JSON lines")
a = ap.parse_args()


def numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def probe(nbytes):
    try:
        out = subprocess.run([os.path.join(ROOT, "tools", "stream_probe"), "--bytes", str(int(nbytes))], capture_output=True,
                             text=True, timeout=300)
        return float(json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])["1R1W_GBps"])
    except Exception as e:  # noqa: BLE001
        print("stream_probe unavailable: %r" % (e,))
        return float("nan")


def model_bytes(table, N, T, M, es, in_place):
    """zeros padding: a channel with shift s reads T - min(|s|, T) frames; in place only the channels with s != 0 are touched"""
    read = sum(T - min(abs(v), T) for v in table if v != 0 or not in_place)
    written = sum(T for v in table if v != 0 or not in_place)
    return N * M * es * (read + written)


def child():
    import torch
    from torchshifts import abi
    from torchshifts.functional import temporal_shift_func, temporal_shift_func_
    from torchshifts.quantized.functional import temporal_shift_quantized, temporal_shift_quantized_

    CL, KEEP = torch.channels_last, torch.preserve_format
    ZP, SCALE = 77, 0.05

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
        quantized = dt == "quint8"
        NT, C, H, W = shape
        N, M = NT // T, H * W
        nbytes = numel(shape) * ES[dt]
        sets = max(2, int(a.rotate_bytes / nbytes) + 1)
        f = C // 8
        published = torch.tensor([-1] * f + [1] * f + [0] * (C - 2 * f), device="cuda")
        random = torch.randint(-2, 3, (C,), generator=torch.Generator().manual_seed(li)).cuda()
        for layout in ("contiguous", "channels-last"):
            cl = layout == "channels-last"

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
                reprs = [torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda") for _ in range(sets)]
                if cl:
                    reprs = [r.contiguous(memory_format=CL) for r in reprs]
                    xs = [torch._make_per_tensor_quantized_tensor(r.permute(0, 2, 3, 1), SCALE, ZP).permute(0, 3, 1, 2) for r in reprs]
                else:
                    xs = [torch._make_per_tensor_quantized_tensor(r, SCALE, ZP) for r in reprs]
                fmt = KEEP if cl else torch.contiguous_format
                inplace, plain = temporal_shift_quantized_, (lambda x, s: temporal_shift_quantized(x, s, T, 0, fmt))
                clones = reprs
                want = plain(xs[0], random).int_repr()
                got = inplace(torch._make_per_tensor_quantized_tensor(xs[0].int_repr(), SCALE, ZP) if not cl else
                              torch._make_per_tensor_quantized_tensor(reprs[0].clone(memory_format=KEEP).permute(0, 2, 3, 1), SCALE, ZP).permute(0, 3, 1, 2),
                              random, T, 0).int_repr()
            else:
                tdt = getattr(torch, dt)
                xs = [torch.rand(shape, device="cuda").to(tdt) for _ in range(sets)]
                if cl:
                    xs = [x.contiguous(memory_format=CL) for x in xs]
                fmt = KEEP if cl else torch.contiguous_format
                inplace, plain = temporal_shift_func_, (lambda x, s: temporal_shift_func(x, s, T, 0, fmt))
                clones = xs
                want = plain(xs[0], random)
                got = inplace(xs[0].clone(memory_format=KEEP), random, T, 0)
            assert got.stride() == want.stride() and torch.equal(got, want), "the in-place op and the out-of-place op disagree"
            del got, want
            forms = [("i", lambda: inplace(pick(xs), published, T, 0)), ("o", lambda: plain(pick(xs), published)),
                     ("c", lambda: idiom(pick(clones))),
                     ("ir", lambda: inplace(pick(xs), random, T, 0)), ("or", lambda: plain(pick(xs), random))]
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
            row = {"line": li, "name": name, "shape": shape, "dtype": dt, "T": T, "layout": layout, "sets": sets,
                   "kernel_i": kernels["i"], "kernel_o": kernels["o"],
                   "ms": {tag: sum(t) / len(t) for (tag, _), t in zip(forms, times)},
                   "bytes": {"i": model_bytes(published.tolist(), N, T, M, ES[dt], True), "o": model_bytes(published.tolist(), N, T, M, ES[dt], False),
                             "ir": model_bytes(random.tolist(), N, T, M, ES[dt], True), "or": model_bytes(random.tolist(), N, T, M, ES[dt], False)}}
            print(json.dumps(row), flush=True)
            del xs, clones, forms
            if quantized:
                del reprs
            torch.cuda.empty_cache()


def parent():
    copy = probe(max(numel(shape) * ES[dt] for _, shape, dt, _ in LINES))
    print("copy stream of this box (1R1W): %.0f GB/s;  %d processes, each %d blocks of >= %.2f s per route" % (copy, a.processes, a.repeats, a.seconds / a.repeats))
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
                runs.setdefault((r["line"], r["layout"]), []).append(r)
    for (li, layout), rs in sorted(runs.items(), key=lambda kv: (kv[0][0], kv[0][1] != "contiguous")):
        r0 = rs[0]
        print("%s  %s %s T=%d %s  (%d operand sets; (i) %s, (o) %s)" % (r0["name"], tuple(r0["shape"]), r0["dtype"], r0["T"], layout, r0["sets"],
                                                                    r0["kernel_i"], r0["kernel_o"]))
        stat = {}
        for tag in ROUTES:
            v = [r["ms"][tag] for r in rs]
            stat[tag] = (sum(v) / len(v), min(v), max(v))
        print("  ms   " + "   ".join("(%s) %.4f [%.4f..%.4f]" % ((tag,) + stat[tag]) for tag in ROUTES))
        for i, o, word in (("i", "o", "published table"), ("ir", "or", "random table   ")):
            spread = (stat[i][2] - stat[i][1]) + (stat[o][2] - stat[o][1])
            rate_i, rate_o = r0["bytes"][i] / (stat[i][0] * 1e-3) / 1e9, r0["bytes"][o] / (stat[o][0] * 1e-3) / 1e9
            print("  %s: (%s) / (%s) = %.2f of the time (byte model %.2f), (%s) - (%s) = %+.4f ms against spreads of %.4f;   (%s): %.0f GB/s, %.2f of copy;"
                  "   (%s): %.0f GB/s, %.2f of copy" % (word, i, o, stat[i][0] / stat[o][0], r0["bytes"][i] / r0["bytes"][o], o, i, stat[o][0] - stat[i][0], spread,
                                                       i, rate_i, rate_i / copy, o, rate_o, rate_o / copy))


if __name__ == "__main__":
    child() if a.child else parent()
