#!/usr/bin/env python3
"""The ONLINE temporal shift against the slicing idiom of the TSM paper's demo, per step, device-event times (GPU box):
    python3 tools/temporal_online_bench.py [--processes 3] [--seconds 0.3] [--repeats 3]
Frames [B, C, H, W] under the default (uni-directional) table, fold_div 8: the first C // 8 channels show the previous frame.  Both
dense layouts.  Routes, alternated block by block inside one process (a figure is the mean of `repeats` blocks that together run at
least `seconds`, after two warm-up calls per route); the whole table is taken in `processes` fresh processes one after the other,
and what is printed is the mean over the processes with min..max of the per-process figures, the run-to-run spread:
  (i)  temporal_shift_online_func_ (temporal_shift_online_quantized_ for quint8) with the table in the kernel's kind, as
       OnlineTemporalShift(inplace=True) calls it: csrc/shiftnd_stream.hip, one launch, nothing allocated
  (o)  temporal_shift_online_func: the same on input.clone()
  (c)  the idiom:  out = torch.cat((buffer, x[:, f:]), 1); buffer = x[:, :f]   -- for quint8 on the int_repr.  It rewrites the whole
       frame and its buffer is a VIEW of the previous frame (no copy: that is one of its costs, the frame stays alive)
The frame of every call is one of several that are rotated call by call, as a video pipeline hands over a new tensor per frame; the
state is one tensor, as in use.  Byte model per step, in frame units (one frame = B * C * H * W * es bytes): (i) reads and writes the
shifted eighth in the frame and in the state, 4 / 8 = 0.5; (o) adds the clone, 2.5; (c) reads and writes the whole frame, 2.  At
B = 1 a frame is a few hundred KiB and every route is a launch or two: the figures there are launch overhead."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "activesparseshifts-pytorch_amd"))

LINES = [("56x56 fp16 B1", (1, 256, 56, 56), "float16"), ("56x56 fp16 B64", (64, 256, 56, 56), "float16"),
         ("14x14 bf16 B64", (64, 1024, 14, 14), "bfloat16"), ("56x56 quint8 B64", (64, 256, 56, 56), "quint8")]
ES = {"float16": 2, "bfloat16": 2, "quint8": 1}
ROUTES = ("i", "o", "c")

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=0.3)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--processes", type=int, default=3)
ap.add_argument("--only", default=None, help="comma-separated line numbers (0-based)")
ap.add_argument("--rotate-bytes", type=float, default=6.0e8, help="frames are added until they hold this many bytes (at most 64)")
ap.add_argument("--child", action="store_true", help="(internal) one process's table as JSON lines")
a = ap.parse_args()


def numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def child():
    import torch
    from torchshifts import abi
    from torchshifts.functional import (temporal_shift_online_func, temporal_shift_online_func_, temporal_shift_online_state,
                                        temporal_shift_online_table)
    from torchshifts.quantized.functional import temporal_shift_online_quantized, temporal_shift_online_quantized_

    ZP, SCALE = 77, 0.05

    def block(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    for li, (name, shape, dt) in enumerate(LINES):
        if a.only and str(li) not in a.only.split(","):
            continue
        quantized = dt == "quint8"
        B, C, H, W = shape
        f = C // 8
        nbytes = numel(shape) * ES[dt]
        sets = min(64, max(2, int(a.rotate_bytes / nbytes) + 1))
        shifts = torch.zeros(C, dtype=torch.int64, device="cuda")
        shifts[:f] = 1
        for layout in ("contiguous", "channels-last"):
            cl = layout == "channels-last"
            if quantized:
                plain = [torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda") for _ in range(sets)]
                if cl:
                    plain = [r.contiguous(memory_format=torch.channels_last) for r in plain]
                    xs = [torch._make_per_tensor_quantized_tensor(r.permute(0, 2, 3, 1), SCALE, ZP).permute(0, 3, 1, 2) for r in plain]
                else:
                    xs = [torch._make_per_tensor_quantized_tensor(r, SCALE, ZP) for r in plain]
                step_, step = temporal_shift_online_quantized_, temporal_shift_online_quantized
            else:
                xs = [torch.rand(shape, device="cuda").to(getattr(torch, dt)) for _ in range(sets)]
                if cl:
                    xs = [x.contiguous(memory_format=torch.channels_last) for x in xs]
                plain = xs
                step_, step = temporal_shift_online_func_, temporal_shift_online_func
            assert all(x.stride() == xs[0].stride() for x in xs)
            state = temporal_shift_online_state(xs[0], shifts, 0)
            table = temporal_shift_online_table(xs[0], shifts)
            buffer = [plain[0][:, :f]]
            turn = [0]

            def pick(lst):
                turn[0] += 1
                return lst[turn[0] % len(lst)]

            def idiom():
                x = pick(plain)
                out = torch.cat((buffer[0], x[:, f:]), 1)
                buffer[0] = x[:, :f]
                return out

            # the routes agree (two steps each from the same two frames): the op against the idiom
            a0, a1 = xs[0].clone(memory_format=torch.preserve_format), xs[1].clone(memory_format=torch.preserve_format)
            st = temporal_shift_online_state(a0, shifts, 0)
            step_(a0, st, table)
            got = step_(a1, st, table)
            want = torch.cat((plain[0][:, :f], plain[1][:, f:]), 1)
            assert torch.equal(got.int_repr() if quantized else got, want), "the online op and the idiom disagree"
            del a0, a1, st, got, want
            forms = [("i", lambda: step_(pick(xs), state, table)), ("o", lambda: step(pick(xs), state, table)), ("c", idiom)]
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
            row = {"line": li, "name": name, "shape": shape, "dtype": dt, "layout": layout, "sets": sets, "kernel_i": kernels["i"],
                   "frame_bytes": nbytes, "ms": {tag: sum(t) / len(t) for (tag, _), t in zip(forms, times)}}
            print(json.dumps(row), flush=True)
            del xs, plain, forms, state, buffer
            torch.cuda.empty_cache()


def parent():
    print("%d processes, each %d blocks of >= %.2f s per route" % (a.processes, a.repeats, a.seconds / a.repeats))
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
        print("%s  %s %s %s  (%d frames in rotation; (i) %s)" % (r0["name"], tuple(r0["shape"]), r0["dtype"], layout, r0["sets"], r0["kernel_i"]))
        stat = {}
        for tag in ROUTES:
            v = [r["ms"][tag] for r in rs]
            stat[tag] = (sum(v) / len(v), min(v), max(v))
        print("  ms per step   " + "   ".join("(%s) %.4f [%.4f..%.4f]" % ((tag,) + stat[tag]) for tag in ROUTES))
        for tag, model in (("i", 0.5 / 2), ("o", 2.5 / 2)):
            spread = (stat[tag][2] - stat[tag][1]) + (stat["c"][2] - stat["c"][1])
            gain = stat["c"][0] - stat[tag][0]
            verdict = "faster than the idiom by more than the spread" if gain > spread else (
                "slower than the idiom by more than the spread" if -gain > spread else "within the spread of the idiom")
            rate = (0.5 if tag == "i" else 2.5) * r0["frame_bytes"] / (stat[tag][0] * 1e-3) / 1e9
            print("  (%s) / (c) = %.2f of the time (byte model %.2f), (c) - (%s) = %+.4f ms against spreads of %.4f: %s;   (%s): %.0f GB/s of its byte model"
                  % (tag, stat[tag][0] / stat["c"][0], model, tag, gain, spread, verdict, tag, rate))


if __name__ == "__main__":
    child() if a.child else parent()
