#!/usr/bin/env python3
"""The quantized temporal shift (TSM) of quint8 [N*T, C, H, W] tensors: the op against every way there was to get the same tensor
before it, zeros padding, the default table, device-event times (GPU box):
    SHIFTND_HIP_LIB=<a build of the parent commit's libshiftnd_hip.so> python3 tools/qtemporal_bench.py [--seconds 0.5] [--repeats 3]
Routes, alternated block by block in one process (each figure the mean of `repeats` blocks that together run at least `seconds`;
min..max of the blocks is the run-to-run spread):
  (a) torch.ops.torchshifts.temporal_shift_quantized (csrc/shiftnd_segment.hip, element-sized units, the zero point as the fill)
  (p) the same C-ABI call, shiftnd_forward_quantized on the permuted views with a [C, 2] int32 table, through torchshifts.abi -- which
      loads SHIFTND_HIP_LIB: with the parent commit's library this is what the call cost before (strided_gather_forward); without
      the variable it is the in-tree kernel without the op's table build.  The line names the kernel (p) ran.
  (c) the slicing idiom on the int_repr: a tensor of the zero point plus three slice copies (the uint8 tensor is taken as given:
      int_repr() on the way in and _make_per_tensor_quantized_tensor on the way out are not timed)
  (q) dequantize -> the float temporal_shift (fp32) -> quantize_per_tensor
  (h) torch.ops.torchshifts.temporal_shift on an fp16 tensor of the same byte count (W halved): the same kernel over the same bytes
      in two-byte units with a zero fill; n/a where the plane is an odd number of bytes
(a), (q) and (h) always use the in-tree library.  Every tensor is one of several sets that are rotated call by call, so that no
route finds its operands in the 256 MB last-level cache.  GB/s = the bytes the result needs -- one read of every plane that is not
filled, one write of every plane -- over (a); "of copy" = that rate over the same box's plain 1-read-1-write stream
(tools/stream_probe on tensors of the largest line's size, a child process that has exited before this one touches the GPU)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "activesparseshifts-pytorch_amd"))

LINES = [("56x56 quint8 (whole pieces)", (256, 256, 56, 56), 8), ("14x14 quint8 (196-byte planes)", (256, 1024, 14, 14), 8),
         ("7x7 quint8 (49-byte planes)", (512, 2048, 7, 7), 8)]
SCALE, ZP = 0.0625, 7

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


PROBE_BYTES = max(numel(shape) for _, shape, _ in LINES)
COPY = probe(PROBE_BYTES)

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


# (the file's name only: the lines below name the kernel (p) ran, which is what tells the builds apart)
print("library of (p):", "SHIFTND_HIP_LIB (%s)" % os.path.basename(os.environ["SHIFTND_HIP_LIB"]) if os.environ.get("SHIFTND_HIP_LIB") else "in-tree")
print("copy stream of this box (1R1W, tensors of %d bytes): %.0f GB/s" % (PROBE_BYTES, COPY))
for li, (name, shape, T) in enumerate(LINES):
    if a.only and str(li) not in a.only.split(","):
        continue
    NT, C, H, W = shape
    N, M = NT // T, H * W
    nbytes = numel(shape)
    sets = max(2, int(a.rotate_bytes / (2 * nbytes)) + 1)
    f = C // 8
    s = torch.tensor([-1] * f + [1] * f + [0] * (C - 2 * f), device="cuda")
    w32 = torch.stack([s, torch.zeros_like(s)], 1).to(torch.int32).contiguous()
    reprs = [torch.randint(0, 256, shape, device="cuda", dtype=torch.uint8) for _ in range(sets)]
    xs = [torch._make_per_tensor_quantized_tensor(r, SCALE, ZP) for r in reprs]
    outs = [torch.empty_like(reprs[0]) for _ in range(sets)]
    half = (M % 2 == 0)
    hs = [torch.rand((NT, C, H, W // 2), device="cuda").to(torch.float16) for _ in range(sets)] if half else []
    turn = [0]

    def pick(lst):
        turn[0] += 1
        return lst[turn[0] % len(lst)]

    def seg(t):   # [N*T, C, H, W] -> the [N, C, T, M] view
        return t.view(N, T, C, M).permute(0, 2, 1, 3)

    def idiom(r):
        v = r.view(N, T, C, H, W)
        out = torch.full_like(v, ZP)
        out[:, :-1, :f] = v[:, 1:, :f]
        out[:, 1:, f:2 * f] = v[:, :-1, f:2 * f]
        out[:, :, 2 * f:] = v[:, :, 2 * f:]
        return out.view(NT, C, H, W)

    def p_forward():
        i = turn[0] = turn[0] + 1
        return abi.forward_quantized(seg(reprs[i % sets]), w32, 0, ZP, 0, out=seg(outs[i % sets]))

    forms = [
        ("a", lambda: OPS.temporal_shift_quantized(pick(xs), s, T, 0)),
        ("p", p_forward),
        ("c", lambda: idiom(pick(reprs))),
        ("q", lambda: torch.quantize_per_tensor(OPS.temporal_shift(pick(xs).dequantize(), s, T, 0), SCALE, ZP, torch.quint8)),
    ]
    if half:
        forms.append(("h", lambda: OPS.temporal_shift(pick(hs), s, T, 0)))
    ref = OPS.temporal_shift_quantized(xs[0], s, T, 0)   # the routes return the same tensor
    assert ref.q_scale() == SCALE and ref.q_zero_point() == ZP
    assert torch.equal(ref.int_repr(), idiom(reprs[0]))
    assert torch.equal(ref.int_repr(), abi.forward_quantized(seg(reprs[0]), w32, 0, ZP, 0, out=seg(outs[0])).permute(0, 2, 1, 3).reshape(shape))
    assert torch.equal(ref.int_repr(), torch.quantize_per_tensor(OPS.temporal_shift(xs[0].dequantize(), s, T, 0), SCALE, ZP, torch.quint8).int_repr())
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
    # planes that are read: every (t, c) whose source frame exists (zeros padding)
    read_planes = sum(T - min(abs(int(v)), T) for v in s.tolist())
    algo = N * M * (read_planes + T * C)
    print("%s  %s T=%d  (%d operand sets; (p) ran %s)" % (name, shape, T, sets, kernels["p"]))
    cells = "   ".join("(%s) %.4f [%.4f..%.4f]" % (forms[k][0], mean[k], min(times[k]), max(times[k])) for k in range(len(forms)))
    gbs = algo / (mean[0] * 1e-3) / 1e9
    print("  forward ms  %s" % cells)
    print("  (p) / (a) = %.2f   fastest of (c), (q) / (a) = %.2f   (a): %.0f GB/s, %.2f of copy" %
          (mean[1] / mean[0], min(mean[2], mean[3]) / mean[0], gbs, gbs / COPY))
    if half:
        spread = max(max(times[k]) - min(times[k]) for k in (0, 4))
        print("  (a) - (h) = %+.4f ms against a spread of %.4f" % (mean[0] - mean[4], spread))
    else:
        print("  (h) n/a: a plane of %d bytes is no whole number of fp16 elements" % M)
    del xs, reprs, outs, hs, ref
    torch.cuda.empty_cache()
