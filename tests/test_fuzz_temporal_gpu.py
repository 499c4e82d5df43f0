"""A seeded, COUNT-boxed fuzz of the whole temporal family (the generator: tests/temporal_plans.py::draw_case; its checks without a
GPU: tests/test_temporal_plans_cases.py): tshift, per-clip, interlace, learnable cl, fixed cl, per-clip cl, quantized segment-major
and cl, in place in both layouts.  A case draws (N, T, C, M) with the largest tensor at most 1 MiB -- the fastest dim around 16,
4096 and 8192 bytes and around piece counts that do not divide 256, T in 1..17 with |w| up to T + 1 -- a dtype, a base offset of zero
or one element, a padding, `active` and a table kind, and runs through its family's existing runner against its family's existing
oracle reference at its family's existing bounds: gathers bit for bit, fp32 / fp64 interpolation bit for bit, 16-bit interpolation
within assert_ulp_close(.., FLOOR16), the tables' gradients within assert_gw_entries (16-bit) or 1e-5 of the largest entry.
Every case's kernel names are the ones the rule of the names gives (temporal_plans.fuzz_kernels), and a seed sees all of them.

A fixed number of cases per seed, no wall-clock box: 60 cases (six visits of each of the ten families, three aligned and three
ragged: tests/test_temporal_plans_cases.py shows without a GPU that every seed then reaches every kernel name).  Measured on an
MI355X: 0.5 s to 1.1 s for seed 0 (which warms a fresh process up), 0.3 s to 0.5 s for seeds 1 and 2 ("FUZZ-TEMPORAL seed ..." in the
output).
"""
import time

import numpy as np
import pytest
import torch

import inplace_cases as IC
import temporal_plans as TP
import test_interlace_gpu as IL
import test_per_clip_cl_gpu as PCL
import test_per_clip_gpu as PC
import test_qtemporal_gpu as QT
import test_temporal_cl_gpu as FCL
import test_temporal_inplace_gpu as IP
import test_tshift_cl_gpu as TCL
import test_tshift_gpu as TS
from exact16_cases import FLOOR16, assert_bits, assert_gw_entries, assert_ulp_close
from oracle import oracle as O
from torchshifts import abi

pytestmark = pytest.mark.gpu

TORCH = {"u8": torch.uint8, "i8": torch.int8, "i32": torch.int32, "f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32,
         "f64": torch.float64}
F32, F64 = torch.float32, torch.float64


def _narrowed(a, dt):
    return torch.from_numpy(np.asarray(a, np.float64)).to(dt).double().numpy()


def _check_learnable(got, want, dt, active, what):
    """the bounds of tests/test_tshift_gpu.py::test_random_data"""
    (out, gx), (want_out, want_gx) = got, want
    if dt in (F32, F64) or not active:
        assert_bits(TS._wide(out), want_out, what + ("out",))
        assert_bits(TS._wide(gx), want_gx, what + ("grad_x",))
    else:
        assert_ulp_close(TS._wide(out), want_out, dt, FLOOR16, what + ("out",))
        assert_ulp_close(TS._wide(gx), want_gx, dt, FLOOR16, what + ("grad_x",))


def _check_table(gw, gw64, dt, what):
    """... for grad_w, per row of a table (a [C] table is one row)"""
    gw, gw64 = TS._wide(gw), np.asarray(gw64)
    for n, (row, want) in enumerate(zip(gw.reshape(-1, gw.shape[-1]), gw64.reshape(-1, gw64.shape[-1]))):
        if dt in (F32, F64):
            err = np.abs(row.astype(np.float64) - want).max() / max(np.abs(want).max(), 1e-30)
            assert err < 1e-5, what + ("grad_w", n, err)
        else:
            assert_gw_entries(row, want, dt, what + ("grad_w", n))


def _segment_learnable(c, rs, what):
    N, T, C, M = c["N"], c["T"], c["C"], c["M"]
    shape, dt, off, pad, active = (N, T, C, M), TORCH[c["dt"]], c["off"], c["pad"], c["active"]
    x, go = _narrowed(rs.uniform(-1, 1, size=shape), dt), _narrowed(rs.uniform(-1, 1, size=shape), dt)
    if c["family"] == "tshift":
        w = _narrowed(TS._weights(rs, C, T, pad, quarters=False), dt)
        want_out, want_gx, gw64 = TS._reference(x, go, w, pad, active, dt)
        out, gx, gw, kf, kb = TS._run(shape, dt, off, x, go, w, pad, active)
    elif c["family"] == "per_clip":
        w = _narrowed(PC._table(rs, N, C, T, pad, quarters=False), dt)
        clips = [TS._reference(x[n:n + 1], go[n:n + 1], w[n], pad, active, dt) for n in range(N)]
        want_out, want_gx = np.concatenate([k[0] for k in clips]), np.concatenate([k[1] for k in clips])
        gw64 = np.stack([k[2] for k in clips])
        out, gx, gw, kf, kb = PC._run_per_clip(shape, dt, off, x, go, w, pad, active)
    else:
        w = _narrowed(PC._table(rs, N, C, T, pad, quarters=False), dt)
        s = _narrowed(rs.uniform(-2, 2, size=(N, T, C)), dt)
        want_out, want_gx, gw64, gsc64 = IL._reference(x, go, w, s, pad, active, dt)
        out, gx, gw, gsc, kf, kb = IL._run_interlace(shape, dt, off, x, go, w, s, pad, active)
        for n in range(N):
            IL._check_table(TS._wide(gsc)[n].reshape(-1), gsc64[n].reshape(-1), dt, what + ("grad_scales", n))
    _check_learnable((out, gx), (want_out, want_gx), dt, active, what)
    _check_table(gw, gw64, dt, what)
    return kf, kb


def _frames_learnable(c, rs, what):
    N, T, C, M = c["N"], c["T"], c["C"], c["M"]
    shape, dt, off, pad, active = (N, T, M, C), TORCH[c["dt"]], c["off"], c["pad"], c["active"]
    x, go = _narrowed(rs.uniform(-1, 1, size=shape), dt), _narrowed(rs.uniform(-1, 1, size=shape), dt)
    if c["family"] == "learnable_cl":
        w = _narrowed(TCL._weights(rs, C, T, pad, quarters=False, table=c["table"], dt=dt), dt)
        want_out, want_gx, gw64 = TCL._reference(x, go, w, pad, active, dt)
        out, gx, gw = TCL._run(shape, dt, off, x, go, w, pad, active)          # (asserts the names itself)
    else:
        w = _narrowed(PCL._table(rs, shape, dt, pad, c["table"], quarters=False), dt)
        clips = [TCL._reference(x[n:n + 1], go[n:n + 1], w[n], pad, active, dt) for n in range(N)]
        want_out, want_gx = np.concatenate([k[0] for k in clips]), np.concatenate([k[1] for k in clips])
        gw64 = np.stack([k[2] for k in clips])
        out, gx, gw = PCL._run_cl(shape, dt, off, x, go, w, pad, active)
    _check_learnable((out, gx), (want_out, want_gx), dt, active, what)
    _check_table(gw, gw64, dt, what)
    return TCL._names(shape, dt, off, active)


def _fixed_cl(c, rs, what):
    N, T, C, M = c["N"], c["T"], c["C"], c["M"]
    dt, off = TORCH[c["dt"]], c["off"]
    kernel = TP.fuzz_kernels(c)[0]
    s = FCL._random_table(rs, C, T) if c["table"] == "specials" else FCL._run_table(C, T, max(1, C // (4 if c["table"] == "runs" else 5)))
    FCL._check_float((N, T, M, C), dt, off, kernel, s, c["pad"], rs, what)       # (asserts the name, the oracle's bits, both routes)
    return (kernel,)


def _integer_table(rs, C, T):
    """(int_repr [C], its zero point): shifts in [-T - 1, T + 1] as one of the three table kinds of the quantized entry point"""
    s = rs.randint(-T - 1, T + 2, size=C).astype(np.int64)
    s[[0, C // 2, C - 1]] = [0, T + 1, -T - 1]
    ndt, zp = ((np.uint8, 128), (np.int8, 0), (np.int32, 0))[rs.randint(3)]
    return (s + zp).astype(ndt), zp


def _quantized(c, rs, what):
    N, T, C, M = c["N"], c["T"], c["C"], c["M"]
    dt, off, pad = TORCH[c["dt"]], c["off"], c["pad"]
    w1, wzp = _integer_table(rs, C, T)
    w2 = np.stack([w1, np.zeros_like(w1) + w1.dtype.type(wzp)], 1)
    if c["layout"] == "segment":          # tests/test_qtemporal_gpu.py::test_c_abi_forward_quantized
        shape, view = (N, T, C, M), QT._view
        x_np = QT._data(rs, shape, dt)
        xv, zp = x_np.transpose(0, 2, 1, 3), QT.ZP[dt]
        x, out = QT._buffer(shape, dt, off * x_np.itemsize), QT._buffer(shape, dt, off * x_np.itemsize, fill=0xA5)
        x.copy_(torch.from_numpy(x_np))
        abi.forward_quantized(view(x), torch.from_numpy(w2).cuda(), wzp, zp, pad, out=view(out))
    else:                                 # tests/test_temporal_cl_gpu.py::test_c_abi_forward_quantized
        shape, view = (N, T, M, C), FCL._view
        x_np = FCL._qdata(rs, shape, dt)
        xv, zp = x_np.transpose(0, 3, 1, 2), FCL.ZP[dt]
        x, out = FCL._buffer(shape, dt, off), FCL._buffer(shape, dt, off, fill=0xA5)
        x.copy_(torch.from_numpy(x_np))
        abi.forward_quantized(view(x), torch.from_numpy(w1).cuda(), wzp, zp, pad, out=view(out), shift_dim0=True)
    name = abi.last_kernel()
    want = O.forward_q(np.ascontiguousarray(xv), w2, wzp, zp, pad)
    assert np.array_equal(view(out).cpu().numpy(), want), what + (name,)
    return (name,)


def _inplace(c, rs, what):
    """tests/test_temporal_inplace_gpu.py::_check, the kernel's name returned"""
    N, T, C, M = c["N"], c["T"], c["C"], c["M"]
    dt, cl = TORCH[c["dt"]], c["layout"] == "frames"
    p = IP.Painted((N, T, C, (M,)), dt, c["off"], cl)
    x = IC.data(rs, tuple(p.t.shape), dt)
    p.t.copy_(x)
    s = IP._runs_table(C, T) if c["table"] == "runs" else IC.random_table(rs, C, T)
    want = IC.reference(x, s, T, c["pad"], IP.ZP.get(dt, 0))
    name, path = IP._call(p, s, dt, c["pad"])
    assert path == (abi.PATH_CL if cl else abi.PATH_PLANE), what + (name, path)
    assert IC.same_bits(p.t, want), what + (name,)
    assert p.guards_intact(), what
    return (name,)


RUNNERS = {"tshift": _segment_learnable, "per_clip": _segment_learnable, "interlace": _segment_learnable, "learnable_cl": _frames_learnable,
           "per_clip_cl": _frames_learnable, "fixed_cl": _fixed_cl, "quantized_segment": _quantized, "quantized_cl": _quantized,
           "inplace_segment": _inplace, "inplace_cl": _inplace}


@pytest.mark.parametrize("seed", TP.FUZZ_SEEDS)
def test_random_cases_against_the_oracle(seed):
    assert torch.cuda.is_available()
    t0 = time.perf_counter()
    seen = {}
    for n, c in enumerate(TP.fuzz_cases(seed)):
        what = ("seed", seed, "case", n, tuple(sorted(c.items())))
        names = RUNNERS[c["family"]](c, np.random.RandomState(7919 * seed + n), what)
        assert tuple(names) == TP.fuzz_kernels(c), what + (names,)
        for k in names:
            seen[k] = seen.get(k, 0) + 1
    torch.cuda.synchronize()
    print("FUZZ-TEMPORAL seed %d: %d cases in %.2f s; %s" % (seed, TP.FUZZ_COUNT, time.perf_counter() - t0, sorted(seen.items())))
    for must in TP.FUZZ_MUST_SEE:
        assert must in seen, (must, seen)
