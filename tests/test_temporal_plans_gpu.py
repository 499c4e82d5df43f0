"""The channels-last temporal kernels in every regime of their launch plans (tests/temporal_plans.py: the restated plans and the case
table; tests/test_temporal_plans_cases.py: their checks without a GPU): frames_forward with two batches per workgroup under each
piece width and each deciding term, frames_active_forward with one, two and three batches on uniform and on mixed pieces,
frames_backward with 1, 2, 4 and 8 row steps, with a kernel rps that is not the plan's, and with both record indices -- the
unsuffixed kernels (16-byte pieces of eight fp16 channels, rows of 24 and of 64 channels) past their first batch and their first row
step as well as the *_ragged forms.

Each case runs through the C ABI under paddings 0 and 3 (frames_backward: both values of `active`) and is compared WHOLE.
Data: the project's exact data -- tensors on eighths, tables on quarters, uint8 tensors that never hold their zero point -- so every
tap, blend and grad_x is exact: out and grad_x are compared bit for bit (equal values and equal sign bits; nothing here is a NaN).
Reference: tests/bigindex_cases.py's plain-torch fp64 restatement of the oracle, on the device, in chunks of clips (no clip reads
another, so the reference of a slice is the slice of the reference); a per-clip table makes (clip, channel) the channel of a
one-clip problem.  Cases under 1 MB are also compared with the C oracle on the CPU (test_tshift_cl_gpu._reference, clip by clip).
grad_w: every term is a multiple of 1/64 and the sums stay below 2^53 / 64, so the fp64 sum is exact in any order; the table must
equal it narrowed ONCE to the table's type, bit for bit (the kernel narrows through fp32: the test asserts that every sum of a
16-bit table is an fp32 value, so the two narrowings are one).  Under padding 3 the 16-bit tensors run with an fp32 table.
The kernel name is asserted, and for the backward the workspace size against the restatement's N * chunks * C * 24.
On a difference the message names the first wrong element as (n, t, row, channel) and the workgroup, batch and step it lies in.

Wall time measured on an MI355X (printed per case as "PLANS ... s"): 0.9 s for the first case of a process (which warms it up),
0.11 s for the case with rows of 257 pieces, 0.05 s and less for every other case -- the 100 and 200 MB ones 0.01 s -- and 0.04 s and
less for the two tests through the ops; the 44 tests take under 3 s together.
"""
import time

import numpy as np
import pytest
import torch

import bigindex_cases as B
import temporal_plans as TP
from oracle import oracle as O
from test_bigindex_gpu import _clips      # [N*T, C, H, W] (contiguous or channels-last) -> the problem view [N, C, T, H*W]
from test_temporal_cl_gpu import ZP
from test_tshift_cl_gpu import _buffer, _reference, _view, _wide
from torchshifts import abi
from torchshifts.functional import temporal_shift_func, temporal_shift_per_clip_func
from torchshifts.quantized.functional import temporal_shift_quantized

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
TORCH = {"u8": torch.uint8, "f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "f64": torch.float64}
CHUNK_BYTES = 32 << 20
CASES = TP.unique_cases()
PADS = (0, 3)
SMALL = 1 << 20


def _id(c):
    return "%s-%s-%s-off%d-%s" % (c[1].replace("frames_", ""), "x".join(map(str, c[2])), c[3], c[4], c[5])


def _draw(seed, shape, dt, off, lo=-7, hi=7):
    """the exact data of a case in a buffer `off` elements past an aligned allocation"""
    t = _buffer(shape, dt, off)
    if dt == torch.uint8:
        b = B.bytes_(seed, 0, shape, dt, DEV)
        b[b == ZP[dt]] += 1                       # never the zero point: a fill shows, and so does a fill that is missing
        t.copy_(b)
    else:
        t.copy_(B.eighths(seed, 0, shape, dt, DEV, lo, hi))
    return t


def _clip_chunks(shape, es):
    per = max(1, CHUNK_BYTES // (int(np.prod(shape[1:])) * es))
    return [(a, min(a + per, shape[0])) for a in range(0, shape[0], per)]


def _as_one_clip(v):
    """[n, C, T, M] -> [1, n * C, T, M]: under a per-clip table (clip, channel) is the channel"""
    return v.reshape(1, v.shape[0] * v.shape[1], v.shape[2], v.shape[3])


def _same_bits(got, want):
    return torch.equal(got, want) and (not want.dtype.is_floating_point or torch.equal(torch.signbit(got), torch.signbit(want)))


def _assert_whole(got_view, a, e, want, kernel, shape, es, off, what):
    """got_view: the [N, C, T, M] view of the (N, T, M, C) buffer; want: [e - a, C, T, M]"""
    got = got_view[a:e]
    assert got.shape == want.shape and got.dtype == want.dtype, what + (got.shape, want.shape, got.dtype, want.dtype)
    if _same_bits(got, want):
        return
    bad = (got != want) | (torch.signbit(got) != torch.signbit(want) if want.dtype.is_floating_point else torch.zeros_like(got, dtype=torch.bool))
    flat = bad.permute(0, 2, 3, 1).reshape(-1)                    # memory order n, t, row, channel
    first = int(torch.nonzero(flat)[0]) + a * int(np.prod(shape[1:]))
    n, t, row, c = np.unravel_index(first, shape)
    raise AssertionError(what + ("%d elements differ in clips %d:%d; the first: got %r, want %r at %s"
                                 % (int(flat.sum()), a, e, got_view[n, c, t, row].item(), want[n - a, c, t, row].item(),
                                    TP.locate(kernel, shape, es, off, first)),))


def _name(kernel, plan):
    return kernel if plan["unit"] == 16 else kernel + "_ragged"


def _cpu_reference(x, go, w, pad, active, dt):
    """the C oracle, clip by clip: out, grad_x, grad_w (fp64) as arrays of the buffer's shape / the table's shape"""
    xn, gn = _wide(x).astype(np.float64), _wide(go).astype(np.float64)
    if w.ndim == 1:
        return _reference(xn, gn, w, pad, active, dt)
    clips = [_reference(xn[n:n + 1], gn[n:n + 1], w[n], pad, active, dt) for n in range(x.shape[0])]
    return np.concatenate([c[0] for c in clips]), np.concatenate([c[1] for c in clips]), np.stack([c[2] for c in clips])


def _buffer_order(want):
    """a reference [N, C, T, M] -> the (N, T, M, C) array"""
    return want.permute(0, 2, 3, 1).contiguous()


def _run_case(case):
    regime, kernel, shape, dtn, off, table = case[:6]
    N, T, M, C = shape
    dt, es = TORCH[dtn], TP.ES[dtn]
    plan = TP.plan_of(case)
    name = _name(kernel, plan)
    clip = table.startswith("clip-")
    quant = dt == torch.uint8
    small = TP.nbytes(case) < SMALL
    flags = dict(shift_dim0=True, clip_frames=True) if clip else dict(shift_dim0=True, frames=True)
    x = _draw(11, shape, dt, off, 0, 7)
    xv = _view(x)
    backward = kernel == TP.FB
    if backward:
        go = _draw(12, shape, dt, off)
        gv = _view(go)
    for pad in PADS:
        w = TP.table_of(case, pad)                                    # float64, on quarters
        w64 = torch.from_numpy(w).to(DEV)
        wdt = torch.float32 if (pad == 3 and es == 2) else dt         # 16-bit tensors: their own type, then an fp32 table
        for active in ((0, 1) if backward else ((1,) if kernel == TP.FA else (0,))):
            what = (_id(case), "pad", pad, "active", active)
            out = _buffer(shape, dt, off, fill=0xA5)
            ov = _view(out)
            if quant:
                assert not clip
                shifts = torch.round(w64).to(torch.int64)
                abi.forward_quantized(xv, shifts.to(torch.int32), 0, ZP[dt], pad, out=ov, shift_dim0=True)
            elif not backward:
                abi.forward(xv, w64.to(wdt), pad, active, out=ov, **flags)
            else:
                wd = w64.to(wdt)
                gw = torch.full_like(wd, float("nan"))
                ws = abi.backward_workspace(xv, pad, active, **flags)
                assert ws.numel() == plan["workspace_bytes"] == N * plan["chunks"] * C * 24, what + (ws.numel(), plan)
                ws.fill_(0xA5)
                abi.backward(gv, wd, xv, pad, active, grad_x=ov, grad_w=gw, workspace=ws, **flags)
            assert abi.last_kernel() == name and abi.last_path() == abi.PATH_CL, what + (abi.last_kernel(), name)
            gw64 = None
            for a, e in _clip_chunks(shape, es):
                xc = xv[a:e]
                wc = w64[a:e].reshape(-1) if clip else w64
                if clip:
                    xc = _as_one_clip(xc)
                if quant:
                    want = B.temporal_forward_q(xc, shifts, ZP[dt], pad)
                elif not backward:
                    want = B.narrow(B.temporal_forward(xc, wc, pad, bool(active)), dt)
                else:
                    gc = _as_one_clip(gv[a:e]) if clip else gv[a:e]
                    gx, part = B.temporal_backward(gc, xc, wc, pad, bool(active))
                    want = B.narrow(gx, dt)
                    part = part.reshape(e - a, C) if clip else part
                    gw64 = part if gw64 is None else (torch.cat([gw64, part]) if clip else gw64 + part)
                _assert_whole(ov, a, e, want.reshape(e - a, C, T, M), kernel, shape, es, off, what + ("grad_x" if backward else "out",))
            if backward:
                assert gw64.shape == gw.shape and bool((gw64.abs() < 2.0 ** 47).all()), what
                if wdt in (torch.float16, torch.bfloat16):
                    assert torch.equal(gw64.to(torch.float32).to(torch.float64), gw64), what + ("a sum that is no fp32 value",)
                want_gw = gw64.to(wdt)
                if not _same_bits(gw, want_gw):
                    i = int(torch.nonzero((gw != want_gw).reshape(-1))[0])
                    raise AssertionError(what + ("grad_w entry %d (clip %d, channel %d): got %r, the fp64 sum %r narrowed once %r; %d steps, "
                                                 "%d chunks, kernel rps %d, plan rps %d" % (i, i // C if clip else -1, i % C, gw.reshape(-1)[i].item(),
                                                 gw64.reshape(-1)[i].item(), want_gw.reshape(-1)[i].item(), plan["steps"], plan["chunks"],
                                                 plan["rps"], plan["plan_rps"]),))
            if small:                                                 # the C oracle on the CPU
                if quant:
                    w2 = np.stack([np.rint(w), np.zeros_like(w)], 1).astype(np.int32)
                    want = O.forward_q(np.ascontiguousarray(xv.cpu().numpy()), w2, 0, ZP[dt], pad)
                    assert np.array_equal(ov.cpu().numpy(), want), what + ("out against the C oracle",)
                else:
                    wr = torch.from_numpy(w).to(wdt).double().numpy()
                    want_out, want_gx, o64 = _cpu_reference(x, go if backward else x, wr, pad, active, dt)
                    assert np.array_equal(_wide(out), want_gx if backward else want_out), what + ("against the C oracle",)
                    if backward:
                        assert np.array_equal(gw64.cpu().numpy(), o64.reshape(gw64.shape)), what + ("the fp64 sums against the C oracle",)


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_whole_tensor_in_its_regime(ci):
    case = CASES[ci]
    assert TP.holds(case[0], case)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _run_case(case)
    torch.cuda.synchronize()
    print("PLANS %s | %s | %d bytes | %.2f s" % (case[0], _id(case), TP.nbytes(case), time.perf_counter() - t0))


# ---- through the ops: the binding's route to each plan -----------------------------------------------------------------------
def _op_input(seed, N, T, C, H, W, dt, lo=-7, hi=7):
    x = torch.empty((N * T, C, H, W), dtype=dt, device=DEV, memory_format=torch.channels_last)
    v = _clips(x, T)
    assert v.data_ptr() == x.data_ptr()
    if dt == torch.uint8:
        b = B.bytes_(seed, 0, (N, T, H * W, C), dt, DEV)
        b[b == ZP[dt]] += 1
        v.copy_(b.permute(0, 3, 1, 2))
    else:
        v.copy_(B.eighths(seed, 0, (N, T, H * W, C), dt, DEV, lo, hi).permute(0, 3, 1, 2))
    return x, v


def _op_case(kernel, shape, dtn, table):
    return ("op", kernel, shape, dtn, 0, table)


def _check_op(got, want_of_chunk, kernel, shape, es, what):
    gv = got
    for a, e in _clip_chunks(shape, es):
        _assert_whole(gv, a, e, want_of_chunk(a, e), kernel, shape, es, 0, what)


def test_the_learnable_op_reaches_the_second_batch_and_the_second_step():
    """temporal_shift_learnable_cl on 3072 frames of 46 x 46 x 8 fp16 (one 16-byte piece of eight channels a row under a table that is
    constant inside it -- the batched loop is the uniform pieces' -- : the unsuffixed kernel, two workgroups per frame, two batches in
    the first) and its backward on 1024 clips of 25 x 41 x 8 (four
    row steps, two workgroups per clip, the second of one row)"""
    ops = torch.ops.torchshifts
    T, C, dt = 2, 8, torch.float16
    fwd = _op_case(TP.FA, (1536, T, 46 * 46, C), "f16", "pieces")
    p = TP.plan_of(fwd)
    assert p["batches"] == 2 and p["unit"] == 16 and p["epp"] == 8 and p["chunks"] == 2, p
    x, xv = _op_input(21, 1536, T, C, 46, 46, dt, 0, 7)
    for pad in PADS:
        w64 = torch.from_numpy(TP.table_of(fwd, pad)).to(DEV)
        out = ops.temporal_shift_learnable_cl(x, w64.float(), T, pad, True)
        assert abi.last_kernel() == "frames_active_forward" and out.stride() == x.stride(), abi.last_kernel()
        _check_op(_clips(out, T), lambda a, e: B.narrow(B.temporal_forward(xv[a:e], w64, pad, True), dt), TP.FA, fwd[2], 2,
                  ("temporal_shift_learnable_cl", "pad", pad, "out"))
    del x, xv, out
    bwd = _op_case(TP.FB, (1024, T, 25 * 41, C), "f16", "specials")
    p = TP.plan_of(bwd)
    assert p["steps"] == 4 and p["chunks"] == 2 and p["unit"] == 16 and p["iterations"] == 4 and p["last_rows"] == 1, p
    x, xv = _op_input(22, 1024, T, C, 25, 41, dt, 0, 7)
    go, gv = _op_input(23, 1024, T, C, 25, 41, dt)
    for pad, active in ((0, True), (3, False)):
        w64 = torch.from_numpy(TP.table_of(bwd, pad)).to(DEV)
        gx, gw = ops._temporal_shift_learnable_cl_backward(go, w64.float(), x, T, pad, active)
        assert abi.last_kernel() == "frames_backward" and gx.stride() == go.stride(), abi.last_kernel()
        ref = B.temporal_backward(gv, xv, w64, pad, active)
        _assert_whole(_clips(gx, T), 0, 1024, B.narrow(ref[0], dt), TP.FB, bwd[2], 2, 0, ("_temporal_shift_learnable_cl_backward", pad, active, "grad_x"))
        assert gw.dtype == torch.float32 and _same_bits(gw.reshape(-1), ref[1].to(torch.float32)), ("grad_w", pad, active)


def test_the_fixed_ops_reach_the_second_batch():
    """temporal_shift_cl, its per-clip form and the quantized op with memory_format=torch.preserve_format on 3072 frames of
    37 x 37 x 6: rows of 12 fp16 bytes (4-byte pieces) and of 6 uint8 bytes (2-byte pieces), two workgroups per frame, two batches;
    the tables are runs of two channels, so every piece is uniform (the batched loop is theirs), and the per-clip rows all differ"""
    T, C, H = 2, 6, 37
    keep = torch.preserve_format
    for dtn, kernel_name in (("f16", "frames_forward_ragged"), ("u8", "frames_forward_ragged")):
        dt = TORCH[dtn]
        case = _op_case(TP.FF, (1536, T, H * H, C), dtn, "runs")
        p = TP.plan_of(case)
        assert p["batches"] == 2 and p["chunks"] == 2 and p["rps"] == 85, p
        x, xv = _op_input(24, 1536, T, C, H, H, dt, 0, 7)
        for pad in PADS:
            base = torch.round(torch.from_numpy(TP.table_of(case, pad))).to(torch.int64)              # [C]: 1, 1, -1, -1, 0, 0
            assert TP.mixed_pieces(case, pad, 0)[0] == 0
            rows = (base[None, :] + (torch.arange(1536) % 5)[:, None]).to(DEV)                        # [N, C], neighbouring rows differ
            if dtn == "u8":
                s = rows[0]
                xq = torch._make_per_tensor_quantized_tensor(x.permute(0, 2, 3, 1).contiguous(), 0.05, ZP[dt]).permute(0, 3, 1, 2)
                assert xq.stride() == x.stride()
                out = temporal_shift_quantized(xq, s, T, pad, memory_format=keep)
                assert abi.last_kernel() == kernel_name and out.stride() == x.stride(), abi.last_kernel()
                _check_op(_clips(out.int_repr(), T), lambda a, e: B.temporal_forward_q(xv[a:e], s, ZP[dt], pad), TP.FF, case[2], 1,
                          ("temporal_shift_quantized", "pad", pad))
                continue
            s = rows[0]
            out = temporal_shift_func(x, s, T, pad, memory_format=keep)
            assert abi.last_kernel() == kernel_name and out.stride() == x.stride(), abi.last_kernel()
            _check_op(_clips(out, T), lambda a, e: B.narrow(B.temporal_forward(xv[a:e], s.double(), pad, False), dt), TP.FF, case[2], 2,
                      ("temporal_shift_func", "pad", pad))
            out = temporal_shift_per_clip_func(x, rows, T, pad, memory_format=keep)
            assert abi.last_kernel() == kernel_name and out.stride() == x.stride(), abi.last_kernel()
            _check_op(_clips(out, T), lambda a, e: B.narrow(B.temporal_forward(_as_one_clip(xv[a:e]), rows[a:e].reshape(-1).double(), pad, False),
                                                          dt).reshape(e - a, C, T, H * H), TP.FF, case[2], 2, ("temporal_shift_per_clip_func", "pad", pad))
