"""The channels-last per-clip temporal shift on the GPU: SHIFTND_SHIFT_DIM0 | SHIFTND_CLIP_FRAMES through the C ABI -- the frame
kernels of csrc/shiftnd_frames.hip and csrc/shiftnd_frames_learn.hip under a [N, C] table, on permuted views of (N, T, M, C) buffers
-- and through torch.ops.torchshifts_per_clip_cl and memory_format=torch.preserve_format of the per-clip functions and modules.

The shapes, the tables, the reference, the exact-data rule and the random-data bounds are those of tests/test_tshift_cl_gpu.py, per
clip: clip n is that file's problem on its own frames under row n of the table.  One shape is added for the backward's record
index, which differs from the per-channel one only with several workgroups per clip and several clips: (3, 2, 300, 8) fp32 -- 2
pieces, 128 rows per workgroup, 3 workgroups per clip, three clips; (2, 8, 196, 64) fp16 of that file has 7 workgroups per clip.

Tables: row n is that file's _weights(..., turn=pad + n, table=...) -- "specials" (every piece mixed), "pieces" (constant inside
every 16-byte piece: the uniform path), "runs" (a run boundary inside a piece; this table does not depend on the turn, so its rows
are equal) -- and group tables [N, G] expanded as torchshifts.functional._per_clip_table expands them: "groups8" (C // G = 8 with
fp16: every piece uniform) and "groups3" (C // G = 3: boundaries inside pieces), whose rows all differ.
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import torchshifts
from torchshifts import abi
from torchshifts.functional import temporal_shift_learnable_per_clip_func, temporal_shift_per_clip_func

import redzone as RZ
from exact16_cases import FLOOR16, assert_bits, assert_gw_entries, assert_ulp_close, round16
from test_per_clip_gpu import _run_per_clip as _run_segment_major_per_clip
from test_tshift_cl_gpu import CASES as CL_CASES
from test_tshift_cl_gpu import GUARDED as CL_GUARDED
from test_tshift_cl_gpu import (TABLES, _buffer, _channels_last_inputs, _eighths, _es, _id, _names, _painted, _put, _reference, _refused,
                                _run, _untouched, _view, _weights, _wide)

pytestmark = pytest.mark.gpu

OPS = torch.ops.torchshifts_per_clip_cl
PLAIN = torch.ops.torchshifts_per_clip
KEEP = torch.preserve_format
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
KW = dict(shift_dim0=True, clip_frames=True)

RECORDS = ((3, 2, 300, 8), F32, 0)      # three workgroups per clip, three clips
CASES = CL_CASES + [RECORDS]
SWEEP = list(itertools.product(range(5), (0, 1)))


def _tables(shape, dt):
    C = shape[-1]
    return TABLES + (("groups8",) if dt == F16 and C % 8 == 0 else ()) + (("groups3",) if C % 3 == 0 else ())


def _table(rs, shape, dt, pad, table, quarters=True):
    """the [N, C] table of a case"""
    N, T, C = shape[0], shape[1], shape[-1]
    if table.startswith("groups"):
        G = C // int(table[6:])
        g = rs.randint(-4 * (T + 1), 4 * (T + 1) + 1, size=(N, G)) / 4.0 if quarters else rs.uniform(-T - 1, T + 1, size=(N, G))
        return np.repeat(g, C // G, axis=1)
    return np.stack([_weights(rs, C, T, pad + n, quarters, table=table, dt=dt) for n in range(N)])


@functools.lru_cache(maxsize=256)
def _inputs(ci, kind, table, pad, active):
    """x, go (N, T, M, C) and the [N, C] table of CASES[ci] -- fp64 arrays holding values of the case's dtype -- and the per-clip
    reference: out, grad_x, and grad_w [N, C] from the fp64 oracle.  Computed once, shared, never written to."""
    shape, dt, _ = CASES[ci]
    N = shape[0]
    rs = np.random.RandomState(1000 * ci + 100 * _tables(shape, dt).index(table) + 10 * pad + active + (50000 if kind == "random" else 0))
    if kind == "exact":
        x, go, w = _eighths(rs, shape), _eighths(rs, shape), _table(rs, shape, dt, pad, table)
    else:
        narrow = (lambda a: torch.from_numpy(a).to(dt).double().numpy())
        x, go = narrow(rs.uniform(-1, 1, size=shape)), narrow(rs.uniform(-1, 1, size=shape))
        w = narrow(_table(rs, shape, dt, pad, table, quarters=False))
    clips = [_reference(x[n:n + 1], go[n:n + 1], w[n], pad, active, dt) for n in range(N)]
    out, gx = np.concatenate([c[0] for c in clips]), np.concatenate([c[1] for c in clips])
    gw64 = np.stack([c[2] for c in clips])
    for a in (out, gx, gw64):
        a.setflags(write=False)
    return x, go, w, out, gx, gw64


def _device_inputs(shape, dt, off, x, go, w, wdt=None):
    return _put(x, dt, off), _put(go, dt, off), torch.from_numpy(np.ascontiguousarray(w)).to(wdt or dt).cuda()


def _run_cl(shape, dt, off, x, go, w, pad, active, wdt=None):
    """the flagged forward and backward on (N, T, M..., C) buffers under the [N, C] table -> out, grad_x, grad_w; the kernel names and
    the path are asserted"""
    xd, gd, wd = _device_inputs(shape, dt, off, x, go, w, wdt)
    out, gx = _buffer(shape, dt, off, fill=0xA5), _buffer(shape, dt, off, fill=0xA5)
    names = _names(shape, dt, off, active)
    abi.forward(_view(xd), wd, pad, active, out=_view(out), **KW)
    assert abi.last_kernel() == names[0] and abi.last_path() == abi.PATH_CL, (shape, dt, off, active, abi.last_kernel())
    gw = torch.full_like(wd, float("nan"))
    abi.backward(_view(gd), wd, _view(xd), pad, active, grad_x=_view(gx), grad_w=gw, **KW)
    assert abi.last_kernel() == names[1] and abi.last_path() == abi.PATH_CL, (shape, dt, off, active, abi.last_kernel())
    return out, gx, gw


def _same_bits(a, b):
    return torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


# ---- 1. exact data ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_exact_data(ci):
    shape, dt, off = CASES[ci]
    for table, (pad, active) in itertools.product(_tables(shape, dt), SWEEP):
        what = (_id(CASES[ci]), table, "pad", pad, "active", active)
        x, go, w, want_out, want_gx, gw64 = _inputs(ci, "exact", table, pad, active)
        out, gx, gw = _run_cl(shape, dt, off, x, go, w, pad, active)
        assert_bits(_wide(out), want_out, what + ("out",))
        assert_bits(_wide(gx), want_gx, what + ("grad_x",))
        assert gw.shape == w.shape
        if dt in (F32, F64):
            assert np.array_equal(_wide(gw).astype(np.float64), gw64), what + ("grad_w",)
        else:
            assert_bits(_wide(gw), round16(gw64.astype(np.float32), dt), what + ("grad_w, the fp64 sum rounded once",))
            # fp32 weights with the 16-bit tensor: the same bits in out and grad_x, grad_w the sum itself
            out2, gx2, gw2 = _run_cl(shape, dt, off, x, go, w, pad, active, wdt=F32)
            assert gw2.dtype == F32, what
            assert torch.equal(out2, out) and torch.equal(gx2, gx), what + ("mixed out / grad_x",)
            assert np.array_equal(_wide(gw2).astype(np.float64), gw64), what + ("mixed grad_w",)


# ---- 2. the same kernels, the same bits -------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_the_bits_of_the_loop_over_clips_and_of_the_segment_major_call(ci):
    shape, dt, off = CASES[ci]
    N = shape[0]
    kw1 = dict(shift_dim0=True, frames=True)
    for table, (pad, active) in itertools.product(_tables(shape, dt), SWEEP):
        what = (_id(CASES[ci]), table, "pad", pad, "active", active)
        x, go, w = _inputs(ci, "exact", table, pad, active)[:3]
        out, gx, gw = _run_cl(shape, dt, off, x, go, w, pad, active)
        # the loop over the clips of the per-channel channels-last call, each on its clip's slice of the same buffers under row n
        xd, gd, wd = _device_inputs(shape, dt, off, x, go, w)
        out1, gx1 = _buffer(shape, dt, off, fill=0xA5), _buffer(shape, dt, off, fill=0xA5)
        for n in range(N):
            abi.forward(_view(xd[n:n + 1]), wd[n], pad, active, out=_view(out1[n:n + 1]), **kw1)
            assert abi.last_kernel().startswith("frames_") and abi.last_path() == abi.PATH_CL, what
            abi.backward(_view(gd[n:n + 1]), wd[n], _view(xd[n:n + 1]), pad, active, grad_x=_view(gx1[n:n + 1]), **kw1)
            assert abi.last_kernel().startswith("frames_backward"), what
        assert _same_bits(out, out1), what + ("out against the loop over clips",)
        assert _same_bits(gx, gx1), what + ("grad_x against the loop over clips",)
        # the segment-major per-clip call on (N, T, C, M) copies of the same values (every case here is (N, T, M, C))
        to_sm = (lambda a: np.ascontiguousarray(np.moveaxis(a, -1, 2)))
        sm = _run_segment_major_per_clip(to_sm(x).shape, dt, 0, to_sm(x), to_sm(go), w, pad, active)
        assert sm[3].startswith("tshift_forward") and sm[4].startswith("tshift_backward"), what
        assert _same_bits(out, sm[0].movedim(2, -1).contiguous()), what + ("out against tshift_forward",)
        assert _same_bits(gx, sm[1].movedim(2, -1).contiguous()), what + ("grad_x against tshift_backward",)


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_equal_rows_are_the_per_channel_call(ci):
    """a table whose rows are all equal: out and grad_x are the per-channel SHIFT_DIM0 | FRAMES call's bit for bit, and on exact data
    the rows of grad_w sum, in fp64, to its grad_w (fp32 tables for the 16-bit tensors: every sum is exact in fp32, none in 16 bits)"""
    shape, dt, off = CASES[ci]
    N = shape[0]
    wdt = F32 if dt in (F16, BF16) else dt
    for pad, active in SWEEP:
        what = (_id(CASES[ci]), "pad", pad, "active", active)
        x, go, w = _inputs(ci, "exact", "specials", pad, active)[:3]
        row = w[N - 1]
        out, gx, gw = _run_cl(shape, dt, off, x, go, np.tile(row, (N, 1)), pad, active, wdt=wdt)
        out1, gx1, gw1 = _run(shape, dt, off, x, go, np.array(row), pad, active, wdt=wdt)
        assert _same_bits(out, out1), what + ("out",)
        assert _same_bits(gx, gx1), what + ("grad_x",)
        assert torch.equal(gw.double().sum(0), gw1.double()), what + ("the rows of grad_w sum to the per-channel grad_w",)


def test_the_per_channel_calls_keep_their_record_index():
    """SHIFT_DIM0 | FRAMES without the new bit on the two shapes with several workgroups per clip: grad_w against the oracle as
    tests/test_tshift_cl_gpu.py::test_exact_data compares it"""
    rs = np.random.RandomState(51)
    for (shape, dt, off), (pad, active) in itertools.product((RECORDS, ((2, 8, 196, 64), F16, 0)), ((0, 0), (3, 1))):
        x, go, w = _eighths(rs, shape), _eighths(rs, shape), _weights(rs, shape[-1], shape[1], pad, dt=dt)
        want_out, want_gx, gw64 = _reference(x, go, w, pad, active, dt)
        out, gx, gw = _run(shape, dt, off, x, go, w, pad, active)
        assert_bits(_wide(out), want_out, (shape, pad, active, "out"))
        assert_bits(_wide(gx), want_gx, (shape, pad, active, "grad_x"))
        assert_bits(_wide(gw), round16(gw64.astype(np.float32), dt), (shape, pad, active, "grad_w"))


# ---- 3. random data: the bounds of tests/test_tshift_cl_gpu.py::test_random_data, per clip ---------------------------------------
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_random_data(ci):
    shape, dt, off = CASES[ci]
    for table, (pad, active) in itertools.product(_tables(shape, dt), SWEEP):
        what = (_id(CASES[ci]), table, "pad", pad, "active", active)
        x, go, w, want_out, want_gx, gw64 = _inputs(ci, "random", table, pad, active)
        out, gx, gw = _run_cl(shape, dt, off, x, go, w, pad, active)
        if dt in (F32, F64) or not active:
            assert_bits(_wide(out), want_out, what + ("out",))
            assert_bits(_wide(gx), want_gx, what + ("grad_x",))
        else:
            assert_ulp_close(_wide(out), want_out, dt, FLOOR16, what + ("out",))
            assert_ulp_close(_wide(gx), want_gx, dt, FLOOR16, what + ("grad_x",))
        for n in range(shape[0]):
            if dt in (F32, F64):
                err = np.abs(_wide(gw)[n].astype(np.float64) - gw64[n]).max() / max(np.abs(gw64[n]).max(), 1e-30)
                print(what, "clip", n, "grad_w relative error", err)
                assert err < 1e-5, what + ("grad_w", n, err)
            else:
                assert_gw_entries(_wide(gw)[n], gw64[n], dt, what + ("grad_w", n))


# ---- 4. determinism ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [((2, 8, 196, 64), F16, 0), RECORDS], ids=_id)
def test_the_weight_gradient_is_deterministic(case):
    ci = CASES.index(case)
    for active in (0, 1):
        x, go, w = _inputs(ci, "random", "specials", 0, active)[:3]
        a = _run_cl(*case, x, go, w, 0, active)[2]
        b = _run_cl(*case, x, go, w, 0, active)[2]
        assert _same_bits(a, b), (case, active)


# ---- 5. refusals launch nothing ----------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    shape = (2, 3, 5, 8)
    N, T, M, C = shape
    x = torch.randn(shape, device="cuda")
    w = torch.randn(N, C, device="cuda")
    inv, uns = "invalid argument", "unsupported dtype"
    ws_bytes = abi.backward_workspace(_view(x), 0, 1, **KW).numel()
    assert ws_bytes == abi.backward_workspace(_view(x), 0, 1, shift_dim0=True, frames=True).numel() >= N * C * 24
    for active in (0, 1):
        out, gx, gw, ws = _painted(shape), _painted(shape), _painted((N, C)), _painted((ws_bytes,), torch.uint8)
        # the bit without SHIFT_DIM0: an unknown dtype bit
        _refused(uns, lambda: abi.forward(_view(x), w, 0, active, out=_view(out), clip_frames=True), out)
        _refused(uns, lambda: abi.backward(_view(x), w, _view(x), 0, active, grad_x=_view(gx), grad_w=gw, workspace=ws, clip_frames=True), gx, gw, ws)
        # beside FRAMES or PER_CLIP, on the channels-last tensors the bit asks for
        for other in (dict(frames=True), dict(per_clip=True)):
            _refused(inv, lambda: abi.forward(_view(x), w, 0, active, out=_view(out), **KW, **other), out)
            _refused(inv, lambda: abi.backward(_view(x), w, _view(x), 0, active, grad_x=_view(gx), grad_w=gw, workspace=ws, **KW, **other),
                     gx, gw, ws)
        # ... and what the neighbours refuse, they refuse: FRAMES | PER_CLIP
        _refused(inv, lambda: abi.forward(_view(x), w, 0, active, out=_view(out), shift_dim0=True, frames=True, per_clip=True), out)
        # out == x
        mine = _painted(shape)
        _refused(inv, lambda: abi.forward(_view(mine), w, 0, active, out=_view(mine), **KW), mine)
        # a segment-major or an NCHW-dense tensor in any one position
        segment, dense = _painted((N, T, C, M)), _painted((N, C, T, M))
        for other in (segment.transpose(1, 2), dense):
            _refused(inv, lambda: abi.forward(_view(x), w, 0, active, out=other, **KW), other)
            _refused(inv, lambda: abi.forward(other, w, 0, active, out=_view(out), **KW), out)
            _refused(inv, lambda: abi.backward(_view(x), w, _view(x), 0, active, grad_x=other, grad_w=gw, workspace=ws, **KW), other, gw, ws)
            _refused(inv, lambda: abi.backward(other, w, _view(x), 0, active, grad_x=_view(gx), grad_w=gw, workspace=ws, **KW), gx, gw, ws)
            _refused(inv, lambda: abi.backward(_view(x), w, other, 0, active, grad_x=_view(gx), grad_w=gw, workspace=ws, **KW), gx, gw, ws)
        # ndim 1, a cut window
        _refused(inv, lambda: abi.forward(x.view(N, T * M, C).permute(0, 2, 1), w, 0, active, out=out.view(N, T * M, C).permute(0, 2, 1), **KW), out)
        b, new = abi.check_borders([N, C, T, M], [[1, 0], [0, 0]], 2)
        cut = _painted((N, new[2], new[3], C))
        _refused(inv, lambda: abi.forward(_view(x), w, 0, active, b, out=_view(cut), **KW), cut)
        # the x == NULL form
        p = abi.problem(_view(x), 0, active, None, **KW)

        def null_form():
            abi.check(abi.lib().shiftnd_backward(ctypes.byref(p), x.data_ptr(), abi.strides5(_view(x)), None, None, w.data_ptr(),
                                                 gx.data_ptr(), abi.strides5(_view(gx)), None, ws.data_ptr(), ws.numel(), None), "x == NULL")

        _refused(inv, null_form, gx, ws)
        # a quantized dtype, and the quantized entry point
        xq, outq = torch.zeros(shape, dtype=torch.int8, device="cuda"), _painted(shape, torch.int8)
        _refused(uns, lambda: abi.forward(_view(xq), w, 0, active, out=_view(outq), **KW), outq)
        pq = abi.problem(_view(xq), 0, active, None, **KW)
        assert abi.lib().shiftnd_backward_workspace_bytes(ctypes.byref(pq)) == 0
        wq = torch.zeros(N, C, dtype=torch.int32, device="cuda")

        def quantized():
            abi.check(abi.lib().shiftnd_forward_quantized(ctypes.byref(pq), xq.data_ptr(), abi.strides5(_view(xq)), wq.data_ptr(), abi.I32, 0, 0,
                                                          outq.data_ptr(), abi.strides5(_view(outq)), None), "shiftnd_forward_quantized")

        _refused(uns, quantized, outq)
        # a workspace one byte short; then the served call with exactly the planned workspace
        _refused("workspace", lambda: abi.backward(_view(x), w, _view(x), 0, active, grad_x=_view(gx), grad_w=gw, workspace=ws[:-1], **KW), gx, gw, ws)
        abi.backward(_view(x), w, _view(x), 0, active, grad_x=_view(gx), grad_w=gw, workspace=ws, **KW)
        assert abi.last_kernel() == "frames_backward" and abi.last_path() == abi.PATH_CL
        assert bool(torch.isfinite(gw).all()) and bool(torch.isfinite(gx).all())


def test_empty_problems_zero_the_whole_table_gradient():
    """PATH_EMPTY, the N * C entries of grad_w zeroed, nothing else written (an empty torch tensor has no address: the pointers are a
    painted buffer's)"""
    L = abi.lib()
    for shape in ((3, 2, 0, 8), (3, 0, 5, 8)):
        N, C = shape[0], shape[-1]
        w = torch.randn(N, C, device="cuda")
        x = torch.empty(shape, device="cuda")
        st = abi.strides5(_view(x))
        for active in (0, 1):
            p = abi.problem(_view(x), 0, active, None, **KW)
            abi.forward(_view(x), w, 0, active, out=_view(torch.empty_like(x)), **KW)
            assert abi.last_path() == abi.PATH_EMPTY
            some, ws = _painted((64,)), _painted((64,), torch.uint8)
            gw = torch.full((N, C), float("nan"), device="cuda")
            abi.check(L.shiftnd_backward(ctypes.byref(p), some.data_ptr(), st, some.data_ptr(), st, w.data_ptr(), some.data_ptr(), st,
                                         gw.data_ptr(), ws.data_ptr(), ws.numel(), None), "an empty backward")
            torch.cuda.synchronize()
            assert abi.last_path() == abi.PATH_EMPTY and bool((gw == 0).all()) and _untouched(some, ws)


# ---- 6. red zones: x, grad_out, out, grad_x, the [N, C] table, grad_w and the workspace between painted zones -------------------------
GUARDED = CL_GUARDED + [((3, 2, 300, 8), F32, 0)]      # (the third entry: the bases' offset in BYTES)


@pytest.mark.parametrize("shape,dt,off", GUARDED, ids=lambda v: str(v).split(".")[-1].replace(" ", ""))
def test_red_zones(shape, dt, off):
    N, T, C = shape[0], shape[1], shape[-1]
    rs = np.random.RandomState(52)
    dev = torch.device("cuda")
    for pad, active, table in itertools.product((0, 3), (0, 1), ("specials", "runs")):
        what = (shape, str(dt), "pad", pad, "offset", off, "active", active, table)
        x, go, w = _eighths(rs, shape), _eighths(rs, shape), _table(rs, shape, dt, pad, table)
        clips = [_reference(x[n:n + 1], go[n:n + 1], w[n], pad, active, dt) for n in range(N)]
        want_out, want_gx = (np.concatenate([c[i] for c in clips]) for i in range(2))
        gw64 = np.stack([c[2] for c in clips])
        as_dt = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt))
        X, OUT, G, GX = (RZ.Guarded(shape, dt, dev, offset_bytes=off) for _ in range(4))
        W, GW = RZ.Guarded((N, C), dt, dev), RZ.Guarded((N, C), dt, dev)      # (the last row of the table ends at its red zone)
        ws_bytes = abi.backward_workspace(_view(X.t), pad, active, **KW).numel()
        assert ws_bytes == abi.backward_workspace(_view(X.t), pad, active, shift_dim0=True, frames=True).numel() >= N * C * 24
        WS = RZ.Guarded((ws_bytes,), torch.uint8, dev)

        def forward():
            abi.forward(_view(X.t), W.t, pad, active, out=_view(OUT.t), **KW)
            return abi.last_kernel()

        def backward():
            abi.backward(_view(G.t), W.t, _view(X.t), pad, active, grad_x=_view(GX.t), grad_w=GW.t, workspace=WS.t, **KW)
            return abi.last_kernel()

        names = _names(shape, dt, off // _es(dt), active)
        assert RZ.run_guarded(forward, [("x", X, as_dt(x)), ("w", W, as_dt(w))], [("out", OUT)], [as_dt(want_out)],
                              what + ("forward",)) == names[0]
        want_gw = as_dt(gw64) if dt in (F32, F64) else as_dt(gw64.astype(np.float32))
        assert RZ.run_guarded(backward, [("grad_out", G, as_dt(go)), ("x", X, as_dt(x)), ("w", W, as_dt(w))],
                              [("grad_x", GX), ("grad_w", GW), ("workspace", WS)], [as_dt(want_gx), want_gw, None],
                              what + ("backward",)) == names[1]


# ---- 7. through the ops and the functions ----------------------------------------------------------------------------------------
def _op_table(rs, x, T, wdt, groups=None):
    N, C = x.shape[0] // T, x.shape[1]
    return torch.from_numpy(rs.uniform(-T - 1, T + 1, size=(N, groups or C))).to(wdt)


@pytest.mark.parametrize("dt,wdt", [(F32, F32), (F64, F64), (F16, F16), (BF16, BF16), (F16, F32), (BF16, F32)],
                         ids=lambda d: str(d).split(".")[-1])
def test_preserve_format_is_the_default_call_in_the_arguments_strides(dt, wdt):
    """out and x.grad: torch.equal to the default-format call, in the input's / the gradient's strides; table.grad: in the table's
    dtype, within the bounds of tests/test_tshift_cl_gpu.py::test_the_op_equals_the_cpu_op against the CPU op (fp32 / fp64 tables: 1e-5
    of the largest entry; 16-bit tables: per entry, against the CPU op on the widened tensors)"""
    rs = np.random.RandomState(53)
    cdt = dt if dt in (F32, F64) else F32
    for (x, T), pad, active, groups in itertools.product(_channels_last_inputs(dt, rs), (0, 1, 2, 3, 4), (False, True), (None, "G")):
        C = x.shape[1]
        G = None if groups is None else (C // 2 if C % 2 == 0 else 1)
        what = (tuple(x.shape), pad, active, G)
        go = torch.from_numpy(rs.uniform(-1, 1, size=tuple(x.shape))).to(dt)
        w = _op_table(rs, x, T, wdt, G)
        xc, wc = x.to(cdt).contiguous().requires_grad_(True), w.to(cdt).clone().requires_grad_(True)
        wc_full = wc if G is None else wc.repeat_interleave(C // G, dim=1)      # (the expansion of _per_clip_table, its gradient kept)
        wc_full.retain_grad()
        torch.autograd.backward(temporal_shift_learnable_per_clip_func(xc, wc_full, T, pad, active), go.to(cdt))
        xg, wg = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
        assert xg.stride() == x.stride()
        go_cl = torch.empty_like(xg).copy_(go.cuda())
        assert go_cl.stride() == x.stride()
        out = temporal_shift_learnable_per_clip_func(xg, wg, T, pad, active, memory_format=KEEP)
        assert abi.last_kernel().startswith("frames_") and abi.last_path() == abi.PATH_CL and out.stride() == xg.stride(), what
        gx, gw = torch.autograd.grad(out, (xg, wg), go_cl)
        assert gx.stride() == go_cl.stride() and gw.shape == w.shape and gw.dtype == wdt, what
        # (autograd ran the backward on its own thread; the kernel names are per thread: the same call from this one)
        full = wg.detach() if G is None else wg.detach().repeat_interleave(C // G, dim=1)
        gx_op, gw_op = OPS._temporal_shift_learnable_per_clip_cl_backward(go_cl, full, xg.detach(), T, pad, active)
        assert abi.last_kernel().startswith("frames_backward") and gx_op.stride() == go_cl.stride() and torch.equal(gx_op, gx), what
        if G is None:
            assert torch.equal(gw_op, gw), what
        # the default-format call: the same values, contiguous
        xp, wp = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
        plain = temporal_shift_learnable_per_clip_func(xp, wp, T, pad, active)
        assert abi.last_kernel().startswith("tshift_forward") and plain.is_contiguous() and torch.equal(plain, out), what
        gxp, gwp = torch.autograd.grad(plain, (xp, wp), go.cuda())
        assert gxp.is_contiguous() and torch.equal(gxp, gx), what
        # a contiguous gradient with the channels-last input: the plain route's contiguous grad_x, the same values
        gx2, gw2 = OPS._temporal_shift_learnable_per_clip_cl_backward(go.cuda(), full, xg.detach(), T, pad, active)
        assert abi.last_kernel().startswith("tshift_backward") and gx2.is_contiguous() and torch.equal(gx2, gx), what
        gw64 = wc.grad.double().numpy()
        for n in range(w.shape[0]):
            if wdt in (F32, F64):
                assert np.abs(_wide(gw)[n].astype(np.float64) - gw64[n]).max() <= 1e-5 * max(np.abs(gw64[n]).max(), 1e-30), what + (n,)
            else:
                # a 16-bit table: the kernel's [N, C] gradient per entry, against the CPU op's gradient of the expanded table; a group's
                # entry is autograd's sum of its k = C // G 16-bit entries e -- in whatever order and whether it adds in 16 bits or in
                # fp32 and rounds once, it lies within k * u * sum |e| of their exact sum (k - 1 additions and one rounding, each within
                # the unit roundoff u = 2^-11 for fp16, 2^-8 for bf16, of a value no larger than sum |e|)
                assert_gw_entries(_wide(gw_op)[n], wc_full.grad.double().numpy()[n], dt, what + ("the expanded table's grad", n))
                if G is not None:
                    k, u = C // G, 2.0 ** (-11 if dt == F16 else -8)
                    e = gw_op[n].double().view(G, k)
                    assert bool(((gw[n].double() - e.sum(1)).abs() <= k * u * e.abs().sum(1)).all()), what + ("a group's grad", n)
        # the fixed op
        s = torch.round(w.float()).long().cuda()
        xf = x.cuda().requires_grad_(True)
        fixed = temporal_shift_per_clip_func(xf, s, T, pad, memory_format=KEEP)
        assert abi.last_kernel().startswith("frames_forward") and fixed.stride() == x.stride(), what
        gxf, = torch.autograd.grad(fixed, xf, go_cl)
        assert OPS._temporal_shift_per_clip_cl_backward(go_cl, s if G is None else s.repeat_interleave(C // G, dim=1), T, pad).stride() == go_cl.stride()
        assert abi.last_kernel().startswith("frames_forward"), what + ("the backward is the forward kernel under the negated table",)
        xf2 = x.cuda().requires_grad_(True)
        fixed2 = temporal_shift_per_clip_func(xf2, s, T, pad)
        gxf2, = torch.autograd.grad(fixed2, xf2, go.cuda())
        assert fixed2.is_contiguous() and torch.equal(fixed, fixed2) and gxf.stride() == go_cl.stride() and torch.equal(gxf, gxf2), what


def test_other_inputs_give_exactly_the_default_result():
    """a contiguous input and a view that is not dense: the plain per-clip route, contiguous results"""
    rs = np.random.RandomState(54)
    T = 3
    base = torch.from_numpy(rs.uniform(-1, 1, size=(6, 8, 4, 10))).float().cuda()
    for x0 in (base[..., :5].contiguous(), base.contiguous(memory_format=torch.channels_last)[..., ::2]):
        assert x0.shape == (6, 8, 4, 5)
        w0 = _op_table(rs, x0, T, F32).cuda()
        go = torch.randn(6, 8, 4, 5, device="cuda")
        res = []
        for fmt in (torch.contiguous_format, KEEP):
            x, w = x0.detach().requires_grad_(True), w0.clone().requires_grad_(True)
            out = temporal_shift_learnable_per_clip_func(x, w, T, 0, True, memory_format=fmt)
            assert abi.last_kernel().startswith("tshift_forward") and out.is_contiguous()
            res.append((out.detach(),) + torch.autograd.grad(out, (x, w), go))
            s = torch.round(w0).long()
            fixed = temporal_shift_per_clip_func(x0, s, T, 0, memory_format=fmt)
            assert abi.last_kernel().startswith("tshift_forward") and fixed.is_contiguous()
            res[-1] += (fixed,)
        assert res[0][1].is_contiguous() and res[1][1].is_contiguous()
        for a, b in zip(*res):
            assert torch.equal(a, b)


# ---- 8. the fixed op ----------------------------------------------------------------------------------------------------------
def test_the_fixed_ops_node_keeps_the_table_alone():
    """the backward works after the input has been overwritten and freed: no kernel reads it"""
    T = 4
    x = torch.randn(8, 16, 5, 5, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
    s = torch.randint(-3, 4, (2, 16), device="cuda")
    go = torch.randn(8, 16, 5, 5, device="cuda").contiguous(memory_format=torch.channels_last)
    want, = torch.autograd.grad(temporal_shift_per_clip_func(x, s, T, 0, memory_format=KEEP), x, go)
    seen = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: seen.append(tuple(t.shape)) or t, lambda t: t):
        out = temporal_shift_per_clip_func(x, s, T, 0, memory_format=KEEP)
    assert seen == [(2, 16)]
    with torch.no_grad():
        x.fill_(float("nan"))
    got, = torch.autograd.grad(out, x, go)
    assert got.stride() == go.stride() and torch.equal(got, want)


def test_a_float_table_is_rounded_half_to_even():
    T, C = 5, 8
    x = torch.randn(2 * T, C, 3, 3, device="cuda").contiguous(memory_format=torch.channels_last)
    halves = torch.tensor([[0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5, 0.49], [-3.5, 0.51, 1.49, 2.51, -0.51, 4.5, -4.5, 0.0]], device="cuda")
    whole = torch.tensor([[0, 2, 2, 0, -2, -2, 4, 0], [-4, 1, 1, 3, -1, 4, -4, 0]], device="cuda")
    for dt, tdt in ((F32, F32), (F16, F16), (BF16, F32), (F64, F64)):
        xs = x.to(dt)
        got = temporal_shift_per_clip_func(xs, halves.to(tdt), T, 2, memory_format=KEEP)
        assert abi.last_kernel() == "frames_forward", dt      # (rows of 16 bytes and more: whole pieces)
        assert got.stride() == xs.stride() and torch.equal(got, temporal_shift_per_clip_func(xs, whole, T, 2, memory_format=KEEP)), dt
        assert torch.equal(got, temporal_shift_per_clip_func(xs, whole, T, 2)), dt


def test_a_bf16_tensor_under_a_shift_above_256_is_exact():
    """257 is no bf16 value: the table of a 16-bit tensor is fp32"""
    T, C = 300, 8
    x = torch.randn(2 * T, C, 2, 1, device="cuda").to(BF16).contiguous(memory_format=torch.channels_last)
    assert x.stride(1) == 1 and not x.is_contiguous()
    s = torch.zeros(2, C, dtype=torch.long, device="cuda")
    s[0, 1], s[1, 2], s[1, 3] = 257, -259, 1
    out = temporal_shift_per_clip_func(x, s, T, 2, memory_format=KEEP)      # periodic: out[t] = x[(t - s) mod T]
    assert abi.last_kernel() == "frames_forward" and out.stride() == x.stride()
    clips, got = x.view(2, T, C, 2), out.view(2, T, C, 2)
    for n, c in itertools.product(range(2), range(C)):
        assert torch.equal(got[n, :, c], torch.roll(clips[n, :, c], int(s[n, c]), 0)), (n, c)


# ---- 9. a module training step, a forward graph capture and replay ---------------------------------------------------------------
def test_the_module_trains_one_step():
    torch.manual_seed(5)
    N, T, C, G = 2, 8, 64, 8
    net = torch.nn.Linear(C, G).cuda()                            # an OffsetNet in one layer: the clip's channel means -> G offsets
    shift = torchshifts.LearnablePerClipTemporalShift(T, active_flag=True, memory_format=KEEP)
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    x = torch.randn(N * T, C, 14, 14, device="cuda").contiguous(memory_format=torch.channels_last)
    before = net.weight.detach().clone()
    out = shift(x, net(x.mean((2, 3)).view(N, T, C).mean(1)))
    assert abi.last_kernel() == "frames_active_forward" and out.stride() == x.stride()
    out.square().mean().backward()
    opt.step()
    assert torch.isfinite(net.weight).all() and not torch.equal(net.weight.detach(), before)


def test_forward_graph_capture_and_replay():
    x = torch.randn(8, 16, 6, 6, device="cuda").contiguous(memory_format=torch.channels_last)
    w = torch.linspace(-2, 2, 32, device="cuda").view(2, 16)
    want = OPS.temporal_shift_learnable_per_clip_cl(x, w, 4, 0, True)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        OPS.temporal_shift_learnable_per_clip_cl(x, w, 4, 0, True)   # (warm-up on the capture stream)
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            out = OPS.temporal_shift_learnable_per_clip_cl(x, w, 4, 0, True)
    x.copy_(torch.randn_like(x))
    want2 = OPS.temporal_shift_learnable_per_clip_cl(x, w, 4, 0, True)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert out.stride() == x.stride() and torch.equal(out, want2) and not torch.equal(want, want2)
    assert torch.equal(want2, PLAIN.temporal_shift_learnable_per_clip(x, w, 4, 0, True))
