"""The per-clip temporal shift on the GPU: SHIFTND_SHIFT_DIM0 | SHIFTND_PER_CLIP through the C ABI (csrc/shiftnd_tshift.hip) and
through torch.ops.torchshifts_per_clip.  Buffers and views are those of tests/test_tshift_gpu.py -- (N, T, C, M) buffers seen as
[N, C, T, M] problems -- with a [N, C] table; the reference is that file's `_reference` (the C oracle's 1-D evaluation) applied to
clip n under row n.  Row n is `_weights(rs, C, T, turn=pad + n)`: the rows differ, so a kernel that ignores n fails every case.

The cases are that file's, and two whose planes are above 8 KiB -- several workgroups per (n, c) line, the only shapes where the
per-clip partial-record index ((chunk * N + n) * C + c) differs from the per-channel one ((n * chunks + chunk) * C + c).
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import torchshifts
from torchshifts import abi
from torchshifts.functional import (temporal_shift_func, temporal_shift_learnable_per_clip_func, temporal_shift_per_clip_func)

import redzone as RZ
from exact16_cases import FLOOR16, assert_bits, assert_gw_entries, assert_ulp_close, round16
from test_tshift_gpu import (BWD, BWD_R, FWD, FWD_R, _buffer, _eighths, _id, _put, _reference, _run, _view, _weights, _whole, _wide)

pytestmark = pytest.mark.gpu

OPS = torch.ops.torchshifts_per_clip
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64

# (N, T, C, M), dtype, elements the bases are offset by
WHOLE_CASES = [((2, 3, 5, 8), F16, 0), ((2, 3, 5, 4), F32, 0), ((2, 3, 5, 2), F64, 0), ((3, 2, 7, 24), BF16, 0), ((1, 9, 3, 16), F32, 0),
               ((2, 8, 64, 32), F16, 0)]
RAGGED_CASES = [((2, 3, 5, 49), F16, 0), ((2, 3, 5, 49), BF16, 0), ((2, 3, 5, 49), F32, 0), ((2, 4, 6, 3), F16, 0), ((2, 3, 5, 5), F16, 1),
                ((2, 8, 64, 196), F16, 0)]
DEGENERATE_CASES = [((2, 1, 5, 8), F32, 0), ((2, 3, 1, 8), F32, 0), ((2, 4, 6, 1), F32, 0)]
CHUNKED_CASES = [((2, 2, 3, 4100), F32, 0),    # 16400-byte planes: three workgroups per (n, c) line
                 ((3, 2, 2, 6152), F16, 0)]    # 12304-byte planes: two
CASES = WHOLE_CASES + RAGGED_CASES + DEGENERATE_CASES + CHUNKED_CASES
SWEEP = list(itertools.product(range(5), (0, 1)))


def _table(rs, N, C, T, pad, quarters=True):
    return np.stack([_weights(rs, C, T, pad + n, quarters) for n in range(N)])


@functools.lru_cache(maxsize=None)
def _inputs(ci, kind, pad, active):
    """x, go (N, T, C, M) and the [N, C] table of CASES[ci] -- fp64 arrays holding values of the case's dtype -- and the per-clip
    reference: out, grad_x, and grad_w [N, C] from the fp64 oracle.  Computed once, shared, never written to."""
    shape, dt, _ = CASES[ci]
    N, T, C, M = shape
    rs = np.random.RandomState(1000 * ci + 10 * pad + active + (500 if kind == "random" else 0))
    if kind == "exact":
        x, go, w = _eighths(rs, shape), _eighths(rs, shape), _table(rs, N, C, T, pad)
    else:
        narrow = (lambda a: torch.from_numpy(a).to(dt).double().numpy())
        x, go = narrow(rs.uniform(-1, 1, size=shape)), narrow(rs.uniform(-1, 1, size=shape))
        w = narrow(_table(rs, N, C, T, pad, quarters=False))
    clips = [_reference(x[n:n + 1], go[n:n + 1], w[n], pad, active, dt) for n in range(N)]
    out, gx = np.concatenate([c[0] for c in clips]), np.concatenate([c[1] for c in clips])
    gw64 = np.stack([c[2] for c in clips])
    for a in (out, gx, gw64):
        a.setflags(write=False)
    return x, go, w, out, gx, gw64


def _run_per_clip(shape, dt, off, x, go, w, pad, active, wdt=None):
    """the per-clip forward and backward on (N, T, C, M) buffers -> out, grad_x, grad_w [N, C], the two kernel names"""
    wd = torch.from_numpy(np.ascontiguousarray(w)).to(wdt or dt).cuda()
    xd, gd = _put(x, dt, off), _put(go, dt, off)
    out, gx = _buffer(shape, dt, off, fill=0xA5), _buffer(shape, dt, off, fill=0xA5)
    abi.forward(_view(xd), wd, pad, active, out=_view(out), shift_dim0=True, per_clip=True)
    kf = abi.last_kernel()
    assert abi.last_path() == abi.PATH_PLANE
    gw = torch.full_like(wd, float("nan"))
    abi.backward(_view(gd), wd, _view(xd), pad, active, grad_x=_view(gx), grad_w=gw, shift_dim0=True, per_clip=True)
    assert abi.last_path() == abi.PATH_PLANE
    return out, gx, gw, kf, abi.last_kernel()


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_exact_data(ci):
    shape, dt, off = CASES[ci]
    names = (FWD, BWD) if _whole(shape, dt, off) else (FWD_R, BWD_R)
    for pad, active in SWEEP:
        what = (_id(CASES[ci]), "pad", pad, "active", active)
        x, go, w, want_out, want_gx, gw64 = _inputs(ci, "exact", pad, active)
        out, gx, gw, kf, kb = _run_per_clip(shape, dt, off, x, go, w, pad, active)
        assert (kf, kb) == names, what + (kf, kb)
        assert_bits(_wide(out), want_out, what + ("out",))
        assert_bits(_wide(gx), want_gx, what + ("grad_x",))
        if dt in (F32, F64):
            assert np.array_equal(_wide(gw).astype(np.float64), gw64), what + ("grad_w",)
        else:
            assert_bits(_wide(gw), round16(gw64.astype(np.float32), dt), what + ("grad_w, the fp64 sum rounded once",))
            # fp32 weights with the 16-bit tensor: the same bits in out and grad_x, grad_w the sum itself
            out2, gx2, gw2, kf2, kb2 = _run_per_clip(shape, dt, off, x, go, w, pad, active, wdt=F32)
            assert (kf2, kb2) == names and gw2.dtype == F32, what
            assert torch.equal(out2, out) and torch.equal(gx2, gx), what + ("mixed out / grad_x",)
            assert np.array_equal(_wide(gw2).astype(np.float64), gw64), what + ("mixed grad_w",)


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_random_data(ci):
    """the bounds of test_tshift_gpu.py::test_random_data, per clip: the reference of clip n is the oracle's on clip n"""
    shape, dt, off = CASES[ci]
    for pad, active in SWEEP:
        what = (_id(CASES[ci]), "pad", pad, "active", active)
        x, go, w, want_out, want_gx, gw64 = _inputs(ci, "random", pad, active)
        out, gx, gw, _, _ = _run_per_clip(shape, dt, off, x, go, w, pad, active)
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


AGREE = [CASES.index(c) for c in (((2, 3, 5, 4), F32, 0), ((2, 3, 5, 49), F32, 0), ((2, 3, 5, 8), F16, 0), ((2, 2, 3, 4100), F32, 0),
                                  ((3, 2, 2, 6152), F16, 0))]


@pytest.mark.parametrize("ci", AGREE, ids=[_id(CASES[i]) for i in AGREE])
def test_equal_rows_are_the_per_channel_call(ci):
    """a table whose rows are all equal: out and grad_x are the per-channel flagged call's, bit for bit, and grad_w summed over the
    clips is its grad_w within the random-data bound (fp32 tables, also for the fp16 tensors: N + 1 narrowings of fp64 sums to fp32,
    6e-8 each, against 1e-5 of the largest entry)"""
    shape, dt, off = CASES[ci]
    N, T, C, M = shape
    for pad, active in SWEEP:
        what = (_id(CASES[ci]), "pad", pad, "active", active)
        x, go, w, _, _, _ = _inputs(ci, "random", pad, active)
        row = w[0]
        out, gx, gw, kf, kb = _run_per_clip(shape, dt, off, x, go, np.tile(row, (N, 1)), pad, active, wdt=F32)
        out1, gx1, gw1, kf1, kb1 = _run(shape, dt, off, x, go, row, pad, active, wdt=F32)
        assert (kf, kb) == (kf1, kb1), what
        assert torch.equal(out.view(torch.uint8), out1.view(torch.uint8)), what + ("out",)
        assert torch.equal(gx.view(torch.uint8), gx1.view(torch.uint8)), what + ("grad_x",)
        total, ref = gw.double().sum(0).cpu().numpy(), gw1.double().cpu().numpy()
        err = np.abs(total - ref).max() / max(np.abs(ref).max(), 1e-30)
        print(what, "sum over clips against the per-channel grad_w", err)
        assert err < 1e-5, what + ("grad_w", err)


@pytest.mark.parametrize("ci", [CASES.index(c) for c in CHUNKED_CASES + [((2, 8, 64, 196), F16, 0)]])
def test_the_weight_gradient_is_deterministic(ci):
    shape, dt, off = CASES[ci]
    for active in (0, 1):
        x, go, w, _, _, _ = _inputs(ci, "random", 0, active)
        a = _run_per_clip(shape, dt, off, x, go, w, 0, active)[2]
        b = _run_per_clip(shape, dt, off, x, go, w, 0, active)[2]
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (shape, active)


@pytest.mark.parametrize("case", [((2, 3, 5, 8), F16, 0), ((2, 3, 5, 49), F32, 0), ((2, 2, 3, 4100), F32, 0)], ids=_id)
def test_per_channel_calls_keep_their_bits(case):
    """the flagged call WITHOUT the new bit, against the oracle as tests/test_tshift_gpu.py::test_exact_data compares it (a shape of
    several workgroups per line included: its records keep their index)"""
    shape, dt, off = case
    N, T, C, M = shape
    rs = np.random.RandomState(31)
    names = (FWD, BWD) if _whole(shape, dt, off) else (FWD_R, BWD_R)
    for pad, active in SWEEP:
        what = (_id(case), "pad", pad, "active", active)
        x, go, w = _eighths(rs, shape), _eighths(rs, shape), _weights(rs, C, T, pad)
        want_out, want_gx, gw64 = _reference(x, go, w, pad, active, dt)
        out, gx, gw, kf, kb = _run(shape, dt, off, x, go, w, pad, active)
        assert (kf, kb) == names, what + (kf, kb)
        assert_bits(_wide(out), want_out, what + ("out",))
        assert_bits(_wide(gx), want_gx, what + ("grad_x",))
        assert_bits(_wide(gw), round16(gw64.astype(np.float32), dt) if dt != F32 else gw64.astype(np.float32), what + ("grad_w",))


def test_refusals_launch_nothing():
    shape = (2, 3, 5, 8)
    N, T, C, M = shape
    x = torch.randn(shape, device="cuda")
    w = torch.randn(N, C, device="cuda")
    L = abi.lib()

    def painted(s=shape, dt=F32):
        return _buffer(s, dt, 0, fill=0xA5)

    def untouched(*ts):
        return all(bool((t.reshape(-1).view(torch.uint8) == 0xA5).all()) for t in ts)

    def refused(text, call, *outs):
        with pytest.raises(RuntimeError, match=text):
            call()
        torch.cuda.synchronize()
        assert untouched(*outs), text

    inv, uns = "invalid argument", "unsupported dtype"
    out, gx, gw, ws = painted(), painted(), painted((N, C)), painted((4096,), torch.uint8)
    # the bit without SHIFTND_SHIFT_DIM0: an unknown dtype bit
    refused(uns, lambda: abi.forward(_view(x), w, 0, 1, out=_view(out), per_clip=True), out)
    refused(uns, lambda: abi.backward(_view(x), w, _view(x), 0, 1, grad_x=_view(gx), grad_w=gw, workspace=ws, per_clip=True), gx, gw, ws)
    # together with SHIFTND_FRAMES, on the channels-last tensors that flag asks for
    xc, outc, gxc = (_buffer((N, T, M, C), F32, 0, fill=0xA5) for _ in range(3))
    cl = (lambda t: t.permute(0, 3, 1, 2))                        # (N, T, M, C) buffer -> [N, C, T, M]
    for active in (0, 1):
        refused(inv, lambda: abi.forward(cl(xc), w, 0, active, out=cl(outc), shift_dim0=True, frames=True, per_clip=True), outc)
        refused(inv, lambda: abi.backward(cl(xc), w, cl(xc), 0, active, grad_x=cl(gxc), grad_w=gw, workspace=ws, shift_dim0=True,
                                          frames=True, per_clip=True), gxc, gw, ws)
    # channels-last tensors without SHIFTND_FRAMES: the sparse forward's second layout takes a [C] table alone
    refused(inv, lambda: abi.forward(cl(xc), w, 0, 0, out=cl(outc), shift_dim0=True, per_clip=True), outc)
    # out == x: the in-place form takes a [C] table alone
    mine = painted()
    refused(inv, lambda: abi.forward(_view(mine), w, 0, 0, out=_view(mine), shift_dim0=True, per_clip=True), mine)
    # the x == NULL && grad_w == NULL form of shiftnd_backward
    p = abi.problem(_view(x), 0, False, None, shift_dim0=True, per_clip=True)

    def null_form():
        abi.check(L.shiftnd_backward(ctypes.byref(p), x.data_ptr(), abi.strides5(_view(x)), None, None, w.data_ptr(), gx.data_ptr(),
                                     abi.strides5(_view(gx)), None, ws.data_ptr(), ws.numel(), None), "x == NULL")

    refused(inv, null_form, gx, ws)
    # a quantized dtype, and the quantized entry point
    xq, outq = torch.zeros(shape, dtype=torch.int8, device="cuda"), painted(shape, torch.int8)
    refused(uns, lambda: abi.forward(_view(xq), w, 0, 0, out=_view(outq), shift_dim0=True, per_clip=True), outq)
    pq = abi.problem(_view(xq), 0, False, None, shift_dim0=True, per_clip=True)
    assert L.shiftnd_backward_workspace_bytes(ctypes.byref(pq)) == 0
    wq = torch.zeros(N, C, dtype=torch.int32, device="cuda")

    def quantized():
        abi.check(L.shiftnd_forward_quantized(ctypes.byref(pq), xq.data_ptr(), abi.strides5(_view(xq)), wq.data_ptr(), abi.I32, 0, 0,
                                              outq.data_ptr(), abi.strides5(_view(outq)), None), "shiftnd_forward_quantized")

    refused(uns, quantized, outq)
    # a workspace below the plan
    refused("workspace too small", lambda: abi.backward(_view(x), w, _view(x), 0, 1, grad_x=_view(gx), grad_w=gw, workspace=ws[:8],
                                                        shift_dim0=True, per_clip=True), gx, gw, ws)


# ---- red zones: the [N, C] table, grad_w and the workspace between painted zones too ----------------------------------------------
GUARDED = [((2, 3, 5, 8), F16), ((2, 3, 5, 49), F32), ((2, 2, 3, 4100), F32)]


@pytest.mark.parametrize("shape,dt", GUARDED, ids=lambda v: str(v).split(".")[-1].replace(" ", ""))
def test_red_zones(shape, dt):
    N, T, C, M = shape
    rs = np.random.RandomState(36)
    dev = torch.device("cuda")
    for pad, active in itertools.product((0, 3), (0, 1)):
        what = (shape, str(dt), "pad", pad, "active", active)
        x, go, w = _eighths(rs, shape), _eighths(rs, shape), _table(rs, N, C, T, pad)
        clips = [_reference(x[n:n + 1], go[n:n + 1], w[n], pad, active, dt) for n in range(N)]
        want_out, want_gx = (np.concatenate([c[i] for c in clips]) for i in range(2))
        gw64 = np.stack([c[2] for c in clips])
        as_dt = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt))
        X, OUT, G, GX = (RZ.Guarded(shape, dt, dev) for _ in range(4))
        W, GW = RZ.Guarded((N, C), dt, dev), RZ.Guarded((N, C), dt, dev)
        ws_bytes = abi.backward_workspace(_view(X.t), pad, active, shift_dim0=True, per_clip=True).numel()
        assert ws_bytes == abi.backward_workspace(_view(X.t), pad, active, shift_dim0=True).numel() >= N * C * 24
        WS = RZ.Guarded((ws_bytes,), torch.uint8, dev)

        def forward():
            abi.forward(_view(X.t), W.t, pad, active, out=_view(OUT.t), shift_dim0=True, per_clip=True)
            return abi.last_kernel()

        def backward():
            abi.backward(_view(G.t), W.t, _view(X.t), pad, active, grad_x=_view(GX.t), grad_w=GW.t, workspace=WS.t, shift_dim0=True,
                         per_clip=True)
            return abi.last_kernel()

        whole = _whole(shape, dt, 0)
        assert RZ.run_guarded(forward, [("x", X, as_dt(x)), ("w", W, as_dt(w))], [("out", OUT)], [as_dt(want_out)],
                              what + ("forward",)) == (FWD if whole else FWD_R)
        want_gw = as_dt(gw64) if dt in (F32, F64) else as_dt(gw64.astype(np.float32))
        assert RZ.run_guarded(backward, [("grad_out", G, as_dt(go)), ("x", X, as_dt(x)), ("w", W, as_dt(w))],
                              [("grad_x", GX), ("grad_w", GW), ("workspace", WS)], [as_dt(want_gx), want_gw, None],
                              what + ("backward",)) == (BWD if whole else BWD_R)


# ---- through the ops ----------------------------------------------------------------------------------------------------------------
def _op_inputs(rs, shape, T, pad):
    N, C = shape[0] // T, shape[1]
    x = torch.from_numpy(rs.uniform(-1, 1, size=shape)).float()
    go = torch.from_numpy(rs.uniform(-1, 1, size=shape)).float()
    w = torch.from_numpy(_table(rs, N, C, T, pad, quarters=False)).float()
    return x, go, w


def test_the_ops_equal_the_cpu_ops():
    """fp32: out and x.grad bit for bit, weights.grad within 1e-5 of the largest entry (the CPU sum is fp32); the fixed op is the
    learnable op's sparse out, and its x.grad the loop of temporal_shift_func"""
    rs = np.random.RandomState(37)
    for (shape, T), pad, active in itertools.product((((6, 5, 4, 8), 3), ((6, 5, 7, 7), 3), ((8, 6), 4), ((4, 3, 4100), 2)), range(5), (False, True)):
        what = (shape, pad, active)
        x, go, w = _op_inputs(rs, shape, T, pad)
        xc, wc = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        ref = temporal_shift_learnable_per_clip_func(xc, wc, T, pad, active)
        ref.backward(go)
        xg, wg = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
        out = temporal_shift_learnable_per_clip_func(xg, wg, T, pad, active)
        assert abi.last_kernel() in (FWD, FWD_R), what
        out.backward(go.cuda())
        assert out.is_contiguous() and wg.grad.shape == w.shape and wg.grad.dtype == F32
        assert torch.equal(out.detach().cpu(), ref.detach()) and torch.equal(xg.grad.cpu(), xc.grad), what
        gw64 = wc.grad.double().numpy()
        assert np.abs(wg.grad.cpu().double().numpy() - gw64).max() <= 1e-5 * max(np.abs(gw64).max(), 1e-30), what
        if not active:
            s = torch.round(w).long()
            xf = x.cuda().requires_grad_(True)
            fixed = temporal_shift_per_clip_func(xf, s.cuda(), T, pad)
            assert abi.last_kernel() in (FWD, FWD_R), what
            assert torch.equal(fixed.detach(), out.detach()), what + ("the fixed op is the sparse out",)
            assert torch.equal(temporal_shift_per_clip_func(x.cuda(), w.cuda(), T, pad), fixed.detach()), what + ("a float table",)
            fixed.backward(go.cuda())
            assert abi.last_kernel() in (FWD, FWD_R), what + ("the backward is the forward kernel under the negated table",)
            xl = x.clone().requires_grad_(True)
            torch.cat([temporal_shift_func(xl[n * T:(n + 1) * T], s[n], T, pad) for n in range(s.shape[0])], 0).backward(go)
            assert torch.equal(xf.grad.cpu(), xl.grad), what + ("the fixed op's x.grad",)


def test_sixteen_bit_tensors_through_the_ops():
    rs = np.random.RandomState(38)
    shape, T = (6, 5, 4, 8), 3
    x, go, w = _op_inputs(rs, shape, T, 0)
    for dt in (F16, BF16):
        xg, wg = x.to(dt).cuda().requires_grad_(True), w.cuda().requires_grad_(True)      # fp32 weights: what autocast hands the op
        out = temporal_shift_learnable_per_clip_func(xg, wg, T, 0, True)
        out.backward(go.to(dt).cuda())
        assert out.dtype == dt and xg.grad.dtype == dt and wg.grad.dtype == F32 and wg.grad.shape == w.shape
        direct = _buffer((2, T, 5, 32), dt, 0, fill=0xA5)
        abi.forward(_view(xg.detach().view(2, T, 5, 32)), w.cuda(), 0, 1, out=_view(direct), shift_dim0=True, per_clip=True)
        assert torch.equal(out.detach().view(torch.int16).view(-1), direct.view(torch.int16).view(-1))
        # the fixed op on a 16-bit tensor: an fp32 table, every shift exact -- the bits of the fp32 tensor's result narrowed
        s = torch.round(w).long().cuda()
        assert torch.equal(temporal_shift_per_clip_func(xg.detach(), s, T, 0).float(),
                           temporal_shift_per_clip_func(xg.detach().float(), s, T, 0))
    with pytest.raises(RuntimeError, match="same type"):
        OPS.temporal_shift_learnable_per_clip(x.cuda(), w.double().cuda(), T, 0, True)


def test_a_channels_last_input_gives_the_contiguous_result():
    rs = np.random.RandomState(39)
    shape, T = (6, 8, 5, 5), 3
    x, go, w = _op_inputs(rs, shape, T, 0)
    xc = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    xp = x.cuda().requires_grad_(True)
    wc, wp = w.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    out, ref = temporal_shift_learnable_per_clip_func(xc, wc, T, 0, True), temporal_shift_learnable_per_clip_func(xp, wp, T, 0, True)
    assert out.is_contiguous() and torch.equal(out, ref)
    out.backward(go.cuda())
    ref.backward(go.cuda())
    assert torch.equal(xc.grad, xp.grad) and torch.equal(wc.grad, wp.grad)
    s = torch.round(w).long().cuda()
    fixed = temporal_shift_per_clip_func(xc.detach(), s, T, 0)
    assert fixed.is_contiguous() and torch.equal(fixed, temporal_shift_per_clip_func(xp.detach(), s, T, 0))


def test_a_transposed_table_through_the_ops():
    """a [N, C] table that is the transpose of a [C, N] tensor (strides (1, N)): the library reads a dense array, so the adapters
    must hand it one in BOTH directions -- the fixed op's backward negates the table the node kept as the caller gave it"""
    rs = np.random.RandomState(40)
    for (shape, T), pad in itertools.product((((6, 5, 4, 8), 3), ((12, 6, 7, 7), 4)), (0, 2)):
        what = (shape, pad)
        x, go, w = _op_inputs(rs, shape, T, pad)
        s = torch.round(w).long()
        s_t, w_t = s.t().contiguous().cuda().t(), w.t().contiguous().cuda().t()
        assert not s_t.is_contiguous() and not w_t.is_contiguous() and torch.equal(s_t.cpu(), s)
        xl = x.clone().requires_grad_(True)
        ref = torch.cat([temporal_shift_func(xl[n * T:(n + 1) * T], s[n], T, pad) for n in range(s.shape[0])], 0)
        ref.backward(go)
        for table in (s_t, s_t.float(), s_t.double()):
            xf = x.cuda().requires_grad_(True)
            fixed = temporal_shift_per_clip_func(xf, table, T, pad)
            fixed.backward(go.cuda())
            assert torch.equal(fixed.detach().cpu(), ref.detach()), what + (table.dtype, "out")
            assert torch.equal(xf.grad.cpu(), xl.grad), what + (table.dtype, "x.grad")
        for active in (False, True):
            xa, wa = x.cuda().requires_grad_(True), w_t.clone(memory_format=torch.preserve_format).requires_grad_(True)
            xb, wb = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
            assert not wa.is_contiguous()
            out, want = temporal_shift_learnable_per_clip_func(xa, wa, T, pad, active), temporal_shift_learnable_per_clip_func(xb, wb, T, pad, active)
            out.backward(go.cuda())
            want.backward(go.cuda())
            assert torch.equal(out, want) and torch.equal(xa.grad, xb.grad) and torch.equal(wa.grad, wb.grad), what + (active,)


def test_the_module_trains_one_step():
    torch.manual_seed(5)
    N, T, C, G = 2, 8, 64, 8
    net = torch.nn.Linear(C, G).cuda()                            # an OffsetNet in one layer: the clip's channel means -> G offsets
    shift = torchshifts.LearnablePerClipTemporalShift(T, active_flag=True)
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    x = torch.randn(N * T, C, 14, 14, device="cuda")
    before = net.weight.detach().clone()
    out = shift(x, net(x.view(N, T, C, -1).mean((1, 3))))
    assert abi.last_kernel() == FWD       # 784-byte planes of fp32 at aligned bases: whole pieces
    out.square().mean().backward()
    opt.step()
    assert torch.isfinite(net.weight).all() and not torch.equal(net.weight.detach(), before)


# ---- the refusals of the three learnable families' HIP adapters that only a HIP tensor reaches ---------------------------------------
# Every case raises before a kernel is launched.  [4, 3, 2, 2], n_segment 2: N = 2 clips, C = 3; contiguous and channels-last.
_SAME_TYPE = "Expected tensor for %s to have the same type as tensor for %s; but type %s does not equal %s (while checking arguments for %s)"
LEARNABLE_FAMILIES = {   # family -> namespace, op stem, the table's shape
    "plain": (torch.ops.torchshifts, "temporal_shift_learnable", (3,)),
    "cl": (torch.ops.torchshifts, "temporal_shift_learnable_cl", (3,)),
    "per_clip": (OPS, "temporal_shift_learnable_per_clip", (2, 3)),
}


def _message(fn, *args):
    with pytest.raises(RuntimeError) as e:
        fn(*args)
    return str(e.value).split("\n")[0]


@pytest.mark.parametrize("channels_last", [False, True], ids=["contiguous", "channels_last"])
@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("family", sorted(LEARNABLE_FAMILIES))
def test_the_refusals_only_a_hip_tensor_reaches(family, backward, channels_last):
    ops, stem, table = LEARNABLE_FAMILIES[family]
    lay = (lambda t: t.contiguous(memory_format=torch.channels_last)) if channels_last else (lambda t: t)
    x, g = lay(torch.randn(4, 3, 2, 2, device="cuda")), lay(torch.randn(4, 3, 2, 2, device="cuda"))
    w = torch.zeros(table, device="cuda")
    # the _cl adapters speak under their own name for dense channels-last tensors and hand every other call to the plain adapters
    said = stem if (family != "cl" or channels_last) else "temporal_shift_learnable"
    if not backward:
        fwd = getattr(ops, "_%s_forward" % stem)
        assert _message(fwd, x, w.double(), 2, 0, True) == _SAME_TYPE % ("input", "weights", "Float", "Double", said + "_cuda")
        return
    bwd = getattr(ops, "_%s_backward" % stem)
    assert _message(bwd, g, w.double(), x, 2, 0, True) == _SAME_TYPE % ("grad", "weights", "Float", "Double", said + "_backward_cuda")
    assert _message(bwd, g.double(), w, x, 2, 0, True) == _SAME_TYPE % ("grad", "input", "Double", "Float", said + "_backward_cuda")
    # a gradient of another size: the _cl adapter falls back to the plain one, which refuses it under the plain name
    plain = "temporal_shift_learnable_per_clip" if family == "per_clip" else "temporal_shift_learnable"
    assert _message(bwd, g[:2], w, x, 2, 0, True) == plain + " backward: grad does not match the input"
