"""The learnable temporal shift on the GPU: SHIFTND_SHIFT_DIM0 through the C ABI (csrc/shiftnd_tshift.hip) -- permuted views of
(N, T, C, M) buffers, i.e. [N, C, T, M] problems with strides {T*C*M, M, C*M, 1} and [C] weights -- and through
torch.ops.torchshifts.temporal_shift_learnable.  The reference is the C oracle's 1-D evaluation on the permuted array
[N*M, C, T], widened to fp32 for 16-bit tensors and narrowed once.

Shapes are (N, T, C, M), the smallest at which these kernels can go wrong: one 16-byte unit per plane, units per plane that do not
divide what a thread keeps in flight, planes that are no whole pieces (8-, 4- and 2-byte units), bases one element off the 16-byte
grid, several workgroups, |w| up to T + 1 (reflect and symmetric fold twice, periodic wraps), and C, T or M of one (no fallback
exists under the flag).

Weight tables: 0, an exact integer, T + 1, -(T + 1), 0.5, -0.25, then quarters in [-(T + 1), T + 1]; a table of fewer than six
channels starts at another special under every padding, so that every special meets every case.  Exact data: tensors on eighths in
[-1, 1]: every product, blend and partial sum is exact in fp32, out and grad_x lie on 1/32 and are representable in fp16 and bf16.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import torchshifts
from torchshifts import abi
from oracle import oracle as O

import redzone as RZ
from exact16_cases import FLOOR16, assert_bits, assert_gw_entries, assert_ulp_close, round16

pytestmark = pytest.mark.gpu

OPS = torch.ops.torchshifts
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
FWD, FWD_R, BWD, BWD_R = "tshift_forward", "tshift_forward_ragged", "tshift_backward", "tshift_backward_ragged"

# (N, T, C, M), dtype, elements the bases are offset by
WHOLE_CASES = [((2, 3, 5, 8), F16, 0), ((2, 3, 5, 4), F32, 0), ((2, 3, 5, 2), F64, 0),
               ((3, 2, 7, 24), BF16, 0),      # three pieces per plane
               ((1, 9, 3, 16), F32, 0),       # |w| up to T + 1 = 10: double folds and wraps
               ((2, 8, 64, 32), F16, 0)]      # several workgroups
RAGGED_CASES = [((2, 3, 5, 49), F16, 0), ((2, 3, 5, 49), BF16, 0), ((2, 3, 5, 49), F32, 0),
                ((2, 4, 6, 3), F16, 0),       # 6-byte planes
                ((2, 3, 4, 3), F64, 0),
                ((2, 3, 5, 5), F16, 1), ((2, 3, 5, 8), F16, 1),   # bases one element off
                ((2, 8, 64, 196), F16, 0)]
DEGENERATE_CASES = [((2, 1, 5, 8), F32, 0), ((2, 3, 1, 8), F32, 0), ((2, 4, 6, 1), F32, 0)]
CASES = WHOLE_CASES + RAGGED_CASES + DEGENERATE_CASES


def _whole(shape, dt, off):
    es = torch.empty(0, dtype=dt).element_size()
    return (shape[3] * es) % 16 == 0 and (off * es) % 16 == 0


def _id(case):
    shape, dt, off = case
    return "%s-%s-off%d" % ("x".join(map(str, shape)), str(dt).split(".")[-1], off)


def _buffer(shape, dt, off, fill=None):
    """a dense device tensor whose base is `off` elements past an aligned allocation"""
    flat = torch.empty(int(np.prod(shape)) + off, dtype=dt, device="cuda")
    t = flat[off:].view(shape)
    if fill is not None:
        t.view(-1).view(torch.uint8).fill_(fill)
    return t


def _view(t):
    """(N, T, C, ...) buffer -> the [N, C, T, ...] problem the library sees"""
    return t.transpose(1, 2)


def _put(a, dt, off):
    t = _buffer(a.shape, dt, off)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dt))
    return t


def _wide(t):
    t = t.detach().cpu().contiguous()
    return (t if t.dtype in (F32, F64) else t.float()).numpy()


def _weights(rs, C, T, turn, quarters=True):
    w = rs.randint(-4 * (T + 1), 4 * (T + 1) + 1, size=C) / 4.0 if quarters else rs.uniform(-T - 1, T + 1, size=C)
    special = [0.0, 2.0, T + 1.0, -(T + 1.0), 0.5, -0.25]
    for i in range(min(C, 6)):
        w[i] = special[(i + turn) % 6]
    return w


def _lines(a):
    """(N, T, C, M...) array -> the 1-D problem [N*M, C, T] (contiguous)"""
    N, T, C = a.shape[:3]
    return np.ascontiguousarray(a.reshape(N, T, C, -1).transpose(0, 3, 2, 1)).reshape(-1, C, T)


def _frames(lines, shape):
    N, T, C = shape[:3]
    return np.ascontiguousarray(lines.reshape(N, -1, C, T).transpose(0, 3, 2, 1)).reshape(shape)


def _reference(x, go, w, pad, active, dt):
    """x, go: (N, T, C, M...) arrays holding values of dt; w: [C] values of the weights' type.  -> out, grad_x (values of dt, as the
    oracle's precision narrowed once) and grad_w from the fp64 oracle"""
    odt = np.float64 if dt == F64 else np.float32
    xl, gl, wl = _lines(x).astype(odt), _lines(go).astype(odt), w.reshape(-1, 1).astype(odt)
    out = _frames(O.forward(xl, wl, pad, active), x.shape)
    gx = _frames(O.backward(gl, wl, xl, pad, active)[0], x.shape)
    gw64 = O.backward(gl.astype(np.float64), wl.astype(np.float64), xl.astype(np.float64), pad, active)[1].reshape(-1)
    if dt in (F16, BF16):
        out, gx = round16(out, dt), round16(gx, dt)
    return out, gx, gw64


def _run(shape, dt, off, x, go, w, pad, active, wdt=None):
    """the flagged forward and backward on (N, T, C, M...) buffers -> out, grad_x, grad_w, the two kernel names"""
    wd = torch.from_numpy(w).to(wdt or dt).cuda()
    xd, gd = _put(x, dt, off), _put(go, dt, off)
    out, gx = _buffer(shape, dt, off, fill=0xA5), _buffer(shape, dt, off, fill=0xA5)
    abi.forward(_view(xd), wd, pad, active, out=_view(out), shift_dim0=True)
    kf = abi.last_kernel()
    assert abi.last_path() == abi.PATH_PLANE
    gw = torch.full_like(wd, float("nan"))
    abi.backward(_view(gd), wd, _view(xd), pad, active, grad_x=_view(gx), grad_w=gw, shift_dim0=True)
    assert abi.last_path() == abi.PATH_PLANE
    return out, gx, gw, kf, abi.last_kernel()


def _eighths(rs, shape):
    return rs.randint(-8, 9, size=shape) / 8.0


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_exact_data(case):
    shape, dt, off = case
    N, T, C, M = shape
    rs = np.random.RandomState(31)
    names = (FWD, BWD) if _whole(shape, dt, off) else (FWD_R, BWD_R)
    for pad, active in itertools.product(range(5), (0, 1)):
        what = (_id(case), "pad", pad, "active", active)
        x, go, w = _eighths(rs, shape), _eighths(rs, shape), _weights(rs, C, T, pad)
        want_out, want_gx, gw64 = _reference(x, go, w, pad, active, dt)
        out, gx, gw, kf, kb = _run(shape, dt, off, x, go, w, pad, active)
        assert (kf, kb) == names, what + (kf, kb)
        assert_bits(_wide(out), want_out, what + ("out",))
        assert_bits(_wide(gx), want_gx, what + ("grad_x",))
        if dt in (F32, F64):
            assert np.array_equal(_wide(gw).astype(np.float64), gw64), what + ("grad_w",)
        else:
            assert_bits(_wide(gw), round16(gw64.astype(np.float32), dt), what + ("grad_w, the fp64 sum rounded once",))
            # fp32 weights with the 16-bit tensor: the same bits in out and grad_x, grad_w the sum itself
            out2, gx2, gw2, kf2, kb2 = _run(shape, dt, off, x, go, w, pad, active, wdt=F32)
            assert (kf2, kb2) == names and gw2.dtype == F32, what
            assert torch.equal(out2, out) and torch.equal(gx2, gx), what + ("mixed out / grad_x",)
            assert np.array_equal(_wide(gw2).astype(np.float64), gw64), what + ("mixed grad_w",)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_random_data(case):
    shape, dt, off = case
    N, T, C, M = shape
    rs = np.random.RandomState(32)
    for pad, active in itertools.product(range(5), (0, 1)):
        what = (_id(case), "pad", pad, "active", active)
        narrow = (lambda a: torch.from_numpy(a).to(dt).double().numpy())
        x, go = narrow(rs.uniform(-1, 1, size=shape)), narrow(rs.uniform(-1, 1, size=shape))
        w = narrow(_weights(rs, C, T, pad, quarters=False))
        want_out, want_gx, gw64 = _reference(x, go, w, pad, active, dt)
        out, gx, gw, _, _ = _run(shape, dt, off, x, go, w, pad, active)
        if dt in (F32, F64) or not active:
            assert_bits(_wide(out), want_out, what + ("out",))
            assert_bits(_wide(gx), want_gx, what + ("grad_x",))
        else:
            assert_ulp_close(_wide(out), want_out, dt, FLOOR16, what + ("out",))
            assert_ulp_close(_wide(gx), want_gx, dt, FLOOR16, what + ("grad_x",))
        if dt in (F32, F64):
            err = np.abs(_wide(gw).astype(np.float64) - gw64).max() / max(np.abs(gw64).max(), 1e-30)
            print(what, "grad_w relative error", err)
            assert err < 1e-5, what + ("grad_w", err)
        else:
            assert_gw_entries(_wide(gw), gw64, dt, what + ("grad_w",))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_sparse_mode_is_the_segment_route_under_rint(case):
    shape, dt, off = case
    N, T, C, M = shape
    rs = np.random.RandomState(33)
    for pad in range(5):
        what = (_id(case), "pad", pad)
        x, go, w = rs.uniform(-1, 1, size=shape), rs.uniform(-1, 1, size=shape), _weights(rs, C, T, pad)
        out, gx, gw, _, _ = _run(shape, dt, off, x, go, w, pad, 0)
        gw_again = _run(shape, dt, off, x, go, w, pad, 0)[2]
        assert torch.equal(gw.view(torch.uint8), gw_again.view(torch.uint8)), what + ("grad_w is deterministic",)
        table = torch.zeros(C, 2, dtype=dt, device="cuda")
        table[:, 0] = torch.round(torch.from_numpy(w).to(dt)).cuda()
        xd, gd = _put(x, dt, off), _put(go, dt, off)
        fixed = _buffer(shape, dt, off, fill=0x5A)
        abi.forward(_view(xd), table, pad, 0, out=_view(fixed))
        assert not abi.last_kernel().startswith("tshift"), what
        assert torch.equal(out.view(torch.uint8), fixed.view(torch.uint8)), what + ("forward",)
        fixed_gx = _buffer(shape, dt, off, fill=0x5A)
        abi.backward_input(_view(gd), table, (N, C, T, M), pad, grad_x=_view(fixed_gx))
        assert torch.equal(gx.view(torch.uint8), fixed_gx.view(torch.uint8)), what + ("grad_x",)


def test_the_sparse_forward_keeps_nan_payloads_and_negative_zero():
    shape = (2, 3, 5, 8)
    bits = torch.randint(-2 ** 15, 2 ** 15, shape, dtype=torch.int16, device="cuda")   # every fp16 pattern, NaNs included
    bits[0, 0, 0, 0] = -2 ** 15                                                        # -0
    w = torch.tensor([0.0, 1.0, -1.0, 0.5, 2.0], dtype=F16, device="cuda")
    out = _buffer(shape, F16, 0, fill=0xA5)
    abi.forward(_view(bits.view(F16)), w, 2, 0, out=_view(out), shift_dim0=True)      # periodic: nothing is filled
    assert abi.last_kernel() == FWD
    shifts = [0, 1, -1, 0, 2]
    for c, s in enumerate(shifts):
        for t in range(3):
            assert torch.equal(out.view(torch.int16)[:, t, c], bits[:, (t - s) % 3, c]), (c, t)


def test_determinism_of_the_active_weight_gradient():
    shape, dt = (2, 8, 64, 196), F16
    rs = np.random.RandomState(34)
    x, go, w = rs.uniform(-1, 1, size=shape), rs.uniform(-1, 1, size=shape), _weights(rs, 64, 8, 0, quarters=False)
    a = _run(shape, dt, 0, x, go, w, 0, 1)[2]
    b = _run(shape, dt, 0, x, go, w, 0, 1)[2]
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("dt,kernels", [(F16, (FWD, BWD)), (F32, (FWD_R, BWD_R))], ids=["float16", "float32"])
def test_three_spatial_dims(dt, kernels):
    """[N, C, T, H, W] in memory order N, T, C, H, W: 4 x 4 planes of fp16 (32 bytes), 3 x 3 of fp32 (36 bytes: 4-byte units)"""
    N, T, C = 2, 3, 5
    H = W = 4 if dt == F16 else 3
    shape = (N, T, C, H, W)
    rs = np.random.RandomState(35)
    for pad, active in itertools.product(range(5), (0, 1)):
        x, go, w = _eighths(rs, shape), _eighths(rs, shape), _weights(rs, C, T, pad)
        want_out, want_gx, gw64 = _reference(x, go, w, pad, active, dt)
        out, gx, gw, kf, kb = _run(shape, dt, 0, x, go, w, pad, active)
        assert (kf, kb) == kernels, (dt, pad, active, kf, kb)
        assert_bits(_wide(out), want_out, (dt, pad, active, "out"))
        assert_bits(_wide(gx), want_gx, (dt, pad, active, "grad_x"))
        assert_bits(_wide(gw), round16(gw64.astype(np.float32), dt), (dt, pad, active, "grad_w"))


def test_unflagged_calls_keep_their_kernels():
    """without the flag nothing moves: the calls of test_temporal_gpu.py::test_declined_calls_keep_their_kernels_and_bits and the
    served sparse call name what they named"""
    shape = (2, 3, 5, 8)
    N, T, C, M = shape
    rs = np.random.RandomState(15)
    x = torch.from_numpy(rs.uniform(-1, 1, size=shape)).float().cuda()
    w = torch.zeros(C, 2, device="cuda")
    w[:, 0] = torch.from_numpy(rs.randint(-T - 1, T + 2, size=C)).float().cuda()
    xv = _view(x)
    out = abi.forward(xv, w + 0.25, 0, 1, out=_view(_buffer(shape, F32, 0)))
    assert abi.last_kernel() == "strided_active_forward" and abi.last_path() == abi.PATH_STRIDED
    assert np.array_equal(_wide(out), O.forward(_wide(xv), _wide(w + 0.25), 0, True))
    abi.forward(xv, w, 0, 0, out=_view(_buffer(shape, F32, 0)))
    assert abi.last_kernel() == "segment_forward"
    abi.forward(xv, w, 0, 0)                                   # x segment-major, out NCHW-contiguous
    assert not abi.last_kernel().startswith(("tshift", "segment"))
    go = torch.from_numpy(rs.uniform(-1, 1, size=shape)).float().cuda()
    gx, gw = abi.backward(_view(go), w + 0.25, xv, 0, 1, grad_x=_view(_buffer(shape, F32, 0)))
    assert abi.last_kernel() == "strided_backward"            # (ACTIVE a run-time argument now: the same bits)
    gx_o, gw_o = O.backward(_wide(_view(go)), _wide(w + 0.25), _wide(xv), 0, True)
    assert np.array_equal(_wide(gx), gx_o) and np.abs(_wide(gw) - gw_o).max() <= 1e-5 * np.abs(gw_o).max()


def test_refusals_launch_nothing():
    shape = (2, 3, 5, 8)
    N, T, C, M = shape
    x = torch.randn(shape, device="cuda")
    w = torch.randn(C, device="cuda")

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
    out = painted()
    refused(inv, lambda: abi.forward(x.view(N, T * C, M), w.repeat(T), 0, 1, out=out.view(N, T * C, M), shift_dim0=True), out)   # ndim 1
    b, new = abi.check_borders([N, C, T, M], [[1, 0], [0, 0]], 2)
    cut = painted((N, new[2], C, new[3]))
    refused(inv, lambda: abi.forward(_view(x), w, 0, 1, b, out=_view(cut), shift_dim0=True), cut)                                # a cut window
    dense = painted((N, C, T, M))
    refused(inv, lambda: abi.forward(_view(x), w, 0, 1, out=dense, shift_dim0=True), dense)                                      # NCHW-dense out
    gx, gw, ws = painted(), painted((C,)), painted((4096,), torch.uint8)
    refused(inv, lambda: abi.backward(_view(x), w, _view(x), 0, 1, grad_x=dense, grad_w=gw, workspace=ws, shift_dim0=True), dense, gw, ws)
    p = abi.problem(_view(x), 0, False, None, shift_dim0=True)

    def null_form():
        abi.check(abi.lib().shiftnd_backward(ctypes.byref(p), x.data_ptr(), abi.strides5(_view(x)), None, None, w.data_ptr(),
                                             gx.data_ptr(), abi.strides5(_view(gx)), None, ws.data_ptr(), ws.numel(), None), "x == NULL")

    refused(inv, null_form, gx, ws)
    xq = torch.zeros(shape, dtype=torch.int8, device="cuda")
    outq = painted(shape, torch.int8)
    refused(uns, lambda: abi.forward(_view(xq), w, 0, 0, out=_view(outq), shift_dim0=True), outq)                                # a quantized dtype
    pq = abi.problem(_view(xq), 0, False, None, shift_dim0=True)
    assert abi.lib().shiftnd_backward_workspace_bytes(ctypes.byref(pq)) == 0
    # the flag combines with SHIFTND_WEIGHTS_F32 on 16-bit tensors only
    p32 = abi.problem(_view(x), 0, True, None, dtype=abi.F32 | abi.WEIGHTS_F32, shift_dim0=True)
    refused(uns, lambda: abi.check(abi.lib().shiftnd_forward(ctypes.byref(p32), x.data_ptr(), abi.strides5(_view(x)), w.data_ptr(),
                                                             out.data_ptr(), abi.strides5(_view(out)), None), "fp32 | WEIGHTS_F32"), out)


# ---- red zones ------------------------------------------------------------------------------------------------------
GUARDED = [((2, 3, 5, 8), F16), ((2, 3, 5, 49), F16), ((2, 3, 5, 49), F32), ((2, 3, 5, 2), F64), ((2, 4, 6, 3), F16)]


@pytest.mark.parametrize("shape,dt", GUARDED, ids=lambda v: str(v).split(".")[-1].replace(" ", ""))
def test_red_zones(shape, dt):
    N, T, C, M = shape
    es = torch.empty(0, dtype=dt).element_size()
    rs = np.random.RandomState(36)
    dev = torch.device("cuda")
    for pad, off, active in itertools.product((0, 3), (0, es), (0, 1)):
        what = (shape, str(dt), "pad", pad, "offset", off, "active", active)
        x, go, w = _eighths(rs, shape), _eighths(rs, shape), _weights(rs, C, T, pad)
        want_out, want_gx, gw64 = _reference(x, go, w, pad, active, dt)
        as_dt = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt))
        X, OUT, G, GX = (RZ.Guarded(shape, dt, dev, offset_bytes=off) for _ in range(4))
        W, GW = RZ.Guarded((C,), dt, dev), RZ.Guarded((C,), dt, dev)
        ws_bytes = abi.backward_workspace(_view(X.t), pad, active, shift_dim0=True).numel()
        assert ws_bytes >= N * C * 24
        WS = RZ.Guarded((ws_bytes,), torch.uint8, dev)

        def forward():
            abi.forward(_view(X.t), W.t, pad, active, out=_view(OUT.t), shift_dim0=True)
            return abi.last_kernel()

        def backward():
            abi.backward(_view(G.t), W.t, _view(X.t), pad, active, grad_x=_view(GX.t), grad_w=GW.t, workspace=WS.t, shift_dim0=True)
            return abi.last_kernel()

        whole = _whole(shape, dt, off // es)
        assert RZ.run_guarded(forward, [("x", X, as_dt(x)), ("w", W, as_dt(w))], [("out", OUT)], [as_dt(want_out)],
                              what + ("forward",)) == (FWD if whole else FWD_R)
        want_gw = as_dt(gw64) if dt in (F32, F64) else as_dt(gw64.astype(np.float32))
        assert RZ.run_guarded(backward, [("grad_out", G, as_dt(go)), ("x", X, as_dt(x)), ("w", W, as_dt(w))],
                              [("grad_x", GX), ("grad_w", GW), ("workspace", WS)], [as_dt(want_gx), want_gw, None],
                              what + ("backward",)) == (BWD if whole else BWD_R)


# ---- through the op ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64, F16, BF16], ids=lambda d: str(d).split(".")[-1])
def test_the_op_equals_the_cpu_op(dt):
    """fp32 / fp64: out and x.grad bit for bit, w.grad within 1e-5; 16-bit: against the CPU op on the widened tensors (the CPU 1-D
    ops take fp32 / fp64), out and x.grad within 1 ulp (the sparse shift bit for bit), w.grad per entry"""
    rs = np.random.RandomState(37)
    cdt = dt if dt in (F32, F64) else F32
    for (shape, T), pad, active in itertools.product((((6, 5, 4, 8), 3), ((6, 5, 7, 7), 3), ((8, 6), 4)), range(5), (False, True)):
        what = (shape, pad, active)
        C = shape[1]
        x = torch.from_numpy(rs.uniform(-1, 1, size=shape)).to(dt)
        go = torch.from_numpy(rs.uniform(-1, 1, size=shape)).to(dt)
        w = torch.from_numpy(_weights(rs, C, T, pad, quarters=False)).to(dt).reshape(C, 1)
        xc, wc = x.to(cdt).clone().requires_grad_(True), w.to(cdt).clone().requires_grad_(True)
        ref = OPS.temporal_shift_learnable(xc, wc, T, pad, active)
        ref.backward(go.to(cdt))
        xg, wg = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
        out = OPS.temporal_shift_learnable(xg, wg, T, pad, active)
        assert abi.last_kernel() in (FWD, FWD_R), what
        out.backward(go.cuda())
        assert wg.grad.shape == w.shape and wg.grad.dtype == dt
        gw64 = wc.grad.double().numpy()
        if dt in (F32, F64):
            assert torch.equal(out.detach().cpu(), ref.detach()) and torch.equal(xg.grad.cpu(), xc.grad), what
            assert np.abs(wg.grad.cpu().double().numpy() - gw64).max() <= 1e-5 * max(np.abs(gw64).max(), 1e-30), what
        else:
            want_out, want_gx = round16(ref.detach().numpy(), dt), round16(xc.grad.numpy(), dt)
            if active:
                assert_ulp_close(_wide(out), want_out, dt, FLOOR16, what + ("out",))
                assert_ulp_close(_wide(xg.grad), want_gx, dt, FLOOR16, what + ("x.grad",))
            else:
                assert_bits(_wide(out), want_out, what + ("out",))
                assert_bits(_wide(xg.grad), want_gx, what + ("x.grad",))
            # (the CPU sum is fp32: its own error is inside the 1e-5 term of the per-entry bound)
            assert_gw_entries(_wide(wg.grad), gw64, dt, what + ("w.grad",))


def test_mixed_precision_through_the_op():
    shape, T = (6, 5, 4, 8), 3
    rs = np.random.RandomState(38)
    x = torch.from_numpy(rs.uniform(-1, 1, size=shape)).to(F16).cuda().requires_grad_(True)
    w = torch.from_numpy(_weights(rs, 5, T, 0, quarters=False)).float().cuda().requires_grad_(True)
    out = OPS.temporal_shift_learnable(x, w, T, 0, True)
    out.backward(torch.ones_like(out))
    assert out.dtype == F16 and w.grad.dtype == F32 and x.grad.dtype == F16
    direct = _buffer((2, T, 5, 32), F16, 0, fill=0xA5)
    abi.forward(_view(x.detach().view(2, T, 5, 32)), w.detach(), 0, 1, out=_view(direct), shift_dim0=True)
    assert torch.equal(out.detach().view(torch.int16).view(-1), direct.view(torch.int16).view(-1))
    with pytest.raises(RuntimeError, match="same type"):
        OPS.temporal_shift_learnable(x.detach().float(), w.detach().double(), T, 0, True)


def test_the_module_trains_one_step():
    torch.manual_seed(5)
    m = torchshifts.LearnableTemporalShift(8, 64, active_flag=True).cuda()
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    x = torch.randn(16, 64, 14, 14, device="cuda")
    before = m.weight.detach().clone()
    out, loss = m(x)
    assert abi.last_kernel() == FWD       # 784-byte planes of fp32 at aligned bases: whole pieces
    (out.square().mean() + loss).backward()
    opt.step()
    assert torch.isfinite(m.weight).all() and not torch.equal(m.weight.detach(), before)
    frozen = torchshifts.TemporalShift.from_shift(torchshifts.LearnableTemporalShift(8, 64).cuda())
    assert frozen.shifts.is_cuda
