"""The channels-last learnable temporal shift on the GPU: SHIFTND_SHIFT_DIM0 | SHIFTND_FRAMES through the C ABI
(csrc/shiftnd_frames_learn.hip; the sparse forward is csrc/shiftnd_frames.hip) -- permuted views of (N, T, M, C) buffers, i.e.
[N, C, T, M] problems with strides {T*M*C, 1, M*C, C} and [C] weights -- and through torch.ops.torchshifts.temporal_shift_learnable_cl.
The reference is the C oracle's 1-D evaluation on the lines [N*M, C, T], widened to fp32 for 16-bit tensors and narrowed once; out
and grad_x are also compared bit for bit with the segment-major kernels (tshift_*) on copies of the same values.

Shapes are (N, T, M, C), the smallest at which these kernels can go wrong: one 16-byte piece per pixel row, pieces per row that do not
divide the workgroup, more pieces than a workgroup has lanes, rows that are no whole pieces (8-, 4- and 2-byte pieces), bases one
element off the 16-byte grid, several workgroups per clip, |w| up to T + 1, and T, M or C of one.  The kernels stage nothing, so
there is no tile and no limit on T beyond the stated sizes: a clip of 40 frames stands where a tile's limit would.

Weight tables: those of test_tshift_gpu.py (0, an integer, T + 1, -(T + 1), 0.5, -0.25 rotated per padding, then quarters: every
piece mixed), one that is constant within every 16-byte piece and a TSM-like run table whose run boundary falls inside a piece (the
uniform-piece path).  Exact data: tensors on eighths, weights on quarters.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import torchshifts
from torchshifts import abi
from torchshifts.functional import temporal_shift_learnable_func
from oracle import oracle as O

import redzone as RZ
from exact16_cases import FLOOR16, assert_bits, assert_gw_entries, assert_ulp_close, round16

pytestmark = pytest.mark.gpu

OPS = torch.ops.torchshifts
KEEP = torch.preserve_format
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
SPARSE, SPARSE_R = "frames_forward", "frames_forward_ragged"
FWD, FWD_R, BWD, BWD_R = "frames_active_forward", "frames_active_forward_ragged", "frames_backward", "frames_backward_ragged"

# (N, T, M, C), dtype, elements the bases are offset by
WHOLE_CASES = [((2, 3, 5, 8), F16, 0), ((2, 3, 5, 4), F32, 0), ((2, 3, 5, 2), F64, 0),
               ((3, 2, 7, 24), BF16, 0),      # three pieces
               ((2, 3, 4, 80), F16, 0),       # 10 pieces: does not divide 256
               ((1, 2, 2, 2112), F16, 0),     # 264 pieces: more than a workgroup's lanes
               ((1, 9, 3, 16), F32, 0),       # |w| up to 10: double folds and wraps
               ((2, 8, 196, 64), F16, 0),     # several workgroups per clip, several rows per thread
               ((1, 40, 3, 8), F16, 0)]       # a long clip (no tile: no limit on T)
RAGGED_CASES = [((2, 3, 5, 5), F16, 0),       # 2-byte pieces
                ((2, 3, 5, 6), F16, 0),       # 4-byte pieces
                ((2, 3, 5, 12), BF16, 0),     # 8-byte pieces
                ((2, 3, 5, 3), F32, 0),       # 4-byte pieces
                ((2, 3, 4, 3), F64, 0),       # 8-byte pieces
                ((2, 3, 5, 8), F16, 1),       # bases one element off the 16-byte grid
                # rows enough for the backward's row loop to iterate: the plan assumes 16-byte pieces (256 rows a step), the kernel
                # steps by its own rows per step (tests/temporal_plans.py: backward_plan)
                ((2, 3, 196, 5), F16, 0),     # 2-byte pieces, 51 rows a step: four trips
                ((2, 3, 90, 6), BF16, 0),     # 4-byte pieces, 85 rows a step: two trips, the second of five rows
                ((1, 2, 130, 3), F64, 0)]     # 8-byte pieces, 85 rows a step under a plan of 128: two workgroups, two trips in the first
DEGENERATE_CASES = [((2, 1, 5, 8), F32, 0), ((2, 3, 1, 8), F32, 0), ((2, 4, 6, 1), F32, 0)]
CASES = WHOLE_CASES + RAGGED_CASES + DEGENERATE_CASES
TABLES = ("specials", "pieces", "runs")


def _es(dt):
    return torch.empty(0, dtype=dt).element_size()


def _whole(shape, dt, off):
    return (shape[-1] * _es(dt)) % 16 == 0 and (off * _es(dt)) % 16 == 0


def _names(shape, dt, off, active):
    whole = _whole(shape, dt, off)
    fwd = (FWD if whole else FWD_R) if active else (SPARSE if whole else SPARSE_R)
    return fwd, (BWD if whole else BWD_R)


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
    """(N, T, M..., C) buffer -> the [N, C, T, M...] problem the library sees"""
    return t.permute(0, t.dim() - 1, *range(1, t.dim() - 1))


def _segment_view(t):
    """(N, T, C, M...) buffer -> the same problem on segment-major strides"""
    return t.transpose(1, 2)


def _put(a, dt, off):
    t = _buffer(a.shape, dt, off)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dt))
    return t


def _wide(t):
    t = t.detach().cpu().contiguous()
    return (t if t.dtype in (F32, F64) else t.float()).numpy()


def _weights(rs, C, T, turn, quarters=True, table="specials", dt=F32):
    w = rs.randint(-4 * (T + 1), 4 * (T + 1) + 1, size=C) / 4.0 if quarters else rs.uniform(-T - 1, T + 1, size=C)
    special = [0.0, 2.0, T + 1.0, -(T + 1.0), 0.5, -0.25]
    if table == "specials":
        for i in range(min(C, 6)):
            w[i] = special[(i + turn) % 6]
    elif table == "pieces":       # constant within every 16-byte piece
        per = 16 // _es(dt)
        w = np.array([special[(c // per + turn) % 6] for c in range(C)])
    else:                         # TSM-like runs +1 / -1 / 0 (a quarter on top, so that the active shift blends); with C = 8 and
        cut = max(1, C // 3)      # fp16 the first boundary lies inside the only piece
        w = np.array([1.25 if c < cut else (-0.75 if c < 2 * cut else 0.25) for c in range(C)])
    return w


def _lines(a):
    """(N, T, M..., C) array -> the 1-D problem [N*M, C, T] (contiguous)"""
    N, T, C = a.shape[0], a.shape[1], a.shape[-1]
    return np.ascontiguousarray(a.reshape(N, T, -1, C).transpose(0, 2, 3, 1)).reshape(-1, C, T)


def _frames(lines, shape):
    N, T, C = shape[0], shape[1], shape[-1]
    return np.ascontiguousarray(lines.reshape(N, -1, C, T).transpose(0, 3, 1, 2)).reshape(shape)


def _reference(x, go, w, pad, active, dt):
    """x, go: (N, T, M..., C) arrays holding values of dt; w: [C] values of the weights' type.  -> out, grad_x (values of dt, as the
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
    """the flagged forward and backward on (N, T, M..., C) buffers -> out, grad_x, grad_w; kernel names and the path are asserted"""
    wd = torch.from_numpy(w).to(wdt or dt).cuda()
    xd, gd = _put(x, dt, off), _put(go, dt, off)
    out, gx = _buffer(shape, dt, off, fill=0xA5), _buffer(shape, dt, off, fill=0xA5)
    names = _names(shape, dt, off, active)
    abi.forward(_view(xd), wd, pad, active, out=_view(out), shift_dim0=True, frames=True)
    assert abi.last_kernel() == names[0] and abi.last_path() == abi.PATH_CL, (shape, dt, off, active, abi.last_kernel())
    gw = torch.full_like(wd, float("nan"))
    abi.backward(_view(gd), wd, _view(xd), pad, active, grad_x=_view(gx), grad_w=gw, shift_dim0=True, frames=True)
    assert abi.last_kernel() == names[1] and abi.last_path() == abi.PATH_CL, (shape, dt, off, active, abi.last_kernel())
    return out, gx, gw


def _run_segment_major(shape, dt, x, go, w, pad, active):
    """the same values through the segment-major kernels (tshift_*): (N, T, C, M) copies -> out, grad_x flat in memory order N, T, M, C"""
    to_sm = (lambda a: np.ascontiguousarray(np.moveaxis(a, -1, 2)))
    wd = torch.from_numpy(w).to(dt).cuda()
    xd, gd = _put(to_sm(x), dt, 0), _put(to_sm(go), dt, 0)
    out, gx = torch.empty_like(xd), torch.empty_like(xd)
    abi.forward(_segment_view(xd), wd, pad, active, out=_segment_view(out), shift_dim0=True)
    assert abi.last_kernel().startswith("tshift_forward")
    abi.backward(_segment_view(gd), wd, _segment_view(xd), pad, active, grad_x=_segment_view(gx), shift_dim0=True)
    assert abi.last_kernel().startswith("tshift_backward")
    return out.movedim(2, -1).reshape(-1), gx.movedim(2, -1).reshape(-1)   # (memory order N, T, M, C, flat)


def _eighths(rs, shape):
    return rs.randint(-8, 9, size=shape) / 8.0


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_exact_data(case):
    shape, dt, off = case
    T, C = shape[1], shape[-1]
    rs = np.random.RandomState(41)
    for table, pad, active in itertools.product(TABLES, range(5), (0, 1)):
        what = (_id(case), table, "pad", pad, "active", active)
        x, go, w = _eighths(rs, shape), _eighths(rs, shape), _weights(rs, C, T, pad, table=table, dt=dt)
        want_out, want_gx, gw64 = _reference(x, go, w, pad, active, dt)
        out, gx, gw = _run(shape, dt, off, x, go, w, pad, active)
        assert_bits(_wide(out), want_out, what + ("out",))
        assert_bits(_wide(gx), want_gx, what + ("grad_x",))
        if dt in (F32, F64):
            assert np.array_equal(_wide(gw).astype(np.float64), gw64), what + ("grad_w",)
        else:
            assert_bits(_wide(gw), round16(gw64.astype(np.float32), dt), what + ("grad_w, the fp64 sum rounded once",))
            # fp32 weights with the 16-bit tensor: the same bits in out and grad_x, grad_w the sum itself
            out2, gx2, gw2 = _run(shape, dt, off, x, go, w, pad, active, wdt=F32)
            assert gw2.dtype == F32, what
            assert torch.equal(out2, out) and torch.equal(gx2, gx), what + ("mixed out / grad_x",)
            assert np.array_equal(_wide(gw2).astype(np.float64), gw64), what + ("mixed grad_w",)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_random_data(case):
    shape, dt, off = case
    T, C = shape[1], shape[-1]
    rs = np.random.RandomState(42)
    for table, pad, active in itertools.product(TABLES, range(5), (0, 1)):
        what = (_id(case), table, "pad", pad, "active", active)
        narrow = (lambda a: torch.from_numpy(a).to(dt).double().numpy())
        x, go = narrow(rs.uniform(-1, 1, size=shape)), narrow(rs.uniform(-1, 1, size=shape))
        w = narrow(_weights(rs, C, T, pad, quarters=False, table=table, dt=dt))
        want_out, want_gx, gw64 = _reference(x, go, w, pad, active, dt)
        out, gx, gw = _run(shape, dt, off, x, go, w, pad, active)
        # the same arithmetic in the same order per element as the segment-major kernels: the same bits
        sm_out, sm_gx = _run_segment_major(shape, dt, x, go, w, pad, active)
        assert torch.equal(out.reshape(-1).view(torch.uint8), sm_out.view(torch.uint8)), what + ("out against tshift_forward",)
        assert torch.equal(gx.reshape(-1).view(torch.uint8), sm_gx.view(torch.uint8)), what + ("grad_x against tshift_backward",)
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


@pytest.mark.parametrize("active", (0, 1))
def test_determinism_of_the_weight_gradient(active):
    shape, dt = (2, 8, 196, 64), F16
    rs = np.random.RandomState(43)
    x, go, w = rs.uniform(-1, 1, size=shape), rs.uniform(-1, 1, size=shape), _weights(rs, 64, 8, 0, quarters=False)
    a = _run(shape, dt, 0, x, go, w, 0, active)[2]
    b = _run(shape, dt, 0, x, go, w, 0, active)[2]
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_the_sparse_forward_under_the_bit_is_frames_forward():
    """the same kernel name and bits as the call without the bit; NaN payloads and -0 survive (periodic: nothing is filled)"""
    shape = (2, 3, 5, 8)
    bits = torch.randint(-2 ** 15, 2 ** 15, shape, dtype=torch.int16, device="cuda")   # every fp16 pattern, NaNs included
    bits[0, 0, 0, 0] = -2 ** 15                                                        # -0
    w = torch.tensor([0.0, 1.0, -1.0, 0.5, 2.0, -2.0, 1.5, 3.0], dtype=F16, device="cuda")
    shifts = [0, 1, -1, 0, 2, -2, 2, 3]
    for pad in range(5):
        out, plain = _buffer(shape, F16, 0, fill=0xA5), _buffer(shape, F16, 0, fill=0x5A)
        abi.forward(_view(bits.view(F16)), w, pad, 0, out=_view(out), shift_dim0=True, frames=True)
        assert abi.last_kernel() == SPARSE and abi.last_path() == abi.PATH_CL
        abi.forward(_view(bits.view(F16)), w, pad, 0, out=_view(plain), shift_dim0=True)
        assert abi.last_kernel() == SPARSE and abi.last_path() == abi.PATH_CL
        assert torch.equal(out.view(torch.int16), plain.view(torch.int16)), pad
        if pad == 2:
            for c, s in enumerate(shifts):
                for t in range(3):
                    assert torch.equal(out.view(torch.int16)[:, t, :, c], bits[:, (t - s) % 3, :, c]), (c, t)
    # the sparse grad_x moves bit patterns too: grad_out at pad(t + s)
    gx, gw = _buffer(shape, F16, 0, fill=0xA5), torch.empty_like(w)
    x = torch.zeros(shape, dtype=F16, device="cuda")
    abi.backward(_view(bits.view(F16)), w, _view(x), 2, 0, grad_x=_view(gx), grad_w=gw, shift_dim0=True, frames=True)
    assert abi.last_kernel() == BWD
    for c, s in enumerate(shifts):
        for t in range(3):
            assert torch.equal(gx.view(torch.int16)[:, t, :, c], bits[:, (t + s) % 3, :, c]), (c, t)


@pytest.mark.parametrize("dt", [F16, F32], ids=["float16", "float32"])
def test_three_spatial_dims(dt):
    """[N, C, T, H, W] in memory order N, T, H, W, C: 4 x 4 pixels of fp16 (C = 8: whole pieces), 3 x 3 of fp32 (C = 5: 4-byte pieces)"""
    N, T = 2, 3
    H, W, C = (4, 4, 8) if dt == F16 else (3, 3, 5)
    shape = (N, T, H, W, C)
    rs = np.random.RandomState(44)
    for pad, active in itertools.product(range(5), (0, 1)):
        x, go, w = _eighths(rs, shape), _eighths(rs, shape), _weights(rs, C, T, pad)
        want_out, want_gx, gw64 = _reference(x, go, w, pad, active, dt)
        out, gx, gw = _run(shape, dt, 0, x, go, w, pad, active)
        assert_bits(_wide(out), want_out, (dt, pad, active, "out"))
        assert_bits(_wide(gx), want_gx, (dt, pad, active, "grad_x"))
        assert_bits(_wide(gw), round16(gw64.astype(np.float32), dt), (dt, pad, active, "grad_w"))


def _painted(s, dt=F32):
    return _buffer(s, dt, 0, fill=0xA5)


def _untouched(*ts):
    return all(bool((t.reshape(-1).view(torch.uint8) == 0xA5).all()) for t in ts)


def _refused(text, call, *outs):
    with pytest.raises(RuntimeError, match=text):
        call()
    torch.cuda.synchronize()
    assert _untouched(*outs), text


def test_nothing_moves_without_the_bit():
    shape = (2, 3, 5, 8)
    N, T, M, C = shape
    rs = np.random.RandomState(45)
    x = torch.from_numpy(rs.uniform(-1, 1, size=shape)).float().cuda()
    w = torch.from_numpy(rs.uniform(-2, 2, size=C)).float().cuda()
    # SHIFT_DIM0 alone on channels-last strides: the interpolating forward and the backward are still refused, the outputs untouched
    out, gx, gw = _painted(shape), _painted(shape), _painted((C,))
    ws = _painted((4096,), torch.uint8)
    _refused("invalid argument", lambda: abi.forward(_view(x), w, 0, 1, out=_view(out), shift_dim0=True), out)
    for active in (0, 1):
        _refused("invalid argument", lambda: abi.backward(_view(x), w, _view(x), 0, active, grad_x=_view(gx), grad_w=gw, workspace=ws,
                                                          shift_dim0=True), gx, gw, ws)
    abi.forward(_view(x), w, 0, 0, out=_view(out), shift_dim0=True)
    assert abi.last_kernel() == SPARSE and abi.last_path() == abi.PATH_CL
    # a segment-major call still names tshift_*
    sm = x.permute(0, 1, 3, 2).contiguous()   # (N, T, C, M)
    sm_out, sm_gx = torch.empty_like(sm), torch.empty_like(sm)
    for active in (0, 1):
        abi.forward(_segment_view(sm), w, 0, active, out=_segment_view(sm_out), shift_dim0=True)
        assert abi.last_kernel() == "tshift_forward_ragged" and abi.last_path() == abi.PATH_PLANE   # (20-byte planes)
        abi.backward(_segment_view(sm), w, _segment_view(sm), 0, active, grad_x=_segment_view(sm_gx), shift_dim0=True)
        assert abi.last_kernel() == "tshift_backward_ragged" and abi.last_path() == abi.PATH_PLANE
    # the unflagged call on the NHWC tensor (a genuine 2-D shift) names what it names without this feature
    w2 = torch.zeros(C, 2, device="cuda")
    w2[:, 0] = w
    got = abi.forward(_view(x), w2, 0, 1, out=_view(_painted(shape)))
    assert not abi.last_kernel().startswith(("frames", "tshift"))
    assert np.array_equal(_wide(got), O.forward(_wide(_view(x)), _wide(w2), 0, True))
    # the plain op on a channels-last tensor still takes the segment-major kernels and returns a contiguous tensor
    xc = torch.randn(6, 8, 3, 4, device="cuda").contiguous(memory_format=torch.channels_last)
    plain = OPS.temporal_shift_learnable(xc, w, 3, 0, True)
    assert abi.last_kernel().startswith("tshift_forward") and plain.is_contiguous()


def test_refusals_launch_nothing():
    shape = (2, 3, 5, 8)
    N, T, M, C = shape
    x = torch.randn(shape, device="cuda")
    w = torch.randn(C, device="cuda")
    inv, uns = "invalid argument", "unsupported dtype"
    kw = dict(shift_dim0=True, frames=True)
    ws_bytes = abi.backward_workspace(_view(x), 0, 1, **kw).numel()
    assert ws_bytes >= N * C * 24
    for active in (0, 1):
        out = _painted(shape)
        # ndim 1
        _refused(inv, lambda: abi.forward(x.view(N, T * M, C).permute(0, 2, 1), w, 0, active, out=out.view(N, T * M, C).permute(0, 2, 1), **kw), out)
        # a cut window
        b, new = abi.check_borders([N, C, T, M], [[1, 0], [0, 0]], 2)
        cut = _painted((N, new[2], new[3], C))
        _refused(inv, lambda: abi.forward(_view(x), w, 0, active, b, out=_view(cut), **kw), cut)
        # a segment-major or an NCHW-dense tensor in any one position
        segment, dense = _painted((N, T, C, M)), _painted((N, C, T, M))
        for other in (_segment_view(segment), dense):
            _refused(inv, lambda: abi.forward(_view(x), w, 0, active, out=other, **kw), other)
            _refused(inv, lambda: abi.forward(other, w, 0, active, out=_view(out), **kw), out)
            gx, gw, ws = _painted(shape), _painted((C,)), _painted((ws_bytes,), torch.uint8)
            _refused(inv, lambda: abi.backward(_view(x), w, _view(x), 0, active, grad_x=other, grad_w=gw, workspace=ws, **kw), other, gw, ws)
            _refused(inv, lambda: abi.backward(other, w, _view(x), 0, active, grad_x=_view(gx), grad_w=gw, workspace=ws, **kw), gx, gw, ws)
            _refused(inv, lambda: abi.backward(_view(x), w, other, 0, active, grad_x=_view(gx), grad_w=gw, workspace=ws, **kw), gx, gw, ws)
        gx, gw, ws = _painted(shape), _painted((C,)), _painted((ws_bytes,), torch.uint8)
        gcut = torch.randn((N, new[2], new[3], C), device="cuda")
        _refused(inv, lambda: abi.backward(_view(gcut), w, _view(x), 0, active, b, grad_x=_view(gx), grad_w=gw, workspace=ws, **kw), gx, gw, ws)
        # a workspace one byte short
        _refused("workspace", lambda: abi.backward(_view(x), w, _view(x), 0, active, grad_x=_view(gx), grad_w=gw, workspace=ws[:-1], **kw),
                 gx, gw, ws)
        # the x == NULL form
        p = abi.problem(_view(x), 0, active, None, **kw)

        def null_form():
            abi.check(abi.lib().shiftnd_backward(ctypes.byref(p), x.data_ptr(), abi.strides5(_view(x)), None, None, w.data_ptr(),
                                                 gx.data_ptr(), abi.strides5(_view(gx)), None, ws.data_ptr(), ws.numel(), None), "x == NULL")

        _refused(inv, null_form, gx, ws)
        # a quantized dtype
        xq = torch.zeros(shape, dtype=torch.int8, device="cuda")
        outq = _painted(shape, torch.int8)
        _refused(uns, lambda: abi.forward(_view(xq), w, 0, active, out=_view(outq), **kw), outq)
        assert abi.lib().shiftnd_backward_workspace_bytes(ctypes.byref(abi.problem(_view(xq), 0, active, None, **kw))) == 0
        # the served call with exactly the planned workspace
        abi.backward(_view(x), w, _view(x), 0, active, grad_x=_view(gx), grad_w=gw, workspace=ws, **kw)
        assert abi.last_kernel() == BWD and abi.last_path() == abi.PATH_CL


def test_empty_problems():
    """PATH_EMPTY, grad_w zeroed, nothing else written (an empty torch tensor has no address: the pointers are a painted buffer's)"""
    w = torch.randn(8, device="cuda")
    kw = dict(shift_dim0=True, frames=True)
    L = abi.lib()
    for shape in ((0, 3, 5, 8), (2, 3, 0, 8)):
        x = torch.empty(shape, device="cuda")
        st = abi.strides5(_view(x))
        for active in (0, 1):
            p = abi.problem(_view(x), 0, active, None, **kw)
            abi.forward(_view(x), w, 0, active, out=_view(torch.empty_like(x)), **kw)
            assert abi.last_path() == abi.PATH_EMPTY
            some, ws = _painted((64,)), _painted((64,), torch.uint8)
            gw = torch.full((8,), float("nan"), device="cuda")
            abi.check(L.shiftnd_backward(ctypes.byref(p), some.data_ptr(), st, some.data_ptr(), st, w.data_ptr(), some.data_ptr(), st,
                                         gw.data_ptr(), ws.data_ptr(), ws.numel(), None), "an empty backward")
            torch.cuda.synchronize()
            assert abi.last_path() == abi.PATH_EMPTY and bool((gw == 0).all()) and _untouched(some, ws)


# ---- red zones ------------------------------------------------------------------------------------------------------
GUARDED = [((2, 3, 5, 8), F16, 0), ((2, 3, 5, 24), F32, 0), ((2, 3, 5, 5), F16, 0), ((2, 3, 4, 3), F64, 0), ((2, 3, 5, 8), F16, 2),
           ((1, 2, 2, 2112), F16, 0)]


@pytest.mark.parametrize("shape,dt,off", GUARDED, ids=lambda v: str(v).split(".")[-1].replace(" ", ""))
def test_red_zones(shape, dt, off):
    T, C = shape[1], shape[-1]
    rs = np.random.RandomState(46)
    dev = torch.device("cuda")
    kw = dict(shift_dim0=True, frames=True)
    for pad, active, table in itertools.product((0, 3), (0, 1), ("specials", "runs")):
        what = (shape, str(dt), "pad", pad, "offset", off, "active", active, table)
        x, go, w = _eighths(rs, shape), _eighths(rs, shape), _weights(rs, C, T, pad, table=table, dt=dt)
        want_out, want_gx, gw64 = _reference(x, go, w, pad, active, dt)
        as_dt = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt))
        X, OUT, G, GX = (RZ.Guarded(shape, dt, dev, offset_bytes=off) for _ in range(4))
        W, GW = RZ.Guarded((C,), dt, dev), RZ.Guarded((C,), dt, dev)
        ws_bytes = abi.backward_workspace(_view(X.t), pad, active, **kw).numel()
        assert ws_bytes >= shape[0] * C * 24
        WS = RZ.Guarded((ws_bytes,), torch.uint8, dev)

        def forward():
            abi.forward(_view(X.t), W.t, pad, active, out=_view(OUT.t), **kw)
            return abi.last_kernel()

        def backward():
            abi.backward(_view(G.t), W.t, _view(X.t), pad, active, grad_x=_view(GX.t), grad_w=GW.t, workspace=WS.t, **kw)
            return abi.last_kernel()

        names = _names(shape, dt, off // _es(dt), active)
        assert RZ.run_guarded(forward, [("x", X, as_dt(x)), ("w", W, as_dt(w))], [("out", OUT)], [as_dt(want_out)],
                              what + ("forward",)) == names[0]
        want_gw = as_dt(gw64) if dt in (F32, F64) else as_dt(gw64.astype(np.float32))
        assert RZ.run_guarded(backward, [("grad_out", G, as_dt(go)), ("x", X, as_dt(x)), ("w", W, as_dt(w))],
                              [("grad_x", GX), ("grad_w", GW), ("workspace", WS)], [as_dt(want_gx), want_gw, None],
                              what + ("backward",)) == names[1]


# ---- through the op and the module ------------------------------------------------------------------------------------
def _channels_last_inputs(dt, rs):
    a = torch.from_numpy(rs.uniform(-1, 1, size=(6, 8, 4, 5))).to(dt).contiguous(memory_format=torch.channels_last)
    b = torch.from_numpy(rs.uniform(-1, 1, size=(6, 7, 5))).to(dt).permute(0, 2, 1)     # [6, 5, 7], strides (35, 1, 5)
    c = torch.from_numpy(rs.uniform(-1, 1, size=(6, 8, 2, 3, 2))).to(dt).contiguous(memory_format=torch.channels_last_3d)
    return [(a, 3), (b, 2), (c, 3)]


@pytest.mark.parametrize("dt", [F32, F64, F16, BF16], ids=lambda d: str(d).split(".")[-1])
def test_the_op_equals_the_cpu_op(dt):
    """values against the CPU op (fp32 / fp64: out and x.grad bit for bit, w.grad within 1e-5; 16-bit: against the CPU op on the widened
    tensors, 1 ulp for the interpolating shift, w.grad per entry) and bit for bit against the plain GPU op; strides: out has the
    input's, grad_x the gradient's"""
    rs = np.random.RandomState(47)
    cdt = dt if dt in (F32, F64) else F32
    for (x, T), pad, active in itertools.product(_channels_last_inputs(dt, rs), range(5), (False, True)):
        what = (tuple(x.shape), pad, active)
        C = x.shape[1]
        go = torch.from_numpy(rs.uniform(-1, 1, size=tuple(x.shape))).to(dt)
        w = torch.from_numpy(_weights(rs, C, T, pad, quarters=False)).to(dt).reshape(C, 1)
        xc, wc = x.to(cdt).contiguous().requires_grad_(True), w.to(cdt).clone().requires_grad_(True)
        ref = OPS.temporal_shift_learnable(xc, wc, T, pad, active)
        ref.backward(go.to(cdt))
        xg, wg = x.cuda(), w.cuda()
        assert xg.stride() == x.stride()
        go_cl = torch.empty_like(xg).copy_(go.cuda())
        out = OPS._temporal_shift_learnable_cl_forward(xg, wg, T, pad, active)
        assert abi.last_kernel().startswith("frames_") and abi.last_path() == abi.PATH_CL and out.stride() == xg.stride(), what
        gx, gw = OPS._temporal_shift_learnable_cl_backward(go_cl, wg, xg, T, pad, active)
        assert abi.last_kernel().startswith("frames_backward") and gx.stride() == go_cl.stride(), what
        # a contiguous gradient: today's route, a contiguous grad_x with the same values
        gx2, gw2 = OPS._temporal_shift_learnable_cl_backward(go.cuda(), wg, xg, T, pad, active)
        assert abi.last_kernel().startswith("tshift_backward") and gx2.is_contiguous(), what
        assert torch.equal(gx2, gx) and gw2.dtype == gw.dtype, what
        plain = OPS.temporal_shift_learnable(xg, wg, T, pad, active)
        assert plain.is_contiguous() and torch.equal(plain, out), what
        assert gw.shape == w.shape and gw.dtype == dt
        gw64 = wc.grad.double().numpy()
        if dt in (F32, F64):
            assert torch.equal(out.cpu(), ref.detach()) and torch.equal(gx.cpu(), xc.grad), what
            assert np.abs(gw.cpu().double().numpy() - gw64).max() <= 1e-5 * max(np.abs(gw64).max(), 1e-30), what
        else:
            want_out, want_gx = round16(ref.detach().numpy(), dt), round16(xc.grad.numpy(), dt)
            if active:
                assert_ulp_close(_wide(out), want_out, dt, FLOOR16, what + ("out",))
                assert_ulp_close(_wide(gx), want_gx, dt, FLOOR16, what + ("x.grad",))
            else:
                assert_bits(_wide(out), want_out, what + ("out",))
                assert_bits(_wide(gx), want_gx, what + ("x.grad",))
            assert_gw_entries(_wide(gw), gw64, dt, what + ("w.grad",))


def test_autograd_through_the_functional():
    rs = np.random.RandomState(48)
    x0 = torch.from_numpy(rs.uniform(-1, 1, size=(6, 8, 4, 5))).float().cuda().contiguous(memory_format=torch.channels_last)
    w0 = torch.from_numpy(_weights(rs, 8, 3, 0, quarters=False)).float().cuda()
    go = torch.randn(6, 8, 4, 5, device="cuda")
    go_cl = go.contiguous(memory_format=torch.channels_last)
    res = {}
    for name, fmt, xin, grad in (("plain", torch.contiguous_format, x0, go), ("keep", KEEP, x0, go_cl), ("keep, contiguous grad", KEEP, x0, go),
                                 ("keep, contiguous input", KEEP, x0.contiguous(), go_cl)):
        x, w = xin.clone(memory_format=torch.preserve_format).requires_grad_(True), w0.clone().requires_grad_(True)
        out = temporal_shift_learnable_func(x, w, 3, 0, True, memory_format=fmt)
        forward_kernel = abi.last_kernel()
        assert out.stride() == (x.stride() if fmt == KEEP else out.contiguous().stride()), name
        gx, gw = torch.autograd.grad(out, (x, w), grad)
        res[name] = (out.detach(), gx, gw, forward_kernel)
    assert res["keep"][3] == FWD and res["plain"][3] == "tshift_forward" and res["keep, contiguous input"][3] == "tshift_forward"
    assert res["keep"][1].stride() == go_cl.stride() and res["keep, contiguous grad"][1].is_contiguous()
    for name in res:
        assert torch.equal(res[name][0], res["plain"][0]) and torch.equal(res[name][1], res["plain"][1]), name
        assert torch.allclose(res[name][2], res["plain"][2], rtol=1e-5, atol=1e-6), name


def test_autocast_keeps_the_parameter_in_fp32():
    torch.manual_seed(6)
    m = torchshifts.LearnableTemporalShift(4, 16, init_shift=2, active_flag=True, memory_format=KEEP).cuda()
    assert m.weight.dtype == F32
    x = torch.randn(8, 16, 5, 5, device="cuda").to(BF16).contiguous(memory_format=torch.channels_last)
    with torch.autocast("cuda", dtype=BF16):
        out, loss = m(x)
    assert abi.last_kernel() == FWD and out.dtype == BF16 and out.stride() == x.stride()
    out.backward(torch.ones_like(out))
    assert m.weight.grad.dtype == F32 and bool(torch.isfinite(m.weight.grad).all())
    # (autograd ran the backward on its own thread; the kernel names are per thread: the same call from this one)
    gx, gw = OPS._temporal_shift_learnable_cl_backward(torch.ones_like(out), m.weight.detach(), x, 4, 0, True)
    assert abi.last_kernel() == BWD and gw.dtype == F32 and torch.equal(gw, m.weight.grad) and gx.stride() == x.stride()
    ref = OPS.temporal_shift_learnable(x, m.weight.detach(), 4, 0, True)
    assert torch.equal(ref, out.detach())


def test_the_module_trains_one_step():
    torch.manual_seed(5)
    m = torchshifts.LearnableTemporalShift(8, 64, active_flag=True, memory_format=KEEP).cuda()
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    x = torch.randn(16, 64, 14, 14, device="cuda").contiguous(memory_format=torch.channels_last)
    before = m.weight.detach().clone()
    out, loss = m(x)
    assert abi.last_kernel() == FWD and out.stride() == x.stride()
    (out.square().mean() + loss).backward()
    opt.step()
    assert torch.isfinite(m.weight).all() and not torch.equal(m.weight.detach(), before)


def test_forward_graph_capture_and_replay():
    x = torch.randn(8, 16, 6, 6, device="cuda").contiguous(memory_format=torch.channels_last)
    w = torch.linspace(-2, 2, 16, device="cuda")
    want = OPS.temporal_shift_learnable_cl(x, w, 4, 0, True)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        OPS.temporal_shift_learnable_cl(x, w, 4, 0, True)   # (warm-up on the capture stream)
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            out = OPS.temporal_shift_learnable_cl(x, w, 4, 0, True)
    x.copy_(torch.randn_like(x))
    want2 = OPS.temporal_shift_learnable_cl(x, w, 4, 0, True)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert out.stride() == x.stride() and torch.equal(out, want2) and not torch.equal(want, want2)
