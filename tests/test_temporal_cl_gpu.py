"""Channels-last temporal shift on the GPU: SHIFTND_SHIFT_DIM0 on dense channels-last views (csrc/shiftnd_frames.hip) through the C
ABI, and the ops / modules with memory_format=torch.preserve_format.  Everything is a pure gather: every comparison is bit for bit.

Buffers are (N, T, M, C); the problem is the view [N, C, T, M] with strides {T*M*C, 1, M*C, C}; the table is [C].  A row is the C
elements of one pixel, R bytes; a piece is 16 bytes of it (frames_forward) or the widest smaller power of two that divides R and both
bases (frames_forward_ragged).  The cases are the smallest at which the kernel takes another path: one piece per row, a piece count
that does not divide the workgroup (3, 10), a row longer than a workgroup (264 pieces), several workgroups per frame and many frames,
|s| up to T + 1 under every padding, T == 1, ragged rows of 10, 12 (fp16), 12 (fp32), 24 (fp64) and 7 (uint8) bytes, bases one
element off.  Quantized data never holds the zero point's value, so a filled piece fails under a zero fill or a missing one."""
import itertools

import numpy as np
import pytest
import torch

import torchshifts
from torchshifts import abi
from torchshifts.functional import temporal_shift_func
from torchshifts.quantized.functional import temporal_shift_quantized
from oracle import oracle as O

import redzone as RZ

pytestmark = pytest.mark.gpu

OPS = torch.ops.torchshifts
KEEP = torch.preserve_format
F32, F64, F16, BF16 = torch.float32, torch.float64, torch.float16, torch.bfloat16
U8, I8, I32 = torch.uint8, torch.int8, torch.int32
WHOLE, RAGGED = "frames_forward", "frames_forward_ragged"
ZP = {U8: 77, I8: -5, I32: 70000}
NP = {U8: np.uint8, I8: np.int8, I32: np.int32}
RANGE = {U8: (0, 256), I8: (-128, 128), I32: (-1000000, 1000000)}

# (N, T, M, C), dtype, base offset in elements, the form
FLOAT_CASES = [
    ((2, 3, 5, 8), F16, 0, WHOLE), ((2, 3, 5, 4), F32, 0, WHOLE), ((2, 3, 5, 2), F64, 0, WHOLE),   # one piece per row
    ((2, 3, 7, 24), BF16, 0, WHOLE), ((2, 3, 5, 40), F32, 0, WHOLE),                               # 3 and 10 pieces per row
    ((2, 2, 3, 1056), F32, 0, WHOLE),                                                              # 264 pieces: longer than a workgroup
    ((2, 8, 49, 64), F16, 0, WHOLE),                                                               # several workgroups per frame
    ((1, 9, 3, 16), F32, 0, WHOLE),                                                                # |s| up to 10 under every padding
    ((3, 1, 4, 8), F16, 0, WHOLE),                                                                 # T == 1
    ((2, 3, 5, 5), F16, 0, RAGGED), ((2, 3, 5, 6), F16, 0, RAGGED), ((2, 3, 5, 3), F32, 0, RAGGED), ((2, 3, 4, 3), F64, 0, RAGGED),
    ((2, 3, 5, 8), F16, 1, RAGGED),
]
QUANT_CASES = [
    ((2, 3, 5, 16), U8, 0, WHOLE), ((2, 3, 5, 16), I8, 0, WHOLE), ((2, 3, 5, 4), I32, 0, WHOLE),
    ((2, 3, 5, 7), U8, 0, RAGGED), ((2, 3, 5, 16), U8, 1, RAGGED), ((2, 3, 5, 3), I32, 0, RAGGED), ((2, 8, 49, 64), U8, 0, WHOLE),
]


def _id(case):
    shape, dt, off, kernel = case
    return "%s-%s-off%d" % ("x".join(map(str, shape)), str(dt).split(".")[-1], off)


def _buffer(shape, dt, off, fill=None):
    """a dense (N, T, M, C) device tensor whose base is `off` elements past an aligned allocation"""
    flat = torch.empty(int(np.prod(shape)) + off, dtype=dt, device="cuda")
    t = flat[off:].view(shape)
    assert t.data_ptr() % 16 == (off * t.element_size()) % 16
    if fill is not None:
        t.view(-1).view(torch.uint8).fill_(fill)
    return t


def _view(t):
    """(N, T, M, C) buffer -> the [N, C, T, M] problem the library sees"""
    return t.permute(0, 3, 1, 2)


def _np(t):
    t = t.detach().cpu().contiguous()
    return (t if t.dtype in (F32, F64) else t.float()).numpy()


def _same(got, want_np, what):
    got = _np(got)
    assert got.shape == want_np.shape and np.array_equal(got, want_np.astype(got.dtype)), what


def _random_table(rs, C, T):
    """0, T + 1 and -T - 1 always; the rest random in [-T - 1, T + 1]: with C >= 4 every piece is mixed"""
    s = rs.randint(-T - 1, T + 2, size=C).astype(np.float32)
    s[[0, C // 2, C - 1][:C]] = [0, T + 1, -T - 1][:C]
    return s


def _run_table(C, T, fold):
    """the published table (-1 on the first `fold` channels, +1 on the next) with runs of T + 1 and -T - 1 behind it"""
    s = np.zeros(C, np.float32)
    for k, v in enumerate((-1, 1, T + 1, -T - 1)):
        s[k * fold:(k + 1) * fold] = v
    return s


def _two_columns(s, dt):
    return torch.stack([s, torch.zeros_like(s)], 1).to(dt).contiguous()


def _data(rs, shape, dt):
    return torch.from_numpy(rs.uniform(-1, 1, size=shape)).to(dt)


def _check_float(shape, dt, off, kernel, s_np, pad, rs, what):
    N, T, M, C = shape
    s = torch.from_numpy(s_np).cuda()
    w = s.to(dt)
    w2 = _two_columns(s, dt)
    x = _buffer(shape, dt, off)
    x.copy_(_data(rs, shape, dt))
    out = _buffer(shape, dt, off, fill=0xA5)
    abi.forward(_view(x), w, pad, 0, out=_view(out), shift_dim0=True)
    assert abi.last_kernel() == kernel and abi.last_path() == abi.PATH_CL, what + (abi.last_kernel(), abi.last_path())
    xc = _view(x).contiguous()
    _same(_view(out), O.forward(_np(xc), _np(w2), pad, False), what + ("forward against the oracle",))
    assert torch.equal(_view(out), abi.forward(xc, w2, pad, 0)), what + ("forward against the contiguous route",)
    # the unflagged call of the same memory: the NHWC 2-D problem under (s, 0), on the kernels it had
    plain = _buffer(shape, dt, off, fill=0xA5)
    abi.forward(_view(x), w2, pad, 0, out=_view(plain))
    assert not abi.last_kernel().startswith("frames"), what + (abi.last_kernel(),)
    assert torch.equal(plain, out), what + ("the unflagged call", abi.last_kernel())
    # the input gradient: the same call under the negated table
    go = _buffer(shape, dt, off)
    go.copy_(_data(rs, shape, dt))
    gx = _buffer(shape, dt, off, fill=0xA5)
    abi.forward(_view(go), -w, pad, 0, out=_view(gx), shift_dim0=True)
    assert abi.last_kernel() == kernel, what + (abi.last_kernel(),)
    goc = _view(go).contiguous()
    _same(_view(gx), O.backward(_np(goc), _np(w2), _np(xc), pad, False)[0], what + ("grad_x against the oracle",))
    assert torch.equal(_view(gx), abi.backward_input(goc, w2, (N, C, T, M), pad)), what + ("grad_x against the contiguous route",)
    if dt in (F16, BF16):   # an fp32 table: the same bits
        mixed = _buffer(shape, dt, off, fill=0xA5)
        abi.forward(_view(x), s.float(), pad, 0, out=_view(mixed), shift_dim0=True)
        assert abi.last_kernel() == kernel and torch.equal(mixed, out), what + ("fp32 table",)


@pytest.mark.parametrize("case", FLOAT_CASES, ids=_id)
def test_c_abi_forward_and_input_gradient(case):
    shape, dt, off, kernel = case
    N, T, M, C = shape
    rs = np.random.RandomState(31)
    for pad in range(5):
        _check_float(shape, dt, off, kernel, _random_table(rs, C, T), pad, rs, (_id(case), "pad", pad))


@pytest.mark.parametrize("shape,dt,fold", [((2, 3, 5, 64), F16, 8), ((2, 3, 5, 24), F16, 3), ((2, 3, 5, 32), F32, 4), ((2, 3, 5, 10), F32, 2)],
                         ids=["fp16-fold8", "fp16-fold3", "fp32-fold4", "fp32-fold2"])
def test_tables_of_runs(shape, dt, fold):
    """fold a multiple of the piece's elements: every piece uniform; fold 3 of 8 / 2 of 4: mixed pieces at the run boundaries only"""
    rs = np.random.RandomState(32)
    for pad in range(5):
        _check_float(shape, dt, 0, WHOLE if (shape[3] * torch.empty(0, dtype=dt).element_size()) % 16 == 0 else RAGGED,
                     _run_table(shape[3], shape[1], fold), pad, rs, (shape, str(dt), fold, "pad", pad))


def _qdata(rs, shape, dt):
    lo, hi = RANGE[dt]
    a = rs.randint(lo, hi, size=shape)
    a[a == ZP[dt]] += 1
    return a.astype(NP[dt])


@pytest.mark.parametrize("case", QUANT_CASES, ids=_id)
def test_c_abi_forward_quantized(case):
    shape, dt, off, kernel = case
    N, T, M, C = shape
    rs = np.random.RandomState(33)
    for pad, uniform in itertools.product(range(5), (False, True)):
        what = (_id(case), "pad", pad, "runs" if uniform else "random")
        fold = 16 if C % 16 == 0 and C >= 64 else max(1, C // 4)
        s = (_run_table(C, T, fold) if uniform else _random_table(rs, C, T)).astype(np.int64)
        x_np = _qdata(rs, shape, dt)
        xv = x_np.transpose(0, 3, 1, 2)
        x = _buffer(shape, dt, off)
        x.copy_(torch.from_numpy(x_np))
        for ndt, wzp in ((np.uint8, 128), (np.int8, 0), (np.int32, 0)):
            w1 = (s + wzp).astype(ndt)
            w2 = np.stack([w1, np.zeros_like(w1) + ndt(wzp)], 1)
            want = O.forward_q(np.ascontiguousarray(xv), w2, wzp, ZP[dt], pad)
            if pad == 0 and T > 1:
                assert (want == ZP[dt]).any()
            out = _buffer(shape, dt, off, fill=0xA5)
            abi.forward_quantized(_view(x), torch.from_numpy(w1).cuda(), wzp, ZP[dt], pad, out=_view(out), shift_dim0=True)
            assert abi.last_kernel() == kernel and abi.last_path() == abi.PATH_CL, what + (abi.last_kernel(),)
            assert np.array_equal(_view(out).cpu().numpy(), want), what + (w1.dtype.name,)
        dense = abi.forward_quantized(_view(x).contiguous(), torch.from_numpy(w2).cuda(), wzp, ZP[dt], pad)
        assert np.array_equal(dense.cpu().numpy(), want), what + ("the contiguous route",)


def test_three_spatial_dims():
    """[N, C, T, H, W] in memory order N, T, H, W, C (NDHWC of the video view)"""
    N, T, H, W, C = 2, 3, 2, 3, 8
    rs = np.random.RandomState(34)
    for pad in range(5):
        s = torch.from_numpy(_random_table(rs, C, T)).cuda()
        x = _data(rs, (N, T, H, W, C), F16).cuda()
        out = torch.empty_like(x).fill_(float("nan"))
        abi.forward(x.permute(0, 4, 1, 2, 3), s.half(), pad, 0, out=out.permute(0, 4, 1, 2, 3), shift_dim0=True)
        assert abi.last_kernel() == WHOLE and abi.last_path() == abi.PATH_CL
        w3 = torch.stack([s, torch.zeros_like(s), torch.zeros_like(s)], 1)
        _same(out.permute(0, 4, 1, 2, 3), O.forward(_np(x.permute(0, 4, 1, 2, 3)), _np(w3), pad, False), ("NDHWC", pad))


def test_refusals_leave_the_output_untouched():
    shape = (2, 3, 5, 8)
    N, T, M, C = shape
    rs = np.random.RandomState(35)
    x = _data(rs, shape, F32).cuda()
    w = torch.from_numpy(_random_table(rs, C, T)).cuda()

    def refused(what, xin, out, view_out, active=0, borders=None, quantized=False):
        with pytest.raises(RuntimeError, match="invalid argument|unsupported dtype"):
            if quantized:
                abi.forward_quantized(xin, w.to(I32), 0, 0, 0, borders, out=view_out, shift_dim0=True)
            else:
                abi.forward(xin, w, 0, active, borders, out=view_out, shift_dim0=True)
        torch.cuda.synchronize()
        assert bool((out.view(-1).view(torch.uint8) == 0xA5).all()), what

    out = _buffer(shape, F32, 0, fill=0xA5)
    refused("active", _view(x), out, _view(out), active=1)
    b, new = abi.check_borders([N, C, T, M], [[1, 0], [0, 0]], 2)
    cut = _buffer((N, new[2], M, C), F32, 0, fill=0xA5)
    refused("cut window", _view(x), cut, _view(cut), borders=b)
    seg = _buffer((N, T, C, M), F32, 0, fill=0xA5)
    refused("segment-major out", _view(x), seg, seg.transpose(1, 2))
    nchw = _buffer((N, C, T, M), F32, 0, fill=0xA5)
    refused("NCHW out", _view(x), nchw, nchw)
    xq = torch.from_numpy(_qdata(rs, (N, T, C, M), U8)).cuda()      # segment-major quantized tensors under the flag
    outq = _buffer((N, T, C, M), U8, 0, fill=0xA5)
    refused("segment-major quantized", xq.transpose(1, 2), outq, outq.transpose(1, 2), quantized=True)
    with pytest.raises(RuntimeError, match="unsupported dtype"):   # shiftnd_forward takes no quantized dtype, flagged or not
        abi.forward(_view(_buffer(shape, U8, 0)), w, 0, 0, out=_view(_buffer(shape, U8, 0)), shift_dim0=True)
    # a layout both descriptions fit (M == 1) stays with the tshift kernels
    x1 = _data(rs, (2, 3, 1, 8), F32).cuda()
    o1 = _buffer((2, 3, 1, 8), F32, 0, fill=0xA5)
    abi.forward(_view(x1), w, 0, 0, out=_view(o1), shift_dim0=True)
    assert abi.last_kernel().startswith("tshift_forward"), abi.last_kernel()
    _same(_view(o1), O.forward(_np(_view(x1)), _np(_two_columns(w, F32)), 0, False), "M == 1")


# ---- red zones ------------------------------------------------------------------------------------------------------
GUARDED = [((2, 3, 5, 8), F16, WHOLE), ((2, 3, 7, 24), BF16, WHOLE), ((2, 3, 5, 5), F16, RAGGED), ((2, 3, 5, 3), F32, RAGGED),
           ((2, 3, 5, 16), U8, WHOLE), ((2, 3, 5, 7), U8, RAGGED)]


@pytest.mark.parametrize("shape,dt,kernel", GUARDED, ids=lambda v: str(v).split(".")[-1].replace(" ", ""))
def test_red_zones(shape, dt, kernel):
    N, T, M, C = shape
    es = torch.empty(0, dtype=dt).element_size()
    rs = np.random.RandomState(36)
    dev = torch.device("cuda")
    quantized = dt == U8
    for pad, off in itertools.product((0, 3), (0, es)):
        what = (shape, str(dt), "pad", pad, "offset", off)
        s = _random_table(rs, C, T)
        if quantized:
            w, x = torch.from_numpy(s.astype(np.int32)), torch.from_numpy(_qdata(rs, (N, C, T, M), dt))
            want_out = torch.from_numpy(O.forward_q(x.numpy(), np.stack([s, 0 * s], 1).astype(np.int32), 0, ZP[dt], pad))
        else:
            w, x, go = torch.from_numpy(s).to(dt), _data(rs, (N, C, T, M), dt), _data(rs, (N, C, T, M), dt)
            w2 = np.stack([s, 0 * s], 1)
            want_out = torch.from_numpy(O.forward(_np(x), w2, pad, False)).to(dt)
            want_gx = torch.from_numpy(O.backward(_np(go), w2, _np(x), pad, False)[0]).to(dt)
        X, OUT, G, GX = (RZ.Guarded((N, C, T, M), dt, dev, layout="channels_last", offset_bytes=off) for _ in range(4))
        W, WN = RZ.Guarded((C,), w.dtype, dev), RZ.Guarded((C,), w.dtype, dev)

        def forward():
            if quantized:
                abi.forward_quantized(X.t, W.t, 0, ZP[dt], pad, out=OUT.t, shift_dim0=True)
            else:
                abi.forward(X.t, W.t, pad, 0, out=OUT.t, shift_dim0=True)
            return abi.last_kernel()

        def gradient():
            abi.forward(G.t, WN.t, pad, 0, out=GX.t, shift_dim0=True)
            return abi.last_kernel()

        expect = kernel if off == 0 else RAGGED
        assert RZ.run_guarded(forward, [("x", X, x), ("w", W, w)], [("out", OUT)], [want_out], what + ("forward",)) == expect
        if not quantized:
            assert RZ.run_guarded(gradient, [("grad_out", G, go), ("w", WN, -w)], [("grad_x", GX)], [want_gx], what + ("gradient",)) == expect


# ---- through the ops ----------------------------------------------------------------------------------------------------
def _channels_last_inputs(rs, dt):
    a = _data(rs, (6, 5, 4, 6), dt).contiguous(memory_format=torch.channels_last)
    b = _data(rs, (6, 7, 8), dt).permute(0, 2, 1)                                   # [6, 8, 7], unit channel stride
    c = _data(rs, (4, 5, 2, 3, 2), dt).contiguous(memory_format=torch.channels_last_3d)
    return [a, b, c]


@pytest.mark.parametrize("dt", [F32, F64, F16, BF16], ids=lambda d: str(d).split(".")[-1])
def test_the_op_equals_the_cpu_op_in_values_and_strides(dt):
    rs = np.random.RandomState(37)
    for x in _channels_last_inputs(rs, dt):
        for pad in range(5):
            what = (tuple(x.shape), pad)
            s = torch.from_numpy(rs.randint(-3, 4, size=x.shape[1]))
            go = torch.empty_like(x).copy_(_data(rs, tuple(x.shape), dt))
            xc = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
            want = OPS.temporal_shift_cl(xc, s, 2, pad)
            want.backward(go)
            xg = torch.empty_strided(x.shape, x.stride(), dtype=dt, device="cuda").copy_(x).requires_grad_(True)
            gg = torch.empty_strided(x.shape, x.stride(), dtype=dt, device="cuda").copy_(go)
            out = OPS.temporal_shift_cl(xg, s.cuda(), 2, pad)
            assert abi.last_kernel() in (WHOLE, RAGGED), what + (abi.last_kernel(),)
            out.backward(gg)
            assert out.stride() == want.stride() == x.stride() and torch.equal(out.detach().cpu(), want.detach()), what
            assert xg.grad.stride() == xc.grad.stride() == x.stride() and torch.equal(xg.grad.cpu(), xc.grad), what
            # a contiguous gradient gives a contiguous x.grad; a contiguous input the plain op's result
            gx = OPS._temporal_shift_cl_backward(gg.contiguous(), s.cuda(), 2, pad)
            assert gx.is_contiguous() and torch.equal(gx.cpu(), xc.grad), what
            plain = OPS.temporal_shift_cl(xg.detach().contiguous(), s.cuda(), 2, pad)
            assert plain.is_contiguous() and not abi.last_kernel().startswith("frames") and torch.equal(plain.cpu(), want.detach()), what


@pytest.mark.parametrize("qtype,dt", [(torch.quint8, U8), (torch.qint8, I8), (torch.qint32, I32)], ids=["quint8", "qint8", "qint32"])
def test_the_quantized_op_equals_the_cpu_op_in_values_and_strides(qtype, dt):
    rs = np.random.RandomState(38)
    for x in _channels_last_inputs(rs, F32):
        order = [0] + list(range(2, x.dim())) + [1]
        back = [0, x.dim() - 1] + list(range(1, x.dim() - 1))
        xq = torch.quantize_per_tensor(x.permute(order).contiguous(), 0.05, ZP[dt], qtype).permute(back)
        xd = torch._make_per_tensor_quantized_tensor(xq.int_repr().permute(order).contiguous().cuda(), 0.05, ZP[dt]).permute(back)
        assert xd.stride() == xq.stride() == x.stride()
        for pad in range(5):
            s = torch.from_numpy(rs.randint(-3, 4, size=x.shape[1]))
            want = OPS.temporal_shift_quantized_cl(xq, s, 2, pad)
            out = temporal_shift_quantized(xd, s.cuda(), 2, pad, memory_format=KEEP)
            assert abi.last_kernel() in (WHOLE, RAGGED), abi.last_kernel()
            assert out.stride() == want.stride() == x.stride() and out.q_scale() == 0.05 and out.q_zero_point() == ZP[dt]
            assert torch.equal(out.int_repr().cpu(), want.int_repr()), (tuple(x.shape), pad)
            assert temporal_shift_quantized(xd, s.cuda(), 2, pad).is_contiguous()


def test_the_module_equals_the_slicing_idiom():
    T, C = 8, 64
    m = torchshifts.TemporalShift(T, C, memory_format=KEEP).cuda()
    x = torch.randn(16, C, 14, 14, device="cuda", dtype=F16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    out = m(x)
    assert abi.last_kernel() == WHOLE and out.is_contiguous(memory_format=torch.channels_last)
    f = C // 8
    v = x.detach().view(2, T, C, 14, 14)
    want = torch.zeros_like(v)
    want[:, :-1, :f] = v[:, 1:, :f]
    want[:, 1:, f:2 * f] = v[:, :-1, f:2 * f]
    want[:, :, 2 * f:] = v[:, :, 2 * f:]
    assert torch.equal(out.detach(), want.view(16, C, 14, 14))
    go = torch.randn_like(out)
    out.backward(go)
    assert x.grad.is_contiguous(memory_format=torch.channels_last)
    g = go.view(2, T, C, 14, 14)
    gx = torch.zeros_like(g)
    gx[:, 1:, :f] = g[:, :-1, :f]
    gx[:, :-1, f:2 * f] = g[:, 1:, f:2 * f]
    gx[:, :, 2 * f:] = g[:, :, 2 * f:]
    assert torch.equal(x.grad, gx.view(16, C, 14, 14))
    # the default memory_format: a contiguous output, as before
    plain = torchshifts.TemporalShift(T, C).cuda()(x.detach())
    assert plain.is_contiguous() and torch.equal(plain, out.detach())


def test_graph_capture_and_replay():
    """one captured preserve-format forward (a single-branch graph): the call neither synchronises nor allocates at the C ABI"""
    T, C = 4, 32
    s = torchshifts.TemporalShift.default_table(C, 8).cuda()
    x = torch.randn(8, C, 7, 7, device="cuda", dtype=F16).contiguous(memory_format=torch.channels_last)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        temporal_shift_func(x, s, T, 0, memory_format=KEEP)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = temporal_shift_func(x, s, T, 0, memory_format=KEEP)
    x.copy_(torch.randn_like(x))
    graph.replay()
    torch.cuda.synchronize()
    assert out.stride() == x.stride() and torch.equal(out, OPS.temporal_shift(x, s, T, 0))
