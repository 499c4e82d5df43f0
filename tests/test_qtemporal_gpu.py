"""Quantized temporal shift on the GPU: int8 / uint8 / int32 tensors on the segment-major route of shiftnd_forward_quantized
(csrc/shiftnd_segment.hip) through the C ABI -- permuted views of (N, T, C, M) buffers, as tests/test_temporal_gpu.py builds them --
against oracle.forward_q on the same strided numpy view, and through torch.ops.torchshifts.temporal_shift_quantized.  Everything is
a pure gather: every comparison is bit for bit.

Shapes are (N, T, C, M).  One-byte elements put planes of an odd number of bytes at bases on any byte: 49, 17 and 15 bytes (pieces
inside one plane and over two, odd splits), 196 bytes, 3- and 2-byte planes (a 16-byte piece reaches over five to eight planes: the
per-element path), each at base offsets of 0 and 1 byte; int32 planes of 16 bytes (whole pieces), 12 bytes, and 16 bytes at a
4-byte offset.  The zero points are 7 (uint8), -3 (int8) and 100000 (int32: a dword fill is told apart from a splatted byte) and the
data never holds the zero point's value, so every filled plane of a zeros-padding case fails under a zero fill or a missing one.

M = 1: memory order N, T, C IS channels-last ([N, C, T, 1] with unit channel stride), which the channel-fastest kernels serve before
the segment route is asked -- for quantized tensors as for the float ones (tests/test_temporal_gpu.py: the route sits behind every
earlier one).  The case runs like the others, both offsets, and names cl_gather_forward; M = 2 stands in for it as the plane size
that puts the most planes into one piece of the segment kernel.
"""
import itertools

import numpy as np
import pytest
import torch

import torchshifts
from torchshifts import abi
from torchshifts.quantized.functional import temporal_shift_quantized
from oracle import oracle as O

import redzone as RZ
from test_temporal_gpu import CASES as FLOAT_CASES, _buffer as _float_buffer, _data as _float_data, _table as _float_table, _view

pytestmark = pytest.mark.gpu

OPS = torch.ops.torchshifts
U8, I8, I32 = torch.uint8, torch.int8, torch.int32
WHOLE, RAGGED, CL = "segment_forward", "segment_forward_ragged", "cl_gather_forward"
ZP = {U8: 7, I8: -3, I32: 100000}
NP = {U8: np.uint8, I8: np.int8, I32: np.int32}
RANGE = {U8: (0, 256), I8: (-128, 128), I32: (-1000000, 1000000)}

# (N, T, C, M), dtype, base offsets in bytes, the kernel at offset 0 (any other offset of a segment case is ragged)
CASES = [((2, 3, 5, 16), dt, (0,), WHOLE) for dt in (U8, I8)] + [((2, 4, 6, 32), dt, (0,), WHOLE) for dt in (U8, I8)]
for _M in (49, 17, 15, 3, 2):
    CASES += [((2, 3, 5, _M), dt, (0, 1), RAGGED) for dt in (U8, I8)]
CASES += [((2, 3, 5, 1), dt, (0, 1), CL) for dt in (U8, I8)]
CASES += [((2, 3, 5, 196), dt, (0, 1), RAGGED) for dt in (U8, I8)]
CASES += [((2, 3, 5, 4), I32, (0,), WHOLE), ((2, 3, 5, 3), I32, (0, 4), RAGGED), ((2, 3, 5, 4), I32, (4,), RAGGED)]


def _name(dt):
    return str(dt).split(".")[-1]


def _id(case):
    shape, dt, offs, kernel = case
    return "%s-%s-off%s" % ("x".join(map(str, shape)), _name(dt), "_".join(map(str, offs)))


def _buffer(shape, dt, off_bytes, fill=None):
    """a dense device tensor of `shape` whose base is `off_bytes` past an aligned allocation"""
    es = torch.empty(0, dtype=dt).element_size()
    assert off_bytes % es == 0
    flat = torch.empty(int(np.prod(shape)) * es + off_bytes, dtype=torch.uint8, device="cuda")
    if fill is not None:
        flat.fill_(fill)
    t = flat[off_bytes:].view(dt).view(shape)
    assert t.data_ptr() % 16 == off_bytes % 16
    return t


def _data(rs, shape, dt):
    """random int_repr values without the zero point's value"""
    lo, hi = RANGE[dt]
    a = rs.randint(lo, hi, size=shape)
    a[a == ZP[dt]] += 1
    return a.astype(NP[dt])


def _shifts(rs, C, T):
    """0, +1, -1, an entry with |s| >= T and one with |s| >= 2 T; the rest random in [-T - 1, T + 1]"""
    s = rs.randint(-T - 1, T + 2, size=C)
    s[:5] = [0, 1, -1, T, -2 * T - 1]
    return s.astype(np.int64)


def _tables(s, cols=2):
    """the same shifts as the three table kinds: (int_repr array, zero point).  The I32 table swaps the |s| >= 2 T entry for 70000
    (beyond 8 and 16 bits), so it has an expectation of its own."""
    out = []
    for ndt, zp in ((np.uint8, 128), (np.int8, 0), (np.int32, 0)):
        w = np.zeros((len(s), cols), np.int64) + zp
        w[:, 0] += s
        if ndt == np.int32:
            w[4, 0] = 70000
        assert np.array_equal(w.astype(ndt).astype(np.int64), w)
        out.append((w.astype(ndt), zp))
    return out


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_c_abi_forward_quantized(case):
    shape, dt, offs, kernel = case
    N, T, C, M = shape
    rs = np.random.RandomState(21)
    path = abi.PATH_CL if kernel == CL else abi.PATH_PLANE
    for pad in range(5):
        x_np = _data(rs, shape, dt)
        xv = x_np.transpose(0, 2, 1, 3)                    # the strided [N, C, T, M] view
        tables = _tables(_shifts(rs, C, T))
        wants = [O.forward_q(xv, w, wzp, ZP[dt], pad) for w, wzp in (tables[0], tables[2])]
        if pad == 0:
            assert (wants[0] == ZP[dt]).any() and (wants[1] == ZP[dt]).any()   # filled planes, and only they hold the zero point
        for off in offs:
            x = _buffer(shape, dt, off)
            x.copy_(torch.from_numpy(x_np))
            for k, (w, wzp) in enumerate(tables):
                what = (_id(case), "pad", pad, "offset", off, "table", w.dtype.name)
                out = _buffer(shape, dt, off, fill=0xA5)
                abi.forward_quantized(_view(x), torch.from_numpy(w).cuda(), wzp, ZP[dt], pad, out=_view(out))
                expect = kernel if (off == 0 or kernel == CL) else RAGGED
                assert abi.last_kernel() == expect and abi.last_path() == path, what + (abi.last_kernel(),)
                assert np.array_equal(_view(out).cpu().numpy(), wants[k // 2]), what


def test_three_spatial_dims_with_inner_shifts():
    """[N, C, T, H, W] in memory order N, T, C, H, W, uint8 3 x 3 planes; channel 1 also shifts H, channel 3 also shifts W (the
    host routes by strides alone: the per-element gather inside the same kernel)"""
    N, T, C, H, W = 2, 3, 5, 3, 3
    rs = np.random.RandomState(22)
    for pad, off in itertools.product(range(5), (0, 1)):
        x_np = _data(rs, (N, T, C, H, W), U8)
        w, wzp = _tables(_shifts(rs, C, T), cols=3)[0]
        w[1, 1], w[3, 2] = wzp - 1, wzp + 2
        x = _buffer(x_np.shape, U8, off)
        x.copy_(torch.from_numpy(x_np))
        out = _buffer(x_np.shape, U8, off, fill=0xA5)
        abi.forward_quantized(_view(x), torch.from_numpy(w).cuda(), wzp, ZP[U8], pad, out=_view(out))
        assert abi.last_kernel() == RAGGED, (pad, off, abi.last_kernel())
        assert np.array_equal(_view(out).cpu().numpy(), O.forward_q(x_np.transpose(0, 2, 1, 3, 4), w, wzp, ZP[U8], pad)), (pad, off)


@pytest.mark.parametrize("shape,dt,kernel", [((2, 3, 5, 16), U8, WHOLE), ((2, 3, 5, 49), I8, RAGGED), ((2, 3, 5, 3), I32, RAGGED)],
                         ids=lambda v: str(v).split(".")[-1].replace(" ", ""))
def test_a_table_with_inner_shifts_is_gathered_exactly(shape, dt, kernel):
    N, T, C, M = shape
    rs = np.random.RandomState(23)
    for pad in range(5):
        x_np = _data(rs, shape, dt)
        for w, wzp in _tables(_shifts(rs, C, T)):
            w[1, 1], w[3, 1] = wzp + 2, wzp - 1
            out = _buffer(shape, dt, 0, fill=0xA5)
            abi.forward_quantized(_view(torch.from_numpy(x_np).cuda()), torch.from_numpy(w).cuda(), wzp, ZP[dt], pad, out=_view(out))
            assert abi.last_kernel() == kernel, (shape, pad, abi.last_kernel())
            assert np.array_equal(_view(out).cpu().numpy(), O.forward_q(x_np.transpose(0, 2, 1, 3), w, wzp, ZP[dt], pad)), (shape, pad)


def test_declined_calls_keep_their_kernels_and_bits():
    shape = (2, 3, 5, 16)
    N, T, C, M = shape
    rs = np.random.RandomState(24)
    x_np = _data(rs, shape, U8)
    w, wzp = _tables(_shifts(rs, C, T))[0]
    wd = torch.from_numpy(w).cuda()

    def run(what, x_np=x_np, wd=wd, w=w, borders=None, out=None):
        xin = _view(torch.from_numpy(x_np).cuda())
        o = abi.forward_quantized(xin, wd, wzp, ZP[U8], 0, borders, out=out)
        name = abi.last_kernel()
        assert not name.startswith("segment"), (what, name)
        assert np.array_equal(o.cpu().numpy(), O.forward_q(x_np.transpose(0, 2, 1, 3), w, wzp, ZP[U8], 0, borders)), (what, name)
        return name

    b, new = abi.check_borders([N, C, T, M], [[1, 0], [0, 0]], 2)
    run("cut window", borders=b, out=_view(_buffer((N, new[2], C, new[3]), U8, 0, fill=0xA5)))
    run("contiguous output", out=None)                 # x segment-major, out NCHW-contiguous: mismatched layouts
    run("C == 1", x_np=_data(rs, (2, 3, 1, 16), U8), wd=wd[:1].contiguous(), w=w[:1], out=_view(_buffer((2, 3, 1, 16), U8, 0, fill=0xA5)))
    run("T == 1", x_np=_data(rs, (2, 1, 5, 16), U8), out=_view(_buffer((2, 1, 5, 16), U8, 0, fill=0xA5)))
    abi.set_path_policy(1)
    try:
        assert run("forced policy", out=_view(_buffer(shape, U8, 0, fill=0xA5))) == "strided_gather_forward"
    finally:
        abi.set_path_policy(0)
    abi.forward_quantized(_view(torch.from_numpy(x_np).cuda()), wd, wzp, ZP[U8], 0, out=_view(_buffer(shape, U8, 0)))
    assert abi.last_kernel() == WHOLE   # (and the same call is served again once the policy is back)


@pytest.mark.parametrize("case", [c for c in FLOAT_CASES if c[1] in (torch.float16, torch.float32)],
                         ids=lambda c: "%s-%s-off%d" % ("x".join(map(str, c[0])), _name(c[1]), c[2]))
def test_float_calls_are_unchanged(case):
    shape, dt, off, kernel = case
    rs = np.random.RandomState(25)
    for pad in range(5):
        w = _float_table(rs, shape[2], shape[1], dt)
        x = _float_buffer(shape, dt, off)
        x.copy_(_float_data(rs, shape, dt))
        out = _float_buffer(shape, dt, off, fill=0xA5)
        abi.forward(_view(x), w, pad, 0, out=_view(out))
        assert abi.last_kernel() == kernel, (shape, dt, pad, abi.last_kernel())
        assert torch.equal(_view(out), abi.forward(_view(x).contiguous(), w, pad, 0)), (shape, dt, pad)


# ---- red zones ------------------------------------------------------------------------------------------------------
GUARDED = [((2, 3, 5, 49), U8, RAGGED), ((2, 3, 5, 3), U8, RAGGED), ((2, 3, 5, 16), U8, WHOLE), ((2, 3, 5, 3), I32, RAGGED)]


@pytest.mark.parametrize("shape,dt,kernel", GUARDED, ids=lambda v: str(v).split(".")[-1].replace(" ", ""))
def test_red_zones(shape, dt, kernel):
    N, T, C, M = shape
    es = torch.empty(0, dtype=dt).element_size()
    rs = np.random.RandomState(26)
    dev = torch.device("cuda")
    for pad, off in itertools.product((0, 3), (0, es)):
        what = (shape, _name(dt), "pad", pad, "offset", off)
        x_np = _data(rs, shape, dt)
        w, wzp = _tables(_shifts(rs, C, T))[0 if dt == U8 else 2]
        want = torch.from_numpy(np.ascontiguousarray(O.forward_q(x_np.transpose(0, 2, 1, 3), w, wzp, ZP[dt], pad).transpose(0, 2, 1, 3)))
        X, OUT = (RZ.Guarded(shape, dt, dev, offset_bytes=off) for _ in range(2))
        wt = torch.from_numpy(w)
        W = RZ.Guarded((C, 2), wt.dtype, dev)

        def forward():
            abi.forward_quantized(_view(X.t), W.t, wzp, ZP[dt], pad, out=_view(OUT.t))
            return abi.last_kernel()

        expect = kernel if off == 0 else RAGGED
        assert RZ.run_guarded(forward, [("x", X, torch.from_numpy(x_np)), ("w", W, wt)], [("out", OUT)], [want], what) == expect


# ---- through the op ---------------------------------------------------------------------------------------------------
QDT = {torch.quint8: U8, torch.qint8: I8, torch.qint32: I32}


def _quantized(rs, shape, qdt, device):
    return torch._make_per_tensor_quantized_tensor(torch.from_numpy(_data(rs, shape, QDT[qdt])).to(device), 0.05, ZP[QDT[qdt]])


@pytest.mark.parametrize("qdt", list(QDT), ids=lambda d: str(d).split(".")[-1])
def test_the_op_equals_the_cpu_op(qdt):
    rs = np.random.RandomState(27)
    for shape, T in (((6, 5, 16), 3), ((8, 6, 7, 7), 4), ((6, 5, 2, 3, 3), 3)):
        for pad in range(5):
            x = _quantized(rs, shape, qdt, "cpu")
            s = torch.from_numpy(_shifts(rs, shape[1], T))
            want = OPS.temporal_shift_quantized(x, s, T, pad)
            xd = torch._make_per_tensor_quantized_tensor(x.int_repr().cuda(), x.q_scale(), x.q_zero_point())
            out = OPS.temporal_shift_quantized(xd, s.cuda(), T, pad)
            assert abi.last_kernel().startswith("segment"), (shape, pad, abi.last_kernel())
            assert out.is_cuda and out.dtype == qdt and out.is_contiguous() and out.shape == x.shape
            assert out.q_scale() == want.q_scale() == x.q_scale() and out.q_zero_point() == want.q_zero_point() == x.q_zero_point()
            assert torch.equal(out.int_repr().cpu(), want.int_repr()), (shape, pad)
            assert torch.equal(temporal_shift_quantized(xd, s.cuda().float().view(-1, 1), T, pad).int_repr(), out.int_repr()), (shape, pad)


def test_the_op_with_an_empty_tensor_launches_nothing():
    x = torch._make_per_tensor_quantized_tensor(torch.zeros(0, 4, 3, dtype=U8, device="cuda"), 0.1, 3)
    before = abi.last_kernel()
    out = OPS.temporal_shift_quantized(x, torch.zeros(4, dtype=torch.long, device="cuda"), 2, 0)
    assert out.shape == x.shape and out.is_quantized and abi.last_kernel() == before


def test_the_module_equals_the_cpu_module():
    T, C = 4, 16
    rs = np.random.RandomState(28)
    m = torchshifts.quantized.TemporalShift(T, C)
    x = _quantized(rs, (8, C, 7, 7), torch.quint8, "cpu")
    want = m(x)
    xd = torch._make_per_tensor_quantized_tensor(x.int_repr().cuda(), x.q_scale(), x.q_zero_point())
    out = m.cuda()(xd)
    assert abi.last_kernel() == RAGGED   # (49-byte planes)
    assert m.shifts.is_cuda and torch.equal(out.int_repr().cpu(), want.int_repr())
    assert out.q_scale() == want.q_scale() and out.q_zero_point() == want.q_zero_point()
    # ... and the slicing idiom on int_repr: the zero point, then three slice copies
    f = C // 8
    v = x.int_repr().view(2, T, C, 7, 7)
    idiom = torch.full_like(v, ZP[U8])
    idiom[:, :-1, :f] = v[:, 1:, :f]
    idiom[:, 1:, f:2 * f] = v[:, :-1, f:2 * f]
    idiom[:, :, 2 * f:] = v[:, :, 2 * f:]
    assert torch.equal(out.int_repr().cpu(), idiom.view(8, C, 7, 7))
