"""Temporal shift on the GPU: the segment-major route of shiftnd_forward (csrc/shiftnd_segment.hip) through the C ABI -- permuted
views of (N, T, C, M) buffers, i.e. [N, C, T, M] problems with strides {T*C*M, M, C*M, 1} -- and through
torch.ops.torchshifts.temporal_shift.  Everything is a pure gather: every comparison is bit for bit, against the C oracle on the
permuted contiguous array and against the same call on contiguous tensors (the kernels that existed before).

Shapes are (N, T, C, M), the smallest at which the kernels can go wrong: one 16-byte piece per plane, pieces per plane that do not
divide the four pieces a thread keeps in flight, planes that are no whole pieces (49 elements, 3 doubles), planes under 16 bytes (6, 8, 10 and 12 bytes), a base one
element off the 16-byte grid, more than one workgroup in either kernel, |shift| up to T + 1 (reflect and symmetric fold twice,
periodic wraps), and a table that also shifts the planes' own dim on two channels (the per-element gather inside the same kernels).
"""
import itertools

import numpy as np
import pytest
import torch

import torchshifts
from torchshifts import abi
from oracle import oracle as O

import redzone as RZ

pytestmark = pytest.mark.gpu

OPS = torch.ops.torchshifts
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
WHOLE, RAGGED, CL = "segment_forward", "segment_forward_ragged", "cl_gather_forward"

# (N, T, C, M), dtype, elements the bases are offset by, the kernel
CASES = [
    ((2, 3, 5, 8), F16, 0, WHOLE),        # one piece per plane
    ((2, 3, 5, 4), F32, 0, WHOLE),
    ((2, 3, 5, 2), F64, 0, WHOLE),
    ((3, 2, 7, 24), BF16, 0, WHOLE),      # 3 pieces per plane: a thread's four pieces straddle planes
    ((1, 9, 3, 16), F32, 0, WHOLE),       # |s| up to T + 1 = 10 on 9 segments
    ((2, 8, 64, 32), F16, 0, WHOLE),      # 4096 pieces: four workgroups
    ((2, 3, 5, 49), F16, 0, RAGGED),      # 98-byte planes: pieces inside one plane and over two, every even split
    ((2, 3, 5, 49), BF16, 0, RAGGED),
    ((2, 3, 5, 49), F32, 0, RAGGED),      # 196 bytes
    # M = 1: memory order N, T, C IS channels-last ([N, C, T, 1] with unit channel stride), which the channel-fastest kernels
    # served before the segment route existed and still do (the route sits behind every earlier one)
    ((2, 4, 6, 1), F32, 0, CL),
    ((2, 3, 4, 3), F64, 0, RAGGED),       # 24 bytes
    # planes under 16 bytes: a 16-byte piece reaches over three and more planes (the two-byte path), or ends with a whole plane
    ((2, 4, 6, 3), F16, 0, RAGGED),       # 6-byte planes: three and four planes per piece
    ((2, 3, 5, 3), F32, 0, RAGGED),       # 12-byte planes: 4 + 12 and 8 + 8 (two planes), 4 + 12 + ... (three)
    ((2, 3, 5, 5), F16, 1, RAGGED),       # 10-byte planes, bases one element off
    ((2, 4, 6, 2), F32, 0, RAGGED),       # 8-byte planes: every piece is two whole planes
    ((2, 3, 5, 8), F16, 1, RAGGED),       # whole pieces, bases one element off
    ((2, 3, 5, 4), F32, 1, RAGGED),
    ((2, 8, 64, 196), F16, 0, RAGGED),    # 392-byte planes, 98 workgroups
]


def _id(case):
    shape, dt, off, kernel = case
    return "%s-%s-off%d" % ("x".join(map(str, shape)), str(dt).split(".")[-1], off)


def _buffer(shape, dt, off, fill=None):
    """a dense (N, T, C, M) device tensor whose base is `off` elements past an aligned allocation"""
    flat = torch.empty(int(np.prod(shape)) + off, dtype=dt, device="cuda")
    t = flat[off:].view(shape)
    assert t.data_ptr() % 16 == (off * t.element_size()) % 16
    if fill is not None:
        t.view(-1).view(torch.uint8).fill_(fill)
    return t


def _view(t):
    """(N, T, C, ...) buffer -> the [N, C, T, ...] problem the library sees"""
    return t.transpose(1, 2)


def _np(t):
    t = t.detach().cpu().contiguous()
    return (t if t.dtype in (F32, F64) else t.float()).numpy()


def _same(got, want_np, what):
    got = _np(got)
    assert got.shape == want_np.shape and np.array_equal(got, want_np.astype(got.dtype)), what


def _table(rs, C, T, dt, cols=2):
    w = np.zeros((C, cols), np.float32)
    w[:, 0] = rs.randint(-T - 1, T + 2, size=C)
    w[0, 0], w[1, 0], w[2, 0] = 0, T + 1, -T - 1
    return torch.from_numpy(w).to(dt).cuda()


def _data(rs, shape, dt):
    return torch.from_numpy(rs.uniform(-1, 1, size=shape)).to(dt)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_c_abi_forward_and_input_gradient(case):
    shape, dt, off, kernel = case
    N, T, C, M = shape
    path = abi.PATH_CL if kernel == CL else abi.PATH_PLANE
    rs = np.random.RandomState(11)
    for pad in range(5):
        what = (_id(case), "pad", pad)
        w = _table(rs, C, T, dt)
        x = _buffer(shape, dt, off)
        x.copy_(_data(rs, shape, dt))
        out = _buffer(shape, dt, off, fill=0xA5)
        abi.forward(_view(x), w, pad, 0, out=_view(out))
        assert abi.last_kernel() == kernel and abi.last_path() == path, what + (abi.last_kernel(),)
        xc = _view(x).contiguous()
        want = O.forward(_np(xc), _np(w), pad, False)
        _same(_view(out), want, what + ("forward against the oracle",))
        dense = abi.forward(xc, w, pad, 0)
        assert not abi.last_kernel().startswith("segment"), what
        assert torch.equal(_view(out), dense), what + ("forward against the contiguous call",)
        # the input gradient alone: the same route under the negated table
        go = _buffer(shape, dt, off)
        go.copy_(_data(rs, shape, dt))
        gx = _buffer(shape, dt, off, fill=0xA5)
        abi.backward_input(_view(go), w, (N, C, T, M), pad, grad_x=_view(gx))
        assert abi.last_kernel() == kernel and abi.last_path() == path, what + (abi.last_kernel(),)
        goc = _view(go).contiguous()
        _same(_view(gx), O.backward(_np(goc), _np(w), _np(xc), pad, False)[0], what + ("grad_x against the oracle",))
        assert torch.equal(_view(gx), abi.backward_input(goc, w, (N, C, T, M), pad)), what + ("grad_x against the contiguous call",)


@pytest.mark.parametrize("shape,dt,kernel", [((2, 3, 5, 8), F16, WHOLE), ((2, 3, 5, 24), F32, WHOLE), ((2, 3, 5, 49), F16, RAGGED),
                                             ((2, 3, 5, 49), F32, RAGGED), ((2, 3, 4, 3), F64, RAGGED)],
                         ids=lambda v: str(v).split(".")[-1].replace(" ", ""))
def test_a_table_with_inner_shifts_is_gathered_exactly(shape, dt, kernel):
    """the host routes by strides alone: channels 1 and 3 also shift the planes' own dim and must come out right"""
    N, T, C, M = shape
    rs = np.random.RandomState(12)
    for pad in range(5):
        w = _table(rs, C, T, dt)
        w[1, 1], w[3, 1] = 2, -1
        x = _data(rs, shape, dt).cuda()
        out = _buffer(shape, dt, 0, fill=0xA5)
        abi.forward(_view(x), w, pad, 0, out=_view(out))
        assert abi.last_kernel() == kernel, (shape, dt, pad, abi.last_kernel())
        _same(_view(out), O.forward(_np(_view(x)), _np(w), pad, False), (shape, dt, pad))


@pytest.mark.parametrize("dt,kernel", [(F16, WHOLE), (F32, RAGGED)], ids=["float16", "float32"])
def test_three_spatial_dims(dt, kernel):
    """[N, C, T, H, W] in memory order N, T, C, H, W; channel 1 shifts H, channel 3 shifts W"""
    N, T, C = 2, 3, 5
    H = W = 4 if dt == F16 else 3   # 32-byte planes; 36-byte planes (4-byte units)
    rs = np.random.RandomState(13)
    for pad in range(5):
        w = _table(rs, C, T, dt, cols=3)
        w[1, 1], w[3, 2] = -1, 2
        x = _data(rs, (N, T, C, H, W), dt).cuda()
        out = _buffer((N, T, C, H, W), dt, 0, fill=0xA5)
        abi.forward(_view(x), w, pad, 0, out=_view(out))
        assert abi.last_kernel() == kernel, (dt, pad, abi.last_kernel())
        _same(_view(out), O.forward(_np(_view(x)), _np(w), pad, False), (dt, pad))


def test_fp32_table_with_fp16_tensor():
    shape = (2, 3, 5, 8)
    rs = np.random.RandomState(14)
    x = _data(rs, shape, F16).cuda()
    for pad in range(5):
        w16 = _table(rs, 5, 3, F16)
        out = _buffer(shape, F16, 0, fill=0xA5)
        abi.forward(_view(x), w16.float(), pad, 0, out=_view(out))   # (abi.problem sets SHIFTND_WEIGHTS_F32)
        assert abi.last_kernel() == WHOLE, abi.last_kernel()
        _same(_view(out), O.forward(_np(_view(x)), _np(w16), pad, False), ("mixed", pad))
        same = _buffer(shape, F16, 0, fill=0xA5)
        abi.forward(_view(x), w16, pad, 0, out=_view(same))
        assert abi.last_kernel() == WHOLE and torch.equal(out, same), ("mixed against the same-dtype call", pad)


def test_declined_calls_keep_their_kernels_and_bits():
    shape = (2, 3, 5, 8)
    N, T, C, M = shape
    rs = np.random.RandomState(15)
    x = _data(rs, shape, F32).cuda()
    w = _table(rs, C, T, F32)
    xv = _view(x)

    def run(what, xin=xv, active=0, borders=None, out=None, weights=w):
        o = abi.forward(xin, weights, 0, active, borders, out=out)
        name = abi.last_kernel()
        assert not name.startswith("segment"), (what, name)
        _same(o, O.forward(_np(xin), _np(weights), 0, bool(active), borders), (what, name))
        return name

    wa = w + 0.25
    run("active", active=1, weights=wa)
    b, new = abi.check_borders([N, C, T, M], [[1, 0], [0, 0]], 2)
    run("cut window", borders=b, out=_view(_buffer((N, new[2], C, new[3]), F32, 0, fill=0xA5)))
    run("contiguous output", out=None)                 # x segment-major, out NCHW-contiguous: mismatched layouts
    x1 = _data(rs, (2, 3, 1, 8), F32).cuda()
    run("C == 1", xin=_view(x1), weights=w[:1].contiguous(), out=_view(_buffer((2, 3, 1, 8), F32, 0, fill=0xA5)))
    x2 = _data(rs, (2, 1, 5, 8), F32).cuda()
    run("T == 1", xin=_view(x2), out=_view(_buffer((2, 1, 5, 8), F32, 0, fill=0xA5)))
    abi.set_path_policy(1)
    try:
        assert run("forced policy", out=_view(_buffer(shape, F32, 0, fill=0xA5))) == "strided_gather_forward"
    finally:
        abi.set_path_policy(0)
    abi.forward(xv, w, 0, 0, out=_view(_buffer(shape, F32, 0)))
    assert abi.last_kernel() == WHOLE   # (and the same call is served again once the policy is back)


# ---- red zones ------------------------------------------------------------------------------------------------------
GUARDED = [((2, 3, 5, 8), F16, WHOLE), ((2, 3, 5, 49), F16, RAGGED), ((2, 3, 5, 4), F32, WHOLE), ((2, 3, 5, 49), F32, RAGGED),
           ((2, 3, 5, 2), F64, WHOLE), ((2, 3, 4, 3), F64, RAGGED),
           ((2, 4, 6, 3), F16, RAGGED), ((2, 3, 5, 3), F32, RAGGED)]   # planes of 6 and 12 bytes


@pytest.mark.parametrize("shape,dt,kernel", GUARDED, ids=lambda v: str(v).split(".")[-1].replace(" ", ""))
def test_red_zones(shape, dt, kernel):
    N, T, C, M = shape
    es = torch.empty(0, dtype=dt).element_size()
    rs = np.random.RandomState(16)
    dev = torch.device("cuda")
    for pad, off in itertools.product((0, 3), (0, es)):
        what = (shape, str(dt), "pad", pad, "offset", off)
        w = _table(rs, C, T, dt)
        x, go = _data(rs, shape, dt), _data(rs, shape, dt)
        xc, goc = _np(x.transpose(1, 2)), _np(go.transpose(1, 2))
        want_out = torch.from_numpy(O.forward(xc, _np(w), pad, False)).to(dt).transpose(1, 2).contiguous()
        want_gx = torch.from_numpy(O.backward(goc, _np(w), xc, pad, False)[0]).to(dt).transpose(1, 2).contiguous()
        X, OUT, G, GX = (RZ.Guarded(shape, dt, dev, offset_bytes=off) for _ in range(4))
        W = RZ.Guarded((C, 2), dt, dev)
        WS = RZ.Guarded((C * 2 * es,), torch.uint8, dev)

        def forward():
            abi.forward(_view(X.t), W.t, pad, 0, out=_view(OUT.t))
            return abi.last_kernel()

        def backward_input():
            abi.backward_input(_view(G.t), W.t, (N, C, T, M), pad, grad_x=_view(GX.t), workspace=WS.t)
            return abi.last_kernel()

        expect = kernel if off == 0 else RAGGED
        assert RZ.run_guarded(forward, [("x", X, x), ("w", W, w)], [("out", OUT)], [want_out], what + ("forward",)) == expect
        assert RZ.run_guarded(backward_input, [("grad_out", G, go), ("w", W, w)], [("grad_x", GX), ("workspace", WS)], [want_gx, None],
                              what + ("backward_input",)) == expect


# ---- through the op ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64, F16, BF16], ids=lambda d: str(d).split(".")[-1])
def test_the_op_equals_the_cpu_op(dt):
    rs = np.random.RandomState(17)
    for shape, T, kernel in (((6, 5, 4, 8), 3, WHOLE), ((6, 5, 7, 7), 3, RAGGED), ((8, 6), 4, None)):   # (M = 1: channels-last kernels)
        for pad in range(5):
            x = _data(rs, shape, dt)
            go = _data(rs, shape, dt)
            s = torch.from_numpy(rs.randint(-T - 1, T + 2, size=shape[1]))
            xc = x.clone().requires_grad_(True)
            OPS.temporal_shift(xc, s, T, pad).backward(go)
            xg = x.cuda().requires_grad_(True)
            out = OPS.temporal_shift(xg, s.cuda(), T, pad)
            assert kernel is None or abi.last_kernel() == kernel, (shape, pad, abi.last_kernel())
            out.backward(go.cuda())
            assert torch.equal(out.detach().cpu(), OPS.temporal_shift(x, s, T, pad)), (shape, pad)
            assert torch.equal(xg.grad.cpu(), xc.grad), (shape, pad)


def test_the_module_equals_the_slicing_idiom():
    T, C = 8, 64
    m = torchshifts.TemporalShift(T, C).cuda()
    x = torch.randn(16, C, 14, 14, device="cuda", dtype=F16, requires_grad=True)
    out = m(x)
    assert abi.last_kernel() == RAGGED   # (392-byte planes)
    f = C // 8
    v = x.detach().view(2, T, C, 14, 14)
    want = torch.zeros_like(v)
    want[:, :-1, :f] = v[:, 1:, :f]
    want[:, 1:, f:2 * f] = v[:, :-1, f:2 * f]
    want[:, :, 2 * f:] = v[:, :, 2 * f:]
    assert torch.equal(out.detach(), want.view_as(x))
    go = torch.randn_like(out)
    out.backward(go)
    g = go.view(2, T, C, 14, 14)
    gx = torch.zeros_like(g)
    gx[:, 1:, :f] = g[:, :-1, :f]
    gx[:, :-1, f:2 * f] = g[:, 1:, f:2 * f]
    gx[:, :, 2 * f:] = g[:, :, 2 * f:]
    assert torch.equal(x.grad, gx.view_as(x))
