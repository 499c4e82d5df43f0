"""Quantized interpolating temporal shift on the GPU: shiftnd_forward_quantized under SHIFTND_SHIFT_DIM0 with an fp32 table
(csrc/shiftnd_tshift_quant.hip, one kernel: tshift_forward_quantized) through the C ABI on permuted views of (N, T, C, M) buffers,
and through torch.ops.torchshifts_quantized_learnable and torchshifts.quantized.LearnableTemporalShift on HIP tensors.

The reference is tests/test_qtshift_cpu.py's `definition` -- the float CPU op on (int_repr - zp) in fp32 / fp64, rint, + zp, clamp
-- and every comparison is bit for bit.  The C-ABI cases reach each unit width at the smallest shape that does: 16-byte units (U8
M = 16, I32 M = 4), 8-byte (M = 8), 4-byte (M = 196; I32 M = 3), 1-byte (I8 M = 49; a U8 base one byte off the 16-byte grid), and
[2, 5, 3, 16 * 77] is 2310 units: three workgroups of 256 threads x 4 units, the last one partial.
"""
import numpy as np
import pytest
import torch

import torchshifts
from torchshifts import abi
from torchshifts.quantized.functional import temporal_shift_learnable_quantized

import redzone as RZ
from test_qtshift_cpu import definition, tables

pytestmark = pytest.mark.gpu

OP = torch.ops.torchshifts_quantized_learnable.temporal_shift_learnable_quantized
KERNEL = "tshift_forward_quantized"
U8, I8, I32 = torch.uint8, torch.int8, torch.int32
QOF = {U8: torch.quint8, I8: torch.qint8, I32: torch.qint32}
ZP = {U8: 3, I8: -7, I32: 11}
NP = {U8: np.uint8, I8: np.int8, I32: np.int32}
RANGE = {U8: (0, 256), I8: (-128, 128), I32: (-2 ** 30, 2 ** 30 + 1)}

# (N, T, C, M), dtype, base offset in bytes
CASES = [((2, 3, 5, 16), U8, 0), ((2, 3, 5, 8), U8, 0), ((2, 3, 5, 196), U8, 0), ((2, 3, 5, 49), I8, 0), ((2, 3, 5, 4), I32, 0),
         ((2, 3, 5, 3), I32, 0), ((2, 3, 5, 16), U8, 1), ((2, 5, 3, 16 * 77), U8, 0)]


def _id(case):
    shape, dt, off = case
    return "%s-%s-off%d" % ("x".join(map(str, shape)), str(dt).split(".")[-1], off)


def _view(t):
    """(N, T, C, M) buffer -> the [N, C, T, M] problem the library sees"""
    return t.transpose(1, 2)


def _buffer(shape, dt, off_bytes, fill=None):
    """a dense device tensor of `shape` whose base is `off_bytes` past an aligned allocation"""
    es = torch.empty(0, dtype=dt).element_size()
    flat = torch.empty(int(np.prod(shape)) * es + off_bytes, dtype=torch.uint8, device="cuda")
    if fill is not None:
        flat.fill_(fill)
    t = flat[off_bytes:].view(dt).view(shape)
    assert t.data_ptr() % 16 == off_bytes % 16
    return t


def _data(rs, shape, dt):
    lo, hi = RANGE[dt]
    return rs.randint(lo, hi, size=shape, dtype=np.int64).astype(NP[dt])


def _want(x_np, dt, w, T, pad):
    """the definition on the CPU, in the buffer's (N, T, C, M) order"""
    N, _, C, M = x_np.shape
    q = torch._make_per_tensor_quantized_tensor(torch.from_numpy(x_np).reshape(N * T, C, M), 0.05, ZP[dt])
    return definition(q, w, T, pad).reshape(x_np.shape)


def _call(x, w, dt, pad, out, **kw):
    kw.setdefault("active", True)
    kw.setdefault("shift_dim0", True)
    return abi.forward_quantized(_view(x), w, kw.pop("wzp", 0), ZP[dt], pad, out=None if out is None else _view(out), **kw)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_c_abi_against_the_definition(case):
    shape, dt, off = case
    N, T, C, M = shape
    rs = np.random.RandomState(71)
    x = _buffer(shape, dt, off)
    for pad in range(5):
        x_np = _data(rs, shape, dt)
        x.copy_(torch.from_numpy(x_np))
        for w in tables(C, T):
            out = _buffer(shape, dt, off, fill=0xA5)
            _call(x, w.cuda(), dt, pad, out)
            assert abi.last_kernel() == KERNEL and abi.last_path() == abi.PATH_PLANE, (_id(case), abi.last_kernel())
            assert torch.equal(out.cpu(), _want(x_np, dt, w, T, pad)), (_id(case), "pad", pad, w.tolist())


# ---- red zones ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dt,off", [((2, 3, 5, 16), U8, 0), ((2, 3, 5, 49), I8, 0), ((2, 3, 5, 16), U8, 1), ((2, 3, 5, 4), I32, 0)],
                         ids=lambda v: str(v).split(".")[-1].replace(" ", ""))
def test_red_zones(shape, dt, off):
    N, T, C, M = shape
    rs = np.random.RandomState(72)
    dev = torch.device("cuda")
    for pad in (0, 3):
        x_np = _data(rs, shape, dt)
        w = tables(C, T)[1]
        X, OUT = (RZ.Guarded(shape, dt, dev, offset_bytes=off) for _ in range(2))
        W = RZ.Guarded((C,), torch.float32, dev)

        def forward():
            _call(X.t, W.t, dt, pad, OUT.t)
            return abi.last_kernel()

        what = (shape, str(dt), "pad", pad, "offset", off)
        assert RZ.run_guarded(forward, [("x", X, torch.from_numpy(x_np)), ("w", W, w)], [("out", OUT)], [_want(x_np, dt, w, T, pad)],
                              what) == KERNEL


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_output_untouched():
    shape = (2, 3, 5, 16)
    N, T, C, M = shape
    rs = np.random.RandomState(73)
    x_np = _data(rs, shape, U8)
    x = torch.from_numpy(x_np).cuda()
    w = tables(C, T)[1].cuda()

    def refused(what, call, out, status="invalid argument"):
        with pytest.raises(RuntimeError, match=status):
            call()
        torch.cuda.synchronize()
        assert bool((out.contiguous().view(-1).view(U8) == 0xA5).all()), what

    b, new = abi.check_borders([N, C, T, M], [[1, 0], [0, 0]], 2)
    out = _buffer((N, new[2], C, new[3]), U8, 0, fill=0xA5)
    refused("cut window", lambda: _call(x, w, U8, 0, out, borders=b), out)
    # channels-last views: memory order N, T, M, C seen as [N, C, T, M]
    xcl = torch.from_numpy(np.ascontiguousarray(x_np.transpose(0, 1, 3, 2))).cuda().permute(0, 3, 1, 2)
    ocl = _buffer((N, T, M, C), U8, 0, fill=0xA5)
    refused("channels-last views", lambda: abi.forward_quantized(xcl, w, 0, ZP[U8], 0, out=ocl.permute(0, 3, 1, 2), shift_dim0=True,
                                                                active=True), ocl)
    out = _buffer(shape, U8, 0, fill=0xA5)
    refused("channels-last x", lambda: abi.forward_quantized(xcl, w, 0, ZP[U8], 0, out=_view(out), shift_dim0=True, active=True), out)
    same = _buffer(shape, U8, 0, fill=0xA5)
    refused("out == x", lambda: _call(same, w, U8, 0, same), same)
    # (active == 0 under a float table keeps the status it had before the kernel existed: tests/test_temporal_cl_cpu.py pins it)
    refused("active == 0", lambda: _call(x, w, U8, 0, out, active=False), out, status="unsupported dtype")
    refused("an integer table under the flag", lambda: _call(x, torch.ones(C, dtype=torch.int32, device="cuda"), U8, 0, out, active=False), out)
    refused("an integer table under the flag, active", lambda: _call(x, torch.ones(C, dtype=torch.int32, device="cuda"), U8, 0, out), out)
    refused("a nonzero w_zero_point", lambda: _call(x, w, U8, 0, out, wzp=1), out)
    with pytest.raises(RuntimeError, match="unsupported dtype"):   # without the flag a float table stays what it was
        _call(x, w, U8, 0, out, shift_dim0=False)
    assert bool((out.view(-1) == 0xA5).all())
    _call(x, w, U8, 0, out)   # ... and the call itself is served
    assert abi.last_kernel() == KERNEL and torch.equal(out.cpu(), _want(x_np, U8, w.cpu(), T, 0))


# ---- through the op and the module --------------------------------------------------------------------------------------
def _quantized(rs, shape, dt):
    return torch._make_per_tensor_quantized_tensor(torch.from_numpy(_data(rs, shape, dt)), 0.05, ZP[dt])


def _to_cuda(x, channels_last=False):
    r = x.int_repr().cuda()
    if not channels_last:
        return torch._make_per_tensor_quantized_tensor(r, x.q_scale(), x.q_zero_point())
    # memory order (dim 0, spatial dims, channels): quantize the permuted contiguous tensor, then permute the view back
    order = [0] + list(range(2, r.dim())) + [1]
    back = [0, r.dim() - 1] + list(range(1, r.dim() - 1))
    return torch._make_per_tensor_quantized_tensor(r.permute(order).contiguous(), x.q_scale(), x.q_zero_point()).permute(back)


@pytest.mark.parametrize("dt", [U8, I8, I32], ids=lambda d: str(d).split(".")[-1])
def test_the_op_equals_the_cpu_op(dt):
    rs = np.random.RandomState(74)
    for shape, T in (((6, 5, 16), 3), ((8, 6, 7, 7), 4), ((6, 5, 2, 3, 3), 3)):
        for pad in range(5):
            x = _quantized(rs, shape, dt)
            w = torch.from_numpy(rs.uniform(-T - 1.5, T + 1.5, size=shape[1]).astype(np.float32))
            w[:2] = torch.tensor([0.5, -2.0])
            want = OP(x, w, T, pad, True)
            for cl in ((False, True) if len(shape) >= 4 else (False,)):
                xd = _to_cuda(x, cl)
                assert xd.is_contiguous() != cl
                out = OP(xd, w.cuda().view(-1, 1), T, pad, True)
                assert abi.last_kernel() == KERNEL, (shape, pad, abi.last_kernel())
                assert out.is_cuda and out.dtype == QOF[dt] and out.is_contiguous() and out.shape == x.shape
                assert out.q_scale() == x.q_scale() and out.q_zero_point() == x.q_zero_point()
                assert torch.equal(out.int_repr().cpu(), want.int_repr()), (shape, pad, cl)
            sparse = temporal_shift_learnable_quantized(_to_cuda(x), w.cuda(), T, pad, False)
            assert abi.last_kernel().startswith("segment"), abi.last_kernel()
            assert torch.equal(sparse.int_repr().cpu(), OP(x, w, T, pad, False).int_repr()), (shape, pad)


def test_the_module_equals_the_cpu_module():
    rs = np.random.RandomState(75)
    f = torchshifts.LearnableTemporalShift(4, 16, padding="reflect", active_flag=True, sparsity_term=0.)
    with torch.no_grad():
        f.weight.copy_(torch.from_numpy(rs.uniform(-5, 5, size=(16, 1)).astype(np.float32)))
    m = torchshifts.quantized.LearnableTemporalShift.from_float(f)
    x = _quantized(rs, (8, 16, 7, 7), U8)
    want = m(x)
    out = m.cuda()(_to_cuda(x))
    assert abi.last_kernel() == KERNEL and m.weight.is_cuda
    assert torch.equal(out.int_repr().cpu(), want.int_repr()) and out.q_scale() == want.q_scale() and out.q_zero_point() == want.q_zero_point()


def test_an_empty_tensor_launches_nothing():
    x = torch._make_per_tensor_quantized_tensor(torch.zeros(0, 4, 3, dtype=U8, device="cuda"), 0.1, 3)
    before = abi.last_kernel()
    out = OP(x, torch.zeros(4, device="cuda"), 2, 0, True)
    assert out.shape == x.shape and out.is_quantized and abi.last_kernel() == before


def test_graph_capture_and_replay():
    rs = np.random.RandomState(76)
    x = _to_cuda(_quantized(rs, (8, 16, 6, 6), U8))
    w = torch.linspace(-2.3, 2.3, 16, device="cuda")
    want = OP(x, w, 4, 0, True)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        OP(x, w, 4, 0, True)   # (warm-up on the capture stream)
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):   # (a host synchronisation would fail the capture)
            out = OP(x, w, 4, 0, True)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.int_repr(), want.int_repr())


def test_the_size_limit_is_refused_before_anything_is_allocated():
    free, _ = torch.cuda.mem_get_info()
    if free < 4 * 2 ** 30:
        pytest.skip("needs 4 GiB of free device memory")
    x = torch._empty_affine_quantized([2 ** 15, 2 ** 8, 2 ** 8], scale=0.1, zero_point=3, dtype=torch.quint8, device="cuda")
    w = torch.zeros(2 ** 8, device="cuda")
    before = torch.cuda.memory_allocated()
    with pytest.raises(RuntimeError, match=r"temporal_shift_learnable_quantized: a tensor of 2147483648 elements is beyond the kernel's "
                                           r"limit of 2\^31 - 16 units"):
        OP(x, w, 2, 0, True)
    assert torch.cuda.memory_allocated() == before
