"""Quantized temporal interlacing and the quantized per-clip temporal shift on the GPU: shiftnd_forward_quantized under
SHIFTND_SHIFT_DIM0 | SHIFTND_PER_CLIP (an fp32 [N, C] table) and SHIFTND_SHIFT_DIM0 | SHIFTND_INTERLACE (the packed fp32 table)
(csrc/shiftnd_interlace_quant.hip, one kernel: tinterlace_forward_quantized) through the C ABI on permuted views of (N, T, C, M)
buffers, and through torch.ops.torchshifts_quantized_interlace and the two quantized modules on HIP tensors.

The references are tests/test_qinterlace_cpu.py's `definition` -- the float CPU ops on (int_repr - zp) in fp32 / fp64, rint, + zp,
clamp -- and the CPU op; every comparison is bit for bit.  The C-ABI cases reach each unit width at the smallest shape that does
(tests/test_qtshift_gpu.py), always with two clips, so that a kernel reading row 0 of the offsets for every clip fails; (2, 4, 8, 16)
is TIN's shape: a fold of four channels, the others passing through under offset 0 and scale 1 (the kernel's copy path).
"""
import numpy as np
import pytest
import torch

import torchshifts
from torchshifts import abi
from torchshifts.quantized.functional import temporal_interlace_quantized

import redzone as RZ
from test_qinterlace_cpu import definition, offset_tables, scale_table, trained
from test_qtshift_gpu import I8, I32, QOF, U8, ZP, _buffer, _data, _quantized, _to_cuda, _view

pytestmark = pytest.mark.gpu

OP = torch.ops.torchshifts_quantized_interlace.temporal_interlace_quantized
KERNEL = "tinterlace_forward_quantized"

# (N, T, C, M), dtype, base offset in bytes
CASES = [((2, 3, 5, 16), U8, 0), ((2, 3, 5, 8), U8, 0), ((2, 3, 5, 196), U8, 0), ((2, 3, 5, 49), I8, 0), ((2, 3, 5, 4), I32, 0),
         ((2, 3, 5, 3), I32, 0), ((2, 3, 5, 16), U8, 1), ((2, 5, 3, 16 * 77), U8, 0), ((2, 1, 5, 16), U8, 0), ((2, 4, 8, 16), U8, 0)]


def _id(case):
    shape, dt, off = case
    return "%s-%s-off%d" % ("x".join(map(str, shape)), str(dt).split(".")[-1], off)


def _tables(N, T, C):
    """[(offsets [N, C], scales [N, T, C])]: the ladders, and for TIN's shape the layer's own form as well"""
    pairs = [(o, scale_table(N, T, C, 4 * i)) for i, o in enumerate(offset_tables(N, C, T))]
    if C == 8:
        o, s = pairs[0][0].clone(), pairs[1][1].clone()
        o[:, :4] = torch.tensor([[0.3, 0.3, -0.3, -0.3], [-1.5, -1.5, 1.5, 1.5]])
        o[:, 4:] = 0
        s[:, :, 4:] = 1
        pairs.append((o, s))
    return pairs


def _want(x_np, dt, offsets, scales, T, pad, active):
    """the definition on the CPU, in the buffer's (N, T, C, M) order"""
    N, _, C, M = x_np.shape
    q = torch._make_per_tensor_quantized_tensor(torch.from_numpy(x_np).reshape(N * T, C, M), 0.05, ZP[dt])
    return definition(q, offsets, scales, T, pad, active).reshape(x_np.shape)


def _table(offsets, scales):
    return (offsets if scales is None else abi.pack_interlace(offsets, scales)).cuda()


def _call(x, w, dt, pad, out, packed, **kw):
    """packed: `w` is the packed table (INTERLACE), else the [N, C] one (PER_CLIP); per_clip= / interlace= override the bits"""
    kw.setdefault("active", True)
    kw.setdefault("shift_dim0", True)
    kw.setdefault("per_clip", not packed)
    kw.setdefault("interlace", packed)
    return abi.forward_quantized(_view(x), w, kw.pop("wzp", 0), ZP[dt], pad, out=None if out is None else _view(out), **kw)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_c_abi_against_the_definition(case):
    shape, dt, off = case
    N, T, C, M = shape
    rs = np.random.RandomState(171)
    x = _buffer(shape, dt, off)
    for pad in range(5):
        x_np = _data(rs, shape, dt)
        x.copy_(torch.from_numpy(x_np))
        for offsets, scales in _tables(N, T, C):
            for interlace in (False, True):
                sc = scales if interlace else None
                w = _table(offsets, sc)
                for active in (True, False):
                    out = _buffer(shape, dt, off, fill=0xA5)
                    _call(x, w, dt, pad, out, interlace, active=active)
                    assert abi.last_kernel() == KERNEL and abi.last_path() == abi.PATH_PLANE, (_id(case), abi.last_kernel())
                    assert torch.equal(out.cpu(), _want(x_np, dt, offsets, sc, T, pad, active)), \
                        (_id(case), "pad", pad, "interlace", interlace, "active", active, offsets.tolist())


# ---- red zones ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dt,off", [((2, 3, 5, 16), U8, 0), ((2, 3, 5, 49), I8, 0), ((2, 3, 5, 16), U8, 1), ((2, 3, 5, 4), I32, 0)],
                         ids=lambda v: str(v).split(".")[-1].replace(" ", ""))
def test_red_zones(shape, dt, off):
    N, T, C, M = shape
    rs = np.random.RandomState(172)
    dev = torch.device("cuda")
    offsets, scales = _tables(N, T, C)[1]
    for pad in (0, 3):
        for interlace in (False, True):
            sc = scales if interlace else None
            table = _table(offsets, sc).cpu().reshape(-1)
            x_np = _data(rs, shape, dt)
            X, OUT = (RZ.Guarded(shape, dt, dev, offset_bytes=off) for _ in range(2))
            W = RZ.Guarded((table.numel(),), torch.float32, dev)

            def forward():
                _call(X.t, W.t, dt, pad, OUT.t, interlace)
                return abi.last_kernel()

            what = (shape, str(dt), "pad", pad, "offset", off, "interlace", interlace)
            assert RZ.run_guarded(forward, [("x", X, torch.from_numpy(x_np)), ("table", W, table)], [("out", OUT)],
                                  [_want(x_np, dt, offsets, sc, T, pad, True)], what) == KERNEL


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_output_untouched():
    shape = (2, 3, 5, 16)
    N, T, C, M = shape
    rs = np.random.RandomState(173)
    x_np = _data(rs, shape, U8)
    x = torch.from_numpy(x_np).cuda()
    offsets, scales = _tables(N, T, C)[1]

    def refused(what, call, out, status="invalid argument"):
        with pytest.raises(RuntimeError, match=status):
            call()
        torch.cuda.synchronize()
        assert bool((out.contiguous().view(-1).view(U8) == 0xA5).all()), what

    for interlace in (False, True):
        sc = scales if interlace else None
        w = _table(offsets, sc)
        bits = dict(per_clip=not interlace, interlace=interlace)
        b, new = abi.check_borders([N, C, T, M], [[1, 0], [0, 0]], 2)
        out = _buffer((N, new[2], C, new[3]), U8, 0, fill=0xA5)
        refused("cut window", lambda: _call(x, w, U8, 0, out, interlace, borders=b), out)
        # channels-last views: memory order N, T, M, C seen as [N, C, T, M]
        xcl = torch.from_numpy(np.ascontiguousarray(x_np.transpose(0, 1, 3, 2))).cuda().permute(0, 3, 1, 2)
        ocl = _buffer((N, T, M, C), U8, 0, fill=0xA5)
        refused("channels-last views", lambda: abi.forward_quantized(xcl, w, 0, ZP[U8], 0, out=ocl.permute(0, 3, 1, 2), shift_dim0=True,
                                                                    active=True, **bits), ocl)
        out = _buffer(shape, U8, 0, fill=0xA5)
        refused("channels-last x", lambda: abi.forward_quantized(xcl, w, 0, ZP[U8], 0, out=_view(out), shift_dim0=True, active=True, **bits), out)
        same = _buffer(shape, U8, 0, fill=0xA5)
        refused("out == x", lambda: _call(same, w, U8, 0, same, interlace), same)
        for active in (True, False):
            # (an integer table under the bits keeps the answer it had: the bits are no part of a quantized dtype)
            refused("an integer table under the new bits",
                    lambda: _call(x, torch.ones(w.numel(), dtype=torch.int32, device="cuda"), U8, 0, out, interlace, active=active), out,
                    status="unsupported dtype")
            refused("a nonzero w_zero_point", lambda: _call(x, w, U8, 0, out, interlace, wzp=1, active=active), out)
            refused("both bits together", lambda: _call(x, w, U8, 0, out, interlace, per_clip=True, interlace=True, active=active), out)
            refused("FRAMES beside the bit", lambda: _call(x, w, U8, 0, out, interlace, frames=True, active=active), out)
        with pytest.raises(RuntimeError, match="unsupported dtype"):   # without the flag the bits are no part of any dtype
            _call(x, w, U8, 0, out, interlace, shift_dim0=False)
        assert bool((out.view(-1) == 0xA5).all())
        for active in (True, False):   # ... and the call itself is served, in both modes
            _call(x, w, U8, 0, out, interlace, active=active)
            assert abi.last_kernel() == KERNEL and torch.equal(out.cpu(), _want(x_np, U8, offsets, sc, T, 0, active))


def test_the_workspace_query_is_zero():
    import ctypes
    x = torch.empty(2, 5, 3, 16, dtype=U8)
    for bits in (dict(per_clip=True), dict(interlace=True)):
        for active in (True, False):
            p = abi.problem(x, 0, active, None, shift_dim0=True, **bits)
            assert int(abi.lib().shiftnd_backward_workspace_bytes(ctypes.byref(p))) == 0


# ---- through the op and the modules -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [U8, I8, I32], ids=lambda d: str(d).split(".")[-1])
def test_the_op_equals_the_cpu_op(dt):
    rs = np.random.RandomState(174)
    for shape, T in (((6, 5, 16), 3), ((8, 6, 7, 7), 4), ((6, 5, 2, 3, 3), 3)):
        N, C = shape[0] // T, shape[1]
        for pad in range(5):
            x = _quantized(rs, shape, dt)
            offsets = torch.from_numpy(rs.uniform(-T - 1.5, T + 1.5, size=(N, C)).astype(np.float32))
            offsets[0, :2] = torch.tensor([0.5, -2.0])
            scales = torch.from_numpy(rs.uniform(0, 2, size=(N, T, C)).astype(np.float32))
            scales[0, :, 1] = 1
            for sc in (scales, None):
                for active in (True, False):
                    want = OP(x, offsets, sc, T, pad, active)
                    for cl in ((False, True) if len(shape) >= 4 else (False,)):
                        xd = _to_cuda(x, cl)
                        assert xd.is_contiguous() != cl
                        out = OP(xd, offsets.cuda(), None if sc is None else sc.cuda(), T, pad, active)
                        assert abi.last_kernel() == KERNEL, (shape, pad, abi.last_kernel())
                        assert out.is_cuda and out.dtype == QOF[dt] and out.is_contiguous() and out.shape == x.shape
                        assert out.q_scale() == x.q_scale() and out.q_zero_point() == x.q_zero_point()
                        assert torch.equal(out.int_repr().cpu(), want.int_repr()), (shape, pad, cl, active, sc is None)


def test_the_per_clip_module_equals_the_cpu_module():
    rs = np.random.RandomState(175)
    for active in (True, False):
        m = torchshifts.quantized.LearnablePerClipTemporalShift.from_float(
            torchshifts.LearnablePerClipTemporalShift(4, padding="reflect", active_flag=active))
        x = _quantized(rs, (8, 16, 7, 7), U8)
        table = torch.from_numpy(rs.uniform(-5, 5, size=(2, 16)).astype(np.float32))
        want = m(x, table)
        for cl in (False, True):
            out = m(_to_cuda(x, cl), table.cuda())
            assert abi.last_kernel() == KERNEL and out.is_contiguous()
            assert torch.equal(out.int_repr().cpu(), want.int_repr()) and out.q_scale() == want.q_scale()


def test_the_interlace_module_equals_the_cpu_op_under_its_own_tables():
    """the nets are float and run on the device, so the module's tables carry that backend's conv / linear / sigmoid bits: the layer's
    output is the CPU op under the device's tables, bit for bit; the descriptor (an integer sum, then one division, one subtraction and
    one multiplication in fp32) is the CPU's to two ulps of the largest mean (255) times the scale; the tables agree with the CPU module's to 1e-5 (values below 2: some
    forty ulps for a dozen accumulated terms and one exp)"""
    rs = np.random.RandomState(176)
    T, C = 4, 16
    for shift_div, dt in ((1, U8), (4, I8)):
        f = trained(T, C, shift_div, "border", 220)
        q = torchshifts.quantized.TemporalInterlace.from_float(f)
        x = _quantized(rs, (3 * T, C, 7, 7), dt)
        cpu_desc, cpu_tables = q.descriptor(x), q.tables(x)
        qd = torchshifts.quantized.TemporalInterlace.from_float(f).cuda()
        for cl in (False, True):
            xd = _to_cuda(x, cl)
            desc = qd.descriptor(xd).cpu()
            assert float((desc - cpu_desc).abs().max()) <= 2.0 ** -22 * 255 * x.q_scale()
            offsets, scales = (t.cpu() for t in qd.tables(xd))
            assert float((offsets - cpu_tables[0]).abs().max()) <= 1e-5 and float((scales - cpu_tables[1]).abs().max()) <= 1e-5
            out = qd(xd)
            assert abi.last_kernel() == KERNEL and out.is_contiguous() and out.q_scale() == x.q_scale()
            assert torch.equal(out.int_repr().cpu(), OP(x, offsets, scales, T, 1, True).int_repr()), (shift_div, cl)


def test_an_empty_tensor_launches_nothing():
    x = torch._make_per_tensor_quantized_tensor(torch.zeros(0, 4, 3, dtype=U8, device="cuda"), 0.1, 3)
    before = abi.last_kernel()
    for sc in (torch.zeros(0, 2, 4, device="cuda"), None):
        out = OP(x, torch.zeros(0, 4, device="cuda"), sc, 2, 0, True)
        assert out.shape == x.shape and out.is_quantized and abi.last_kernel() == before


def test_graph_capture_and_replay():
    rs = np.random.RandomState(177)
    x = _to_cuda(_quantized(rs, (8, 16, 6, 6), U8))
    offsets = torch.linspace(-2.3, 2.3, 32, device="cuda").view(2, 16)
    scales = torch.linspace(0, 2, 2 * 4 * 16, device="cuda").view(2, 4, 16)
    for sc in (scales, None):
        want = OP(x, offsets, sc, 4, 0, True)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            OP(x, offsets, sc, 4, 0, True)   # (warm-up on the capture stream)
            stream.synchronize()
            with torch.cuda.graph(graph, stream=stream):   # (a host synchronisation would fail the capture)
                out = OP(x, offsets, sc, 4, 0, True)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.int_repr(), want.int_repr())


def test_the_size_limit_is_refused_before_anything_is_allocated():
    free, _ = torch.cuda.mem_get_info()
    if free < 4 * 2 ** 30:
        pytest.skip("needs 4 GiB of free device memory")
    x = torch._empty_affine_quantized([2 ** 15, 2 ** 8, 2 ** 8], scale=0.1, zero_point=3, dtype=torch.quint8, device="cuda")
    offsets, scales = torch.zeros(2 ** 14, 2 ** 8, device="cuda"), torch.ones(2 ** 14, 2, 2 ** 8, device="cuda")
    before = torch.cuda.memory_allocated()
    for sc in (scales, None):
        with pytest.raises(RuntimeError, match=r"temporal_interlace_quantized: a tensor of 2147483648 elements is beyond the kernel's "
                                               r"limit of 2\^31 - 16 units"):
            OP(x, offsets, sc, 2, 0, True)
        assert torch.cuda.memory_allocated() == before
