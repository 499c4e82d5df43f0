"""Channels-last temporal shift on CPU tensors: memory_format=torch.preserve_format in temporal_shift_func, temporal_shift_quantized
and the two TemporalShift modules, the dispatcher ops temporal_shift_cl / _temporal_shift_cl_backward / temporal_shift_quantized_cl,
and the host-side validation of SHIFTND_SHIFT_DIM0 on channels-last strides at the C ABI.

The values are those of temporal_shift / temporal_shift_quantized in every case (torch.equal: a pure gather); what the option adds is
the layout: a dense channels-last input comes back in the input's strides, x.grad in the gradient's, anything else as today."""
import ctypes

import pytest
import torch

import torchshifts
from torchshifts.functional import temporal_shift_func
from torchshifts.quantized.functional import temporal_shift_quantized

OPS = torch.ops.torchshifts
KEEP = torch.preserve_format


def channels_last_inputs(dtype=torch.float32, seed=0):
    """the three dense channels-last kinds: NHWC, [N*T, C, L] with unit channel stride, NDHWC"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(6, 5, 4, 6, generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
    b = torch.randn(6, 7, 5, generator=g).to(dtype).permute(0, 2, 1)                       # [6, 5, 7], strides (35, 1, 5)
    c = torch.randn(4, 5, 2, 3, 2, generator=g).to(dtype).contiguous(memory_format=torch.channels_last_3d)
    assert tuple(b.shape) == (6, 5, 7) and b.stride() == (35, 1, 5)
    return [a, b, c]


def tables(C, frames):
    """0, T + 1 and -T - 1 always; then every |s| up to T + 1"""
    base = [0, frames + 1, -frames - 1] + list(range(-frames - 1, frames + 2))
    return torch.tensor([base[i % len(base)] for i in range(C)], dtype=torch.int64)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16, torch.bfloat16], ids=lambda d: str(d).split(".")[-1])
def test_float_functional_and_ops_keep_the_layout(dtype):
    for x in channels_last_inputs(dtype):
        for frames in (1, 2):
            s = tables(x.shape[1], frames)
            for pad in range(5):
                what = (tuple(x.shape), frames, pad)
                want = OPS.temporal_shift(x, s, frames, pad)
                xa = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
                assert xa.stride() == x.stride()
                out = temporal_shift_func(xa, s, frames, pad, memory_format=KEEP)
                assert out.stride() == x.stride() and out.dtype == dtype and torch.equal(out, want), what
                assert torch.equal(OPS.temporal_shift_cl(x, s, frames, pad), want) and OPS.temporal_shift_cl(x, s, frames, pad).stride() == x.stride()
                # a channels-last gradient gives a channels-last x.grad, a contiguous one a contiguous x.grad
                go = torch.randn(x.shape).to(dtype)
                go_cl = torch.empty_like(x).copy_(go)
                assert go_cl.stride() == x.stride()
                want_gx = OPS._temporal_shift_backward(go, s, frames, pad)
                out.backward(go_cl)
                assert xa.grad.stride() == x.stride() and torch.equal(xa.grad, want_gx), what
                gx = OPS._temporal_shift_cl_backward(go_cl, s, frames, pad)
                assert gx.stride() == x.stride() and torch.equal(gx, want_gx), what
                gx = OPS._temporal_shift_cl_backward(go, s, frames, pad)
                assert gx.is_contiguous() and torch.equal(gx, want_gx), what
                # the default is today's call
                assert temporal_shift_func(x, s, frames, pad).is_contiguous()
                assert temporal_shift_func(x, s, frames, pad, memory_format=torch.contiguous_format).is_contiguous()


def test_other_inputs_give_what_the_op_gives_today():
    s = torch.tensor([1, -1, 0, 3, -3])
    contiguous = torch.randn(6, 5, 4, 3)
    strided = torch.randn(5, 6, 4, 3).permute(1, 0, 3, 2)   # [6, 5, 3, 4]: no dense layout at all
    two_dims = torch.randn(6, 5)
    one_channel = torch.randn(6, 1, 4, 3).contiguous(memory_format=torch.channels_last)
    for x in (contiguous, strided, two_dims):
        for pad in range(5):
            want = OPS.temporal_shift(x, s, 3, pad)
            got = temporal_shift_func(x, s, 3, pad, memory_format=KEEP)
            assert torch.equal(got, want) and got.stride() == want.stride() and got.is_contiguous(), (tuple(x.shape), pad)
            go = torch.randn(x.shape)
            gx = OPS._temporal_shift_cl_backward(go, s, 3, pad)
            assert torch.equal(gx, OPS._temporal_shift_backward(go, s, 3, pad)) and gx.is_contiguous()
    got = temporal_shift_func(one_channel, torch.tensor([1]), 3, 0, memory_format=KEEP)
    assert torch.equal(got, OPS.temporal_shift(one_channel, torch.tensor([1]), 3, 0)) and got.is_contiguous()


QTYPES = [(torch.quint8, 77), (torch.qint8, -5), (torch.qint32, 70000)]


@pytest.mark.parametrize("qtype,zp", QTYPES, ids=["quint8", "qint8", "qint32"])
def test_quantized_functional_and_op_keep_the_layout(qtype, zp):
    for x in channels_last_inputs():
        # a quantized tensor in the input's strides: quantize the dense storage, then view it
        order = [0] + list(range(2, x.dim())) + [1]
        back = [0, x.dim() - 1] + list(range(1, x.dim() - 1))
        xq = torch.quantize_per_tensor(x.permute(order).contiguous(), 0.05, zp, qtype).permute(back)
        assert xq.stride() == x.stride() and tuple(xq.shape) == tuple(x.shape)
        for frames in (1, 2):
            s = tables(x.shape[1], frames)
            for pad in range(5):
                what = (tuple(x.shape), frames, pad)
                want = OPS.temporal_shift_quantized(xq, s, frames, pad)
                for got in (temporal_shift_quantized(xq, s, frames, pad, memory_format=KEEP), OPS.temporal_shift_quantized_cl(xq, s, frames, pad)):
                    assert got.stride() == xq.stride() and got.dtype == qtype, what
                    assert got.q_scale() == xq.q_scale() and got.q_zero_point() == zp, what
                    assert torch.equal(got.int_repr(), want.int_repr()), what
                if pad == 0 and frames == 2:   # the filled channels hold the zero point
                    filled = (s.abs() > frames)
                    assert bool((want.int_repr()[:, filled] == zp).all())
                assert temporal_shift_quantized(xq, s, frames, pad).is_contiguous()
        plain = torch.quantize_per_tensor(x.contiguous(), 0.05, zp, qtype)
        got = temporal_shift_quantized(plain, s, 2, 0, memory_format=KEEP)
        assert got.is_contiguous() and torch.equal(got.int_repr(), OPS.temporal_shift_quantized(plain, s, 2, 0).int_repr())


def test_a_bad_memory_format_raises():
    x = torch.randn(6, 5, 4, 6)
    s = torch.zeros(5, dtype=torch.int64)
    xq = torch.quantize_per_tensor(x, 0.1, 3, torch.quint8)
    for bad in (torch.channels_last, torch.channels_last_3d, None, "preserve"):
        with pytest.raises(AssertionError):
            temporal_shift_func(x, s, 2, 0, memory_format=bad)
        with pytest.raises(AssertionError):
            temporal_shift_quantized(xq, s, 2, 0, memory_format=bad)
        with pytest.raises(AssertionError):
            torchshifts.TemporalShift(2, 5, memory_format=bad)
    # the ops keep the plain ops' argument checks
    with pytest.raises(RuntimeError, match="must be a multiple of n_segment"):
        OPS.temporal_shift_cl(x, s, 4, 0)
    with pytest.raises(RuntimeError, match="padding_mode must be 0..4"):
        OPS._temporal_shift_cl_backward(x, s, 2, 7)
    with pytest.raises(RuntimeError, match="quantized"):
        OPS.temporal_shift_cl(xq, s, 2, 0)
    with pytest.raises(RuntimeError):
        OPS.temporal_shift_quantized_cl(xq, torch.zeros(4, dtype=torch.int64), 2, 0)


def test_a_second_backward_raises_and_the_node_saves_the_table_alone():
    x = torch.randn(4, 3, 5, 2).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    seen = []

    def pack(t):
        seen.append(t.numel())
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = temporal_shift_func(x, torch.tensor([1, 0, -1]), 2, memory_format=KEEP)
    assert seen == [3], seen
    g, = torch.autograd.grad(out, x, torch.ones_like(out, requires_grad=True), create_graph=True)
    with pytest.raises(RuntimeError, match="double backwards"):
        g.sum().backward()


def test_the_modules_carry_the_option():
    plain = torchshifts.TemporalShift(2, 8, padding="border")
    keep = torchshifts.TemporalShift(2, 8, padding="border", memory_format=KEEP)
    assert plain.memory_format == torch.contiguous_format and keep.memory_format == KEEP
    assert list(keep.state_dict().keys()) == ["shifts"] and list(plain.state_dict().keys()) == ["shifts"]
    assert torch.equal(keep.state_dict()["shifts"], plain.state_dict()["shifts"])
    keep.load_state_dict(plain.state_dict())
    assert "memory_format=torch.preserve_format" in repr(keep) and "memory_format=torch.contiguous_format" in repr(plain)
    x = torch.randn(6, 8, 3, 4).contiguous(memory_format=torch.channels_last)
    out, ref = keep(x), plain(x)
    assert out.stride() == x.stride() and ref.is_contiguous() and torch.equal(out, ref)
    # from_shift keeps the default, the quantized from_float carries the float module's value
    learnable = torchshifts.LearnableTemporalShift(2, 8)
    assert torchshifts.TemporalShift.from_shift(learnable).memory_format == torch.contiguous_format
    QT = torchshifts.quantized.TemporalShift
    assert QT.from_float(keep).memory_format == KEEP and QT.from_float(plain).memory_format == torch.contiguous_format
    assert QT(2, 8, memory_format=KEEP).memory_format == KEEP and QT(2, 8).memory_format == torch.contiguous_format
    # convert still swaps the module, and the swapped one keeps the layout
    net = torch.nn.Sequential(torch.ao.quantization.QuantStub(), torchshifts.TemporalShift(2, 8, memory_format=KEEP))
    net.eval()
    net.qconfig = torch.ao.quantization.default_qconfig
    torch.ao.quantization.prepare(net, inplace=True)
    net(x)
    q = torch.ao.quantization.convert(net, mapping=torchshifts.quant_mapping)
    assert isinstance(q[1], QT) and q[1].memory_format == KEEP
    xq = q[0](x)
    assert xq.stride() == x.stride()
    outq = q[1](xq)
    assert outq.stride() == x.stride() and torch.equal(outq.int_repr(), OPS.temporal_shift_quantized(xq, q[1].shifts, 2, 0).int_repr())


# ---- SHIFTND_SHIFT_DIM0 on channels-last strides at the C ABI, host side only: validation happens before any device work.  With NULL
# tensors an accepted geometry ends in INVALID_ARGUMENT (the tensors are refused); a refused dtype in UNSUPPORTED_DTYPE before that.
def _problem(ndim, dtype, sizes=(2, 5, 3, 8, 1), borders=(0, 3, 0, 8, 0, 1), active=0):
    from torchshifts import abi
    p = abi.Problem()
    p.ndim, p.dtype, p.padding_mode, p.active = ndim, dtype, 0, active
    for i, v in enumerate(sizes):
        p.sizes[i] = v
    for i, v in enumerate(borders):
        p.borders[i] = v
    return p


def test_the_flag_on_channels_last_strides_host_side():
    from torchshifts import abi
    INVALID, UNSUPPORTED = -1, -2
    L = abi.lib()
    assert L.shiftnd_abi_version() == 5
    st = (ctypes.c_int64 * 5)(3 * 8 * 5, 1, 8 * 5, 5, 0)   # [N, C, T, M] = [2, 5, 3, 8] in memory order N, T, M, C
    byref = ctypes.byref

    def quantized(p, wkind=abi.I32):
        return L.shiftnd_forward_quantized(byref(p), None, st, None, wkind, 0, 0, None, st, None)

    for dt in (abi.U8, abi.I8, abi.I32):
        # the dtype is accepted under the flag (UNSUPPORTED_DTYPE before this feature); the NULL tensors are refused
        assert quantized(_problem(2, dt | abi.SHIFT_DIM0)) == INVALID
        assert quantized(_problem(2, dt | abi.SHIFT_DIM0 | abi.WEIGHTS_F32)) == UNSUPPORTED
        assert quantized(_problem(2, dt | abi.SHIFT_DIM0), wkind=abi.F32) == UNSUPPORTED
        assert quantized(_problem(2, dt | abi.SHIFT_DIM0, borders=(1, 3, 0, 8, 0, 1))) == INVALID                            # a cut window
        assert quantized(_problem(1, dt | abi.SHIFT_DIM0, sizes=(2, 5, 24, 1, 1), borders=(0, 24, 0, 1, 0, 1))) == INVALID   # ndim 1
        assert quantized(_problem(3, dt | abi.SHIFT_DIM0, sizes=(2, 5, 3, 4, 2), borders=(0, 3, 0, 4, 0, 2))) == INVALID     # (accepted; NULL tensors)
    assert quantized(_problem(2, abi.F32 | abi.SHIFT_DIM0)) == UNSUPPORTED
    assert quantized(_problem(2, abi.U8)) == INVALID   # without the flag: as before (NULL tensors)
    # beyond the stated bounds: N * S0 of 2^31
    assert quantized(_problem(2, abi.U8 | abi.SHIFT_DIM0, sizes=(1 << 20, 5, 1 << 11, 8, 1), borders=(0, 1 << 11, 0, 8, 0, 1))) == INVALID
    for dt in (abi.F32, abi.F64, abi.F16, abi.BF16, abi.F16 | abi.WEIGHTS_F32):
        for active in (0, 1):
            assert L.shiftnd_forward(byref(_problem(2, dt | abi.SHIFT_DIM0, active=active)), None, st, None, None, st, None) == INVALID
    for dt in (abi.U8, abi.F32 | abi.WEIGHTS_F32):
        assert L.shiftnd_forward(byref(_problem(2, dt | abi.SHIFT_DIM0)), None, st, None, None, st, None) == UNSUPPORTED
