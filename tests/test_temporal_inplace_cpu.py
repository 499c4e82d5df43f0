"""In-place temporal shift on CPU tensors: temporal_shift_func_, temporal_shift_quantized_, TemporalShift(inplace=True) and its
quantized counterpart against the oracle's 2-D sparse forward of the [N, C, T, M] view under (s, 0) (inplace_cases.reference, from a
clone taken before the call), bit for bit; the autograd contract; the pinned surface of the torchshifts_inplace:: namespace; the
module surface; and the C ABI's host-side refusals of out == x under SHIFTND_SHIFT_DIM0, which need no device."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import torchshifts
from torchshifts import abi
from torchshifts.functional import temporal_shift_func, temporal_shift_func_
from torchshifts.modules import LearnableTemporalShift, TemporalShift
from torchshifts.quantized import TemporalShift as QTemporalShift
from torchshifts.quantized.functional import temporal_shift_quantized_

import inplace_cases as IC
from inplace_cases import F16, BF16, F32, F64, PADS

IOPS = torch.ops.torchshifts_inplace
FRAMES = (1, 2, 3, 8, 17)
QTYPES = {torch.quint8: (IC.U8, 77), torch.qint8: (IC.I8, -5), torch.qint32: (IC.I32, 70000)}


def _quantized(int_repr, zp):
    return torch._make_per_tensor_quantized_tensor(int_repr, 0.05, zp)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("T", FRAMES)
def test_function_against_the_reference(T, pad):
    rs = np.random.RandomState(100 * T + pad)
    for shape, dt, tdt in (((2 * T, 5, 3, 2), F32, torch.int64), ((T, 4, 3), F64, torch.int32), ((2 * T, 6), F16, torch.float32),
                           ((T, 3, 2, 2, 2), BF16, torch.int64)):
        x = IC.data(rs, shape, dt)
        s = IC.random_table(rs, shape[1], T, tdt)
        want = IC.reference(x.clone(), s, T, pad)
        version = x._version
        got = temporal_shift_func_(x, s, T, pad)
        assert got is x and x._version > version, (shape, dt)
        assert IC.same_bits(x, want), (shape, dt, s)


@pytest.mark.parametrize("pad", PADS)
def test_float_tables_round_half_to_even(pad):
    rs = np.random.RandomState(7 + pad)
    T = 8
    s = torch.tensor([0.5, 1.5, -2.5, 2.5, -0.5, 3.49, -17.0, 0.0])
    for dt in (F32, F16):
        x = IC.data(rs, (2 * T, 8, 3), dt)
        want = IC.reference(x.clone(), s, T, pad)
        assert IC.same_bits(want, IC.reference(x.clone(), torch.tensor([0, 2, -2, 2, 0, 3, -17, 0]), T, pad))
        assert IC.same_bits(temporal_shift_func_(x, s.to(torch.float64), T, pad), want), dt


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("T", FRAMES)
def test_quantized_function_against_the_reference(T, pad):
    rs = np.random.RandomState(200 * T + pad)
    for qdt, (dt, zp) in QTYPES.items():
        x = _quantized(IC.data(rs, (2 * T, 5, 3, 2), dt), zp)
        s = IC.random_table(rs, 5, T, torch.int32 if qdt == torch.qint8 else torch.int64)
        want = IC.reference(x.int_repr(), s, T, pad, zp)
        version = x._version
        got = temporal_shift_quantized_(x, s, T, pad)
        assert got is x and x._version > version, qdt
        assert x.q_scale() == 0.05 and x.q_zero_point() == zp and x.dtype == qdt
        assert IC.same_bits(x.int_repr(), want), (qdt, s)


@pytest.mark.parametrize("pad", PADS)
def test_modules_against_the_reference(pad):
    rs = np.random.RandomState(300 + pad)
    name = {0: "zeros", 1: "border", 2: "periodic", 3: "reflect", 4: "symmetric"}[pad]
    for T in FRAMES:
        s = IC.random_table(rs, 16, T)
        for table in (None, s):   # the published table, a table of its own
            m = TemporalShift(T, 16, shifts=table, padding=name, inplace=True)
            x = IC.data(rs, (2 * T, 16, 3), F32)
            want = IC.reference(x.clone(), m.shifts, T, pad)
            assert m(x) is x and IC.same_bits(x, want), (T, table)
            q = QTemporalShift.from_float(m)
            assert q.inplace
            xq = _quantized(IC.data(rs, (2 * T, 16, 3), IC.U8), 77)
            want = IC.reference(xq.int_repr(), m.shifts, T, pad, 77)
            assert q(xq) is xq and IC.same_bits(xq.int_repr(), want), (T, table)


def test_channels_last_input_keeps_its_layout():
    rs = np.random.RandomState(5)
    s = IC.random_table(rs, 6, 4)
    x = IC.data(rs, (8, 6, 3, 3), F32).contiguous(memory_format=torch.channels_last)
    want, strides = IC.reference(x.clone(), s, 4, 0), x.stride()
    assert temporal_shift_func_(x, s, 4, 0) is x and x.stride() == strides and IC.same_bits(x, want)


def test_a_slice_is_updated_through_its_base():
    rs = np.random.RandomState(6)
    s = IC.random_table(rs, 4, 3)
    base = IC.data(rs, (6, 9, 5), F32)
    before = base.clone()
    piece = base[:, 2:6, 1:4]
    want = IC.reference(piece.clone(), s, 3, 2)
    assert temporal_shift_func_(piece, s, 3, 2) is piece
    assert IC.same_bits(base[:, 2:6, 1:4], want)
    outside = torch.ones_like(base, dtype=torch.bool)
    outside[:, 2:6, 1:4] = False
    assert torch.equal(base[outside], before[outside])
    qbase = _quantized(IC.data(rs, (6, 9, 5), IC.U8), 9)
    qpiece = qbase[:, 2:6]
    want = IC.reference(qpiece.int_repr(), s, 3, 0, 9)
    temporal_shift_quantized_(qpiece, s, 3, 0)
    assert IC.same_bits(qbase.int_repr()[:, 2:6], want)


# ---- autograd -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [torch.contiguous_format, torch.channels_last])
def test_gradient_equals_the_out_of_place_gradient(fmt):
    rs = np.random.RandomState(11)
    s = IC.random_table(rs, 6, 4)
    for pad in PADS:
        a = IC.data(rs, (8, 6, 3, 3), F64).contiguous(memory_format=fmt).requires_grad_()
        b = a.detach().clone(memory_format=torch.preserve_format).requires_grad_()
        g = IC.data(rs, (8, 6, 3, 3), F64).contiguous(memory_format=fmt)
        out = temporal_shift_func_(a * 1, s, 4, pad)
        out.backward(g)
        keep = torch.preserve_format if fmt == torch.channels_last else torch.contiguous_format
        temporal_shift_func(b * 1, s, 4, pad, keep).backward(g)
        assert IC.same_bits(a.grad, b.grad) and a.grad.stride() == b.grad.stride(), pad
        assert IC.same_bits(out, temporal_shift_func(b.detach(), s, 4, pad))


def test_a_leaf_that_requires_grad_raises():
    x = torch.randn(4, 3, 5, requires_grad=True)
    with pytest.raises(RuntimeError, match="leaf Variable that requires grad"):
        temporal_shift_func_(x, torch.tensor([1, 0, -1]), 2)


def test_the_node_saves_the_table_alone():
    shapes = []

    def pack(t):
        shapes.append(tuple(t.shape))
        return t

    x = torch.randn(8, 6, 3, 3, requires_grad=True)
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        y = x * 1
        del shapes[:]   # (what the multiplication saved)
        temporal_shift_func_(y, torch.tensor([1, 0, -1, 2, 0, 0]), 4)
    assert shapes == [(6,)], shapes


def test_double_backward_raises_under_the_ops_name():
    x = torch.randn(4, 3, 5, requires_grad=True)
    out = temporal_shift_func_(x * 1, torch.tensor([1, 0, -1]), 2)
    g, = torch.autograd.grad(out, x, torch.ones_like(out, requires_grad=True), create_graph=True)
    with pytest.raises(RuntimeError, match="double backwards on temporal_shift_ not supported"):
        g.sum().backward()


# ---- the dispatcher surface of torchshifts_inplace::, pinned like torchshifts:: in test_binding_surface.py -------------------------
SCHEMAS = {
    "temporal_shift_": "torchshifts_inplace::temporal_shift_(Tensor(a!) input, Tensor shifts, int n_segment, int padding_mode) -> Tensor(a!)",
    "temporal_shift_quantized_":
        "torchshifts_inplace::temporal_shift_quantized_(Tensor(a!) input, Tensor shifts, int n_segment, int padding_mode) -> Tensor(a!)",
}
KEYS = {"temporal_shift_": {"Autograd", "CPU", "CUDA"}, "temporal_shift_quantized_": {"QuantizedCPU", "QuantizedCUDA"}}
ALL_KEYS = ["CPU", "CUDA", "QuantizedCPU", "QuantizedCUDA", "Autograd", "AutogradCPU", "AutogradCUDA", "CompositeImplicitAutograd",
            "CompositeExplicitAutograd", "Meta", "ADInplaceOrView", "SparseCPU", "SparseCUDA"]


def test_the_op_set_schemas_and_keys_are_pinned():
    names = {n.split("::")[1] for n in torch._C._dispatch_get_all_op_names() if n.startswith("torchshifts_inplace::")}
    assert names == set(SCHEMAS)
    for name, schema in SCHEMAS.items():
        assert str(torch._C._get_schema("torchshifts_inplace::" + name, "")) == schema
        keys = {k for k in ALL_KEYS if torch._C._dispatch_has_kernel_for_dispatch_key("torchshifts_inplace::" + name, k)}
        assert keys == KEYS[name], (name, keys)


# ---- module surface --------------------------------------------------------------------------------------------------------------
def test_module_surface():
    m = TemporalShift(8, 16)
    assert m.inplace is False and "inplace" not in m.extra_repr()
    assert m.extra_repr() == ("n_segment=8, in_channels=16, fold_div=8, padding_method=zeros, "
                              "memory_format=torch.contiguous_format, fixed integer shifts")
    mi = TemporalShift(8, 16, inplace=True)
    assert mi.extra_repr() == m.extra_repr() + ", inplace=True"
    assert list(mi.state_dict()) == ["shifts"] and list(QTemporalShift(8, 16, inplace=True).state_dict()) == ["shifts"]
    m.load_state_dict(mi.state_dict())
    assert m.inplace is False
    assert QTemporalShift.from_float(mi).inplace is True and QTemporalShift.from_float(m).inplace is False
    assert TemporalShift.from_shift(LearnableTemporalShift(8, 16)).inplace is False
    # the keyword comes last: the positional order of before still means what it meant
    assert TemporalShift(8, 16, 4, None, "border", torch.preserve_format).inplace is False
    x = torch.randn(8, 16, 2)
    assert m(x) is not x and mi(x) is x


# ---- argument refusals name the new ops ---------------------------------------------------------------------------------------------
def test_refusals_name_the_op():
    x, s = torch.randn(6, 4, 3), torch.zeros(4, dtype=torch.int64)
    for args, text in (((x, s, 4, 0), "multiple of n_segment"), ((x, s[:3], 3, 0), r"shifts must have shape \[C\]"),
                       ((x, s, 3, 5), "padding_mode must be 0..4"), ((x, s > 0, 3, 0), "integers or floats"),
                       ((torch.randn(6), s, 3, 0), "2 to 5 dims")):
        with pytest.raises(RuntimeError, match="temporal_shift_: .*" + text):
            IOPS.temporal_shift_(*args)
    q = _quantized(torch.zeros(6, 4, 3, dtype=torch.uint8), 3)
    with pytest.raises(RuntimeError, match="temporal_shift_: quantized inputs are not supported"):
        IOPS.temporal_shift_(q, s, 3, 0)
    with pytest.raises((RuntimeError, NotImplementedError)):
        IOPS.temporal_shift_quantized_(x, s, 3, 0)
    with pytest.raises(RuntimeError, match="temporal_shift_quantized_: .*multiple of n_segment"):
        IOPS.temporal_shift_quantized_(q, s, 4, 0)
    with pytest.raises(ValueError, match="temporal_shift_quantized_"):
        temporal_shift_quantized_(x, s, 3, 0)
    with pytest.raises(AssertionError, match=r"temporal_shift_func_\(\)"):
        temporal_shift_func_(x, s, 4, 0)


# ---- C ABI: out == x under SHIFTND_SHIFT_DIM0 is validated on the host, before any device work ----------------------------------
def _inplace_rc(T, dtype=abi.DTYPES[F32], active=0, borders=None, strides=None, quantized=False, extra=0):
    N, C, M = 2, 4, 6
    p = abi.Problem()
    p.ndim, p.dtype, p.padding_mode, p.active = 2, dtype | abi.SHIFT_DIM0 | extra, 0, active
    for i, v in enumerate((N, C, T, M, 1)):
        p.sizes[i] = v
    for i, v in enumerate(borders or (0, T, 0, M, 0, 1)):
        p.borders[i] = v
    st = (ctypes.c_int64 * 5)(*(strides or (T * C * M, M, C * M, 1, 0)))
    same = ctypes.c_void_p(0x10000)   # never dereferenced: every one of these calls is refused first
    L = abi.lib()
    if quantized:
        return L.shiftnd_forward_quantized(ctypes.byref(p), same, st, same, abi.DTYPES[IC.I32], 0, 0, same, st, None)
    return L.shiftnd_forward(ctypes.byref(p), same, st, same, same, st, None)


def test_host_refusals_of_the_in_place_call():
    assert _inplace_rc(17) == -1 and _inplace_rc(17, abi.DTYPES[IC.U8], quantized=True) == -1   # more frames than slots
    assert _inplace_rc(8, active=1) == -1 and _inplace_rc(8, abi.DTYPES[IC.U8], active=1, quantized=True) == -1
    assert _inplace_rc(8, borders=(1, 8, 0, 6, 0, 1)) == -1 and _inplace_rc(8, borders=(0, 8, 0, 5, 0, 1)) == -1   # a cut window
    assert _inplace_rc(8, extra=abi.FRAMES) == -1
    assert _inplace_rc(8, strides=(8 * 4 * 6 * 2, 6, 4 * 6, 1, 0)) == -1   # neither dense layout
    assert _inplace_rc(8, strides=(8 * 4 * 6, 6, 4 * 6, 2, 0)) == -1
    assert _inplace_rc(8, abi.DTYPES[IC.U8]) == -2 and _inplace_rc(8, quantized=True) == -2   # the entry points keep their dtypes
