"""Quantized temporal interlacing and the quantized per-clip temporal shift on the CPU (QuantizedCPU key):
torch.ops.torchshifts_quantized_interlace.temporal_interlace_quantized, the two functional wrappers,
torchshifts.quantized.LearnablePerClipTemporalShift / TemporalInterlace and torchshifts.quant_mapping_interlacing.

The op is defined in the integer domain: with q = int_repr, zp the zero point and F = fp32 (quint8, qint8) / fp64 (qint32)

    out = clamp(zp + rint(temporal_interlace_func((q - zp).to(F), offsets.to(F), scales.to(F), T, padding_mode, active_flag)))

(scales None: temporal_shift_learnable_per_clip_func), so the reference of this file is that expression on the existing float CPU
ops, and int_repr is compared bit for bit.  Against the composite quantize_per_tensor(float op(dequantize)) the op is bit-identical
under a power-of-two scale with dyadic offsets and scales (every product is exact in both) and within one level otherwise.
"""
import copy
import ctypes
import inspect

import numpy as np
import pytest
import torch
from torch import nn

import torchshifts
from torchshifts import abi
from torchshifts import (LearnablePerClipTemporalShift, LearnableTemporalShift, PerClipTemporalShift, TemporalInterlace, quant_mapping,
                         quant_mapping_interlacing, quant_mapping_interpolating)
from torchshifts.functional import temporal_interlace_func, temporal_shift_learnable_per_clip_func
from torchshifts.quantized.functional import (temporal_interlace_quantized, temporal_shift_learnable_per_clip_quantized,
                                              temporal_shift_learnable_quantized)

from test_qtshift_cpu import QDT, SHAPES, ladder, quantized

NS = "torchshifts_quantized_interlace"
OP = torch.ops.torchshifts_quantized_interlace.temporal_interlace_quantized
QPC = torchshifts.quantized.LearnablePerClipTemporalShift
QTIN = torchshifts.quantized.TemporalInterlace

# both clamps (2, -1), ties in both directions (0.5 on an odd q - zp), the copy path (1 beside offset 0), one ulp above 1 and two below 2
SCALE_LADDER = np.array([1.0, 0.0, 2.0, 0.5, 1.5, -1.0, 0.3, 1 + 2.0 ** -23, 2 - 2.0 ** -22], np.float32)


def offset_tables(N, C, T):
    """the shift ladder cut into [N, C] tables (the last one wraps around): the rows of two clips differ"""
    w = ladder(T)
    return [torch.from_numpy(np.take(w, np.arange(i, i + N * C), mode="wrap").reshape(N, C)) for i in range(0, len(w), N * C)]


def scale_table(N, T, C, k=0):
    """the scale ladder over (n, t, c): entry (t + 3 c + 5 n + k) mod 9, so the T <= 9 frames of a channel all differ"""
    n, t, c = np.meshgrid(np.arange(N), np.arange(T), np.arange(C), indexing="ij")
    return torch.from_numpy(SCALE_LADDER[(t + 3 * c + 5 * n + k) % len(SCALE_LADDER)])


def definition(x, offsets, scales, T, pad, active=True):
    """the issue's definition, on the float ops: -> int_repr"""
    F = torch.float64 if x.dtype == torch.qint32 else torch.float32
    zp = x.q_zero_point()
    lo, hi = QDT[x.dtype][3]
    z = (x.int_repr().to(torch.int64) - zp).to(F)
    if scales is None:
        r = temporal_shift_learnable_per_clip_func(z, offsets.to(F), T, pad, active)
    else:
        r = temporal_interlace_func(z, offsets.to(F), scales.to(F), T, pad, active)
    return (torch.round(r) + zp).clamp(lo, hi).to(x.int_repr().dtype)


def composite(x, offsets, scales, T, pad):
    return torch.quantize_per_tensor(temporal_interlace_func(x.dequantize(), offsets, scales, T, pad, True), x.q_scale(), x.q_zero_point(),
                                     x.dtype)


@pytest.mark.parametrize("active", [True, False], ids=["active", "sparse"])
@pytest.mark.parametrize("qdt", list(QDT), ids=lambda d: str(d).split(".")[-1])
def test_the_op_is_the_definition(qdt, active):
    rs = np.random.RandomState(161)
    for shape, T in SHAPES:
        N, C = shape[0] // T, shape[1]
        for pad in range(5):
            x = quantized(rs, shape, qdt)
            for i, offsets in enumerate(offset_tables(N, C, T)):
                assert N == 1 or not torch.equal(offsets[0], offsets[1])
                scales = scale_table(N, T, C, 4 * i)
                assert all(len(set(scales[n, :, c].tolist())) == T for n in range(N) for c in range(C))
                what = (shape, pad, offsets.tolist(), i)
                assert torch.equal(OP(x, offsets, scales, T, pad, active).int_repr(), definition(x, offsets, scales, T, pad, active)), what
                assert torch.equal(OP(x, offsets, None, T, pad, active).int_repr(), definition(x, offsets, None, T, pad, active)), what


def test_the_ladders_reach_both_clamps_ties_and_the_copy_path():
    """on full-range quint8 data the scale ladder saturates at both ends, resolves exact ties to even in both directions, and meets
    offset 0 under scale 1"""
    rs = np.random.RandomState(162)
    T, C, N = 5, 3, 2
    x = quantized(rs, (N * T, C, 64), torch.quint8)
    z = (x.int_repr().to(torch.int64) - 3).float()
    offsets, scales = torch.zeros(N, C), scale_table(N, T, C)
    assert offset_tables(N, C, T)[0][0, 0] == 0 and scales[0, 0, 0] == 1   # the first table's first plane: a copy
    r = z.view(N, T, C, 64) * scales.view(N, T, C, 1)
    got = OP(x, offsets, scales, T, 0, True).int_repr().view(N, T, C, 64).to(torch.int64)
    assert bool(((r + 3 > 255.5) & (got == 255)).any()) and bool(((r + 3 < -0.5) & (got == 0)).any())
    half = (scales.view(N, T, C, 1) == 0.5) & (z.view(N, T, C, 64) % 2 == 1)
    assert bool(half.any())
    ties = got[half] - 3
    assert bool((ties % 2 == 0).all()) and bool((ties > r[half]).any()) and bool((ties < r[half]).any())
    assert torch.equal(got[0, 0, 0], x.int_repr().view(N, T, C, 64)[0, 0, 0].to(torch.int64))


@pytest.mark.parametrize("qdt", list(QDT), ids=lambda d: str(d).split(".")[-1])
def test_no_scales_is_scales_of_ones(qdt):
    rs = np.random.RandomState(163)
    for shape, T in SHAPES:
        N, C = shape[0] // T, shape[1]
        for pad in range(5):
            x = quantized(rs, shape, qdt)
            for offsets in offset_tables(N, C, T):
                for active in (True, False):
                    a = OP(x, offsets, None, T, pad, active)
                    assert torch.equal(a.int_repr(), OP(x, offsets, torch.ones(N, T, C), T, pad, active).int_repr())
                    assert torch.equal(a.int_repr(), temporal_shift_learnable_per_clip_quantized(x, offsets, T, pad, active).int_repr())


@pytest.mark.parametrize("qdt", list(QDT), ids=lambda d: str(d).split(".")[-1])
def test_one_row_for_every_clip_is_the_per_channel_op(qdt):
    rs = np.random.RandomState(164)
    for shape, T in SHAPES:
        N, C = shape[0] // T, shape[1]
        for pad in range(5):
            x = quantized(rs, shape, qdt)
            for offsets in offset_tables(N, C, T):
                row = offsets[-1]
                for active in (True, False):
                    want = temporal_shift_learnable_quantized(x, row, T, pad, active).int_repr()
                    assert torch.equal(OP(x, row.repeat(N, 1), torch.ones(N, T, C), T, pad, active).int_repr(), want)
                    assert torch.equal(OP(x, row.repeat(N, 1), None, T, pad, active).int_repr(), want)


def test_a_group_table_is_its_expansion():
    rs = np.random.RandomState(165)
    T, N, C, G = 4, 2, 6, 3
    x = quantized(rs, (N * T, C, 3, 3), torch.quint8)
    og = torch.from_numpy(rs.uniform(-3, 3, size=(N, G)).astype(np.float32))
    sg = torch.from_numpy(rs.uniform(0, 2, size=(N, T, G)).astype(np.float32))
    oe, se = og.repeat_interleave(C // G, dim=1), sg.repeat_interleave(C // G, dim=2)
    for active in (True, False):
        want = OP(x, oe, se, T, 2, active).int_repr()
        assert torch.equal(temporal_interlace_quantized(x, og, sg, T, 2, active).int_repr(), want)
        assert torch.equal(temporal_interlace_quantized(x, oe, sg, T, 2, active).int_repr(), want)
        assert torch.equal(temporal_shift_learnable_per_clip_quantized(x, og, T, 2, active).int_repr(), OP(x, oe, None, T, 2, active).int_repr())
    with pytest.raises(RuntimeError, match=r"offsets must have shape \[N, C\] = \[2, 6\]"):   # 6 % 4 != 0: left to the op
        temporal_interlace_quantized(x, torch.zeros(N, 4), sg, T)


@pytest.mark.parametrize("qdt", [torch.quint8, torch.qint8], ids=lambda d: str(d).split(".")[-1])
def test_exact_case_equals_the_composite(qdt):
    rs = np.random.RandomState(166)
    for scale in (0.25, 0.5):
        for shape, T in SHAPES:
            N, C = shape[0] // T, shape[1]
            for pad in range(5):
                x = quantized(rs, shape, qdt, scale=scale)
                offsets = torch.from_numpy(rs.randint(-8 * (T + 2), 8 * (T + 2) + 1, size=(N, C)).astype(np.float32) / 8)
                scales = torch.from_numpy(rs.randint(-4, 9, size=(N, T, C)).astype(np.float32) / 4)
                assert torch.equal(OP(x, offsets, scales, T, pad, True).int_repr(), composite(x, offsets, scales, T, pad).int_repr()), \
                    (scale, shape, pad, offsets.tolist(), scales.tolist())


@pytest.mark.parametrize("qdt", [torch.quint8, torch.qint8], ids=lambda d: str(d).split(".")[-1])
def test_general_case_is_within_one_level_of_the_composite(qdt):
    """both round numbers that differ by a few ulps of at most 510 (255 levels times a scale below 2): only ties can move"""
    rs = np.random.RandomState(167)
    N, T, C = 4, 8, 16
    for pad in range(5):
        x = quantized(rs, (N * T, C, 5, 5), qdt, scale=0.05)
        offsets = torch.from_numpy(rs.uniform(-9.5, 9.5, size=(N, C)).astype(np.float32))
        scales = torch.from_numpy(rs.uniform(0, 2, size=(N, T, C)).astype(np.float32))
        got = OP(x, offsets, scales, T, pad, True).int_repr().to(torch.int32)
        want = composite(x, offsets, scales, T, pad).int_repr().to(torch.int32)
        assert int((got - want).abs().max()) <= 1, pad


@pytest.mark.parametrize("qdt", list(QDT), ids=lambda d: str(d).split(".")[-1])
def test_output_properties(qdt):
    rs = np.random.RandomState(168)
    x = quantized(rs, (6, 4, 3, 5), qdt, scale=0.125)
    offsets = torch.tensor([[0.25, -1.5, 3.75, 0.0], [1.0, 0.5, -0.25, 2.0]])
    scales = scale_table(2, 3, 4)
    for active in (True, False):
        for sc in (scales, None):
            out = temporal_interlace_quantized(x, offsets, sc, 3, 1, active)
            assert out.is_quantized and out.dtype == qdt and out.qscheme() == torch.per_tensor_affine
            assert out.q_scale() == 0.125 and out.q_zero_point() == x.q_zero_point() and out.shape == x.shape and out.is_contiguous()
            cl = x.contiguous(memory_format=torch.channels_last)
            assert not cl.is_contiguous()
            got = temporal_interlace_quantized(cl, offsets, sc, 3, 1, active)
            assert got.is_contiguous() and torch.equal(got.int_repr(), out.int_repr())
    assert torch.equal(temporal_interlace_quantized(x, offsets, scales, 3).int_repr(), OP(x, offsets, scales, 3, 0, True).int_repr())   # the defaults
    assert torch.equal(temporal_shift_learnable_per_clip_quantized(x, offsets, 3).int_repr(), OP(x, offsets, None, 3, 0, True).int_repr())
    empty = torch._make_per_tensor_quantized_tensor(torch.zeros(0, 4, 3, dtype=x.int_repr().dtype), 0.125, 3)
    out = OP(empty, torch.zeros(0, 4), torch.zeros(0, 3, 4), 3, 0, True)
    assert out.shape == empty.shape and out.dtype == qdt and out.q_zero_point() == 3


# ---- the dispatcher surface ----------------------------------------------------------------------------------------------------------
SCHEMA = ("torchshifts_quantized_interlace::temporal_interlace_quantized(Tensor input, Tensor offsets, Tensor? scales, int n_segment, "
          "int padding_mode, bool active_flag) -> Tensor")
ALL_KEYS = ["CPU", "CUDA", "QuantizedCPU", "QuantizedCUDA", "Autograd", "AutogradCPU", "AutogradCUDA", "CompositeImplicitAutograd",
            "CompositeExplicitAutograd", "Meta", "ADInplaceOrView", "SparseCPU", "SparseCUDA"]


def test_the_op_set_schema_and_keys_are_pinned():
    names = {n.split("::")[1] for n in torch._C._dispatch_get_all_op_names() if n.startswith(NS + "::")}
    assert names == {"temporal_interlace_quantized"}
    assert str(torch._C._get_schema(NS + "::temporal_interlace_quantized", "")) == SCHEMA
    keys = {k for k in ALL_KEYS if torch._C._dispatch_has_kernel_for_dispatch_key(NS + "::temporal_interlace_quantized", k)}
    assert keys == {"QuantizedCPU", "QuantizedCUDA"}


def test_refusals_and_their_messages():
    x = quantized(np.random.RandomState(169), (6, 4, 3), torch.quint8)
    o, s = torch.zeros(2, 4), torch.ones(2, 3, 4)
    OP(x, o, s, 3, 0, True)
    name = "temporal_interlace_quantized: "
    with pytest.raises(ValueError, match="Input to 'temporal_interlace_quantized' must be quantized!"):
        temporal_interlace_quantized(torch.zeros(6, 4, 3), o, s, 3)
    with pytest.raises(ValueError, match="Input to 'temporal_shift_learnable_per_clip_quantized' must be quantized!"):
        temporal_shift_learnable_per_clip_quantized(torch.zeros(6, 4, 3), o, 3)
    with pytest.raises(RuntimeError):                       # a float input has no kernel on this op
        OP(torch.zeros(6, 4, 3), o, s, 3, 0, True)
    per_channel = torch.quantize_per_channel(torch.zeros(6, 4, 3), torch.ones(4), torch.zeros(4, dtype=torch.long), 1, torch.quint8)
    with pytest.raises(RuntimeError, match=name + "expected a per-tensor quantized input"):
        OP(per_channel, o, s, 3, 0, True)
    for bad in (quantized(np.random.RandomState(1), (6,), torch.quint8), quantized(np.random.RandomState(1), (6, 4, 1, 1, 1, 1), torch.quint8)):
        with pytest.raises(RuntimeError, match=name + r"expected a \[N\*T, C, ...\] tensor of 2 to 5 dims"):
            OP(bad, o, s, 3, 0, True)
    for T in (4, 0):
        with pytest.raises(RuntimeError, match=name + r"dim 0 \(6\) must be a multiple of n_segment \(%d\)" % T):
            OP(x, o, s, T, 0, True)
    for bad in (torch.zeros(4), torch.zeros(1, 4), torch.zeros(2, 2), torch.zeros(2, 4, 1)):
        for sc in (s, None):
            with pytest.raises(RuntimeError, match=name + r"offsets must have shape \[N, C\] = \[2, 4\]"):
                OP(x, bad, sc, 3, 0, True)
    for bad in (torch.zeros(2, 4, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.float16), torch.zeros(2, 4, dtype=torch.long),
                torch.quantize_per_tensor(torch.zeros(2, 4), 1.0, 0, torch.qint32)):
        with pytest.raises(RuntimeError, match=name + "offsets must be fp32"):
            OP(x, bad, s, 3, 0, True)
    for bad in (torch.ones(2, 4), torch.ones(2, 3, 2), torch.ones(1, 3, 4), torch.ones(2, 4, 3), torch.ones(6, 4)):
        with pytest.raises(RuntimeError, match=name + r"scales must have shape \[N, T, C\] = \[2, 3, 4\]"):
            OP(x, o, bad, 3, 0, True)
    for bad in (torch.ones(2, 3, 4, dtype=torch.float64), torch.ones(2, 3, 4, dtype=torch.bfloat16), torch.ones(2, 3, 4, dtype=torch.int32)):
        with pytest.raises(RuntimeError, match=name + "scales must be fp32"):
            OP(x, o, bad, 3, 0, True)
    for pad in (-1, 5):
        for sc in (s, None):
            with pytest.raises(RuntimeError, match=name + r"padding_mode must be 0\.\.4"):
                OP(x, o, sc, 3, pad, True)
    with pytest.raises(RuntimeError, match=name + r"scales must have shape"):   # the tables come before the padding mode
        OP(x, o, torch.ones(2, 4), 3, 7, True)
    for active in (True, False):
        with pytest.raises(RuntimeError, match=name + "offsets must not require grad"):
            OP(x, torch.zeros(2, 4, requires_grad=True), s, 3, 0, active)
        with pytest.raises(RuntimeError, match=name + "scales must not require grad"):
            OP(x, o, torch.ones(2, 3, 4, requires_grad=True), 3, 0, active)
    if torch.cuda.is_available():
        with pytest.raises(RuntimeError, match=name + "offsets must be on the input's device"):
            OP(x, o.cuda(), s, 3, 0, True)
        with pytest.raises(RuntimeError, match=name + "scales must be on the input's device"):
            OP(x, o, s.cuda(), 3, 0, True)


# ---- the modules -----------------------------------------------------------------------------------------------------------------------
PADS = ("zeros", "border", "periodic", "reflect", "symmetric")


def test_per_clip_from_float():
    rs = np.random.RandomState(170)
    T, N, C = 4, 2, 8
    x = quantized(rs, (N * T, C, 3, 3), torch.quint8)
    table = torch.from_numpy(rs.uniform(-T - 1, T + 1, size=(N, C)).astype(np.float32))
    table[0, :3] = torch.tensor([0.5, -1.5, 0.0])
    for k, pad in enumerate(PADS):
        for active in (True, False):
            q = QPC.from_float(LearnablePerClipTemporalShift(T, padding=pad, active_flag=active))
            assert type(q) is QPC and q.n_segment == T and q.padding == k and q._active_flag is active
            assert q._get_name() == "QuantizedLearnablePerClipTemporalShift" and not list(q.parameters()) and not q.state_dict()
            out = q(x, table.double().requires_grad_())   # (converted to fp32, detached)
            assert isinstance(out, torch.Tensor) and out.is_quantized
            assert torch.equal(out.int_repr(), temporal_shift_learnable_per_clip_quantized(x, table, T, k, active).int_repr())
            assert torch.equal(out.int_repr(), definition(x, table, None, T, k, active))
        q = QPC.from_float(PerClipTemporalShift(T, padding=pad))
        assert type(q) is QPC and q._active_flag is False and q.padding == k
        whole = torch.from_numpy(rs.randint(-T - 1, T + 2, size=(N, C)))
        assert torch.equal(q(x, whole).int_repr(), definition(x, whole.float(), None, T, k, False))
        assert torch.equal(q(x, whole[:, :2]).int_repr(), q(x, whole[:, :2].repeat_interleave(4, dim=1)).int_repr())   # a group table
    with pytest.raises(AssertionError, match="expected a LearnablePerClipTemporalShift or a PerClipTemporalShift"):
        QPC.from_float(LearnableTemporalShift(4, 8))


def trained(T, C, shift_div, pad, seed):
    torch.manual_seed(seed)
    m = TemporalInterlace(T, C, shift_div=shift_div, padding=pad).eval()
    with torch.no_grad():   # (away from the initial state, where every clip gets the same offsets)
        for p in m.parameters():
            p.add_(torch.randn_like(p) * 0.5)
    return m


def test_interlace_from_float_and_forward_is_the_functional_under_its_own_tables():
    rs = np.random.RandomState(171)
    T, N, C = 4, 3, 16
    for k, pad in enumerate(PADS):
        for shift_div, qdt in ((1, torch.quint8), (2, torch.qint8), (4, torch.qint32)):
            f = trained(T, C, shift_div, pad, 180 + k)
            q = QTIN.from_float(f)
            assert type(q) is QTIN and (q.n_segment, q.in_channels, q.shift_div, q.fold, q.padding) == (T, C, shift_div, C // shift_div, k)
            assert q._get_name() == "QuantizedTemporalInterlace" and "QuantizedTemporalInterlace" in repr(q)
            assert type(q.offset_net) is torchshifts.OffsetNet and type(q.weight_net) is torchshifts.WeightNet
            assert list(q.state_dict()) == list(f.state_dict())
            for (name, a), b in zip(q.state_dict().items(), f.state_dict().values()):
                assert a.dtype == torch.float32 and torch.equal(a, b) and a.data_ptr() != b.data_ptr(), name
            x = quantized(rs, (N * T, C, 3, 3), qdt, scale=0.05 if qdt != torch.qint32 else 1e-9)
            offsets, scales = q.tables(x)
            assert offsets.shape == (N, C) and scales.shape == (N, T, C) and offsets.dtype == scales.dtype == torch.float32
            assert not offsets.requires_grad and not scales.requires_grad
            fold = C // shift_div
            assert bool((offsets[:, fold:] == 0).all()) and bool((scales[:, :, fold:] == 1).all())
            assert torch.equal(offsets[:, :fold // 2], -offsets[:, fold // 2:fold]) and bool((offsets[:, :fold] != 0).all())
            out = q(x)
            assert isinstance(out, torch.Tensor) and out.is_quantized and out.q_scale() == x.q_scale()
            assert torch.equal(out.int_repr(), temporal_interlace_quantized(x, offsets, scales, T, k, True).int_repr())
            assert torch.equal(out.int_repr(), definition(x, offsets, scales, T, k, True))
    with pytest.raises(AssertionError, match="expected a TemporalInterlace"):
        QTIN.from_float(LearnablePerClipTemporalShift(4))


def test_tables_agree_with_the_float_module():
    """tables(x), formed from integer sums, against the float module's tables(x.dequantize()): both are fp32 evaluations of one
    quantity in different summation orders, so the new module is allowed four times the float module's own distance from its fp64
    evaluation on this data.  Measured here (offsets / scales): that distance is 1.6e-6 / 6.4e-7 on the quint8 data and 4.0e-7 /
    1.8e-7 on the qint8 data; the new module's distance from the float module is 3.6e-6 / 1.2e-6 and 7.2e-7 / 2.4e-7."""
    rs = np.random.RandomState(172)
    T, N, C = 8, 4, 16
    f = trained(T, C, 2, "zeros", 190)
    q = QTIN.from_float(f)
    for qdt in (torch.quint8, torch.qint8):
        x = quantized(rs, (N * T, C, 7, 7), qdt, scale=0.05)
        got = q.tables(x)
        with torch.no_grad():
            f32 = f.tables(x.dequantize())
            f64 = copy.deepcopy(f).double().tables(x.dequantize().double())
        for name, a, b, c in zip(("offsets", "scales"), got, f32, f64):
            assert b.dtype == torch.float32 and c.dtype == torch.float64
            own = float((b.double() - c).abs().max())
            dist = float((a - b).abs().max())
            print("%s %s: float module fp32 vs fp64 %.3g, quantized module vs float module %.3g" % (qdt, name, own, dist))
            assert own > 0 and dist <= 4 * own, (qdt, name, own, dist)


def test_state_dict_round_trip_from_a_float_checkpoint():
    rs = np.random.RandomState(173)
    T, C = 4, 8
    x = quantized(rs, (2 * T, C, 3, 3), torch.qint8)
    f = trained(T, C, 1, "reflect", 200)
    q = QTIN(T, C, padding="reflect")
    q.load_state_dict(f.state_dict(), strict=True)
    assert torch.equal(q(x).int_repr(), QTIN.from_float(f)(x).int_repr())
    fresh = QTIN(T, C, padding="reflect")
    assert not torch.equal(fresh(x).int_repr(), q(x).int_repr())
    fresh.load_state_dict(q.state_dict())
    assert torch.equal(fresh(x).int_repr(), q(x).int_repr())
    back = TemporalInterlace(T, C, padding="reflect")
    back.load_state_dict(q.state_dict(), strict=True)   # ... and back into a float module


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.quant = torch.ao.quantization.QuantStub()
        self.tin = trained(4, 8, 2, "border", 210)
        self.learned = LearnablePerClipTemporalShift(4, padding="reflect", active_flag=True)
        self.jitter = PerClipTemporalShift(4)
        self.dequant = torch.ao.quantization.DeQuantStub()
        self.register_buffer("table", torch.linspace(-2.25, 2.25, 16).view(2, 8))
        self.register_buffer("steps", torch.tensor([[0, 1, -1, 2, 0, -2, 1, 0], [1, 0, 0, -1, 2, 0, -3, 1]]))

    def forward(self, x):
        return self.dequant(self.jitter(self.learned(self.tin(self.quant(x)), self.table), self.steps))


def _prepared(keep_the_nets_float):
    net = nn.Sequential(Net()).eval()
    net.qconfig = torch.ao.quantization.default_qconfig
    if keep_the_nets_float:
        net[0].tin.offset_net.qconfig = net[0].tin.weight_net.qconfig = None
    torch.ao.quantization.prepare(net, inplace=True)
    x = torch.rand(8, 8, 5, 5)
    with torch.no_grad():
        net(x)   # calibrate
    return net, x


def test_convert_with_quant_mapping_interlacing():
    net, x = _prepared(True)
    f = copy.deepcopy(net[0])
    torch.ao.quantization.convert(net, inplace=True, mapping=quant_mapping_interlacing)
    m = net[0]
    assert type(m.tin) is QTIN and type(m.learned) is QPC and type(m.jitter) is QPC
    assert m.learned._active_flag is True and m.learned.padding == 3 and m.jitter._active_flag is False
    assert type(m.tin.offset_net.conv) is nn.Conv1d and type(m.tin.offset_net.fc1) is nn.Linear and type(m.tin.weight_net.conv) is nn.Conv1d
    out = net(x)
    # the converted net is the three ops on the stub's quantized tensor, under the float nets' tables
    xq = m.quant(x)
    assert xq.is_quantized
    offsets, scales = QTIN.from_float(f.tin).tables(xq)
    y = temporal_interlace_quantized(xq, offsets, scales, 4, 1, True)
    y = temporal_shift_learnable_per_clip_quantized(y, f.table, 4, 3, True)
    y = temporal_shift_learnable_per_clip_quantized(y, f.steps.float(), 4, 0, False)
    assert torch.equal(out, y.dequantize())


def test_convert_refuses_quantized_nets():
    net, _ = _prepared(False)
    with pytest.raises(ValueError, match="offset_net.qconfig = layer.weight_net.qconfig = None"):
        torch.ao.quantization.convert(net, inplace=True, mapping=quant_mapping_interlacing)


def test_the_mappings():
    new = {PerClipTemporalShift: QPC, LearnablePerClipTemporalShift: QPC, TemporalInterlace: QTIN}
    assert all(quant_mapping_interlacing[k] is v for k, v in new.items())
    assert {k: v for k, v in quant_mapping_interlacing.items() if k not in new} == quant_mapping_interpolating
    assert torchshifts.quantized.quant_mapping_interlacing is quant_mapping_interlacing
    # quant_mapping and quant_mapping_interpolating are what they were
    assert not any(k in quant_mapping or k in quant_mapping_interpolating for k in new)
    assert quant_mapping[LearnableTemporalShift] is torchshifts.quantized.TemporalShift
    assert quant_mapping_interpolating[LearnableTemporalShift] is torchshifts.quantized.LearnableTemporalShift
    assert {k: v for k, v in quant_mapping_interpolating.items() if k is not LearnableTemporalShift} == \
        {k: v for k, v in quant_mapping.items() if k is not LearnableTemporalShift}


# ---- the C ABI, host side: what is accepted, what is refused before anything is launched ----------------------------------------------
OK, INVALID, UNSUPPORTED = 0, -1, -2
DIM0, PC, IL = abi.SHIFT_DIM0, abi.PER_CLIP, abi.INTERLACE


def _problem(ndim, dtype, ncTM=(2, 5, 3, 8), window=None, active=1, pad=0, channels_last=False):
    n, c, t, m = ncTM
    inner = (m,) if ndim == 2 else (2, m // 2)
    p = abi.Problem()
    p.ndim, p.dtype, p.padding_mode, p.active = ndim, dtype, pad, active
    for i in range(5):
        p.sizes[i] = 1
    for i, v in enumerate((n, c, t) + inner):
        p.sizes[i] = v
    for i in range(3):
        p.borders[2 * i], p.borders[2 * i + 1] = 0, 1
    for i, v in enumerate((t,) + inner):
        p.borders[2 * i], p.borders[2 * i + 1] = 0, v
    if window:
        p.borders[0], p.borders[1] = window
    if channels_last:   # memory order N, T, M, C
        st = [t * m * c, 1, m * c] + ([c] if ndim == 2 else [inner[1] * c, c])
    else:               # segment-major: memory order N, T, C, M
        st = [t * c * m, m, c * m] + ([1] if ndim == 2 else [inner[1], 1])
    return p, (ctypes.c_int64 * 5)(*(st + [0] * (5 - len(st))))


def _quantized(p, st, wkind=abi.F32, wzp=0, xzp=0, x=None, w=None, out=None):
    return abi.lib().shiftnd_forward_quantized(ctypes.byref(p), x, st, w, wkind, wzp, xzp, out, st, None)


def test_the_keywords_default_to_what_callers_send_today():
    x = torch.empty(2, 4, 3, 6, dtype=torch.uint8)
    assert abi.problem(x, 0, True, None, shift_dim0=True, per_clip=True).dtype == abi.U8 | DIM0 | PC
    assert abi.problem(x, 0, True, None, shift_dim0=True, interlace=True).dtype == abi.U8 | DIM0 | IL
    sig = inspect.signature(abi.forward_quantized).parameters
    assert sig["per_clip"].default is False and sig["interlace"].default is False


@pytest.mark.parametrize("bit", [PC, IL], ids=["per_clip", "interlace"])
@pytest.mark.parametrize("ndim", [2, 3])
def test_the_new_bits_with_a_float_table_host_side(ndim, bit):
    assert abi.lib().shiftnd_abi_version() == 5
    empty = (0, 5, 3, 8)
    x, w, out = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(12288)
    for dt in (abi.U8, abi.I8, abi.I32):
        for active in (0, 1):
            for pad in range(5):
                assert _quantized(*_problem(ndim, dt | DIM0 | bit, pad=pad, active=active)) == INVALID   # accepted up to the NULL tensors ...
            for k in range(3):                                                                         # ... which an empty problem never reaches
                size = tuple(0 if i == k else v for i, v in enumerate((2, 5, 3, 8)))
                assert _quantized(*_problem(ndim, dt | DIM0 | bit, size, active=active)) == OK, size
            # a further flag bit is refused before the sizes are looked at
            for extra in (PC | IL, abi.FRAMES, abi.STREAM, abi.CLIP_FRAMES, abi.INTERLACE_FRAMES, abi.WEIGHTS_F32):
                assert _quantized(*_problem(ndim, dt | DIM0 | bit | extra, empty, active=active)) == INVALID, extra
            assert _quantized(*_problem(ndim, dt | DIM0 | bit, empty, window=(1, 3), active=active)) == INVALID   # a cut window, empty or not
            assert _quantized(*_problem(ndim, dt | DIM0 | bit, window=(1, 3), active=active)) == INVALID
            assert _quantized(*_problem(ndim, dt | DIM0 | bit, empty, active=active), wzp=1) == INVALID           # a nonzero w_zero_point
            assert _quantized(*_problem(ndim, dt | DIM0 | bit, empty, active=active), x=x, out=x) == INVALID      # out == x
            # channels-last views, a misaligned table, and the limits: N * T * C, and 2^31 - 16 elements
            assert _quantized(*_problem(ndim, dt | DIM0 | bit, active=active, channels_last=True), x=x, w=w, out=out) == INVALID
            assert _quantized(*_problem(ndim, dt | DIM0 | bit, active=active), x=x, w=ctypes.c_void_p(8194), out=out) == INVALID
            assert _quantized(*_problem(ndim, dt | DIM0 | bit, (1 << 15, 1 << 8, 1 << 8, 2), active=active)) == INVALID
            assert _quantized(*_problem(ndim, dt | DIM0 | bit, (1 << 15, 1, 1 << 8, 1 << 8), active=active)) == INVALID
            # an integer table under the bit is what it was: the bit is no part of a quantized dtype
            assert _quantized(*_problem(ndim, dt | DIM0 | bit, empty, active=active), wkind=abi.I32) == UNSUPPORTED
        lo, hi = {abi.U8: (0, 255), abi.I8: (-128, 127), abi.I32: (-2 ** 31, 2 ** 31 - 1)}[dt]
        for zp, rc in ((lo, OK), (hi, OK), (lo - 1, INVALID), (hi + 1, INVALID)):                                  # the zero point's range
            assert _quantized(*_problem(ndim, dt | DIM0 | bit, empty), xzp=zp) == rc, zp
        p, st = _problem(ndim, dt | DIM0 | bit)
        assert int(abi.lib().shiftnd_backward_workspace_bytes(ctypes.byref(p))) == 0                               # no workspace
    assert _quantized(*_problem(1, abi.U8 | DIM0 | bit, (2, 5, 3, 1))) == INVALID                                  # ndim 1
    for dt in (abi.F32, abi.F16):
        assert _quantized(*_problem(ndim, dt | DIM0 | bit, empty)) == UNSUPPORTED                                  # a float dtype
    # the calls that were pinned before keep their answers: the flag alone with active == 0, FRAMES with a further bit
    assert _quantized(*_problem(ndim, abi.U8 | DIM0, active=0)) == UNSUPPORTED
    assert _quantized(*_problem(ndim, abi.U8 | DIM0 | abi.FRAMES | bit, empty)) == INVALID
