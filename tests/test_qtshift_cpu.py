"""Quantized interpolating temporal shift on the CPU (QuantizedCPU key):
torch.ops.torchshifts_quantized_learnable.temporal_shift_learnable_quantized, the functional wrapper,
torchshifts.quantized.LearnableTemporalShift and torchshifts.quant_mapping_interpolating.

The op is defined in the integer domain: with q = int_repr, zp the zero point and F = fp32 (quint8, qint8) / fp64 (qint32)

    out = clamp(zp + rint(temporal_shift_learnable_func((q - zp).to(F), w.to(F), T, padding_mode, active_flag=True)))

so the reference of this file is that expression on the existing float op, and int_repr is compared bit for bit.  Against the
composite quantize_per_tensor(float op(dequantize)) the op is bit-identical under a power-of-two scale with dyadic fractions (every
product is exact in both) and within one level otherwise (the composite resolves ties through scale * (1 / scale) != 1).
"""
import numpy as np
import pytest
import torch
from torch import nn

import torchshifts
from torchshifts import LearnableTemporalShift, quant_mapping, quant_mapping_interpolating
from torchshifts.functional import temporal_shift_learnable_func
from torchshifts.quantized.functional import temporal_shift_learnable_quantized, temporal_shift_quantized

NS = "torchshifts_quantized_learnable"
OP = torch.ops.torchshifts_quantized_learnable.temporal_shift_learnable_quantized
QLTS = torchshifts.quantized.LearnableTemporalShift
QTS = torchshifts.quantized.TemporalShift

# qdtype -> (int_repr dtype, zero point, value range [lo, hi), dtype range)
QDT = {torch.quint8: (np.uint8, 3, (0, 256), (0, 255)),
       torch.qint8: (np.int8, -7, (-128, 128), (-128, 127)),
       torch.qint32: (np.int32, 11, (-2 ** 30, 2 ** 30 + 1), (-2 ** 31, 2 ** 31 - 1))}   # (to +-2^30: q - zp is not exact in fp32)
SHAPES = [((2 * 5, 3, 4), 5), ((2 * 5, 3, 2, 3), 5), ((1 * 1, 2, 3), 1), ((2 * 3, 2, 2, 2, 2), 3)]


def ladder(T):
    """exact integers, exact halves, negatives, |w| > T, fractions, and values 1e-7 above and below an integer"""
    return np.array([0.0, 1.0, -2.0, 0.5, -1.5, 2.5, 0.3, -0.7, T + 1.25, -(T + 2.5), float(T), 1 + 1e-7, 1 - 1e-7, 1e-7, -1e-7,
                     -2 - 1e-7, -2 + 1e-7, 0.125], np.float32)


def tables(C, T):
    """the ladder cut into [C] tables (the last one wraps around)"""
    w = ladder(T)
    return [torch.from_numpy(np.take(w, np.arange(i, i + C), mode="wrap")) for i in range(0, len(w), C)]


def quantized(rs, shape, qdt, scale=0.05, zp=None):
    npdt, zp0, (lo, hi), _ = QDT[qdt]
    a = rs.randint(lo, hi, size=shape, dtype=np.int64).astype(npdt)
    return torch._make_per_tensor_quantized_tensor(torch.from_numpy(a), scale, zp0 if zp is None else zp)


def definition(x, w, T, pad):
    """the issue's definition, on the float op: -> int_repr"""
    F = torch.float64 if x.dtype == torch.qint32 else torch.float32
    zp = x.q_zero_point()
    lo, hi = QDT[x.dtype][3]
    r = temporal_shift_learnable_func((x.int_repr().to(torch.int64) - zp).to(F), w.to(F), T, pad, True)
    return (torch.round(r) + zp).clamp(lo, hi).to(x.int_repr().dtype)


def composite(x, w, T, pad):
    return torch.quantize_per_tensor(temporal_shift_learnable_func(x.dequantize(), w, T, pad, True), x.q_scale(), x.q_zero_point(), x.dtype)


@pytest.mark.parametrize("qdt", list(QDT), ids=lambda d: str(d).split(".")[-1])
def test_the_op_is_the_definition(qdt):
    rs = np.random.RandomState(61)
    for shape, T in SHAPES:
        for pad in range(5):
            x = quantized(rs, shape, qdt)
            for w in tables(shape[1], T):
                for wt in (w, w.view(-1, 1)):
                    out = OP(x, wt, T, pad, True)
                    assert torch.equal(out.int_repr(), definition(x, w, T, pad)), (shape, pad, w.tolist())


def test_qint32_needs_fp64():
    """the qint32 data of this file tells fp64 from fp32: the same expression in fp32 gives other bits"""
    rs = np.random.RandomState(62)
    x = quantized(rs, (10, 3, 4), torch.qint32)
    w = torch.tensor([0.3, -0.7, 2.5])
    r32 = temporal_shift_learnable_func((x.int_repr().to(torch.int64) - 11).float(), w, 5, 0, True)
    assert not torch.equal((torch.round(r32.double()) + 11).clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32), definition(x, w, 5, 0))


@pytest.mark.parametrize("qdt", [torch.quint8, torch.qint8], ids=lambda d: str(d).split(".")[-1])
def test_exact_case_equals_the_composite(qdt):
    rs = np.random.RandomState(63)
    for scale in (0.25, 0.5):
        for shape, T in SHAPES:
            for pad in range(5):
                x = quantized(rs, shape, qdt, scale=scale)
                w = torch.from_numpy(rs.randint(-8 * (T + 2), 8 * (T + 2) + 1, size=shape[1]).astype(np.float32) / 8)
                assert torch.equal(OP(x, w, T, pad, True).int_repr(), composite(x, w, T, pad).int_repr()), (scale, shape, pad, w.tolist())


@pytest.mark.parametrize("qdt", [torch.quint8, torch.qint8], ids=lambda d: str(d).split(".")[-1])
def test_general_case_is_within_one_level_of_the_composite(qdt):
    rs = np.random.RandomState(64)
    for pad in range(5):
        x = quantized(rs, (4 * 8, 16, 5, 5), qdt, scale=0.05)
        w = torch.from_numpy(rs.uniform(-9.5, 9.5, size=16).astype(np.float32))
        got, want = OP(x, w, 8, pad, True).int_repr().to(torch.int32), composite(x, w, 8, pad).int_repr().to(torch.int32)
        assert int((got - want).abs().max()) <= 1, pad


@pytest.mark.parametrize("qdt", list(QDT), ids=lambda d: str(d).split(".")[-1])
def test_sparse_mode_is_temporal_shift_quantized(qdt):
    rs = np.random.RandomState(65)
    for shape, T in SHAPES:
        for pad in range(5):
            x = quantized(rs, shape, qdt)
            for w in tables(shape[1], T):
                assert torch.equal(OP(x, w, T, pad, False).int_repr(), temporal_shift_quantized(x, w, T, pad).int_repr()), (shape, pad)
            whole = torch.from_numpy(rs.randint(-T - 2, T + 3, size=shape[1]).astype(np.float32))
            assert torch.equal(OP(x, whole, T, pad, True).int_repr(), temporal_shift_quantized(x, whole, T, pad).int_repr()), (shape, pad)


@pytest.mark.parametrize("qdt", list(QDT), ids=lambda d: str(d).split(".")[-1])
def test_output_properties(qdt):
    rs = np.random.RandomState(66)
    x = quantized(rs, (6, 4, 3, 5), qdt, scale=0.125)
    w = torch.tensor([0.25, -1.5, 3.75, 0.0])
    for active in (True, False):
        out = temporal_shift_learnable_quantized(x, w, 3, 1, active)
        assert out.is_quantized and out.dtype == qdt and out.qscheme() == torch.per_tensor_affine
        assert out.q_scale() == 0.125 and out.q_zero_point() == x.q_zero_point() and out.shape == x.shape and out.is_contiguous()
        cl = x.contiguous(memory_format=torch.channels_last)
        assert not cl.is_contiguous()
        got = temporal_shift_learnable_quantized(cl, w, 3, 1, active)
        assert got.is_contiguous() and torch.equal(got.int_repr(), out.int_repr())
    assert torch.equal(temporal_shift_learnable_quantized(x, w, 3).int_repr(), OP(x, w, 3, 0, True).int_repr())   # the defaults
    empty = torch._make_per_tensor_quantized_tensor(torch.zeros(0, 4, 3, dtype=x.int_repr().dtype), 0.125, 3)
    out = OP(empty, w, 3, 0, True)
    assert out.shape == empty.shape and out.dtype == qdt and out.q_zero_point() == 3


# ---- the dispatcher surface ----------------------------------------------------------------------------------------------------------
SCHEMA = ("torchshifts_quantized_learnable::temporal_shift_learnable_quantized(Tensor input, Tensor weights, int n_segment, "
          "int padding_mode, bool active_flag) -> Tensor")
ALL_KEYS = ["CPU", "CUDA", "QuantizedCPU", "QuantizedCUDA", "Autograd", "AutogradCPU", "AutogradCUDA", "CompositeImplicitAutograd",
            "CompositeExplicitAutograd", "Meta", "ADInplaceOrView", "SparseCPU", "SparseCUDA"]


def test_the_op_set_schema_and_keys_are_pinned():
    names = {n.split("::")[1] for n in torch._C._dispatch_get_all_op_names() if n.startswith(NS + "::")}
    assert names == {"temporal_shift_learnable_quantized"}
    assert str(torch._C._get_schema(NS + "::temporal_shift_learnable_quantized", "")) == SCHEMA
    keys = {k for k in ALL_KEYS if torch._C._dispatch_has_kernel_for_dispatch_key(NS + "::temporal_shift_learnable_quantized", k)}
    assert keys == {"QuantizedCPU", "QuantizedCUDA"}


def test_refusals_and_their_messages():
    x = quantized(np.random.RandomState(67), (6, 4, 3), torch.quint8)
    w = torch.zeros(4)
    OP(x, w, 3, 0, True)
    name = "temporal_shift_learnable_quantized: "
    with pytest.raises(ValueError, match="Input to 'temporal_shift_learnable_quantized' must be quantized!"):
        temporal_shift_learnable_quantized(torch.zeros(6, 4, 3), w, 3)
    with pytest.raises(RuntimeError):                       # a float input has no kernel on this op
        OP(torch.zeros(6, 4, 3), w, 3, 0, True)
    per_channel = torch.quantize_per_channel(torch.zeros(6, 4, 3), torch.ones(4), torch.zeros(4, dtype=torch.long), 1, torch.quint8)
    with pytest.raises(RuntimeError, match=name + "expected a per-tensor quantized input"):
        OP(per_channel, w, 3, 0, True)
    for bad in (quantized(np.random.RandomState(1), (6,), torch.quint8), quantized(np.random.RandomState(1), (6, 4, 1, 1, 1, 1), torch.quint8)):
        with pytest.raises(RuntimeError, match=name + r"expected a \[N\*T, C, ...\] tensor of 2 to 5 dims"):
            OP(bad, w, 3, 0, True)
    for T in (4, 0):
        with pytest.raises(RuntimeError, match=name + r"dim 0 \(6\) must be a multiple of n_segment \(%d\)" % T):
            OP(x, w, T, 0, True)
    for bad in (torch.zeros(5), torch.zeros(4, 2), torch.zeros(1, 4)):
        with pytest.raises(RuntimeError, match=name + r"weights must have shape \[C\] or \[C, 1\]"):
            OP(x, bad, 3, 0, True)
    for bad in (torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float16), torch.zeros(4, dtype=torch.long),
                torch.quantize_per_tensor(torch.zeros(4), 1.0, 0, torch.qint32)):
        with pytest.raises(RuntimeError, match=name + "weights must be fp32"):
            OP(x, bad, 3, 0, True)
    for pad in (-1, 5):
        with pytest.raises(RuntimeError, match=name + r"padding_mode must be 0\.\.4"):
            OP(x, w, 3, pad, True)
    for active in (True, False):
        with pytest.raises(RuntimeError, match=name + "weights must not require grad"):
            OP(x, torch.zeros(4, requires_grad=True), 3, 0, active)
    if torch.cuda.is_available():
        with pytest.raises(RuntimeError, match=name + "weights must be on the input's device"):
            OP(x, w.cuda(), 3, 0, True)


# ---- the module ------------------------------------------------------------------------------------------------------------------------
def trained(T, C, pad, active, seed):
    m = LearnableTemporalShift(T, C, padding=pad, init_shift=3, sparsity_term=0., active_flag=active)
    with torch.no_grad():
        m.weight.copy_(torch.from_numpy(np.random.RandomState(seed).uniform(-T - 1, T + 1, size=(C, 1)).astype(np.float32)))
        m.weight[:4, 0] = torch.tensor([0.5, 1.5, -2.5, 0.0])
    return m


def test_from_float_active_and_not():
    rs = np.random.RandomState(68)
    x = quantized(rs, (8, 8, 3, 3), torch.quint8)
    for k, pad in enumerate(("zeros", "border", "periodic", "reflect", "symmetric")):
        for active in (True, False):
            f = trained(4, 8, pad, active, 70 + k)
            q = QLTS.from_float(f)
            assert type(q) is QLTS and q.n_segment == 4 and q.padding == f.padding and q._active_flag is active and q.in_channels == 8
            assert q._get_name() == "QuantizedLearnableTemporalShift" and "QuantizedLearnableTemporalShift" in repr(q)
            assert not list(q.parameters()) and list(q.state_dict()) == ["weight"]
            assert q.weight.dtype == torch.float32 and q.weight.shape == (8, 1) and not q.weight.requires_grad
            assert torch.equal(q.weight, f.weight.detach()) and q.weight.data_ptr() != f.weight.data_ptr()
            out = q(x)
            assert isinstance(out, torch.Tensor) and out.is_quantized
            assert torch.equal(out.int_repr(), temporal_shift_learnable_quantized(x, f.weight.detach(), 4, k, active).int_repr())
            if not active:   # ... which is the frozen module quant_mapping gives
                assert torch.equal(out.int_repr(), QTS.from_float(f)(x).int_repr())
    with pytest.raises(AssertionError, match="expected a LearnableTemporalShift"):
        QLTS.from_float(torchshifts.TemporalShift(4, 8))


def test_state_dict_round_trip_from_a_float_checkpoint():
    rs = np.random.RandomState(69)
    x = quantized(rs, (8, 8, 3, 3), torch.qint8)
    f = trained(4, 8, "reflect", True, 80)
    q = QLTS(4, 8, padding="reflect")
    assert torch.equal(q.weight, torch.zeros(8, 1))
    q.load_state_dict(f.state_dict(), strict=True)
    assert torch.equal(q.weight, f.weight.detach())
    assert torch.equal(q(x).int_repr(), QLTS.from_float(f)(x).int_repr())
    fresh = QLTS(4, 8, padding="reflect")
    fresh.load_state_dict(q.state_dict())
    assert torch.equal(fresh(x).int_repr(), q(x).int_repr())


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.quant = torch.ao.quantization.QuantStub()
        self.learned = trained(4, 8, "border", True, 90)
        self.dequant = torch.ao.quantization.DeQuantStub()

    def forward(self, x):
        out = self.learned(self.quant(x))
        out = out[0] if isinstance(out, tuple) else out   # (the float module returns (out, loss), the quantized one the tensor)
        return self.dequant(out)


def test_convert_with_quant_mapping_interpolating():
    assert quant_mapping_interpolating[LearnableTemporalShift] is QLTS
    assert {k: v for k, v in quant_mapping_interpolating.items() if k is not LearnableTemporalShift} == \
        {k: v for k, v in quant_mapping.items() if k is not LearnableTemporalShift}
    torch.manual_seed(0)
    net = nn.Sequential(Net()).eval()
    x = torch.rand(8, 8, 5, 5)
    ref = net(x)
    net.qconfig = torch.ao.quantization.default_qconfig
    torch.ao.quantization.prepare(net, inplace=True)
    net(x)   # calibrate the stubs
    torch.ao.quantization.convert(net, inplace=True, mapping=quant_mapping_interpolating)
    assert type(net[0].learned) is QLTS and net[0].learned._active_flag is True
    out = net(x)
    # a convex blend of two quantized values, rounded once: the input's quantisation step plus half a level
    assert out.shape == ref.shape and (out - ref).abs().max() < 2.0 / 127


def test_quant_mapping_is_unchanged():
    assert quant_mapping[LearnableTemporalShift] is QTS and torchshifts.quantized.quant_mapping is quant_mapping
    with pytest.raises(ValueError, match="cannot be frozen"):
        QTS.from_float(LearnableTemporalShift(4, 8, active_flag=True))
