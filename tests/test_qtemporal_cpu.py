"""Quantized temporal shift on the CPU (QuantizedCPU key): torch.ops.torchshifts.temporal_shift_quantized, the functional wrapper,
torchshifts.quantized.TemporalShift and its place in quant_mapping.

The op is a pure gather on the int_repr, so every comparison is bit for bit: against tests/golden/qtemporal.npz (recorded from the
reference's quantized shift2d of the [N, C, T, M] view, tests/golden/make_golden_qtemporal.py), against a numpy restatement, and --
dequantized -- against the float op on dequantized data.
"""
import os

import numpy as np
import pytest
import torch
from torch import nn

import torchshifts
from torchshifts import LearnableTemporalShift, TemporalShift, quant_mapping
from torchshifts.quantized.functional import temporal_shift_quantized

OPS = torch.ops.torchshifts
QTS = torchshifts.quantized.TemporalShift
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qtemporal.npz"))
QDT = {"quint8": (torch.quint8, np.uint8, (0, 256)), "qint8": (torch.qint8, np.int8, (-128, 128)),
       "qint32": (torch.qint32, np.int32, (-100000, 100001))}
ZP = {"quint8": 7, "qint8": -3, "qint32": 100000}
SCALE = 0.05


def _quantized(int_repr, zp, scale=SCALE):
    return torch._make_per_tensor_quantized_tensor(torch.from_numpy(np.ascontiguousarray(int_repr)), scale, int(zp))


def _pad_index(i, n, pad):
    """the padding maps of the package, restated: source index in [0, n), or -1 for the fill"""
    if pad == 0:
        return i if 0 <= i < n else -1
    if pad == 1:
        return min(max(i, 0), n - 1)
    if pad == 2:
        return i % n
    if n == 1:
        return 0
    if pad == 3:                     # reflect: period 2 (n - 1), the edges are not repeated
        i %= 2 * (n - 1)
        return i if i < n else 2 * (n - 1) - i
    i %= 2 * n                       # symmetric: period 2 n, the edges are repeated
    return i if i < n else 2 * n - 1 - i


def restate(x, shifts, T, pad, zp):
    """numpy: out[(n, t), c] = x[(n, pad(t - s_c)), c], the zero point where the map says fill"""
    x = np.ascontiguousarray(x)
    v = x.reshape((x.shape[0] // T, T, x.shape[1], -1))
    out = np.full_like(v, zp)
    for c, s in enumerate(np.rint(np.asarray(shifts, np.float64).reshape(-1)).astype(np.int64)):
        for t in range(T):
            ts = _pad_index(t - int(s), T, pad) if T > 1 else 0
            if ts >= 0:
                out[:, t, c] = v[:, ts, c]
    return out.reshape(x.shape)


@pytest.mark.parametrize("name", list(QDT))
def test_the_op_equals_the_golden_and_the_restatement(name):
    for T in (3, 4):
        xi, zp, s = GOLDEN["x_%s_T%d" % (name, T)], int(GOLDEN["zp_" + name]), GOLDEN["shifts_T%d" % T]
        assert zp != 0 and {0, 1, -1} <= set(s.tolist()) and any(T <= abs(v) < 2 * T for v in s) and any(abs(v) >= 2 * T for v in s)
        x = _quantized(xi, zp)
        for pad in range(5):
            want = GOLDEN["out_%s_T%d_p%d" % (name, T, pad)]
            assert np.array_equal(restate(xi, s, T, pad, zp), want), (name, T, pad, "the restatement itself")
            for table in (torch.from_numpy(s), torch.from_numpy(s).view(-1, 1), torch.from_numpy(s).double(), torch.from_numpy(s).int()):
                for out in (OPS.temporal_shift_quantized(x, table, T, pad), temporal_shift_quantized(x, table, T, pad)):
                    assert np.array_equal(out.int_repr().numpy(), want), (name, T, pad, table.dtype, tuple(table.shape))
                    assert out.dtype == QDT[name][0] and out.is_contiguous() and out.shape == x.shape
                    assert out.q_scale() == x.q_scale() and out.q_zero_point() == zp and out.qscheme() == torch.per_tensor_affine


@pytest.mark.parametrize("shape,T", [((6, 5), 3), ((8, 4, 7), 4), ((6, 5, 3, 4), 3), ((4, 3, 2, 3, 2), 2), ((3, 4, 5), 1)],
                         ids=lambda v: str(v).replace(" ", ""))
def test_two_to_five_dims_and_float_tables(shape, T):
    rs = np.random.RandomState(31)
    C = shape[1]
    for name, (qdt, ndt, (lo, hi)) in QDT.items():
        xi = rs.randint(lo, hi, size=shape).astype(ndt)
        x = _quantized(xi, ZP[name])
        for pad in range(5):
            s = rs.randint(-2 * T - 1, 2 * T + 2, size=C)
            # floats round half to even: .5 goes to the even neighbour, on both sides of zero
            f = s + rs.choice([-0.5, -0.25, 0.0, 0.25, 0.5], size=C)
            for table in (torch.from_numpy(s), torch.from_numpy(f).float(), torch.from_numpy(f).view(C, 1)):
                out = temporal_shift_quantized(x, table, T, pad)
                assert np.array_equal(out.int_repr().numpy(), restate(xi, table.numpy(), T, pad, ZP[name])), (name, shape, pad, table.dtype)
    assert np.array_equal(np.rint([0.5, 1.5, 2.5, -0.5, -1.5]), [0, 2, 2, -0, -2])   # (what the restatement rounds with)
    x = _quantized(rs.randint(0, 256, size=shape).astype(np.uint8), 7)
    half = temporal_shift_quantized(x, torch.full((C,), 0.5), T, 2)
    assert torch.equal(half.int_repr(), x.int_repr())   # 0.5 -> 0: the identity


@pytest.mark.parametrize("name", list(QDT))
def test_dequantized_result_equals_the_float_op_bit_for_bit(name):
    rs = np.random.RandomState(32)
    qdt, ndt, (lo, hi) = QDT[name]
    T, shape = 4, (8, 6, 3, 5)
    xi = rs.randint(lo, hi, size=shape).astype(ndt)
    xi[xi == ZP[name]] += 1
    x = _quantized(xi, ZP[name])
    s = torch.tensor([0, 1, -1, 4, -9, 2])
    for pad in range(5):
        out = temporal_shift_quantized(x, s, T, pad)
        want = OPS.temporal_shift(x.dequantize(), s, T, pad)
        assert torch.equal(out.dequantize(), want), (name, pad)
        if pad == 0:
            filled = out.int_repr() == ZP[name]
            assert filled.any() and bool((out.dequantize()[filled] == 0).all()) and torch.equal(filled, want == 0)


def test_a_strided_input_is_taken_as_its_values():
    rs = np.random.RandomState(33)
    T, s = 3, torch.tensor([1, -1, 0, 5, 2])
    x = _quantized(rs.randint(0, 256, size=(6, 5, 4, 6)).astype(np.uint8), 9)
    want = temporal_shift_quantized(x, s, T, 0)
    for view in (x.contiguous(memory_format=torch.channels_last), x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)):
        assert not view.is_contiguous() and torch.equal(view.int_repr(), x.int_repr())
        out = temporal_shift_quantized(view, s, T, 0)
        assert out.is_contiguous() and torch.equal(out.int_repr(), want.int_repr())
    empty = temporal_shift_quantized(_quantized(np.zeros((0, 5, 2), np.uint8), 9), s, T, 0)
    assert empty.shape == (0, 5, 2) and empty.is_quantized


def test_argument_checks_raise():
    x = _quantized(np.zeros((6, 4, 3), np.uint8), 3)
    s = torch.zeros(4, dtype=torch.long)
    op = OPS.temporal_shift_quantized
    op(x, s, 3, 0)
    with pytest.raises(RuntimeError, match="multiple of n_segment"):
        op(x, s, 4, 0)
    with pytest.raises(RuntimeError, match="multiple of n_segment"):
        op(x, s, 0, 0)
    with pytest.raises(RuntimeError, match=r"\[C\] or \[C, 1\]"):
        op(x, torch.zeros(5, dtype=torch.long), 3, 0)
    with pytest.raises(RuntimeError, match=r"\[C\] or \[C, 1\]"):
        op(x, torch.zeros(4, 2, dtype=torch.long), 3, 0)
    with pytest.raises(RuntimeError, match="integers or floats"):
        op(x, torch.zeros(4, dtype=torch.bool), 3, 0)
    with pytest.raises(RuntimeError, match="padding_mode"):
        op(x, s, 3, 5)
    with pytest.raises(RuntimeError, match="2 to 5 dims"):
        op(_quantized(np.zeros((6,), np.uint8), 3), s, 3, 0)
    with pytest.raises(RuntimeError, match="2 to 5 dims"):
        op(_quantized(np.zeros((6, 4, 1, 1, 1, 1), np.uint8), 3), s, 3, 0)
    per_channel = torch.quantize_per_channel(torch.zeros(6, 4, 3), torch.ones(4), torch.zeros(4, dtype=torch.long), 1, torch.quint8)
    with pytest.raises(RuntimeError, match="per-tensor"):
        op(per_channel, s, 3, 0)
    with pytest.raises(RuntimeError):                       # a float input has no kernel on this op
        op(torch.zeros(6, 4, 3), s, 3, 0)
    with pytest.raises(ValueError, match="Input to 'temporal_shift_quantized' must be quantized!"):
        temporal_shift_quantized(torch.zeros(6, 4, 3), s, 3)
    with pytest.raises(RuntimeError):                       # and the float op still refuses a quantized tensor
        OPS.temporal_shift(x, s, 3, 0)


# ---- the module -----------------------------------------------------------------------------------------------------
def _clip(rs, C, T=4, n=2, zp=5):
    xi = rs.randint(0, 256, size=(n * T, C, 3, 3)).astype(np.uint8)
    return _quantized(xi, zp)


def test_module_state_dict_and_float_checkpoints():
    rs = np.random.RandomState(34)
    m = QTS(4, 16)
    assert isinstance(m, TemporalShift) and m._get_name() == "QuantizedTemporalShift" and "QuantizedTemporalShift" in repr(m)
    assert list(m.state_dict()) == ["shifts"] and not list(m.parameters())
    assert torch.equal(m.shifts, TemporalShift.default_table(16, 8))
    x = _clip(rs, 16)
    out = m(x)
    assert isinstance(out, torch.Tensor) and out.is_quantized
    assert torch.equal(out.int_repr(), torch.from_numpy(restate(x.int_repr().numpy(), m.shifts.numpy(), 4, 0, 5)))
    # round trip, and a float module's checkpoint
    custom = QTS(4, 16, shifts=[3, -2] * 8, padding="periodic")
    fresh = QTS(4, 16, padding="periodic")
    fresh.load_state_dict(custom.state_dict())
    assert torch.equal(fresh.shifts, custom.shifts) and torch.equal(fresh(x).int_repr(), custom(x).int_repr())
    floating = TemporalShift(4, 16, shifts=list(range(-8, 8)), padding="reflect")
    loaded = QTS(4, 16, padding="reflect")
    loaded.load_state_dict(floating.state_dict(), strict=True)
    assert torch.equal(loaded.shifts, floating.shifts)
    assert torch.equal(loaded(x).dequantize(), floating(x.dequantize()))


def test_from_float():
    rs = np.random.RandomState(35)
    x = _clip(rs, 8)
    for pad in ("zeros", "border", "periodic", "reflect", "symmetric"):
        f = TemporalShift(4, 8, fold_div=4, padding=pad)
        q = QTS.from_float(f)
        assert type(q) is QTS and q.n_segment == 4 and q.padding == f.padding and q.fold_div == 4 and torch.equal(q.shifts, f.shifts)
        assert q.shifts.data_ptr() != f.shifts.data_ptr()
        assert torch.equal(q(x).dequantize(), f(x.dequantize()))
        learnable = LearnableTemporalShift(4, 8, padding=pad, init_shift=3, sparsity_term=0.)
        learnable.weight.data[:4, 0] = torch.tensor([0.5, 1.5, -2.5, -0.5])   # ties: half to even
        frozen = TemporalShift.from_shift(learnable)
        q = QTS.from_float(learnable)
        assert type(q) is QTS and torch.equal(q.shifts, frozen.shifts) and q.shifts[:4].tolist() == [0, 2, -2, 0]
        assert torch.equal(q(x).dequantize(), frozen(x.dequantize()))
        assert torch.equal(q(x).dequantize(), learnable(x.dequantize())[0].detach())
    with pytest.raises(ValueError, match="cannot be frozen"):
        QTS.from_float(LearnableTemporalShift(4, 8, active_flag=True))


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.quant = torch.ao.quantization.QuantStub()
        self.fixed = TemporalShift(4, 8, padding="border")
        self.learned = LearnableTemporalShift(4, 8, init_shift=2, sparsity_term=0.)
        self.dequant = torch.ao.quantization.DeQuantStub()

    def forward(self, x):
        x = self.fixed(self.quant(x))
        out = self.learned(x)
        out = out[0] if isinstance(out, tuple) else out   # (the float module returns (out, loss), the quantized one the tensor)
        return self.dequant(out)


def test_convert_with_quant_mapping():
    assert quant_mapping[TemporalShift] is QTS and quant_mapping[LearnableTemporalShift] is QTS
    assert torchshifts.quantized.modules.TemporalShift is QTS
    torch.manual_seed(0)
    net = Net().eval()
    x = torch.rand(8, 8, 5, 5)
    ref = net(x)
    net.qconfig = torch.ao.quantization.default_qconfig
    torch.ao.quantization.prepare(net, inplace=True)
    net(x)   # calibrate the stubs
    torch.ao.quantization.convert(net, inplace=True, mapping=quant_mapping)
    assert type(net.fixed) is QTS and type(net.learned) is QTS
    out = net(x)
    # a pure gather: the quantized result is the float result up to the input's quantisation step
    assert out.shape == ref.shape and (out - ref).abs().max() < 2.0 / 127
