"""Temporal shift (TSM) on CPU tensors: torch.ops.torchshifts.temporal_shift, temporal_shift_func and the TemporalShift module against
a numpy restatement and against the composed definition

    shift2d_fixed_func(x.view(N, T, C, M).permute(0, 2, 1, 3), stack([shifts, 0], 1), pad).permute(0, 2, 1, 3).reshape(x.shape)

bit for bit, in both directions (the op moves whole planes: a pure gather).  The CPU backend of shift2d_fixed serves fp32 / fp64
only, so for fp16 / bf16 the composed definition runs on the widened tensor and is narrowed back -- exact, nothing is computed.
"""
import itertools

import numpy as np
import pytest
import torch

import torchshifts
from torchshifts.functional import shift2d_fixed_func, temporal_shift_func

OPS = torch.ops.torchshifts
DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]
SHAPES = [(6, 5), (6, 5, 3), (6, 5, 7, 7), (4, 3, 2, 3, 2)]
BITS = {2: torch.int16, 4: torch.int32, 8: torch.int64}


def pad_index(i, L, pad):
    """source index in [0, L) or -1 (fill): include/shiftnd_hip.h's padding modes, written out"""
    if pad == 0:
        return i if 0 <= i < L else -1
    if pad == 1:
        return min(max(i, 0), L - 1)
    if pad == 2:
        return i % L
    if pad == 3:
        m = i % (2 * (L - 1))
        return m if m < L else 2 * (L - 1) - m
    m = i % (2 * L)
    return m if m < L else 2 * L - 1 - m


def np_temporal(x, s, T, pad, sign=+1):
    """out[(n, t), c] = x[(n, pad(t - sign * s[c])), c] on the tensor's bits (no arithmetic: every float type alike)"""
    bits = x.contiguous().view(BITS[x.element_size()]).numpy()
    NT, C = bits.shape[:2]
    v = bits.reshape(NT // T, T, C, -1)
    out = np.zeros_like(v)
    for c, t in itertools.product(range(C), range(T)):
        ts = t if T == 1 else pad_index(t - sign * int(s[c]), T, pad)   # (a size-1 dim ignores its shift)
        if ts >= 0:
            out[:, t, c] = v[:, ts, c]
    return torch.from_numpy(out.reshape(bits.shape)).view(x.dtype)


def composed(x, s, T, pad):
    wide = x if x.dtype in (torch.float32, torch.float64) else x.float()
    NT, C = x.shape[:2]
    v = wide.reshape(NT // T, T, C, -1).permute(0, 2, 1, 3)
    out = shift2d_fixed_func(v, torch.stack([s, torch.zeros_like(s)], 1), pad)
    return out.permute(0, 2, 1, 3).reshape(x.shape).to(x.dtype)


def _table(rs, C, T):
    s = rs.randint(-T - 1, T + 2, size=C)
    s[0], s[1], s[2] = 0, T + 1, -T - 1
    return torch.from_numpy(s.astype(np.int64))


def _cases():
    for shape, T in itertools.product(SHAPES, (1, 2, 3)):
        if shape[0] % T == 0:
            yield shape, T


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_op_and_functional_match_numpy_and_the_composed_definition(dtype):
    rs = np.random.RandomState(7)
    n = 0
    for (shape, T), pad in itertools.product(_cases(), range(5)):
        x = torch.from_numpy(rs.uniform(-1, 1, size=shape)).to(dtype)
        go = torch.from_numpy(rs.uniform(-1, 1, size=shape)).to(dtype)
        s = _table(rs, shape[1], T)
        key = (shape, T, pad)
        want = np_temporal(x, s, T, pad)
        xt = x.clone().requires_grad_(True)
        out = temporal_shift_func(xt, s, T, pad)
        assert out.dtype == dtype and out.shape == x.shape and out.is_contiguous(), key
        assert torch.equal(out.detach(), want), ("functional", key)
        assert torch.equal(OPS.temporal_shift(x, s, T, pad), want), ("op", key)
        assert torch.equal(OPS.temporal_shift(x, s.to(torch.int32).reshape(-1, 1), T, pad), want), ("[C, 1] int32 table", key)
        assert torch.equal(OPS.temporal_shift(x, s.double(), T, pad), want), ("float table", key)
        out.backward(go)
        assert torch.equal(xt.grad, np_temporal(go, s, T, pad, sign=-1)), ("grad_x", key)
        assert torch.equal(OPS._temporal_shift_backward(go, s, T, pad), xt.grad), ("backward op", key)
        # the composed definition, forward and x.grad
        xc = (x if dtype in (torch.float32, torch.float64) else x.float()).clone().requires_grad_(True)
        outc = composed(xc, s, T, pad)
        assert torch.equal(out.detach(), outc.detach().to(dtype)), ("composed", key)
        outc.backward(go.to(xc.dtype))
        assert torch.equal(xt.grad, xc.grad.to(dtype)), ("composed grad_x", key)
        n += 1
    assert n == 11 * 5


def test_a_float_table_rounds_half_to_even():
    x = torch.randn(8, 4, 3)
    s = torch.tensor([0.5, 1.5, -0.5, -2.5])
    assert torch.equal(OPS.temporal_shift(x, s, 4, 2), np_temporal(x, [0, 2, 0, -2], 4, 2))


def test_a_strided_input_is_taken_as_its_values():
    x = torch.randn(5, 6, 4, 3).permute(1, 0, 3, 2)   # [6, 5, 3, 4], not contiguous
    s = torch.tensor([1, -1, 0, 2, -2])
    assert torch.equal(OPS.temporal_shift(x, s, 3, 0), np_temporal(x, s, 3, 0))


@pytest.mark.parametrize("C,fold_div", [(16, 8), (20, 8), (6, 8), (12, 4)])
def test_the_default_table_is_the_published_slicing(C, fold_div):
    T, N = 4, 3
    m = torchshifts.TemporalShift(T, C, fold_div=fold_div)
    f = C // fold_div
    assert m.shifts.dtype == torch.int64 and m.shifts.tolist() == [-1] * f + [1] * f + [0] * (C - 2 * f)
    x = torch.randn(N * T, C, 5, 5)
    v = x.view(N, T, C, 5, 5)
    want = torch.zeros_like(v)
    want[:, :-1, :f] = v[:, 1:, :f]
    want[:, 1:, f:2 * f] = v[:, :-1, f:2 * f]
    want[:, :, 2 * f:] = v[:, :, 2 * f:]
    out = m(x)
    assert isinstance(out, torch.Tensor) and torch.equal(out, want.view_as(x))
    assert torch.equal(torch.nn.Sequential(m, torch.nn.Identity())(x), out)


def test_module_has_a_buffer_no_parameters_and_round_trips():
    m = torchshifts.TemporalShift(3, 10, shifts=torch.randint(-3, 4, (10,)), padding="reflect")
    assert list(m.parameters()) == []
    sd = m.state_dict()
    assert list(sd.keys()) == ["shifts"]
    m2 = torchshifts.TemporalShift(3, 10, padding="reflect")
    m2.load_state_dict(sd)
    assert torch.equal(m2.shifts, m.shifts)
    x = torch.randn(6, 10, 4)
    assert torch.equal(m2(x), np_temporal(x, m.shifts, 3, 3))
    assert "n_segment=3" in repr(m) and "reflect" in repr(m)
    explicit = torchshifts.TemporalShift(2, 4, fold_div=2, shifts=[0, 2.0, -1, 0])   # an explicit table overrides fold_div
    assert explicit.shifts.tolist() == [0, 2, -1, 0]


def _packed_numels(fn):
    seen = []

    def pack(t):
        seen.append(t.numel())
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        fn()
    return seen


def test_the_node_saves_the_table_alone():
    x = torch.randn(8, 6, 10, 12, requires_grad=True)
    s = torch.randint(-2, 3, (6,))
    saved = _packed_numels(lambda: temporal_shift_func(x, s, 4, 0))
    assert saved == [6], saved
    w = torch.zeros(6, 2, requires_grad=True)
    learnable = _packed_numels(lambda: OPS.shift2d(x, w, torch.Tensor(), 0, False))
    assert x.numel() in learnable, learnable   # what "saves no input" is measured against


def test_double_backward_raises():
    x = torch.randn(4, 3, 5, requires_grad=True)
    out = temporal_shift_func(x, torch.tensor([1, 0, -1]), 2)
    g, = torch.autograd.grad(out, x, torch.ones_like(out, requires_grad=True), create_graph=True)
    with pytest.raises(RuntimeError, match="double backwards"):
        g.sum().backward()


def test_every_argument_check_raises():
    x = torch.randn(6, 5, 4)
    s = torch.zeros(5, dtype=torch.int64)
    bad = [
        (torch.randn(6), s, 2, 0),                               # fewer than 2 dims
        (torch.randn(6, 5, 2, 2, 2, 2), s, 2, 0),                # more than 5
        (x, s, 4, 0),                                            # 6 % 4
        (x, s, 0, 0),                                            # n_segment < 1
        (x, torch.zeros(4, dtype=torch.int64), 2, 0),            # wrong channel count
        (x, torch.zeros(5, 2, dtype=torch.int64), 2, 0),         # [C, 2]
        (x, torch.zeros(5, 1, 1, dtype=torch.int64), 2, 0),      # 3 dims
        (x, s, 2, 5),                                            # padding_mode
        (x, s, 2, -1),
    ]
    for args in bad:
        with pytest.raises(AssertionError):
            temporal_shift_func(*args)
        with pytest.raises(RuntimeError):
            OPS.temporal_shift(*args)
        with pytest.raises(RuntimeError):
            OPS._temporal_shift_backward(*args)
    with pytest.raises(RuntimeError, match="integers or floats"):
        OPS.temporal_shift(x, torch.zeros(5, dtype=torch.bool), 2, 0)
    with pytest.raises(RuntimeError, match="quantized"):
        OPS.temporal_shift(torch.quantize_per_tensor(x, 0.1, 0, torch.qint8), s, 2, 0)
    with pytest.raises(RuntimeError):
        OPS.temporal_shift(torch.zeros(6, 5, 4, dtype=torch.int32), s, 2, 0)   # not a float tensor
