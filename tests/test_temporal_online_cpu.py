"""Online temporal shift on CPU tensors: T steps on the frames of a clip against the oracle's 2-D sparse forward of the [B, C, T, M]
view under (s, 0) (online_cases.reference_frames), bit for bit; the state after the steps; the pinned surface of the
torchshifts_online:: namespace; the refusals; the modules; and the host side of the C ABI under SHIFTND_STREAM, which needs no
device."""
import ctypes

import numpy as np
import pytest
import torch

import torchshifts
from torchshifts import abi
from torchshifts.functional import (temporal_shift_func, temporal_shift_online_func, temporal_shift_online_func_,
                                    temporal_shift_online_state)
from torchshifts.modules import LearnableTemporalShift, OnlineTemporalShift, TemporalShift
from torchshifts.quantized import OnlineTemporalShift as QOnlineTemporalShift
from torchshifts.quantized.functional import temporal_shift_online_quantized, temporal_shift_online_quantized_

import online_cases as OC
from online_cases import F16, BF16, F32, F64, U8, I8, I32, T

OOPS = torch.ops.torchshifts_online


def _tables(C):
    return [OC.WRAP if C == 5 else OC.causal_table(np.random.RandomState(C), C, 3), OC.default_table(C)]


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("pad", [0, 1])
def test_stacked_steps_equal_the_reference(pad, channels_last):
    rs = np.random.RandomState(pad + 2 * channels_last)
    for dt, B, C, sp in ((F32, 2, 5, (3, 4)), (F16, 3, 16, (2, 2)), (F64, 1, 5, ()), (BF16, 2, 5, (2, 2, 2))):
        for s in _tables(C):
            X, frames = OC.clip(rs, B, C, sp, dt)
            want = OC.reference_frames(X, s, T, pad)
            first = OC.layout(frames[0], channels_last)
            state = temporal_shift_online_state(first, s, pad)
            initial = state.clone()
            assert state.shape == (int(s.max()),) + first.shape and state.dtype == dt
            assert state.shape[0] == 0 or state.stride()[1:] == first.stride()
            for t in range(T):
                f = OC.layout(frames[t], channels_last)
                keep = f.clone()
                out = temporal_shift_online_func(f, state, s)
                assert OC.same_bits(f, keep) and out is not f and out.stride() == f.stride()   # out of place: the input as it was
                assert OC.same_bits(out, want[t]), (dt, pad, t)
            assert OC.same_bits(state, OC.expected_state(frames, s, initial)), (dt, pad)


def test_the_in_place_step_returns_its_input_and_bumps_both_versions():
    rs = np.random.RandomState(5)
    X, frames = OC.clip(rs, 2, 5, (3, 3), F32)
    want = OC.reference_frames(X, OC.WRAP, T, 0)
    state = temporal_shift_online_state(frames[0], OC.WRAP, 0)
    for t in range(T):
        f = frames[t].clone()
        versions = f._version, state._version
        assert temporal_shift_online_func_(f, state, OC.WRAP) is f
        assert f._version > versions[0] and state._version > versions[1]
        assert OC.same_bits(f, want[t])


def test_the_state_after_the_steps_and_untouched_slots():
    rs = np.random.RandomState(6)
    X, frames = OC.clip(rs, 2, 5, (2, 3), F32)
    state = torch.from_numpy(rs.uniform(-1, 1, size=(3, 2, 5, 2, 3))).to(F32)   # any initial bytes: slots k >= s_c must keep them
    initial = state.clone()
    for t in range(T):
        temporal_shift_online_func_(frames[t].clone(), state, OC.WRAP)
    for c, s in enumerate(OC.WRAP.tolist()):
        for k in range(3):
            if k < s:
                assert OC.same_bits(state[k][:, c], frames[T - 1 - k][:, c]), (c, k)
            else:
                assert OC.same_bits(state[k][:, c], initial[k][:, c]), (c, k)


def test_an_all_zero_table_is_a_no_op():
    x = torch.randn(2, 4, 3)
    s = torch.zeros(4, dtype=torch.int64)
    state = temporal_shift_online_state(x, s)
    assert state.shape == (0, 2, 4, 3)
    keep = x.clone()
    assert temporal_shift_online_func_(x, state, s) is x and OC.same_bits(x, keep)
    # ... and so are channels with shift 0 beside shifted ones, in the frame and in the state
    s = torch.tensor([0, 1, 0, 0])
    state = torch.full((1, 2, 4, 3), 7.0)
    temporal_shift_online_func_(x, state, s)
    assert OC.same_bits(x[:, [0, 2, 3]], keep[:, [0, 2, 3]]) and bool((state[:, :, [0, 2, 3]] == 7.0).all())
    assert bool((x[:, 1] == 7.0).all()) and OC.same_bits(state[0][:, 1], keep[:, 1])


def test_more_slots_than_the_kernel_serves_and_shifts_beyond_the_state():
    rs = np.random.RandomState(8)
    s = torch.tensor([16, 0, 3, 1, 7])
    X, frames = OC.clip(rs, 2, 5, (2,), F32, steps=18)
    want = OC.reference_frames(X, s, 18, 0)
    state = temporal_shift_online_state(frames[0], s, 0)
    assert state.shape[0] == 16
    for t in range(18):
        assert OC.same_bits(temporal_shift_online_func(frames[t], state, s), want[t]), t


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("pad", [0, 1])
def test_quantized_steps_on_the_int_repr(pad, channels_last):
    rs = np.random.RandomState(20 + pad)
    for dt, qdt, zp in ((U8, torch.quint8, 77), (I8, torch.qint8, -5), (I32, torch.qint32, 70000)):
        for s in _tables(5):
            X, frames = OC.clip(rs, 2, 5, (3, 3), dt)
            want = OC.reference_frames(X, s, T, pad, zp)
            first = OC.quantized(frames[0], zp, channels_last)
            state = temporal_shift_online_state(first, s, pad)
            assert state.is_quantized and state.dtype == qdt and state.q_zero_point() == zp and state.q_scale() == 0.05
            assert state.shape[0] == 0 or state.stride()[1:] == first.stride()
            if pad == 0:
                assert bool((state.int_repr() == zp).all())
            for t in range(T):
                q = OC.quantized(frames[t], zp, channels_last)
                out = temporal_shift_online_quantized(q, state, s)
                assert out.q_zero_point() == zp and out.q_scale() == 0.05 and out.dtype == qdt and out.stride() == q.stride()
                assert OC.same_bits(out.int_repr(), want[t]), (dt, pad, t)
                assert OC.same_bits(q.int_repr(), frames[t])
            q = OC.quantized(frames[0], zp, channels_last)
            assert temporal_shift_online_quantized_(q, state, s) is q


# ---- the dispatcher surface of torchshifts_online:: ---------------------------------------------------------------------------------
SCHEMAS = {
    "temporal_shift_online_": "torchshifts_online::temporal_shift_online_(Tensor(a!) input, Tensor(b!) state, Tensor shifts) -> Tensor(a!)",
    "temporal_shift_online_quantized_":
        "torchshifts_online::temporal_shift_online_quantized_(Tensor(a!) input, Tensor(b!) state, Tensor shifts) -> Tensor(a!)",
}
KEYS = {"temporal_shift_online_": {"CPU", "CUDA"}, "temporal_shift_online_quantized_": {"QuantizedCPU", "QuantizedCUDA"}}
ALL_KEYS = ["CPU", "CUDA", "QuantizedCPU", "QuantizedCUDA", "Autograd", "AutogradCPU", "AutogradCUDA", "CompositeImplicitAutograd",
            "CompositeExplicitAutograd", "Meta", "ADInplaceOrView", "SparseCPU", "SparseCUDA"]


def test_the_op_set_schemas_and_keys_are_pinned():
    names = {n.split("::")[1] for n in torch._C._dispatch_get_all_op_names() if n.startswith("torchshifts_online::")}
    assert names == set(SCHEMAS)
    for name, schema in SCHEMAS.items():
        assert str(torch._C._get_schema("torchshifts_online::" + name, "")) == schema
        keys = {k for k in ALL_KEYS if torch._C._dispatch_has_kernel_for_dispatch_key("torchshifts_online::" + name, k)}
        assert keys == KEYS[name], (name, keys)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_their_messages():
    x, s = torch.randn(2, 4, 3), torch.tensor([1, 0, 2, 0])
    with pytest.raises(ValueError, match=r"temporal_shift_online_state\(\): a negative shift \(-1\) reads the future"):
        temporal_shift_online_state(x, torch.tensor([1, 0, -1, 0]))
    with pytest.raises(ValueError, match="shifts must hold integers"):
        temporal_shift_online_state(x, torch.tensor([1.0, 0.5, 0.0, 0.0]))
    for pad in (2, 3, 4):
        with pytest.raises(ValueError, match="padding_mode must be 0 .zeros. or 1 .border.; periodic, reflect and symmetric padding look into the future"):
            temporal_shift_online_state(x, s, pad)
    with pytest.raises(RuntimeError, match="temporal_shift_online_: a negative shift reads the future"):
        temporal_shift_online_func_(x.clone(), torch.zeros(2, 2, 4, 3), torch.tensor([1, 0, -1, 0]))
    state = temporal_shift_online_state(x, s)
    for bad, text in ((state[:, :1], r"state must have shape \[D, \[2, 4, 3\]\]"), (state[0], r"state must have shape \[D, "),
                      (state.double(), "state must have the input's dtype")):
        with pytest.raises(RuntimeError, match="temporal_shift_online_: " + text):
            temporal_shift_online_func_(x.clone(), bad, s)
    with pytest.raises(RuntimeError, match=r"temporal_shift_online_: shifts must have shape \[C\]"):
        OOPS.temporal_shift_online_(x.clone(), state, s[:3])
    with pytest.raises(RuntimeError, match="temporal_shift_online_: shifts must be integers or floats"):
        OOPS.temporal_shift_online_(x.clone(), state, s > 0)
    whole = torch.randn(3, 2, 4, 3)
    with pytest.raises(RuntimeError, match="temporal_shift_online_: input and state overlap in memory"):
        temporal_shift_online_func_(whole[1], whole[:2], s)
    temporal_shift_online_func_(whole[2], whole[:2], s)   # (the same storage without an overlap is served)
    with pytest.raises(RuntimeError, match="temporal_shift_online_: an inference op without an autograd formula, but an argument requires grad"):
        temporal_shift_online_func_(x.clone().requires_grad_(), state, s)
    with pytest.raises(RuntimeError, match="requires grad"):
        temporal_shift_online_func_(x.clone(), state.clone().requires_grad_(), s)
    with pytest.raises(AssertionError, match=r"temporal_shift_online_func_\(\): expected \[4\] tensor as shifts"):
        temporal_shift_online_func_(x.clone(), state, s[:3])


def test_quantized_refusals():
    s = torch.tensor([1, 0, 2, 0])
    q = OC.quantized(torch.zeros(2, 4, 3, dtype=U8), 3)
    state = temporal_shift_online_state(q, s)
    name = "temporal_shift_online_quantized_: "
    with pytest.raises(RuntimeError, match=name + "expected a per-tensor quantized state"):
        temporal_shift_online_quantized_(q, state.int_repr(), s)
    for bad in (torch._make_per_tensor_quantized_tensor(state.int_repr(), 0.05, 4), torch._make_per_tensor_quantized_tensor(state.int_repr(), 0.1, 3)):
        with pytest.raises(RuntimeError, match=name + r"state must have the input's scale and zero point \(0.05, 3\)"):
            temporal_shift_online_quantized_(q, bad, s)
    with pytest.raises(RuntimeError, match=name + "state must have the input's dtype"):
        temporal_shift_online_quantized_(q, torch._make_per_tensor_quantized_tensor(state.int_repr().to(I8), 0.05, 3), s)
    with pytest.raises((RuntimeError, NotImplementedError)):   # (a quantized argument takes the float op to a key without a kernel)
        OOPS.temporal_shift_online_(torch.zeros(2, 4, 3), state, s)
    with pytest.raises((RuntimeError, NotImplementedError)):
        OOPS.temporal_shift_online_quantized_(torch.zeros(2, 4, 3), torch.zeros(2, 2, 4, 3), s)
    with pytest.raises(ValueError, match="temporal_shift_online_quantized_"):
        temporal_shift_online_quantized_(torch.zeros(2, 4, 3), state, s)
    with pytest.raises(AssertionError, match="quantized inputs go through"):
        temporal_shift_online_func_(q, state, s)


# ---- modules -------------------------------------------------------------------------------------------------------------------------
def test_module_surface_and_streams():
    m = OnlineTemporalShift(16)
    assert m.extra_repr() == "in_channels=16, fold_div=8, padding_method=zeros, fixed integer shifts, online"
    assert OnlineTemporalShift(16, inplace=True).extra_repr() == m.extra_repr() + ", inplace=True"
    assert torch.equal(m.shifts, OC.default_table(16)) and m.shifts.dtype == torch.int64
    assert list(m.state_dict()) == ["shifts"] and m.state is None
    rs = np.random.RandomState(30)
    X, frames = OC.clip(rs, 2, 16, (3, 3), F32)
    for pad, name in ((0, "zeros"), (1, "border")):
        for inplace in (False, True):
            m = OnlineTemporalShift(16, padding=name, inplace=inplace)
            want = OC.reference_frames(X, m.shifts, T, pad)
            for t in range(T):
                f = frames[t].clone()
                out = m(f)
                assert (out is f) == inplace and OC.same_bits(out, want[t])
                assert inplace or OC.same_bits(f, frames[t])
            assert list(m.state_dict()) == ["shifts"] and m.state.shape == (1, 2, 16, 3, 3)
            m.reset()
            assert m.state is None
            assert OC.same_bits(m(frames[0].clone()), want[0])   # a new stream
    with pytest.raises(RuntimeError, match=r"the state was made for frames of shape \(2, 16, 3, 3\).*reset\(\) starts a new stream"):
        m(torch.randn(2, 16, 3, 4))
    with pytest.raises(RuntimeError, match="the state was made for frames"):
        m(frames[0].double())
    with pytest.raises(RuntimeError, match="the state was made for frames"):
        m(OC.layout(frames[0], True))
    for pad in ("periodic", "reflect", "symmetric"):
        with pytest.raises(ValueError, match="looks into the future"):
            OnlineTemporalShift(16, padding=pad)
    with pytest.raises(ValueError, match="a negative shift reads the future"):
        OnlineTemporalShift(4, shifts=[0, 1, -1, 0])


def test_from_shift_from_float_and_quant_mapping():
    with pytest.raises(ValueError, match="reads the future"):
        OnlineTemporalShift.from_shift(TemporalShift(T, 16))   # the published bidirectional table
    fixed = TemporalShift(T, 5, shifts=OC.WRAP, padding="border")
    m = OnlineTemporalShift.from_shift(fixed)
    assert torch.equal(m.shifts, OC.WRAP) and m.padding == 1 and m.inplace is False
    rs = np.random.RandomState(31)
    X, frames = OC.clip(rs, 2, 5, (3,), F32)
    assert OC.same_bits(torch.stack([m(f) for f in frames], 1).reshape(X.shape), fixed(X))
    assert OC.same_bits(fixed(X), temporal_shift_func(X, OC.WRAP, T, 1))
    with pytest.raises(AssertionError, match="expected a TemporalShift module"):
        OnlineTemporalShift.from_shift(LearnableTemporalShift(T, 5))
    q = QOnlineTemporalShift.from_float(OnlineTemporalShift(5, shifts=OC.WRAP, inplace=True))
    assert q.inplace is True and torch.equal(q.shifts, OC.WRAP) and list(q.state_dict()) == ["shifts"]
    assert q._get_name() == "QuantizedOnlineTemporalShift"
    assert torchshifts.quant_mapping[OnlineTemporalShift] is QOnlineTemporalShift
    assert torchshifts.OnlineTemporalShift is OnlineTemporalShift and torchshifts.quantized.OnlineTemporalShift is QOnlineTemporalShift
    X, frames = OC.clip(rs, 2, 5, (3,), U8)
    want = OC.reference_frames(X, OC.WRAP, T, 0, 9)
    for t in range(T):
        f = OC.quantized(frames[t], 9)
        assert q(f) is f and OC.same_bits(f.int_repr(), want[t])
    with pytest.raises(RuntimeError, match="state must have the input's scale and zero point"):
        q(OC.quantized(frames[0], 10))


# ---- C ABI: SHIFTND_STREAM is validated on the host, before any device work ------------------------------------------------------------
B, C, M = 2, 4, 6


def _problem(D, dtype=abi.F32, extra=0, pad=0, active=0, borders=None, flags=abi.SHIFT_DIM0 | abi.STREAM, sizes=None):
    p = abi.Problem()
    p.ndim, p.dtype, p.padding_mode, p.active = 2, dtype | flags | extra, pad, active
    for i, v in enumerate(sizes or (B, C, D, M, 1)):
        p.sizes[i] = v
    for i, v in enumerate(borders or (0, D, 0, M, 0, 1)):
        p.borders[i] = v
    return p


def _rc(D, dtype=abi.F32, quantized=False, state_strides=None, frame_strides=None, **kw):
    """the online call with NULL tensors: an accepted problem reaches the NULL check and answers -1 with nothing launched"""
    p = _problem(D, dtype, **kw)
    ss = (ctypes.c_int64 * 5)(*(state_strides or (C * M, M, B * C * M, 1, 0)))
    fs = (ctypes.c_int64 * 5)(*(frame_strides or (C * M, M, 0, 1, 0)))
    L = abi.lib()
    if quantized:
        return L.shiftnd_forward_quantized(ctypes.byref(p), None, ss, None, abi.I32, 0, 0, None, fs, None)
    return L.shiftnd_forward(ctypes.byref(p), None, ss, None, None, fs, None)


def test_host_side_of_the_stream_flag():
    L = abi.lib()
    assert abi.STREAM == 0x2000
    assert abi.problem(torch.empty(2, 4, 3, 6), 0, False, None, shift_dim0=True, stream=True).dtype == abi.F32 | 0x200 | 0x2000
    # accepted problems reach the NULL check; empty ones are served
    for dt, quantized in ((abi.F32, False), (abi.F64, False), (abi.F16, False), (abi.BF16 | abi.WEIGHTS_F32, False), (abi.U8, True),
                          (abi.I8, True), (abi.I32, True)):
        for D in (1, 3, 15):
            for pad in (0, 1):
                assert _rc(D, dt, quantized, pad=pad) == -1, (dt, D, pad)
        assert _rc(0, dt, quantized) == 0 and L.shiftnd_last_path() == abi.PATH_EMPTY
        assert _rc(3, dt, quantized, sizes=(0, C, 3, M, 1)) == 0 and _rc(3, dt, quantized, sizes=(B, C, 3, 0, 1), borders=(0, 3, 0, 0, 0, 1)) == 0
    # the entry points keep their dtypes under the flag
    assert _rc(3, abi.U8) == -2 and _rc(3, abi.F32, True) == -2 and _rc(3, abi.F32 | abi.WEIGHTS_F32) == -2
    # the refusals
    for quantized, dt in ((False, abi.F32), (True, abi.U8)):
        assert _rc(3, dt, quantized, extra=abi.FRAMES) == -1 and _rc(3, dt, quantized, extra=abi.PER_CLIP) == -1
        assert _rc(16, dt, quantized) == -1
        assert _rc(3, dt, quantized, borders=(1, 3, 0, M, 0, 1)) == -1 and _rc(3, dt, quantized, borders=(0, 3, 0, M - 1, 0, 1)) == -1
        assert _rc(3, dt, quantized, active=1) == -1
        for pad in (2, 3, 4):
            assert _rc(3, dt, quantized, pad=pad) == -1
    # shiftnd_backward and the workspace query
    p = _problem(3)
    st = (ctypes.c_int64 * 5)(C * M, M, B * C * M, 1, 0)
    assert L.shiftnd_backward(ctypes.byref(p), None, st, None, st, None, None, st, None, None, 0, None) == -1
    assert L.shiftnd_backward_workspace_bytes(ctypes.byref(p)) == 0
    assert L.shiftnd_backward_workspace_bytes(ctypes.byref(_problem(3, flags=abi.STREAM))) == 0


def test_layout_and_overlap_refusals_with_host_pointers():
    """never dereferenced: every one of these calls is refused on the host first"""
    L = abi.lib()
    F = B * C * M * 4
    state, frame = ctypes.c_void_p(0x100000), ctypes.c_void_p(0x100000 + 3 * F)
    cont, cl = (C * M, M, B * C * M, 1, 0), (M * C, 1, B * M * C, C, 0)

    def rc(ss, fs, st=state, fr=frame, D=3):
        p = _problem(D)
        return L.shiftnd_forward(ctypes.byref(p), st, (ctypes.c_int64 * 5)(*ss), st, fr, (ctypes.c_int64 * 5)(*fs), None)

    assert rc((C * M * 2, M, B * C * M, 1, 0), cont) == -1      # neither dense form
    assert rc((C * M, M, B * C * M + 1, 1, 0), cont) == -1      # slots not one frame batch apart
    assert rc(cont, (C * M, M, 0, 2, 0)) == -1
    assert rc(cl, cont) == -1 and rc(cont, cl) == -1            # frame and state in different layouts
    for at in (0x100000, 0x100000 + F, 0x100000 + 3 * F - 4, 0x100000 - F + 4):   # the frame inside or across an end of the state
        assert rc(cont, cont, fr=ctypes.c_void_p(at)) == -1, hex(at)
    assert rc(cont, cont, st=ctypes.c_void_p(0x100002)) == -1   # a base off the element grid


def test_the_bit_alone_is_an_unknown_dtype_on_every_entry_point():
    L = abi.lib()
    st = (ctypes.c_int64 * 5)(C * M, M, B * C * M, 1, 0)
    pool = (ctypes.c_int32 * 2)(2, 2)
    sizes = (ctypes.c_int64 * 3)()
    for bit in (abi.STREAM, 0x800):
        p = _problem(3, flags=bit)
        q = _problem(3, abi.U8, flags=bit)
        assert L.shiftnd_forward(ctypes.byref(p), None, st, None, None, st, None) == -2
        assert L.shiftnd_forward_quantized(ctypes.byref(q), None, st, None, abi.I32, 0, 0, None, st, None) == -2
        assert L.shiftnd_backward(ctypes.byref(p), None, st, None, st, None, None, st, None, None, 0, None) == -2
        assert L.shiftnd_forward_pooled(ctypes.byref(p), pool, None, None, None, None) == -2
        assert L.shiftnd_backward_pooled(ctypes.byref(p), pool, None, None, None, None, None, None, 0, None) == -2
        assert L.shiftnd_forward_quantized_pooled(ctypes.byref(q), pool, None, None, abi.I32, 0, 0, 0, None, None) == -2
        assert L.shiftnd_pooled_sizes(ctypes.byref(p), pool, sizes) == -2
        assert L.shiftnd_forward_serves_channels_last(ctypes.byref(p), None, st, None, st) == 0
        assert L.shiftnd_backward_serves_channels_last(ctypes.byref(p), None, st, None, st, None, st) == 0
    # 0x800 beside SHIFT_DIM0 is still unknown, with and without the new bit
    assert _rc(3, extra=0x800) == -2 and _rc(3, abi.U8, True, extra=0x800) == -2
    assert L.shiftnd_forward(ctypes.byref(_problem(3, flags=abi.SHIFT_DIM0 | 0x800)), None, st, None, None, st, None) == -2
