"""Channels-last quantized interpolating temporal shift on the CPU:
torch.ops.torchshifts_quantized_learnable_cl.temporal_shift_learnable_quantized_cl (QuantizedCPU key), memory_format= of the
functional wrapper and of torchshifts.quantized.LearnableTemporalShift, and SHIFTND_SHIFT_DIM0 | SHIFTND_FRAMES with an fp32 table
at the C ABI with NULL tensors (nothing can launch: the validation happens before any device work).

No new arithmetic: for a dense channels-last input the new route returns the values of temporal_shift_learnable_quantized, bit for
bit, in the input's strides; every other input, and the default memory_format, is exactly the existing call.  The reference is
tests/test_qtshift_cpu.py's `definition`; every comparison is bit for bit.
"""
import ctypes

import numpy as np
import pytest
import torch

import torchshifts
from torchshifts import LearnableTemporalShift, abi
from torchshifts.quantized.functional import temporal_shift_learnable_quantized, temporal_shift_quantized

from test_qtshift_cpu import QDT, definition, quantized, tables

NS = "torchshifts_quantized_learnable_cl"
OP = torch.ops.torchshifts_quantized_learnable_cl.temporal_shift_learnable_quantized_cl
PLAIN = torch.ops.torchshifts_quantized_learnable.temporal_shift_learnable_quantized
QLTS = torchshifts.quantized.LearnableTemporalShift
PRESERVE = torch.preserve_format

# (shape, T): channels-last inputs of 3, 4 and 5 dims
SHAPES = [((2 * 3, 5, 4), 3), ((2 * 5, 3, 2, 3), 5), ((2 * 3, 4, 2, 2, 3), 3)]


def channels_last(x):
    """the same quantized values in memory order (dim 0, spatial dims, channels), seen with the channels as dim 1"""
    order = [0] + list(range(2, x.dim())) + [1]
    back = [0, x.dim() - 1] + list(range(1, x.dim() - 1))
    r = x.int_repr().permute(order).contiguous()
    out = torch._make_per_tensor_quantized_tensor(r, x.q_scale(), x.q_zero_point()).permute(back)
    assert out.stride(1) == 1 and not out.is_contiguous() and torch.equal(out.int_repr(), x.int_repr())
    return out


def test_the_op_set_schema_and_keys_are_pinned():
    names = {n.split("::")[1] for n in torch._C._dispatch_get_all_op_names() if n.startswith(NS + "::")}
    assert names == {"temporal_shift_learnable_quantized_cl"}
    assert str(torch._C._get_schema(NS + "::temporal_shift_learnable_quantized_cl", "")) == \
        (NS + "::temporal_shift_learnable_quantized_cl(Tensor input, Tensor weights, int n_segment, int padding_mode, "
         "bool active_flag) -> Tensor")
    all_keys = ["CPU", "CUDA", "QuantizedCPU", "QuantizedCUDA", "Autograd", "AutogradCPU", "AutogradCUDA", "CompositeImplicitAutograd",
                "CompositeExplicitAutograd", "Meta", "ADInplaceOrView", "SparseCPU", "SparseCUDA"]
    keys = {k for k in all_keys if torch._C._dispatch_has_kernel_for_dispatch_key(NS + "::temporal_shift_learnable_quantized_cl", k)}
    assert keys == {"QuantizedCPU", "QuantizedCUDA"}


@pytest.mark.parametrize("qdt", list(QDT), ids=lambda d: str(d).split(".")[-1])
def test_channels_last_inputs_keep_their_strides_and_the_values(qdt):
    rs = np.random.RandomState(81)
    for shape, T in SHAPES:
        for pad in range(5):
            x = quantized(rs, shape, qdt)
            xcl = channels_last(x)
            for w in tables(shape[1], T)[:3]:
                want = PLAIN(x, w, T, pad, True)
                assert torch.equal(want.int_repr(), definition(x, w, T, pad))
                for out in (OP(xcl, w, T, pad, True), temporal_shift_learnable_quantized(xcl, w.view(-1, 1), T, pad, True, memory_format=PRESERVE)):
                    assert out.stride() == xcl.stride() and out.shape == x.shape and out.dtype == qdt, (shape, pad)
                    assert out.q_scale() == x.q_scale() and out.q_zero_point() == x.q_zero_point()
                    assert torch.equal(out.int_repr(), want.int_repr()), (shape, pad, w.tolist())


def test_torch_memory_formats_are_dense_channels_last():
    rs = np.random.RandomState(82)
    w4, w5 = tables(5, 3)[1], tables(4, 3)[1]
    x4 = quantized(rs, (6, 5, 3, 2), torch.quint8).contiguous(memory_format=torch.channels_last)
    x5 = quantized(rs, (6, 4, 2, 3, 2), torch.qint8).contiguous(memory_format=torch.channels_last_3d)
    for x, w in ((x4, w4), (x5, w5)):
        out = OP(x, w, 3, 0, True)
        assert out.stride() == x.stride() and torch.equal(out.int_repr(), PLAIN(x, w, 3, 0, True).int_repr())


@pytest.mark.parametrize("qdt", list(QDT), ids=lambda d: str(d).split(".")[-1])
def test_every_other_input_and_the_default_are_the_existing_call(qdt):
    rs = np.random.RandomState(83)
    x = quantized(rs, (6, 4, 3, 5), qdt)
    w = torch.tensor([0.25, -1.5, 3.75, 0.0])
    for pad in range(5):
        want = PLAIN(x, w, 3, pad, True)
        # a contiguous input under the new op and under preserve_format
        for out in (OP(x, w, 3, pad, True), temporal_shift_learnable_quantized(x, w, 3, pad, True, memory_format=PRESERVE)):
            assert out.is_contiguous() and torch.equal(out.int_repr(), want.int_repr())
        # a view that is not dense (every second pixel column of a channels-last tensor)
        wide = channels_last(quantized(rs, (6, 4, 3, 10), qdt))
        view = wide[..., ::2]
        assert view.stride(1) == 1 and not view.is_contiguous()
        out = OP(view, w, 3, pad, True)
        assert out.is_contiguous() and torch.equal(out.int_repr(), PLAIN(view, w, 3, pad, True).int_repr())
        # the default memory_format on a channels-last input: the contiguous result
        xcl = channels_last(x)
        for out in (temporal_shift_learnable_quantized(xcl, w, 3, pad), temporal_shift_learnable_quantized(xcl, w, 3, pad, True, torch.contiguous_format)):
            assert out.is_contiguous() and torch.equal(out.int_repr(), want.int_repr())
    empty = torch._make_per_tensor_quantized_tensor(torch.zeros(0, 4, 3, dtype=x.int_repr().dtype), 0.125, 3)
    out = OP(empty, w, 3, 0, True)
    assert out.shape == empty.shape and out.dtype == qdt and out.q_zero_point() == 3


@pytest.mark.parametrize("qdt", list(QDT), ids=lambda d: str(d).split(".")[-1])
def test_sparse_mode_is_temporal_shift_quantized_preserving(qdt):
    rs = np.random.RandomState(84)
    for shape, T in SHAPES:
        for pad in range(5):
            xcl = channels_last(quantized(rs, shape, qdt))
            for w in tables(shape[1], T)[:3]:
                want = temporal_shift_quantized(xcl, w, T, pad, memory_format=PRESERVE)
                for out in (OP(xcl, w, T, pad, False), temporal_shift_learnable_quantized(xcl, w, T, pad, False, memory_format=PRESERVE)):
                    assert out.stride() == want.stride() == xcl.stride() and torch.equal(out.int_repr(), want.int_repr()), (shape, pad)


# ---- the module --------------------------------------------------------------------------------------------------------------------------
def test_the_module_keyword():
    rs = np.random.RandomState(85)
    default = QLTS(3, 4, padding="border")
    assert default.memory_format == torch.contiguous_format
    assert repr(default) == ("QuantizedLearnableTemporalShift(n_segment=3, in_channels=4, padding_method=border, "
                             "Active shift on forward pass: Yes)")   # (the repr before the keyword existed)
    m = QLTS(3, 4, padding="border", active_flag=True, memory_format=PRESERVE)
    assert m.memory_format == PRESERVE and "memory_format=torch.preserve_format" in repr(m)
    assert list(m.state_dict()) == ["weight"] and not list(m.parameters())
    m.weight.copy_(torch.tensor([[0.25], [-1.5], [3.75], [0.0]]))
    default.load_state_dict(m.state_dict())
    x = quantized(rs, (6, 4, 3, 5), torch.quint8)
    xcl = channels_last(x)
    out, plain = m(xcl), default(xcl)
    assert out.stride() == xcl.stride() and plain.is_contiguous() and torch.equal(out.int_repr(), plain.int_repr())
    assert m(x).is_contiguous() and torch.equal(m(x).int_repr(), plain.int_repr())
    for bad in (torch.channels_last, torch.channels_last_3d, None, "preserve"):
        with pytest.raises(AssertionError, match="memory_format must be torch.contiguous_format or torch.preserve_format"):
            QLTS(3, 4, memory_format=bad)
        with pytest.raises(AssertionError, match="temporal_shift_learnable_quantized expected memory_format"):
            temporal_shift_learnable_quantized(x, m.weight, 3, 0, True, bad)


def test_from_float_carries_the_option():
    rs = np.random.RandomState(86)
    x = channels_last(quantized(rs, (8, 8, 3, 3), torch.qint8))
    for fmt in (torch.contiguous_format, PRESERVE):
        for active in (True, False):
            f = LearnableTemporalShift(4, 8, padding="reflect", init_shift=3, sparsity_term=0., active_flag=active, memory_format=fmt)
            with torch.no_grad():
                f.weight.copy_(torch.from_numpy(rs.uniform(-5, 5, size=(8, 1)).astype(np.float32)))
            q = QLTS.from_float(f)
            assert q.memory_format == fmt and q._active_flag is active and list(q.state_dict()) == ["weight"]
            out = q(x)
            assert (out.stride() == x.stride()) == (fmt == PRESERVE) and out.is_contiguous() == (fmt != PRESERVE)
            assert torch.equal(out.int_repr(), PLAIN(x, f.weight.detach(), 4, 3, active).int_repr())


def test_refusals_and_their_messages():
    x = channels_last(quantized(np.random.RandomState(87), (6, 4, 3), torch.quint8))
    w = torch.zeros(4)
    OP(x, w, 3, 0, True)
    name = "temporal_shift_learnable_quantized_cl: "
    with pytest.raises(ValueError, match="Input to 'temporal_shift_learnable_quantized' must be quantized!"):
        temporal_shift_learnable_quantized(torch.zeros(6, 4, 3), w, 3, memory_format=PRESERVE)
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


# ---- SHIFTND_SHIFT_DIM0 | SHIFTND_FRAMES with an fp32 table at the C ABI, host side only.  With NULL tensors an accepted geometry ends
# in INVALID_ARGUMENT at the NULL check, an empty one in OK before it; what is refused earlier says so before either.
OK, INVALID, UNSUPPORTED = 0, -1, -2
PAIR = abi.SHIFT_DIM0 | abi.FRAMES


def _problem(ndim, dtype, ncTM=(2, 5, 3, 8), window=None, active=1, pad=0):
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
    st = [t * m * c, 1, m * c] + ([c] if ndim == 2 else [inner[1] * c, c])   # memory order N, T, M, C
    return p, (ctypes.c_int64 * 5)(*(st + [0] * (5 - len(st))))


def _quantized(p, st, wkind=abi.F32, wzp=0, x=None, out=None):
    return abi.lib().shiftnd_forward_quantized(ctypes.byref(p), x, st, None, wkind, wzp, 0, out, st, None)


@pytest.mark.parametrize("ndim", [2, 3])
def test_the_flag_pair_with_a_float_table_host_side(ndim):
    assert abi.lib().shiftnd_abi_version() == 5
    for dt in (abi.U8, abi.I8, abi.I32):
        for pad in range(5):
            assert _quantized(*_problem(ndim, dt | PAIR, pad=pad)) == INVALID          # accepted up to the NULL tensors ...
        for k in range(3):                                                             # ... which an empty problem never reaches
            size = tuple(0 if i == k else v for i, v in enumerate((2, 5, 3, 8)))
            assert _quantized(*_problem(ndim, dt | PAIR, size)) == OK, size
            # (what tells the accepted pair from a refused one: an extra bit is refused before the sizes are looked at)
            assert _quantized(*_problem(ndim, dt | PAIR | abi.PER_CLIP, size)) == INVALID, size
        assert _quantized(*_problem(ndim, dt | PAIR, active=0)) == UNSUPPORTED
        assert _quantized(*_problem(ndim, dt | PAIR, (0, 5, 3, 8), active=0)) == UNSUPPORTED
        for extra in (abi.PER_CLIP, abi.STREAM, abi.CLIP_FRAMES, abi.INTERLACE, abi.INTERLACE_FRAMES):
            assert _quantized(*_problem(ndim, dt | PAIR | extra, (0, 5, 3, 8))) == INVALID, extra
        assert _quantized(*_problem(ndim, dt | PAIR | abi.WEIGHTS_F32, (0, 5, 3, 8))) == INVALID
        assert _quantized(*_problem(ndim, dt | PAIR, (0, 5, 3, 8), window=(1, 3))) == INVALID     # a cut window, empty or not
        assert _quantized(*_problem(ndim, dt | PAIR, window=(1, 3))) == INVALID
        assert _quantized(*_problem(ndim, dt | PAIR, (0, 5, 3, 8)), wzp=1) == INVALID             # a nonzero w_zero_point
        same = ctypes.c_void_p(4096)
        assert _quantized(*_problem(ndim, dt | PAIR, (0, 5, 3, 8)), x=same, out=same) == INVALID   # out == x
        # the integer table's calls are what they were: the sparse shift under the flag alone, FRAMES an unknown bit beside it
        assert _quantized(*_problem(ndim, dt | abi.SHIFT_DIM0, (0, 5, 3, 8), active=0), wkind=abi.I32) == OK
        assert _quantized(*_problem(ndim, dt | PAIR, (0, 5, 3, 8), active=0), wkind=abi.I32) == UNSUPPORTED
    for dt in (abi.F32, abi.F16):
        assert _quantized(*_problem(ndim, dt | PAIR, (0, 5, 3, 8))) == UNSUPPORTED    # a float dtype
    p, st = _problem(ndim, abi.U8 | PAIR, (0, 5, 3, 8))
    assert abi.lib().shiftnd_forward_quantized(ctypes.byref(p), None, st, None, abi.F32, 0, 256, None, st, None) == INVALID   # the zero point's range
