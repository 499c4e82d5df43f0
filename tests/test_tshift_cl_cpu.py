"""Channels-last learnable temporal shift on CPU tensors: memory_format=torch.preserve_format in temporal_shift_learnable_func and
LearnableTemporalShift, the dispatcher ops temporal_shift_learnable_cl / _temporal_shift_learnable_cl_forward / _backward, and the
host-side validation of SHIFTND_SHIFT_DIM0 | SHIFTND_FRAMES at the C ABI.

The values and gradients are those of temporal_shift_learnable_func on x.contiguous() in every case (torch.equal: the CPU key runs
the same routine); what the option adds is the layout: a dense channels-last input comes back in the input's strides, x.grad in the
gradient's, anything else as today."""
import ctypes
import itertools

import pytest
import torch

import torchshifts
from torchshifts.functional import temporal_shift_learnable_func

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


def weights(C, frames, dtype, turn):
    """0, an integer, T + 1, -(T + 1), 0.5, -0.25 rotated by `turn`, then quarters up to |T + 1|"""
    special = [0.0, 2.0, frames + 1.0, -(frames + 1.0), 0.5, -0.25, frames + 0.75, -frames - 0.5]
    return torch.tensor([special[(i + turn) % len(special)] for i in range(C)], dtype=dtype).reshape(C, 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=lambda d: str(d).split(".")[-1])
def test_functional_and_ops_keep_the_layout(dtype):
    for x in channels_last_inputs(dtype):
        for frames, pad, active in itertools.product((1, 2), range(5), (False, True)):
            what = (tuple(x.shape), frames, pad, active)
            w = weights(x.shape[1], frames, dtype, pad)
            go = torch.randn(x.shape).to(dtype)
            go_cl = torch.empty_like(x).copy_(go)
            assert go_cl.stride() == x.stride()
            # the definition: the default call on x.contiguous()
            xr, wr = x.contiguous().requires_grad_(True), w.clone().requires_grad_(True)
            want = temporal_shift_learnable_func(xr, wr, frames, pad, active)
            want.backward(go)
            for grad in (go_cl, go):
                xa = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
                wa = w.clone().requires_grad_(True)
                assert xa.stride() == x.stride()
                out = temporal_shift_learnable_func(xa, wa, frames, pad, active, memory_format=KEEP)
                assert out.stride() == x.stride() and out.dtype == dtype and torch.equal(out, want), what
                out.backward(grad)
                # (a leaf's .grad is laid out by autograd's accumulation; the op's own rule -- a channels-last gradient gives a
                # channels-last grad_x, a contiguous one a contiguous grad_x -- is checked on the backward op below)
                assert torch.equal(xa.grad, xr.grad) and (grad is go or xa.grad.stride() == x.stride()), what
                assert wa.grad.shape == w.shape and wa.grad.dtype == dtype and torch.equal(wa.grad, wr.grad), what
            out = OPS.temporal_shift_learnable_cl(x, w, frames, pad, active)
            assert out.stride() == x.stride() and torch.equal(out, want), what
            gx, gw = OPS._temporal_shift_learnable_cl_backward(go_cl, w, x, frames, pad, active)
            assert gx.stride() == x.stride() and torch.equal(gx, xr.grad) and torch.equal(gw, wr.grad), what
            gx, gw = OPS._temporal_shift_learnable_cl_backward(go, w, x, frames, pad, active)
            today = OPS._temporal_shift_learnable_backward(go, w, x, frames, pad, active)[0]   # (contiguous unless T == 1)
            assert gx.stride() == today.stride() and (frames == 1 or gx.is_contiguous()), what
            assert torch.equal(gx, xr.grad) and torch.equal(gw, wr.grad), what
            # the default is today's call: a contiguous result from the channels-last input
            plain = temporal_shift_learnable_func(x, w, frames, pad, active)
            assert (frames == 1 or plain.is_contiguous()) and torch.equal(plain, want), what


def test_a_contiguous_input_gives_what_the_default_gives():
    g = torch.Generator().manual_seed(1)
    for shape, frames in (((6, 5, 4, 6), 3), ((6, 5, 7), 2), ((6, 5), 3), ((4, 5, 2, 3, 2), 2), ((6, 1, 4, 6), 2)):
        for pad, active in itertools.product(range(5), (False, True)):
            x = torch.randn(shape, generator=g)
            w = weights(shape[1], frames, torch.float32, pad)
            go = torch.randn(shape, generator=g)
            res = []
            for fmt in (torch.contiguous_format, KEEP):
                xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
                out = temporal_shift_learnable_func(xa, wa, frames, pad, active, memory_format=fmt)
                out.backward(go)
                res.append((out.detach(), xa.grad, wa.grad))
            for a, b in zip(*res):
                assert a.stride() == b.stride() and torch.equal(a, b), (shape, pad, active)


def test_a_bad_memory_format_raises():
    x, w = torch.randn(4, 3, 2, 2), torch.zeros(3)
    for fmt in (torch.channels_last, torch.channels_last_3d, None):
        with pytest.raises(AssertionError):
            temporal_shift_learnable_func(x, w, 2, memory_format=fmt)
        with pytest.raises(AssertionError):
            torchshifts.LearnableTemporalShift(2, 3, memory_format=fmt)


def test_the_node_keeps_the_input_as_it_lies_and_a_second_backward_raises():
    x = torch.randn(4, 3, 2, 5).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    w = torch.tensor([0.5, -1.25, 2.0], requires_grad=True)
    seen = []

    def pack(t):
        seen.append((t.data_ptr(), tuple(t.stride())))
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = temporal_shift_learnable_func(x, w, 2, 0, True, memory_format=KEEP)
    assert (x.data_ptr(), tuple(x.stride())) in seen and len(seen) == 2, seen   # the input itself and the weights
    g, _ = torch.autograd.grad(out, (x, w), torch.ones_like(out, requires_grad=True), create_graph=True)
    with pytest.raises(RuntimeError, match="double backwards"):
        g.sum().backward()


def test_the_module_carries_the_option():
    torch.manual_seed(3)
    plain = torchshifts.LearnableTemporalShift(2, 8, padding="border", init_shift=2, active_flag=True)
    keep = torchshifts.LearnableTemporalShift(2, 8, padding="border", init_shift=2, active_flag=True, memory_format=KEEP)
    assert plain.memory_format == torch.contiguous_format and keep.memory_format == KEEP
    assert list(keep.state_dict().keys()) == ["weight"] and list(plain.state_dict().keys()) == ["weight"]
    keep.load_state_dict(plain.state_dict())   # a checkpoint of a default module loads
    assert torch.equal(keep.weight, plain.weight)
    assert "memory_format=torch.preserve_format" in repr(keep) and "memory_format=torch.contiguous_format" in repr(plain)
    x = torch.randn(6, 8, 3, 4).contiguous(memory_format=torch.channels_last)
    (out, loss), (ref, ref_loss) = keep(x), plain(x)
    assert out.stride() == x.stride() and ref.is_contiguous() and torch.equal(out, ref) and torch.equal(loss, ref_loss)
    out.sum().backward()
    ref.sum().backward()
    assert torch.equal(keep.weight.grad, plain.weight.grad)
    # from_shift is unchanged: the fixed module's default
    frozen = torchshifts.TemporalShift.from_shift(torchshifts.LearnableTemporalShift(2, 8, memory_format=KEEP))
    assert frozen.memory_format == torch.contiguous_format


# ---- SHIFTND_SHIFT_DIM0 | SHIFTND_FRAMES at the C ABI, host side only: validation happens before any device work.  With NULL tensors an
# accepted geometry ends in INVALID_ARGUMENT (the tensors are refused); a refused dtype in UNSUPPORTED_DTYPE before that.
def _problem(ndim, dtype, sizes=(2, 5, 3, 8, 1), borders=(0, 3, 0, 8, 0, 1), active=0):
    from torchshifts import abi
    p = abi.Problem()
    p.ndim, p.dtype, p.padding_mode, p.active = ndim, dtype, 0, active
    for i, v in enumerate(sizes):
        p.sizes[i] = v
    for i, v in enumerate(borders):
        p.borders[i] = v
    return p


def test_the_frames_flag_host_side():
    from torchshifts import abi
    INVALID, UNSUPPORTED = -1, -2
    L = abi.lib()
    assert L.shiftnd_abi_version() == 5 and len(abi.EXPORTS) == 20
    assert abi.FRAMES == 0x400 and abi.SHIFT_DIM0 == 0x200 and abi.WEIGHTS_F32 == 0x100
    st = (ctypes.c_int64 * 5)(3 * 8 * 5, 1, 8 * 5, 5, 0)   # [N, C, T, M] = [2, 5, 3, 8] in memory order N, T, M, C
    byref = ctypes.byref
    BOTH = abi.SHIFT_DIM0 | abi.FRAMES

    def forward(p):
        return L.shiftnd_forward(byref(p), None, st, None, None, st, None)

    def backward(p):
        return L.shiftnd_backward(byref(p), None, st, None, st, None, None, st, None, None, 0, None)

    def workspace(p):
        return L.shiftnd_backward_workspace_bytes(byref(p))

    for dt in (abi.F32, abi.F64, abi.F16, abi.BF16, abi.F16 | abi.WEIGHTS_F32, abi.BF16 | abi.WEIGHTS_F32):
        for active in (0, 1):
            # accepted geometries: the NULL tensors are refused
            assert forward(_problem(2, dt | BOTH, active=active)) == INVALID
            assert backward(_problem(2, dt | BOTH, active=active)) == INVALID
            assert forward(_problem(3, dt | BOTH, sizes=(2, 5, 3, 4, 2), borders=(0, 3, 0, 4, 0, 2), active=active)) == INVALID
            assert workspace(_problem(2, dt | BOTH, active=active)) >= 2 * 5 * 24            # a record per clip and channel at least
            assert workspace(_problem(2, dt | BOTH, sizes=(0, 5, 3, 8, 1), active=active)) == 8   # an empty problem: sizeof(double)
            assert workspace(_problem(2, dt | BOTH, sizes=(2, 5, 3, 0, 1), borders=(0, 3, 0, 0, 0, 1), active=active)) == 8
            cut = _problem(2, dt | BOTH, borders=(1, 3, 0, 8, 0, 1), active=active)
            assert forward(cut) == INVALID and backward(cut) == INVALID and workspace(cut) == 0
            one = _problem(1, dt | BOTH, sizes=(2, 5, 24, 1, 1), borders=(0, 24, 0, 1, 0, 1), active=active)
            assert forward(one) == INVALID and backward(one) == INVALID and workspace(one) == 0
            # beyond the stated bounds: N * S0 of 2^31
            big = _problem(2, dt | BOTH, sizes=(1 << 20, 5, 1 << 11, 8, 1), borders=(0, 1 << 11, 0, 8, 0, 1), active=active)
            assert forward(big) == INVALID and backward(big) == INVALID and workspace(big) == 0
    # the plan is a function of the geometry alone: the same bytes for both modes and with fp32 weights
    assert len({workspace(_problem(2, dt | BOTH, active=a)) for dt in (abi.F16, abi.F16 | abi.WEIGHTS_F32, abi.BF16) for a in (0, 1)}) == 1
    for dt in (abi.U8, abi.I8, abi.I32, abi.F32 | abi.WEIGHTS_F32):
        p = _problem(2, dt | BOTH)
        assert forward(p) == UNSUPPORTED and backward(p) == UNSUPPORTED and workspace(p) == 0
        assert L.shiftnd_forward_quantized(byref(p), None, st, None, abi.I32, 0, 0, None, st, None) == UNSUPPORTED
    # the bit without SHIFT_DIM0 is an unknown dtype bit, as before the flag existed: UNSUPPORTED_DTYPE, and the workspace query answers
    # what it answers for any unknown bit (0x800 here)
    for dt in (abi.F32, abi.F16, abi.F16 | abi.WEIGHTS_F32, abi.U8):
        p, other = _problem(2, dt | abi.FRAMES), _problem(2, dt | 0x800)
        assert forward(p) == UNSUPPORTED and backward(p) == UNSUPPORTED
        assert L.shiftnd_forward_quantized(byref(p), None, st, None, abi.I32, 0, 0, None, st, None) == UNSUPPORTED
        assert workspace(p) == workspace(other)
    assert workspace(_problem(2, abi.F32 | abi.FRAMES)) == 512 and workspace(_problem(2, abi.F16 | abi.WEIGHTS_F32 | abi.FRAMES)) == 0
    # SHIFT_DIM0 alone on these strides keeps its answers: the sparse forward accepted, the interpolating one and the backward refused
    assert forward(_problem(2, abi.F32 | abi.SHIFT_DIM0)) == INVALID and backward(_problem(2, abi.F32 | abi.SHIFT_DIM0)) == INVALID
