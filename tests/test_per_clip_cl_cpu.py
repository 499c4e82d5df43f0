"""The channels-last per-clip temporal shift without a GPU: the op surface of torchshifts_per_clip_cl::, the values of
memory_format=torch.preserve_format on CPU tensors (the per-clip CPU routines laid into the argument's strides), the argument
handling of the functions and the modules, and SHIFTND_CLIP_FRAMES at the C ABI with NULL pointers (nothing can launch: the
validation happens before any device work).
"""
import ctypes

import pytest
import torch

import torchshifts
from torchshifts import abi
from torchshifts.functional import temporal_shift_learnable_per_clip_func, temporal_shift_per_clip_func

from test_temporal_abi_status import SIZES, problem_and_strides

KEEP = torch.preserve_format
NS = "torchshifts_per_clip_cl"
OPS = torch.ops.torchshifts_per_clip_cl

SCHEMAS = {
    "temporal_shift_learnable_per_clip_cl":
        "(Tensor input, Tensor weights, int n_segment, int padding_mode, bool active_flag) -> Tensor",
    "_temporal_shift_learnable_per_clip_cl_forward":
        "(Tensor input, Tensor weights, int n_segment, int padding_mode, bool active_flag) -> Tensor",
    "_temporal_shift_learnable_per_clip_cl_backward":
        "(Tensor grad, Tensor weights, Tensor input, int n_segment, int padding_mode, bool active_flag) -> (Tensor, Tensor)",
    "temporal_shift_per_clip_cl": "(Tensor input, Tensor shifts, int n_segment, int padding_mode) -> Tensor",
    "_temporal_shift_per_clip_cl_backward": "(Tensor grad, Tensor shifts, int n_segment, int padding_mode) -> Tensor",
}


# ---- the op surface ------------------------------------------------------------------------------------------------------
def test_the_namespace_holds_the_five_ops_and_no_other():
    names = sorted(n.split("::")[1] for n in torch._C._dispatch_get_all_op_names() if n.startswith(NS + "::"))
    assert names == sorted(SCHEMAS)
    for name, text in SCHEMAS.items():
        assert str(torch._C._get_schema(NS + "::" + name, "")) == "%s::%s%s" % (NS, name, text)
    # ... and the per-clip namespace keeps its own five
    plain = sorted(n.split("::")[1] for n in torch._C._dispatch_get_all_op_names() if n.startswith("torchshifts_per_clip::"))
    assert plain == sorted(n.replace("per_clip_cl", "per_clip") for n in SCHEMAS)


def test_the_dispatch_keys_mirror_the_per_clip_ops():
    has = torch._C._dispatch_has_kernel_for_dispatch_key
    public = NS + "::temporal_shift_learnable_per_clip_cl"
    assert has(public, "CompositeImplicitAutograd")
    for key in ("Autograd", "CPU", "CUDA"):
        assert not has(public, key), key
        for name in SCHEMAS:
            if name != "temporal_shift_learnable_per_clip_cl":
                assert has(NS + "::" + name, key), (name, key)
                assert has("torchshifts_per_clip::" + name.replace("per_clip_cl", "per_clip"), key), (name, key)


# ---- values on CPU tensors -----------------------------------------------------------------------------------------------
def _inputs(dt=torch.float32, seed=7):
    """(x, n_segment, what) in the three channels-last forms and contiguous"""
    gen = torch.Generator().manual_seed(seed)
    rnd = (lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).to(dt))
    return [(rnd(6, 6, 4, 5).contiguous(memory_format=torch.channels_last), 3, "channels_last"),
            (rnd(6, 6, 2, 3, 2).contiguous(memory_format=torch.channels_last_3d), 3, "channels_last_3d"),
            (rnd(6, 7, 6).permute(0, 2, 1), 2, "[N*T, C, L] with unit channel stride"),      # [6, 6, 7], strides (42, 1, 6)
            (rnd(6, 6, 4, 5), 3, "contiguous")]


def _table(x, T, groups=None, seed=8):
    gen = torch.Generator().manual_seed(seed)
    N, C = x.shape[0] // T, x.shape[1]
    return (torch.rand(N, groups or C, generator=gen, dtype=torch.float64) * 2 * (T + 1) - (T + 1)).to(x.dtype)


def _like(x, values):
    return torch.empty_strided(x.shape, x.stride(), dtype=x.dtype).copy_(values)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("groups", [None, 2], ids=["full table", "group table"])
def test_preserve_format_gives_the_default_values_in_the_arguments_strides(dt, groups):
    for (x0, T, what), pad, active in ((i, p, a) for i in _inputs(dt) for p in (0, 3) for a in (False, True)):
        keeps = what != "contiguous"
        w0 = _table(x0, T, groups)
        go = torch.randn(x0.shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64).to(dt)
        res = {}
        for fmt, grad in ((torch.contiguous_format, go), (KEEP, _like(x0, go) if keeps else go)):
            x, w = x0.clone(memory_format=KEEP).requires_grad_(True), w0.clone().requires_grad_(True)
            assert x.stride() == x0.stride()
            out = temporal_shift_learnable_per_clip_func(x, w, T, pad, active, memory_format=fmt)
            gx, gw = torch.autograd.grad(out, (x, w), grad)      # (x.grad itself is laid out by autograd, like its leaf)
            res[fmt] = (out.detach(), gx, gw)
        plain, kept = res[torch.contiguous_format], res[KEEP]
        assert plain[0].is_contiguous() and plain[1].is_contiguous(), what
        assert kept[0].stride() == (x0.stride() if keeps else plain[0].stride()), what
        assert kept[1].stride() == (x0.stride() if keeps else plain[1].stride()), (what, "x.grad in the gradient's strides")
        for a, b in zip(plain, kept):
            assert torch.equal(a, b), (what, pad, active)
        assert kept[2].shape == w0.shape and kept[2].dtype == dt      # a group table collects its channels' gradients
        # the fixed op
        s0 = torch.round(w0.float()).long()
        x = x0.clone(memory_format=KEEP).requires_grad_(True)
        out = temporal_shift_per_clip_func(x, s0, T, pad, memory_format=KEEP)
        gx, = torch.autograd.grad(out, x, _like(x0, go) if keeps else go)
        x2 = x0.clone(memory_format=KEEP).requires_grad_(True)
        ref = temporal_shift_per_clip_func(x2, s0, T, pad)
        gx2, = torch.autograd.grad(ref, x2, go)
        assert torch.equal(out, ref) and torch.equal(gx, gx2) and ref.is_contiguous() and gx2.is_contiguous(), what
        assert out.stride() == (x0.stride() if keeps else ref.stride()) and gx.stride() == out.stride(), what


def test_a_group_table_collects_its_channels_gradients():
    x0, T, _ = _inputs(torch.float64)[0]
    g0 = _table(x0, T, groups=3)
    go = _like(x0, torch.randn(x0.shape, generator=torch.Generator().manual_seed(10), dtype=torch.float64))
    g = g0.clone().requires_grad_(True)
    temporal_shift_learnable_per_clip_func(x0, g, T, 0, True, memory_format=KEEP).backward(go)
    full = g0.repeat_interleave(2, dim=1).requires_grad_(True)
    temporal_shift_learnable_per_clip_func(x0, full, T, 0, True, memory_format=KEEP).backward(go)
    assert torch.allclose(g.grad, full.grad.view(2, 3, 2).sum(2), rtol=1e-12, atol=1e-12) and g.grad.abs().sum() > 0


def test_gradcheck_on_the_interpolating_op():
    """in the table, under every padding.  (In the input the project's grad_x is the reference's rule, which is the adjoint only where
    tests/test_tshift_cpu.py::test_gradcheck says so -- T = 2 under periodic and reflect padding -- so the input is checked there.)"""
    N, T, C, M = 2, 3, 4, 2
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(N * T, C, M, 1, generator=gen, dtype=torch.float64).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    # (away from the integers, where the interpolation has a kink)
    w = (torch.randint(-3, 3, (N, C), generator=gen).double() + 0.25 + 0.5 * torch.rand(N, C, generator=gen, dtype=torch.float64)).requires_grad_(True)
    assert x.stride(1) == 1 and not x.is_contiguous()
    xd = x.detach()
    for pad in range(5):
        assert torch.autograd.gradcheck(lambda b: OPS.temporal_shift_learnable_per_clip_cl(xd, b, T, pad, True), (w,), eps=1e-6, atol=1e-6)
    x2 = torch.randn(N * 2, C, M, 1, generator=gen, dtype=torch.float64).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    for pad in (2, 3):
        assert torch.autograd.gradcheck(lambda a, b: OPS.temporal_shift_learnable_per_clip_cl(a, b, 2, pad, True), (x2, w), eps=1e-6, atol=1e-6)


# ---- argument handling ------------------------------------------------------------------------------------------------------
def test_a_wrong_memory_format_raises():
    x, w = torch.zeros(6, 4, 2, 2), torch.zeros(2, 4)
    for fmt in (torch.channels_last, torch.channels_last_3d, None):
        with pytest.raises(AssertionError, match="expected memory_format to be torch.contiguous_format or torch.preserve_format"):
            temporal_shift_learnable_per_clip_func(x, w, 3, 0, True, memory_format=fmt)
        with pytest.raises(AssertionError, match="expected memory_format to be torch.contiguous_format or torch.preserve_format"):
            temporal_shift_per_clip_func(x, w.long(), 3, 0, memory_format=fmt)
        with pytest.raises(AssertionError, match="memory_format must be"):
            torchshifts.PerClipTemporalShift(3, memory_format=fmt)
        with pytest.raises(AssertionError, match="memory_format must be"):
            torchshifts.LearnablePerClipTemporalShift(3, memory_format=fmt)
    # the keyword comes last
    assert torch.equal(temporal_shift_per_clip_func(x, w.long(), 3, 0, KEEP), x)
    assert torch.equal(temporal_shift_learnable_per_clip_func(x, w, 3, 0, False, KEEP), x)


def test_the_modules_carry_the_attribute():
    fixed = torchshifts.PerClipTemporalShift(4, padding="border", memory_format=KEEP)
    learn = torchshifts.LearnablePerClipTemporalShift(4, padding="reflect", active_flag=True, memory_format=KEEP)
    for m in (fixed, learn):
        assert m.memory_format == KEEP and len(m.state_dict()) == 0 and not list(m.parameters()) and not list(m.buffers())
    assert repr(fixed) == "PerClipTemporalShift(n_segment=4, padding_method=border, per-clip integer shifts, memory_format=torch.preserve_format)"
    assert repr(learn) == ("LearnablePerClipTemporalShift(n_segment=4, padding_method=reflect, Active shift on forward pass: Yes, "
                           "per-clip weights, memory_format=torch.preserve_format)")
    # the defaults: the attribute is there, the reprs are what they were
    d_fixed, d_learn = torchshifts.PerClipTemporalShift(4, padding="border"), torchshifts.LearnablePerClipTemporalShift(4, "reflect", True)
    assert d_fixed.memory_format == d_learn.memory_format == torch.contiguous_format
    assert repr(d_fixed) == "PerClipTemporalShift(n_segment=4, padding_method=border, per-clip integer shifts)"
    assert repr(d_learn) == ("LearnablePerClipTemporalShift(n_segment=4, padding_method=reflect, Active shift on forward pass: Yes, "
                             "per-clip weights)")
    x = torch.randn(8, 6, 3, 3, generator=torch.Generator().manual_seed(12)).contiguous(memory_format=torch.channels_last)
    w = _table(x, 4)
    out = learn(x, w)
    assert out.stride() == x.stride() and torch.equal(out, d_learn(x, w)) and d_learn(x, w).is_contiguous()
    s = torch.round(w).long()
    assert fixed(x, s).stride() == x.stride() and torch.equal(fixed(x, s), d_fixed(x, s)) and d_fixed(x, s).is_contiguous()


# ---- SHIFTND_CLIP_FRAMES at the C ABI, host side only --------------------------------------------------------------------------
INVALID, UNSUPPORTED = -1, -2
N, C, T, M = 2, 5, 3, 8
NHWC = (T * M * C, 1, M * C, C, 0)          # [N, C, T, M] in memory order N, T, M, C
SEGMENT = (T * C * M, M, C * M, 1, 0)       # ... in memory order N, T, C, M
FLOATS = (abi.F32, abi.F64, abi.F16, abi.BF16, abi.F16 | abi.WEIGHTS_F32, abi.BF16 | abi.WEIGHTS_F32)
DIM0, CF = abi.SHIFT_DIM0, abi.CLIP_FRAMES


def _problem(ndim, dtype, sizes=(N, C, T, M, 1), borders=(0, T, 0, M, 0, 1), active=0):
    p = abi.Problem()
    p.ndim, p.dtype, p.padding_mode, p.active = ndim, dtype, 0, active
    for i, v in enumerate(sizes):
        p.sizes[i] = v
    for i, v in enumerate(borders):
        p.borders[i] = v
    return p


def _st(strides):
    return (ctypes.c_int64 * 5)(*strides)


def _forward(p, x=None, out=None, s=NHWC):
    return abi.lib().shiftnd_forward(ctypes.byref(p), x, _st(s), None, out, _st(s), None)


def _backward(p, s=NHWC, go=None, x=None, gx=None, gw=None, w=None):
    return abi.lib().shiftnd_backward(ctypes.byref(p), go, _st(s), x, _st(s), w, gx, _st(s), gw, None, 0, None)


def _workspace(p):
    return int(abi.lib().shiftnd_backward_workspace_bytes(ctypes.byref(p)))


def test_the_constant_and_the_keyword():
    assert abi.CLIP_FRAMES == 0x4000 and abi.lib().shiftnd_abi_version() == 5 and len(abi.EXPORTS) == 20
    x = torch.zeros(N, C, T, M)
    assert abi.problem(x, 0, 0, None, shift_dim0=True, clip_frames=True).dtype == 0x4200
    assert abi.problem(x, 0, 0, None, shift_dim0=True).dtype == 0x200
    assert abi.problem(x.half(), 0, 0, None, w=torch.zeros(N, C), shift_dim0=True, clip_frames=True).dtype == abi.F16 | 0x4300
    import inspect
    for fn in (abi.problem, abi.forward, abi.backward_workspace, abi.backward):
        assert inspect.signature(fn).parameters["clip_frames"].default is False, fn.__name__


def test_the_bit_alone_is_an_unknown_dtype_on_every_entry_point():
    L = abi.lib()
    st = _st(NHWC)
    pool = (ctypes.c_int32 * 2)(2, 2)
    sizes = (ctypes.c_int64 * 3)()
    for dt in FLOATS:
        p = _problem(2, dt | CF)
        q = _problem(2, abi.U8 | CF)
        assert _forward(p) == UNSUPPORTED and _backward(p) == UNSUPPORTED and _workspace(p) == 0
        assert L.shiftnd_forward_quantized(ctypes.byref(q), None, st, None, abi.I32, 0, 0, None, st, None) == UNSUPPORTED
        assert L.shiftnd_forward_pooled(ctypes.byref(p), pool, None, None, None, None) == UNSUPPORTED
        assert L.shiftnd_backward_pooled(ctypes.byref(p), pool, None, None, None, None, None, None, 0, None) == UNSUPPORTED
        assert L.shiftnd_forward_quantized_pooled(ctypes.byref(q), pool, None, None, abi.I32, 0, 0, 0, None, None) == UNSUPPORTED
        assert L.shiftnd_pooled_sizes(ctypes.byref(p), pool, sizes) == UNSUPPORTED
        assert L.shiftnd_forward_serves_channels_last(ctypes.byref(p), None, st, None, st) == 0
        assert L.shiftnd_backward_serves_channels_last(ctypes.byref(p), None, st, None, st, None, st) == 0
        # ... and with SHIFT_DIM0 on the quantized and the pooled entry points
        ok = _problem(2, dt | DIM0 | CF)
        assert L.shiftnd_forward_quantized(ctypes.byref(ok), None, st, None, abi.I32, 0, 0, None, st, None) == UNSUPPORTED
        assert L.shiftnd_forward_pooled(ctypes.byref(ok), pool, None, None, None, None) == UNSUPPORTED
        assert L.shiftnd_backward_pooled(ctypes.byref(ok), pool, None, None, None, None, None, None, 0, None) == UNSUPPORTED
    # 0x800 stays unassigned, beside the new bit too
    assert _forward(_problem(2, abi.F32 | DIM0 | CF | 0x800)) == UNSUPPORTED and _workspace(_problem(2, abi.F32 | DIM0 | CF | 0x800)) == 0


@pytest.mark.parametrize("active", (0, 1))
def test_what_is_refused_and_what_is_accepted(active):
    for dt in FLOATS:
        ok = _problem(2, dt | DIM0 | CF, active=active)
        # accepted: with NULL tensors the call ends in INVALID_ARGUMENT, but the workspace query answers the FRAMES plan's bytes
        assert _forward(ok) == INVALID and _backward(ok) == INVALID
        assert _workspace(ok) == _workspace(_problem(2, dt | DIM0 | abi.FRAMES, active=active)) >= N * C * 24
        three = dict(sizes=(N, C, T, 2, 4), borders=(0, T, 0, 2, 0, 4), active=active)
        assert _workspace(_problem(3, dt | DIM0 | CF, **three)) == _workspace(_problem(3, dt | DIM0 | abi.FRAMES, **three)) > 0
        # beside FRAMES, PER_CLIP or STREAM
        for other in (abi.FRAMES, abi.PER_CLIP, abi.STREAM, abi.FRAMES | abi.PER_CLIP):
            both = _problem(2, dt | DIM0 | CF | other, active=active)
            for s in (NHWC, SEGMENT):
                assert _forward(both, s=s) == INVALID and _backward(both, s=s) == INVALID, (dt, other)
            assert _workspace(both) == 0, (dt, other)
        # what the neighbours answer is what they answered
        assert _workspace(_problem(2, dt | DIM0 | abi.FRAMES | abi.PER_CLIP, active=active)) == 0
        assert _workspace(_problem(2, dt | DIM0 | abi.PER_CLIP, active=active)) == _workspace(_problem(2, dt | DIM0, active=active)) > 0
        # out == x: refused before the pointer is looked at (4096 is no allocation)
        assert _forward(ok, x=ctypes.c_void_p(4096), out=ctypes.c_void_p(4096)) == INVALID
        # ndim 1, a cut window
        one = _problem(1, dt | DIM0 | CF, sizes=(N, C, T * M, 1, 1), borders=(0, T * M, 0, 1, 0, 1), active=active)
        assert _forward(one, s=(T * M * C, 1, C, 0, 0)) == INVALID and _backward(one, s=(T * M * C, 1, C, 0, 0)) == INVALID and _workspace(one) == 0
        cut = _problem(2, dt | DIM0 | CF, borders=(1, T, 0, M, 0, 1), active=active)
        assert _forward(cut) == INVALID and _backward(cut) == INVALID and _workspace(cut) == 0
        # N * C = 2^31 (every other factor is 1, so nothing else is large); one row fewer is accepted
        wide = dict(borders=(0, 1, 0, 1, 0, 1), active=active)
        assert _workspace(_problem(2, dt | DIM0 | CF, sizes=(1 << 16, 1 << 15, 1, 1, 1), **wide)) == 0
        assert _forward(_problem(2, dt | DIM0 | CF, sizes=(1 << 16, 1 << 15, 1, 1, 1), **wide), s=(1 << 15, 1, 1 << 15, 1 << 15, 0)) == INVALID
        assert _workspace(_problem(2, dt | DIM0 | abi.FRAMES, sizes=(1 << 16, 1 << 15, 1, 1, 1), **wide)) > 0
        assert _workspace(_problem(2, dt | DIM0 | CF, sizes=((1 << 16) - 1, 1 << 15, 1, 1, 1), **wide)) > 0
        # an empty problem is OK: sizeof(double) of workspace, the forward answers before it looks at a pointer
        for sizes in ((0, C, T, M, 1), (N, 0, T, M, 1), (N, C, T, 0, 1)):
            empty = _problem(2, dt | DIM0 | CF, sizes=sizes, borders=(0, T, 0, sizes[3], 0, 1), active=active)
            assert _workspace(empty) == 8 and _forward(empty) == 0 and abi.last_path() == abi.PATH_EMPTY
    # a quantized dtype
    for dt in (abi.I8, abi.U8, abi.I32):
        q = _problem(2, dt | DIM0 | CF, active=active)
        assert _forward(q) == UNSUPPORTED and _backward(q) == UNSUPPORTED and _workspace(q) == 0
        assert _forward(q, x=ctypes.c_void_p(4096), out=ctypes.c_void_p(4096)) == UNSUPPORTED


@pytest.mark.parametrize("active", (0, 1))
def test_segment_major_strides_and_null_forms_with_host_pointers(active):
    """never dereferenced: every one of these calls is refused on the host first"""
    p = _problem(2, abi.F32 | DIM0 | CF, active=active)
    a, b, c, d, e = (ctypes.c_void_p(0x100000 + i * 0x10000) for i in range(5))
    L = abi.lib()
    # segment-major and NCHW-dense strides in any one position
    for other in (SEGMENT, (C * T * M, T * M, M, 1, 0)):
        assert L.shiftnd_forward(ctypes.byref(p), a, _st(other), c, b, _st(NHWC), None) == INVALID
        assert L.shiftnd_forward(ctypes.byref(p), a, _st(NHWC), c, b, _st(other), None) == INVALID
        for k in range(3):
            sts = [_st(other if i == k else NHWC) for i in range(3)]
            assert L.shiftnd_backward(ctypes.byref(p), a, sts[0], b, sts[1], c, d, sts[2], e, e, 1 << 20, None) == INVALID
    # a base off the element grid
    assert L.shiftnd_forward(ctypes.byref(p), ctypes.c_void_p(0x100002), _st(NHWC), c, b, _st(NHWC), None) == INVALID
    # the x == NULL form of the backward, with and without grad_w
    assert L.shiftnd_backward(ctypes.byref(p), a, _st(NHWC), None, None, c, d, _st(NHWC), None, e, 1 << 20, None) == INVALID
    assert L.shiftnd_backward(ctypes.byref(p), a, _st(NHWC), None, _st(NHWC), c, d, _st(NHWC), e, e, 1 << 20, None) == INVALID
    # a workspace one byte short
    need = _workspace(p)
    assert L.shiftnd_backward(ctypes.byref(p), a, _st(NHWC), b, _st(NHWC), c, d, _st(NHWC), e, e, need - 1, None) == -3


def test_the_workspace_query_is_the_frames_query_on_the_recorded_sizes():
    """the sizes of tests/test_temporal_abi_status.py: the bytes of SHIFT_DIM0 | FRAMES for the same geometry, except where N * C is 2^31"""
    seen = 0
    for size in SIZES:
        dims = (1, 2, 3) if 0 in size[:3] else (2, 3)
        for dt in (abi.F32, abi.F64, abi.F16, abi.BF16, abi.BF16 | abi.WEIGHTS_F32):
            for nd in dims:
                for active, pad in ((0, 0), (1, 4)):
                    ours = problem_and_strides(dt | DIM0 | CF, nd, active, pad, size)[0]
                    theirs = problem_and_strides(dt | DIM0 | abi.FRAMES, nd, active, pad, size)[0]
                    want = 0 if size[0] * size[1] >= 1 << 31 else _workspace(theirs)
                    assert _workspace(ours) == want, (size, dt, nd, active)
                    seen += want > 0
        for dt in (abi.I8, abi.U8, abi.I32):
            assert _workspace(problem_and_strides(dt | DIM0 | CF, 2, 0, 0, size)[0]) == 0
    assert seen > 100
