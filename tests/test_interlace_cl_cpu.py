"""Channels-last temporal interlacing without a GPU: memory_format=torch.preserve_format of temporal_interlace_func and
TemporalInterlace on CPU tensors (the definition on the channels-last per-clip ops, laid into the argument's strides), the surface of
torchshifts_interlace_cl::, and SHIFTND_INTERLACE_FRAMES at the C ABI with NULL pointers (nothing can launch: the validation
happens before any device work).

The composition the op is compared with is the one a channels-last user had before it:
    temporal_shift_learnable_per_clip_func(x, offsets, T, pad, active, memory_format=torch.preserve_format) * scales
"""
import ctypes
import inspect
import itertools

import pytest
import torch

import torchshifts
from torchshifts import abi
from torchshifts.functional import temporal_interlace_func, temporal_shift_learnable_per_clip_func

from test_binding_surface import COMPOSITE, FLOAT, KEYS, registered_ops
from test_interlace_cpu import INTERLACE_SCHEMAS, TIN_BWD, TIN_FWD
from test_per_clip_cl_cpu import FLOATS, INVALID, NHWC, SEGMENT, UNSUPPORTED, _backward, _forward, _inputs, _like, _problem, _st, _workspace
from test_per_clip_cpu import _saved_shapes, _table

KEEP = torch.preserve_format
NS = "torchshifts_interlace_cl"
OPS = torch.ops.torchshifts_interlace_cl
DIM0, ILF = abi.SHIFT_DIM0, abi.INTERLACE_FRAMES
N, C, T, M = 2, 5, 3, 8          # the geometry of test_per_clip_cl_cpu._problem


def _composition(x, offsets, scales, T, pad, active):
    y = temporal_shift_learnable_per_clip_func(x, offsets, T, pad, active, memory_format=KEEP)
    return y * scales.reshape((x.shape[0], x.shape[1]) + (1,) * (x.dim() - 2))


def _tables(x, T, dt, seed):
    gen = torch.Generator().manual_seed(seed)
    N, C = x.shape[0] // T, x.shape[1]
    return _table(gen, N, C, T, dt), torch.randn(N, T, C, generator=gen, dtype=torch.float64).to(dt)


# ---- values and gradients ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["float32", "float64"])
def test_preserve_format_gives_the_default_values_and_the_compositions_gradients(dt):
    """3-, 4- and 5-D channels-last inputs and a contiguous one, every padding, both modes"""
    for (x0, T, what), pad, active in itertools.product(_inputs(dt, seed=61), range(5), (False, True)):
        keeps = what != "contiguous"
        w0, s0 = _tables(x0, T, dt, 62)
        go = torch.randn(x0.shape, generator=torch.Generator().manual_seed(63), dtype=torch.float64).to(dt)
        grad = _like(x0, go) if keeps else go
        res = {}
        for key, fn in (("default", lambda *a: temporal_interlace_func(*a, T, pad, active)),
                        ("kept", lambda *a: temporal_interlace_func(*a, T, pad, active, memory_format=KEEP)),
                        ("composition", lambda *a: _composition(*a, T, pad, active))):
            x, w, s = x0.clone(memory_format=KEEP).requires_grad_(True), w0.clone().requires_grad_(True), s0.clone().requires_grad_(True)
            assert x.stride() == x0.stride()
            out = fn(x, w, s)
            res[key] = (out.detach(),) + torch.autograd.grad(out, (x, w, s), go if key == "default" else grad)
        plain, kept, comp = res["default"], res["kept"], res["composition"]
        assert plain[0].is_contiguous() and plain[1].is_contiguous(), what
        assert kept[0].stride() == (x0.stride() if keeps else plain[0].stride()), what
        assert kept[1].stride() == (x0.stride() if keeps else plain[1].stride()), (what, "input.grad in the gradient's strides")
        # the default call's values, in the input's strides
        assert torch.equal(kept[0], plain[0]) and torch.equal(kept[1], plain[1]) and torch.equal(kept[2], plain[2]), (what, pad, active)
        assert torch.allclose(kept[3], plain[3], rtol=1e-6 if dt == torch.float32 else 1e-14, atol=1e-5 if dt == torch.float32 else 1e-13)
        # the composition on the channels-last per-clip op: out and all three gradients, bit for bit
        assert kept[0].stride() == comp[0].stride() and kept[1].stride() == comp[1].stride(), what
        for a, b, name in zip(kept, comp, ("out", "input.grad", "offsets.grad", "scales.grad")):
            assert a.shape == b.shape and a.dtype == dt and torch.equal(a, b), (what, pad, active, name)
        if not keeps:   # a contiguous input: exactly the default result, scales.grad included
            assert torch.equal(kept[3], plain[3]), what


def test_gradcheck():
    """where tests/test_interlace_cpu.py::test_gradcheck runs it, on channels-last inputs"""
    N, T, C, M = 2, 3, 4, 2
    gen = torch.Generator().manual_seed(64)
    cl = (lambda t: t.contiguous(memory_format=torch.channels_last))
    x = cl(torch.randn(N * T, C, M, 1, generator=gen, dtype=torch.float64))
    assert x.stride(1) == 1 and not x.is_contiguous()
    w = (torch.randint(-3, 3, (N, C), generator=gen).double() + 0.25 + 0.5 * torch.rand(N, C, generator=gen, dtype=torch.float64)).requires_grad_(True)
    s = torch.randn(N, T, C, generator=gen, dtype=torch.float64, requires_grad=True)
    wd = w.detach()
    for pad in range(5):
        assert torch.autograd.gradcheck(lambda b, c: temporal_interlace_func(x, b, c, T, pad, True, KEEP), (w, s), eps=1e-6, atol=1e-6)
        assert torch.autograd.gradcheck(lambda c: temporal_interlace_func(x, wd, c, T, pad, False, KEEP), (s,), eps=1e-6, atol=1e-6)
    x2 = cl(torch.randn(N * 2, C, M, 1, generator=gen, dtype=torch.float64)).requires_grad_(True)
    s2 = torch.randn(N, 2, C, generator=gen, dtype=torch.float64, requires_grad=True)
    for pad in (2, 3):
        assert torch.autograd.gradcheck(lambda a, b, c: temporal_interlace_func(a, b, c, 2, pad, True, KEEP), (x2, w, s2), eps=1e-6, atol=1e-6)
    assert torch.autograd.gradcheck(lambda a, c: temporal_interlace_func(a, wd, c, 2, 2, False, KEEP), (x2, s2), eps=1e-6, atol=1e-6)


def test_group_tables_are_the_expanded_tables():
    x0, T, _ = _inputs(torch.float32, seed=65)[0]
    N, C, G = x0.shape[0] // T, x0.shape[1], 3
    gen = torch.Generator().manual_seed(66)
    go = _like(x0, torch.randn(x0.shape, generator=gen))
    wg, sg = _table(gen, N, G, T, torch.float32), torch.randn(N, T, G, generator=gen)
    for pad, active in itertools.product((0, 3), (False, True)):
        a = [t.clone().requires_grad_(True) for t in (wg, sg)]
        b = [wg.repeat_interleave(C // G, dim=1).requires_grad_(True), sg.repeat_interleave(C // G, dim=2).requires_grad_(True)]
        out, ref = temporal_interlace_func(x0, *a, T, pad, active, KEEP), temporal_interlace_func(x0, *b, T, pad, active, KEEP)
        out.backward(go)
        ref.backward(go)
        assert torch.equal(out, ref) and out.stride() == x0.stride()
        assert a[0].grad.shape == (N, G) and torch.equal(a[0].grad, b[0].grad.view(N, G, C // G).sum(2))
        assert a[1].grad.shape == (N, T, G) and torch.equal(a[1].grad, b[1].grad.view(N, T, G, C // G).sum(3))


# ---- the default path ---------------------------------------------------------------------------------------------------------------
def test_the_default_call_and_inputs_that_are_not_dense():
    gen = torch.Generator().manual_seed(67)
    T = 3
    base = torch.randn(6, 6, 4, 10, generator=gen)
    views = [("contiguous", base[..., :5].contiguous()), ("a sliced contiguous view", base[..., ::2]),
             ("a sliced channels-last view", base.contiguous(memory_format=torch.channels_last)[:, :, :, ::2]),
             ("2-D", base[:, :, 0, 0].contiguous())]
    for what, x0 in views:
        w0, s0 = _tables(x0, T, torch.float32, 68)
        go = torch.randn(x0.shape, generator=gen)
        res = []
        for kw in ({}, {"memory_format": torch.contiguous_format}, {"memory_format": KEEP}):
            x, w, s = x0.detach().requires_grad_(True), w0.clone().requires_grad_(True), s0.clone().requires_grad_(True)
            assert x.stride() == x0.stride()      # (the view itself: a clone would be dense)
            out = temporal_interlace_func(x, w, s, T, 3, True, **kw)
            res.append((out.detach(),) + torch.autograd.grad(out, (x, w, s), go))
        for other in res[1:]:
            for a, b in zip(res[0], other):
                assert torch.equal(a, b) and a.stride() == b.stride(), what
        assert res[0][0].is_contiguous(), what


def test_a_wrong_memory_format_raises():
    x, w, s = torch.zeros(6, 4, 2, 2), torch.zeros(2, 4), torch.ones(2, 3, 4)
    for fmt in (torch.channels_last, torch.channels_last_3d, None):
        with pytest.raises(AssertionError, match="expected memory_format to be torch.contiguous_format or torch.preserve_format"):
            temporal_interlace_func(x, w, s, 3, 0, True, memory_format=fmt)
        with pytest.raises(AssertionError, match="memory_format must be"):
            torchshifts.TemporalInterlace(3, 4, memory_format=fmt)
    params = list(inspect.signature(temporal_interlace_func).parameters)
    assert params[-1] == "memory_format" and params[-2] == "active_flag"            # the keyword comes last
    assert inspect.signature(temporal_interlace_func).parameters["memory_format"].default == torch.contiguous_format
    assert torch.equal(temporal_interlace_func(x, w, s, 3, 0, False, KEEP), x)
    assert list(inspect.signature(torchshifts.TemporalInterlace.__init__).parameters)[-1] == "memory_format"


# ---- the op surface ---------------------------------------------------------------------------------------------------------------
CL_SCHEMAS = {"temporal_interlace_cl": TIN_FWD, "_temporal_interlace_cl_forward": TIN_FWD, "_temporal_interlace_cl_backward": TIN_BWD}
CL_KERNELS = {"temporal_interlace_cl": COMPOSITE, "_temporal_interlace_cl_forward": FLOAT, "_temporal_interlace_cl_backward": FLOAT}


def test_the_surface_of_the_new_namespace():
    assert registered_ops(NS) == sorted(CL_SCHEMAS)
    for op, schema in CL_SCHEMAS.items():
        name = NS + "::" + op
        assert str(torch._C._get_schema(name, "")) == name + schema
        assert tuple(k for k in KEYS if torch._C._dispatch_has_kernel_for_dispatch_key(name, k)) == CL_KERNELS[op], op
    assert registered_ops("torchshifts_interlace") == sorted(INTERLACE_SCHEMAS)       # ... and the plain namespace keeps its three


def test_what_the_node_keeps_and_the_double_backward():
    x0, T, _ = _inputs(torch.float32, seed=69)[0]
    N, C = x0.shape[0] // T, x0.shape[1]
    x = x0.clone(memory_format=KEEP).requires_grad_(True)
    w, s = torch.zeros(N, C, requires_grad=True), torch.ones(N, T, C, requires_grad=True)
    assert _saved_shapes(lambda: OPS.temporal_interlace_cl(x, w, s, T, 0, True)) == [tuple(x0.shape), (N, C), (N, T, C)]
    gx, gw, gs = OPS._temporal_interlace_cl_backward(_like(x0, torch.ones(x0.shape)), w, s, x, T, 0, True)
    assert gx.stride() == x0.stride() and gw.shape == (N, C) and gs.shape == (N, T, C)
    with pytest.raises(RuntimeError, match="double backwards on temporal_interlace_cl not supported"):
        gs.sum().backward()
    with pytest.raises(RuntimeError, match=r"scales must have shape \[N, T, C\]"):
        OPS.temporal_interlace_cl(x, w, torch.ones(N, C, T), T, 0, True)


# ---- the layer --------------------------------------------------------------------------------------------------------------------
def test_the_layer_carries_the_attribute_and_trains_channels_last():
    torch.manual_seed(70)
    kept, plain = torchshifts.TemporalInterlace(4, 16, shift_div=2, memory_format=KEEP), torchshifts.TemporalInterlace(4, 16, shift_div=2)
    assert kept.memory_format == KEEP and plain.memory_format == torch.contiguous_format
    assert plain.extra_repr() == "n_segment=4, in_channels=16, shift_div=2, padding_method=zeros"     # the default repr is what it was
    assert kept.extra_repr() == "n_segment=4, in_channels=16, shift_div=2, padding_method=zeros, memory_format=torch.preserve_format"
    assert sorted(kept.state_dict()) == sorted(plain.state_dict()) == [
        "offset_net.conv.bias", "offset_net.conv.weight", "offset_net.fc1.bias", "offset_net.fc1.weight", "offset_net.fc2.bias",
        "offset_net.fc2.weight", "weight_net.conv.bias", "weight_net.conv.weight"]
    kept.load_state_dict(plain.state_dict())
    for p in list(kept.parameters()) + list(plain.parameters()):
        assert p.grad is None
    x = torch.randn(8, 16, 3, 3).contiguous(memory_format=torch.channels_last)
    out, ref = kept(x), plain(x)
    assert out.stride() == x.stride() and ref.is_contiguous() and torch.equal(out, ref)
    out.square().mean().backward()
    assert all(p.grad is not None and p.grad.abs().sum() > 0 for p in kept.parameters())
    xc = x.contiguous()   # (its own reference: the descriptor's spatial mean sums in the layout's order)
    assert torch.equal(kept(xc), plain(xc)) and kept(xc).is_contiguous()


# ---- SHIFTND_INTERLACE_FRAMES at the C ABI, host side only ------------------------------------------------------------------------
def _plan_bytes(n, c, t, m, es):
    """the formula include/shiftnd_hip.h states"""
    pieces = -(-c * es // 16)
    rps = 256 // pieces if pieces < 256 else 1
    steps = 8
    while steps > 1 and n * -(-m // (rps * steps)) < 768:
        steps //= 2
    return -(-m // (rps * steps)) * n * c * (1 + t) * 8


def test_the_constant_and_the_keyword():
    assert abi.INTERLACE_FRAMES == 0x10000 and abi.lib().shiftnd_abi_version() == 5 and len(abi.EXPORTS) == 20
    x = torch.zeros(N, C, T, M)
    assert abi.problem(x, 0, 0, None, shift_dim0=True, interlace_frames=True).dtype == 0x10200
    assert abi.problem(x, 0, 0, None, shift_dim0=True, interlace=True).dtype == 0x8200
    assert abi.problem(x.half(), 0, 0, None, w=torch.zeros(N * C * (1 + T)), shift_dim0=True, interlace_frames=True).dtype == abi.F16 | 0x10300
    for fn in (abi.problem, abi.forward, abi.backward_workspace, abi.backward):
        assert inspect.signature(fn).parameters["interlace_frames"].default is False, fn.__name__


@pytest.mark.parametrize("active", (0, 1))
def test_the_interlace_frames_flag_host_side(active):
    L = abi.lib()
    byref = ctypes.byref
    st = _st(NHWC)
    pool = (ctypes.c_int32 * 3)(2, 2, 1)
    for dt in FLOATS:
        es = {abi.F32: 4, abi.F64: 8}.get(dt, 2)
        ok = _problem(2, dt | DIM0 | ILF, active=active)
        # accepted: the NULL tensors are refused, the workspace query answers the plan's bytes -- a function of the geometry alone
        assert _forward(ok) == INVALID and _backward(ok) == INVALID
        assert _workspace(ok) == _plan_bytes(N, C, T, M, es) == N * C * (1 + T) * 8
        for sizes in ((2, 5, 3, 5000, 1), (3, 64, 8, 3136, 1), (32, 256, 8, 3136, 1), (700, 2056, 2, 3, 1), (1, 8, 33, 300, 1)):
            big = _problem(2, dt | DIM0 | ILF, sizes=sizes, borders=(0, sizes[2], 0, sizes[3], 0, 1), active=active)
            assert _workspace(big) == _plan_bytes(sizes[0], sizes[1], sizes[2], sizes[3], es), sizes
        three = _problem(3, dt | DIM0 | ILF, sizes=(N, C, T, 2, 4), borders=(0, T, 0, 2, 0, 4), active=active)
        assert _workspace(three) == _plan_bytes(N, C, T, 8, es)
        # an empty problem: sizeof(double), and the forward answers before it looks at a pointer
        for sizes in ((0, C, T, M, 1), (N, 0, T, M, 1), (N, C, T, 0, 1)):
            empty = _problem(2, dt | DIM0 | ILF, sizes=sizes, borders=(0, T, 0, sizes[3], 0, 1), active=active)
            assert _workspace(empty) == 8 and _forward(empty) == 0 and abi.last_path() == abi.PATH_EMPTY
        # the bit without SHIFT_DIM0: an unknown dtype bit on every entry point
        alone = _problem(2, dt | ILF, active=active)
        assert _forward(alone) == UNSUPPORTED and _backward(alone) == UNSUPPORTED and _workspace(alone) == 0
        for p in (alone, ok):   # ... and the quantized and the pooled entry points, with and without SHIFT_DIM0
            assert L.shiftnd_forward_quantized(byref(p), None, st, None, abi.I32, 0, 0, None, st, None) == UNSUPPORTED
            assert L.shiftnd_forward_pooled(byref(p), pool, None, None, None, None) == UNSUPPORTED
            assert L.shiftnd_backward_pooled(byref(p), pool, None, None, None, None, None, None, 0, None) == UNSUPPORTED
            assert L.shiftnd_forward_quantized_pooled(byref(p), pool, None, None, abi.I32, 0, 0, 0, None, None) == UNSUPPORTED
        # beside every other bit of the family, INTERLACE included
        for other in (abi.FRAMES, abi.PER_CLIP, abi.STREAM, abi.CLIP_FRAMES, abi.INTERLACE, abi.INTERLACE | abi.CLIP_FRAMES):
            both = _problem(2, dt | DIM0 | other | ILF, active=active)
            for s in (NHWC, SEGMENT):
                assert _forward(both, s=s) == INVALID and _backward(both, s=s) == INVALID, hex(other)
            assert _workspace(both) == 0, hex(other)
        # out == x: refused before the pointer is looked at (4096 is no allocation)
        assert _forward(ok, x=ctypes.c_void_p(4096), out=ctypes.c_void_p(4096)) == INVALID
        # a cut window, ndim 1
        cut = _problem(2, dt | DIM0 | ILF, borders=(1, T, 0, M, 0, 1), active=active)
        assert _forward(cut) == INVALID and _backward(cut) == INVALID and _workspace(cut) == 0
        one = _problem(1, dt | DIM0 | ILF, sizes=(N, C, T * M, 1, 1), borders=(0, T * M, 0, 1, 0, 1), active=active)
        assert _forward(one, s=(T * M * C, 1, C, 0, 0)) == INVALID and _backward(one, s=(T * M * C, 1, C, 0, 0)) == INVALID and _workspace(one) == 0
        # sizes beyond the frame kernels' bounds: S0 = 2^30 (the 32-bit padding map), N * S0 = 2^31
        for sizes in ((1, 1, 1 << 30, 1, 1), (1 << 16, 1, 1 << 15, 1, 1)):
            far = _problem(2, dt | DIM0 | ILF, sizes=sizes, borders=(0, sizes[2], 0, 1, 0, 1), active=active)
            assert _forward(far, s=(sizes[2] * sizes[1], 1, sizes[1], sizes[1], 0)) == INVALID and _workspace(far) == 0, sizes
    # what the neighbours answer is what they answered
    assert _workspace(_problem(2, abi.F32 | DIM0 | abi.INTERLACE, active=active)) == 2 * 5 * (1 + 4 * 3) * 24
    assert _forward(_problem(2, abi.F32 | DIM0 | abi.INTERLACE, active=active), x=ctypes.c_void_p(4096), out=ctypes.c_void_p(8192)) == INVALID
    # a quantized dtype, and WEIGHTS_F32 on a dtype that has no mixed form
    for dt in (abi.U8, abi.I8, abi.I32, abi.F32 | abi.WEIGHTS_F32):
        p = _problem(2, dt | DIM0 | ILF, active=active)
        assert _forward(p) == UNSUPPORTED and _backward(p) == UNSUPPORTED and _workspace(p) == 0
        assert L.shiftnd_forward_quantized(byref(p), None, st, None, abi.I32, 0, 0, None, st, None) == UNSUPPORTED
    # 0x800 stays unassigned: an unknown bit, with and without the new one
    for bits in (0x800 | DIM0 | ILF, 0x800 | ILF):
        p = _problem(2, abi.F32 | bits, active=active)
        assert _forward(p) == UNSUPPORTED and _backward(p) == UNSUPPORTED and _workspace(p) == 0


@pytest.mark.parametrize("active", (0, 1))
def test_segment_major_strides_and_null_forms_with_host_pointers(active):
    """never dereferenced: every one of these calls is refused on the host first"""
    p = _problem(2, abi.F32 | DIM0 | ILF, active=active)
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


def test_the_size_bound_of_the_packed_table_on_both_sides():
    """N * T * C = 2^31: refused; one clip fewer: accepted (M = 1, so nothing else is large)"""
    def workspace(n, c, t, dt=abi.F16):
        return _workspace(_problem(2, dt | DIM0 | ILF, sizes=(n, c, t, 1, 1), borders=(0, t, 0, 1, 0, 1)))

    def forward(n, c, t, dt=abi.F16):
        p = _problem(2, dt | DIM0 | ILF, sizes=(n, c, t, 1, 1), borders=(0, t, 0, 1, 0, 1))
        return _forward(p, s=(t * c, 1, c, c, 0))

    assert workspace(1 << 8, 1 << 15, 1 << 8) == 0 and forward(1 << 8, 1 << 15, 1 << 8) == INVALID
    below = ((1 << 8) - 1, 1 << 15, 1 << 8)
    assert workspace(*below) == _plan_bytes(below[0], below[1], below[2], 1, 2) and forward(*below) == INVALID   # (accepted; the NULL tensors)
    # ... also when T carries the product: N = 1, C = 2^15, T = 2^16
    assert workspace(1, 1 << 15, 1 << 16) == 0 and workspace(1, (1 << 15) - 1, 1 << 16) > 0
    assert workspace(1, 1 << 15, 1 << 16, abi.F32) == 0 and workspace(1, (1 << 15) - 1, 1 << 16, abi.F32) > 0
