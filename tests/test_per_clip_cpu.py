"""The per-clip temporal shifts on CPU tensors, and SHIFTND_PER_CLIP at the C ABI host side.

The definition: for a [N*T, C, ...] input and a [N, C] table, clip n is the per-channel op on x[n*T:(n+1)*T] under row n --
temporal_shift_learnable_func for the learnable form (out, x.grad and weights.grad[n] are that call's), temporal_shift_func for the
fixed one.  The CPU key is that loop, so every comparison here is torch.equal.

Shapes: [2*3, 5, 4] and [3*4, 6, 2, 3] -- two and three clips, a 3-D and a 4-D tensor; every row of a table differs, with |w| up to T + 1 (double folds, wraps).
"""
import ctypes
import itertools

import pytest
import torch

import torchshifts
from torchshifts.functional import (temporal_shift_func, temporal_shift_learnable_func, temporal_shift_learnable_per_clip_func,
                                    temporal_shift_per_clip_func)

OPS = torch.ops.torchshifts_per_clip
SHAPES = [((2 * 3, 5, 4), 3), ((3 * 4, 6, 2, 3), 4)]


def _table(gen, N, C, T, dt):
    """[N, C] weights in [-(T + 1), T + 1] on quarters, rows that differ, the specials 0, T + 1, -(T + 1), 0.5 in every table"""
    w = torch.randint(-4 * (T + 1), 4 * (T + 1) + 1, (N, C), generator=gen).to(dt) / 4
    w[0, 0], w[0, 1], w[1, 0], w[1, 1] = 0.0, T + 1.0, -(T + 1.0), 0.5
    assert all(not torch.equal(w[a], w[b]) for a, b in itertools.combinations(range(N), 2))
    return w


def _loop(fn, x, table, T, *args):
    return torch.cat([fn(x[n * T:(n + 1) * T], table[n], T, *args) for n in range(table.shape[0])], 0)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("shape,T", SHAPES, ids=["6x5x4", "12x6x2x3"])
def test_the_ops_are_the_loop_over_clips(shape, T, dt):
    gen = torch.Generator().manual_seed(41)
    N, C = shape[0] // T, shape[1]
    for pad, active in itertools.product(range(5), (False, True)):
        what = (shape, pad, active)
        x = torch.randn(shape, generator=gen, dtype=dt)
        go = torch.randn(shape, generator=gen, dtype=dt)
        w = _table(gen, N, C, T, dt)
        xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        xb, wb = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        out = temporal_shift_learnable_per_clip_func(xa, wa, T, pad, active)
        ref = _loop(temporal_shift_learnable_func, xb, wb, T, pad, active)
        out.backward(go)
        ref.backward(go)
        assert out.is_contiguous() and torch.equal(out, ref), what
        assert torch.equal(xa.grad, xb.grad), what
        assert wa.grad.shape == (N, C) and torch.equal(wa.grad, wb.grad), what
        # the fixed form: an integer table, and the same table as floats
        s = torch.round(w).to(torch.int64)
        xc, xd = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        fixed = temporal_shift_per_clip_func(xc, s, T, pad)
        fixed_ref = _loop(temporal_shift_func, xd, s, T, pad)
        fixed.backward(go)
        fixed_ref.backward(go)
        assert torch.equal(fixed, fixed_ref) and torch.equal(xc.grad, xd.grad), what
        assert torch.equal(temporal_shift_per_clip_func(x, w, T, pad), _loop(temporal_shift_func, x, w, T, pad)), what   # rounded half to even
        if not active:
            assert torch.equal(fixed, out), what + ("the sparse mode is the fixed op",)


def test_a_group_table_is_the_expanded_table():
    gen = torch.Generator().manual_seed(42)
    (shape, T), G = SHAPES[1], 3
    N, C = shape[0] // T, shape[1]
    x, go = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    wg = _table(gen, N, G, T, torch.float32)
    full = wg.repeat_interleave(C // G, dim=1)
    for active in (False, True):
        a, b = wg.clone().requires_grad_(True), full.clone().requires_grad_(True)
        out = temporal_shift_learnable_per_clip_func(x, a, T, 0, active)
        ref = temporal_shift_learnable_per_clip_func(x, b, T, 0, active)
        out.backward(go)
        ref.backward(go)
        assert torch.equal(out, ref)
        assert a.grad.shape == (N, G) and torch.equal(a.grad, b.grad.view(N, G, C // G).sum(2))
    s = torch.round(wg).long()
    assert torch.equal(temporal_shift_per_clip_func(x, s, T, 0), temporal_shift_per_clip_func(x, s.repeat_interleave(C // G, dim=1), T, 0))


def test_the_assertions_name_the_expected_shape():
    (shape, T) = SHAPES[1]
    N, C = shape[0] // T, shape[1]
    x = torch.randn(shape)
    for fn, table in ((temporal_shift_learnable_per_clip_func, torch.zeros), (temporal_shift_per_clip_func, lambda *s: torch.zeros(*s, dtype=torch.long))):
        for bad in ((C,), (N,), (C, N), (N + 1, C), (N, 4), (N, C, 1), (N, 0)):
            with pytest.raises(AssertionError, match=r"expected \[%d, %d\] tensor" % (N, C)):
                fn(x, table(*bad), T)
        with pytest.raises(AssertionError, match="multiple of n_segment"):
            fn(x, table(N, C), 5)
        with pytest.raises(AssertionError, match="padding_mode"):
            fn(x, table(N, C), T, 5)
        with pytest.raises(AssertionError, match="quantized inputs are not supported"):
            fn(torch.quantize_per_tensor(x, 0.1, 0, torch.quint8), table(N, C), T)
    with pytest.raises(AssertionError, match="expected float weights"):
        temporal_shift_learnable_per_clip_func(x, torch.zeros(N, C, dtype=torch.long), T)


def test_the_ops_refuse_what_the_wrappers_refuse():
    (shape, T) = SHAPES[0]
    N, C = shape[0] // T, shape[1]
    x = torch.randn(shape)
    with pytest.raises(RuntimeError, match=r"weights must have shape \[N, C\] = \[2, 5\]"):
        OPS.temporal_shift_learnable_per_clip(x, torch.zeros(C), T, 0, True)
    with pytest.raises(RuntimeError, match=r"shifts must have shape \[N, C\] = \[2, 5\]"):
        OPS.temporal_shift_per_clip(x, torch.zeros(C, N), T, 0)
    with pytest.raises(RuntimeError, match="must be a multiple of n_segment"):
        OPS.temporal_shift_per_clip(x, torch.zeros(N, C), 4, 0)
    with pytest.raises(RuntimeError, match="quantized inputs are not supported"):
        OPS.temporal_shift_learnable_per_clip(torch.quantize_per_tensor(x, 0.1, 0, torch.quint8), torch.zeros(N, C), T, 0, False)
    with pytest.raises(RuntimeError, match="weights must be floats"):
        OPS.temporal_shift_learnable_per_clip(x, torch.zeros(N, C, dtype=torch.long), T, 0, False)
    xr, wr = x.clone().requires_grad_(True), torch.zeros(N, C, requires_grad=True)
    gx, gw = OPS._temporal_shift_learnable_per_clip_backward(torch.ones(shape), wr, xr, T, 0, True)
    with pytest.raises(RuntimeError, match="double backwards on temporal_shift_learnable_per_clip not supported"):
        gx.sum().backward()


def test_empty_tensors():
    x = torch.zeros(0, 5, 4, requires_grad=True)
    w = torch.zeros(0, 5, requires_grad=True)
    out = temporal_shift_learnable_per_clip_func(x, w, 3, 0, True)
    out.sum().backward()
    assert out.shape == (0, 5, 4) and x.grad.shape == (0, 5, 4) and w.grad.shape == (0, 5)
    x0 = torch.zeros(6, 5, 0, requires_grad=True)
    w0 = torch.ones(2, 5, requires_grad=True)
    out = temporal_shift_learnable_per_clip_func(x0, w0, 3, 0, True)
    out.sum().backward()
    assert out.shape == (6, 5, 0) and torch.equal(w0.grad, torch.zeros(2, 5))
    assert temporal_shift_per_clip_func(x0.detach(), torch.ones(2, 5, dtype=torch.long), 3, 0).shape == (6, 5, 0)


def _saved_shapes(fn):
    seen = []

    def pack(t):
        seen.append(tuple(t.shape))
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = fn()
    assert out.requires_grad
    return seen


def test_what_the_nodes_keep():
    (shape, T) = SHAPES[1]
    N, C = shape[0] // T, shape[1]
    x = torch.randn(shape, requires_grad=True)
    # the fixed op: the table alone, nothing of the input's size
    assert _saved_shapes(lambda: temporal_shift_per_clip_func(x, torch.ones(N, C, dtype=torch.long), T)) == [(N, C)]
    w = torch.zeros(N, C, requires_grad=True)
    assert _saved_shapes(lambda: OPS.temporal_shift_learnable_per_clip(x, w, T, 0, True)) == [shape, (N, C)]


def test_the_modules_hold_nothing():
    fixed = torchshifts.PerClipTemporalShift(4, padding="border")
    learn = torchshifts.LearnablePerClipTemporalShift(4, padding="reflect", active_flag=True)
    for m in (fixed, learn):
        assert len(m.state_dict()) == 0 and not list(m.parameters()) and not list(m.buffers())
    assert repr(fixed) == "PerClipTemporalShift(n_segment=4, padding_method=border, per-clip integer shifts)"
    assert repr(learn) == ("LearnablePerClipTemporalShift(n_segment=4, padding_method=reflect, Active shift on forward pass: Yes, "
                           "per-clip weights)")
    (shape, T) = SHAPES[1]
    N, C = shape[0] // T, shape[1]
    gen = torch.Generator().manual_seed(43)
    x, w = torch.randn(shape, generator=gen), _table(gen, N, C, T, torch.float32)
    out = learn(x, w)
    assert isinstance(out, torch.Tensor) and torch.equal(out, temporal_shift_learnable_per_clip_func(x, w, T, 3, True))
    s = torch.round(w).long()
    assert torch.equal(fixed(x, s), temporal_shift_per_clip_func(x, s, T, 1))
    # a net in front: the gradient reaches its parameters through the table
    net = torch.nn.Linear(C, 2)
    table = net(x.view(N, T, C, -1).mean((1, 3)))          # [N, 2]: two groups of three channels
    learn(x, table).square().mean().backward()
    assert net.weight.grad is not None and net.weight.grad.abs().sum() > 0


# ---- SHIFTND_PER_CLIP at the C ABI, host side only: validation happens before any device work.  With NULL tensors an accepted geometry
# ends in INVALID_ARGUMENT (the tensors are refused) and its workspace query answers the plan's bytes; a refused problem answers 0.
def _problem(ndim, dtype, sizes=(2, 5, 3, 8, 1), borders=(0, 3, 0, 8, 0, 1), active=0):
    from torchshifts import abi
    p = abi.Problem()
    p.ndim, p.dtype, p.padding_mode, p.active = ndim, dtype, 0, active
    for i, v in enumerate(sizes):
        p.sizes[i] = v
    for i, v in enumerate(borders):
        p.borders[i] = v
    return p


def test_the_per_clip_flag_host_side():
    from torchshifts import abi
    INVALID, UNSUPPORTED = -1, -2
    L = abi.lib()
    assert L.shiftnd_abi_version() == 5 and len(abi.EXPORTS) == 20
    assert abi.PER_CLIP == 0x1000 and abi.problem(torch.zeros(2, 5, 3, 8), 0, 0, None, shift_dim0=True, per_clip=True).dtype == 0x1200
    st = (ctypes.c_int64 * 5)(3 * 5 * 8, 8, 5 * 8, 1, 0)   # [N, C, T, M] = [2, 5, 3, 8] in memory order N, T, C, M
    nhwc = (ctypes.c_int64 * 5)(3 * 8 * 5, 1, 8 * 5, 5, 0)
    byref = ctypes.byref
    DIM0, PC = abi.SHIFT_DIM0, abi.PER_CLIP

    def forward(p, x=None, out=None, s=st):
        return L.shiftnd_forward(byref(p), x, s, None, out, s, None)

    def backward(p, s=st):
        return L.shiftnd_backward(byref(p), None, s, None, s, None, None, s, None, None, 0, None)

    def workspace(p):
        return L.shiftnd_backward_workspace_bytes(byref(p))

    pool = (ctypes.c_int32 * 3)(2, 2, 1)
    for dt in (abi.F32, abi.F64, abi.F16, abi.BF16, abi.F16 | abi.WEIGHTS_F32, abi.BF16 | abi.WEIGHTS_F32):
        for active in (0, 1):
            ok = _problem(2, dt | DIM0 | PC, active=active)
            assert forward(ok) == INVALID and backward(ok) == INVALID                 # accepted: the NULL tensors are refused
            # the partial records are re-indexed, not multiplied: the bytes of the per-channel plan, also with several chunks per line
            assert workspace(ok) == workspace(_problem(2, dt | DIM0, active=active)) >= 2 * 5 * 24
            big = dict(sizes=(2, 5, 3, 5000, 1), borders=(0, 3, 0, 5000, 0, 1), active=active)
            assert workspace(_problem(2, dt | DIM0 | PC, **big)) == workspace(_problem(2, dt | DIM0, **big)) >= 2 * 2 * 5 * 24
            assert workspace(_problem(2, dt | DIM0 | PC, sizes=(0, 5, 3, 8, 1), active=active)) == 8   # an empty problem: sizeof(double)
            # the bit without SHIFT_DIM0: an unknown dtype bit on every entry point
            alone = _problem(2, dt | PC, active=active)
            assert forward(alone) == UNSUPPORTED and backward(alone) == UNSUPPORTED and workspace(alone) == 0
            assert L.shiftnd_forward_pooled(byref(alone), pool, None, None, None, None) == UNSUPPORTED
            assert L.shiftnd_backward_pooled(byref(alone), pool, None, None, None, None, None, None, 0, None) == UNSUPPORTED
            # ... and on the quantized and the pooled entry points with SHIFT_DIM0 too
            assert L.shiftnd_forward_quantized(byref(ok), None, st, None, abi.I32, 0, 0, None, st, None) == UNSUPPORTED
            assert L.shiftnd_forward_pooled(byref(ok), pool, None, None, None, None) == UNSUPPORTED
            assert L.shiftnd_backward_pooled(byref(ok), pool, None, None, None, None, None, None, 0, None) == UNSUPPORTED
            # together with SHIFTND_FRAMES
            both = _problem(2, dt | DIM0 | abi.FRAMES | PC, active=active)
            assert forward(both, s=nhwc) == INVALID and backward(both, s=nhwc) == INVALID and workspace(both) == 0
            assert workspace(_problem(2, dt | DIM0 | abi.FRAMES, active=active)) > 0   # (what the bit took away)
            # out == x: refused before the pointer is looked at (4096 is no allocation)
            assert forward(ok, x=ctypes.c_void_p(4096), out=ctypes.c_void_p(4096)) == INVALID
            # what SHIFT_DIM0 refuses stays refused: a cut window, ndim 1
            cut = _problem(2, dt | DIM0 | PC, borders=(1, 3, 0, 8, 0, 1), active=active)
            assert forward(cut) == INVALID and backward(cut) == INVALID and workspace(cut) == 0
            one = _problem(1, dt | DIM0 | PC, sizes=(2, 5, 24, 1, 1), borders=(0, 24, 0, 1, 0, 1), active=active)
            assert forward(one) == INVALID and backward(one) == INVALID and workspace(one) == 0
            # N * C of 2^31: refused (every other factor is 1, so nothing else is large)
            wide = _problem(2, dt | DIM0 | PC, sizes=(1 << 16, 1 << 15, 1, 1, 1), borders=(0, 1, 0, 1, 0, 1), active=active)
            assert forward(wide) == INVALID and backward(wide) == INVALID and workspace(wide) == 0
    # the x == NULL && grad_w == NULL form does not exist under the flag (here: on an accepted geometry, every other pointer NULL too)
    ok = _problem(2, abi.F32 | DIM0 | PC)
    assert backward(ok) == INVALID
    # a quantized dtype
    for dt in (abi.U8, abi.I8, abi.I32, abi.F32 | abi.WEIGHTS_F32):
        p = _problem(2, dt | DIM0 | PC)
        assert forward(p) == UNSUPPORTED and backward(p) == UNSUPPORTED and workspace(p) == 0
        assert L.shiftnd_forward_quantized(byref(p), None, st, None, abi.I32, 0, 0, None, st, None) == UNSUPPORTED
    # 0x800 stays unassigned: an unknown bit, with and without the new one
    for bits in (0x800, 0x800 | DIM0, 0x800 | DIM0 | PC):
        p = _problem(2, abi.F32 | bits)
        assert forward(p) == UNSUPPORTED and backward(p) == UNSUPPORTED
