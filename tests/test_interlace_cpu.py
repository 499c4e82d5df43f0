"""Temporal interlacing on CPU tensors, SHIFTND_INTERLACE at the C ABI host side, the TemporalInterlace layer, and the surface of
torchshifts_interlace::.

The definition: out = temporal_shift_learnable_per_clip_func(x, offsets, T, pad, active) * scales.reshape(N*T, C, 1, ...), with the
gradients of that composition.  The CPU key is that expression, so out is compared with torch.equal.

gradcheck.  scales enter linearly: checked under every padding in both modes.  offsets: checked under every padding where the shift
interpolates (the sparse shift is piecewise constant in them; its table gradient is the reference's surrogate), away from the
integers, where the interpolation has a kink.  input: the project's grad_x is the reference's rule, which is the adjoint only where
tests/test_tshift_cpu.py::test_gradcheck says so -- T = 2 under periodic and reflect padding -- so the input is checked there, as
tests/test_per_clip_cl_cpu.py does for the per-clip op (the gradients of the interlace op are the composition's BY DEFINITION, so
it inherits exactly that set).
"""
import ctypes
import itertools

import pytest
import torch

import torchshifts
from torchshifts.functional import temporal_interlace_func, temporal_shift_learnable_per_clip_func

from test_binding_surface import COMPOSITE, FLOAT, KEYS, LATER_SCHEMAS, SCHEMAS, registered_ops
from test_per_clip_cpu import _problem, _saved_shapes, _table

OPS = torch.ops.torchshifts_interlace
SHAPES = [((2 * 3, 5, 4), 3), ((3 * 4, 6, 2, 3), 4)]


def _composition(x, offsets, scales, T, pad, active):
    y = temporal_shift_learnable_per_clip_func(x, offsets, T, pad, active)
    return y * scales.reshape((x.shape[0], x.shape[1]) + (1,) * (x.dim() - 2))


# ---- the op -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("shape,T", SHAPES, ids=["6x5x4", "12x6x2x3"])
def test_the_op_is_the_composition(shape, T, dt):
    gen = torch.Generator().manual_seed(51)
    N, C = shape[0] // T, shape[1]
    for pad, active in itertools.product(range(5), (False, True)):
        what = (shape, pad, active)
        x, go = torch.randn(shape, generator=gen, dtype=dt), torch.randn(shape, generator=gen, dtype=dt)
        w, s = _table(gen, N, C, T, dt), torch.randn(N, T, C, generator=gen, dtype=dt)
        a = [t.clone().requires_grad_(True) for t in (x, w, s)]
        b = [t.clone().requires_grad_(True) for t in (x, w, s)]
        out, ref = temporal_interlace_func(*a, T, pad, active), _composition(*b, T, pad, active)
        assert out.shape == x.shape and torch.equal(out, ref), what
        out.backward(go)
        ref.backward(go)
        assert torch.equal(a[0].grad, b[0].grad), what + ("input.grad",)
        assert a[1].grad.shape == (N, C) and torch.equal(a[1].grad, b[1].grad), what + ("offsets.grad",)
        assert a[2].grad.shape == (N, T, C) and torch.allclose(a[2].grad, b[2].grad, rtol=1e-6 if dt == torch.float32 else 1e-14,
                                                              atol=1e-5 if dt == torch.float32 else 1e-13), what + ("scales.grad",)
    assert torch.equal(temporal_interlace_func(x, w, s, T), temporal_interlace_func(x, w, s, T, 0, True))   # the defaults


def test_gradcheck():
    N, T, C, M = 2, 3, 4, 2
    gen = torch.Generator().manual_seed(52)
    x = torch.randn(N * T, C, M, generator=gen, dtype=torch.float64)
    w = (torch.randint(-3, 3, (N, C), generator=gen).double() + 0.25 + 0.5 * torch.rand(N, C, generator=gen, dtype=torch.float64)).requires_grad_(True)
    s = torch.randn(N, T, C, generator=gen, dtype=torch.float64, requires_grad=True)
    wd = w.detach()
    for pad in range(5):
        assert torch.autograd.gradcheck(lambda b, c: temporal_interlace_func(x, b, c, T, pad, True), (w, s), eps=1e-6, atol=1e-6)
        assert torch.autograd.gradcheck(lambda c: temporal_interlace_func(x, wd, c, T, pad, False), (s,), eps=1e-6, atol=1e-6)
    x2 = torch.randn(N * 2, C, M, generator=gen, dtype=torch.float64, requires_grad=True)
    s2 = torch.randn(N, 2, C, generator=gen, dtype=torch.float64, requires_grad=True)
    for pad in (2, 3):
        assert torch.autograd.gradcheck(lambda a, b, c: temporal_interlace_func(a, b, c, 2, pad, True), (x2, w, s2), eps=1e-6, atol=1e-6)
    assert torch.autograd.gradcheck(lambda a, c: temporal_interlace_func(a, wd, c, 2, 2, False), (x2, s2), eps=1e-6, atol=1e-6)


def test_group_tables_are_the_expanded_tables():
    gen = torch.Generator().manual_seed(53)
    (shape, T), G = SHAPES[1], 3
    N, C = shape[0] // T, shape[1]
    x, go = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    wg, sg = _table(gen, N, G, T, torch.float32), torch.randn(N, T, G, generator=gen)
    for pad, active in itertools.product((0, 3), (False, True)):
        a = [t.clone().requires_grad_(True) for t in (wg, sg)]
        b = [wg.repeat_interleave(C // G, dim=1).requires_grad_(True), sg.repeat_interleave(C // G, dim=2).requires_grad_(True)]
        out, ref = temporal_interlace_func(x, *a, T, pad, active), temporal_interlace_func(x, *b, T, pad, active)
        out.backward(go)
        ref.backward(go)
        assert torch.equal(out, ref)
        assert a[0].grad.shape == (N, G) and torch.equal(a[0].grad, b[0].grad.view(N, G, C // G).sum(2))
        assert a[1].grad.shape == (N, T, G) and torch.equal(a[1].grad, b[1].grad.view(N, T, G, C // G).sum(3))


def test_the_assertions_name_the_expected_shape():
    (shape, T) = SHAPES[1]
    N, C = shape[0] // T, shape[1]
    x, w, s = torch.randn(shape), torch.zeros(N, C), torch.ones(N, T, C)
    for bad in ((C,), (N,), (C, N), (N + 1, C), (N, 4), (N, C, 1)):
        with pytest.raises(AssertionError, match=r"expected \[%d, %d\] tensor" % (N, C)):
            temporal_interlace_func(x, torch.zeros(*bad), s, T)
    for bad in ((N, C), (N, T), (T, N, C), (N, T + 1, C), (N, T, 4), (N + 1, T, C)):
        with pytest.raises(AssertionError, match=r"expected \[%d, %d, %d\] tensor" % (N, T, C)):
            temporal_interlace_func(x, w, torch.ones(*bad), T)
    with pytest.raises(AssertionError, match="multiple of n_segment"):
        temporal_interlace_func(x, w, s, 5)
    with pytest.raises(AssertionError, match="padding_mode"):
        temporal_interlace_func(x, w, s, T, 5)
    with pytest.raises(AssertionError, match="quantized inputs are not supported"):
        temporal_interlace_func(torch.quantize_per_tensor(x, 0.1, 0, torch.quint8), w, s, T)
    with pytest.raises(AssertionError, match="expected float offsets"):
        temporal_interlace_func(x, w.long(), s, T)
    with pytest.raises(AssertionError, match="expected float scales"):
        temporal_interlace_func(x, w, s.long(), T)
    with pytest.raises(AssertionError, match="of one dtype"):
        temporal_interlace_func(x, w, s.double(), T)


def test_the_op_refuses_what_the_wrapper_refuses():
    (shape, T) = SHAPES[0]
    N, C = shape[0] // T, shape[1]
    x, w, s = torch.randn(shape), torch.zeros(N, C), torch.ones(N, T, C)
    with pytest.raises(RuntimeError, match=r"offsets must have shape \[N, C\] = \[2, 5\]"):
        OPS.temporal_interlace(x, torch.zeros(C), s, T, 0, True)
    with pytest.raises(RuntimeError, match=r"scales must have shape \[N, T, C\] = \[2, 3, 5\]"):
        OPS.temporal_interlace(x, w, torch.ones(N, C, T), T, 0, True)
    with pytest.raises(RuntimeError, match="must be a multiple of n_segment"):
        OPS.temporal_interlace(x, w, s, 4, 0, True)
    with pytest.raises(RuntimeError, match="padding_mode must be 0..4"):
        OPS.temporal_interlace(x, w, s, T, 7, True)
    with pytest.raises(RuntimeError, match="quantized inputs are not supported"):
        OPS.temporal_interlace(torch.quantize_per_tensor(x, 0.1, 0, torch.quint8), w, s, T, 0, False)
    with pytest.raises(RuntimeError, match="offsets must be floats"):
        OPS.temporal_interlace(x, w.long(), s, T, 0, False)
    with pytest.raises(RuntimeError, match="scales must have the offsets' type"):
        OPS.temporal_interlace(x, w, s.double(), T, 0, False)
    xr, wr, sr = x.clone().requires_grad_(True), w.clone().requires_grad_(True), s.clone().requires_grad_(True)
    gx, gw, gs = OPS._temporal_interlace_backward(torch.ones(shape), wr, sr, xr, T, 0, True)
    assert gx.shape == shape and gw.shape == (N, C) and gs.shape == (N, T, C)
    with pytest.raises(RuntimeError, match="double backwards on temporal_interlace not supported"):
        gs.sum().backward()


def test_empty_tensors():
    x = torch.zeros(0, 5, 4, requires_grad=True)
    w, s = torch.zeros(0, 5, requires_grad=True), torch.zeros(0, 3, 5, requires_grad=True)
    out = temporal_interlace_func(x, w, s, 3, 0, True)
    out.sum().backward()
    assert out.shape == (0, 5, 4) and x.grad.shape == (0, 5, 4) and w.grad.shape == (0, 5) and s.grad.shape == (0, 3, 5)
    x0 = torch.zeros(6, 5, 0, requires_grad=True)
    w0, s0 = torch.ones(2, 5, requires_grad=True), torch.ones(2, 3, 5, requires_grad=True)
    out = temporal_interlace_func(x0, w0, s0, 3, 0, True)
    out.sum().backward()
    assert out.shape == (6, 5, 0) and torch.equal(w0.grad, torch.zeros(2, 5)) and torch.equal(s0.grad, torch.zeros(2, 3, 5))


def test_what_the_node_keeps():
    (shape, T) = SHAPES[1]
    N, C = shape[0] // T, shape[1]
    x = torch.randn(shape, requires_grad=True)
    w, s = torch.zeros(N, C, requires_grad=True), torch.ones(N, T, C, requires_grad=True)
    assert _saved_shapes(lambda: OPS.temporal_interlace(x, w, s, T, 0, True)) == [shape, (N, C), (N, T, C)]


# ---- the layer --------------------------------------------------------------------------------------------------------------------
def _restated(layer, x):
    """the TIN layer in plain torch, as published: slice, OffsetNet, WeightNet, the interpolating shift as a sampler that reads
    x[t + offset], the weight, cat"""
    T, fold = layer.n_segment, layer.fold
    N = x.shape[0] // T
    head, tail = x[:, :fold], x[:, fold:]
    desc = head.reshape(N, T, fold, -1).mean(3).permute(0, 2, 1)                     # [N, fold, T]
    o = layer.offset_net.conv(desc).view(N, T)
    o = 4 * (torch.sigmoid(layer.offset_net.fc2(torch.relu(layer.offset_net.fc1(o)))) - 0.5)   # [N, 2]
    w = 2 * torch.sigmoid(layer.weight_net.conv(desc).permute(0, 2, 1))             # [N, T, 2]
    table, weight = torch.cat((o, -o), 1), torch.cat((w, w), 2)                     # [N, 4], [N, T, 4]
    g = fold // 4
    offsets = (-table).repeat_interleave(g, dim=1)                                  # reading x[t + offset] is out[t] = x[t - (-offset)]
    scales = weight.repeat_interleave(g, dim=2)
    y = temporal_shift_learnable_per_clip_func(head.contiguous(), offsets, T, layer.padding, True)
    y = y * scales.reshape((N * T, fold) + (1,) * (x.dim() - 2))
    return torch.cat((y, tail), 1)


@pytest.mark.parametrize("shift_div", [1, 2])
def test_the_layer_is_its_restatement(shift_div):
    torch.manual_seed(54)
    T, C = 4, 16
    for shape, padding in (((2 * T, C, 3, 2), "zeros"), ((3 * T, C, 5), "border")):
        layer = torchshifts.TemporalInterlace(T, C, shift_div=shift_div, padding=padding).double()
        for p in layer.parameters():                                                # (away from the initial point: every net matters)
            torch.nn.init.normal_(p, std=0.5)
        x = torch.randn(shape, dtype=torch.float64)
        out = layer(x)
        assert isinstance(out, torch.Tensor) and out.shape == x.shape
        assert torch.equal(out, _restated(layer, x))
        if shift_div > 1:
            assert torch.equal(out[:, layer.fold:], x[:, layer.fold:])              # untouched channels: bit-identical
            assert not torch.equal(out[:, :layer.fold], x[:, :layer.fold])
        out.square().mean().backward()
        assert all(p.grad is not None and p.grad.abs().sum() > 0 for p in layer.parameters())


def test_the_initial_offset():
    """the last Linear's bias starts at 0.5108, the WeightNet's conv bias at 0: with the earlier layers' output at zero the offsets
    are 4 * (sigmoid(0.5108) - 0.5) (one frame, roughly 0.5) and the weights 2 * sigmoid(0) = 1"""
    T, C = 8, 8
    layer = torchshifts.TemporalInterlace(T, C)
    assert isinstance(layer.offset_net, torchshifts.OffsetNet) and isinstance(layer.weight_net, torchshifts.WeightNet)
    assert torch.equal(layer.offset_net.fc2.bias, torch.full((2,), 0.5108)) and torch.equal(layer.weight_net.conv.bias, torch.zeros(2))
    x = torch.zeros(2 * T, C, 3, 3)
    with torch.no_grad():
        layer.offset_net.conv.bias.zero_()
        layer.offset_net.fc1.bias.zero_()
    offsets, scales = layer.tables(x)
    first = 4 * (torch.sigmoid(torch.tensor(0.5108)) - 0.5)
    assert offsets.shape == (2, C) and scales.shape == (2, T, C)
    assert torch.allclose(offsets[:, :C // 2], -first.expand(2, C // 2)) and torch.allclose(offsets[:, C // 2:], first.expand(2, C // 2))
    assert torch.equal(scales, torch.ones(2, T, C))
    assert torch.equal(torchshifts.OffsetNet(C, T).fc2.bias, torch.full((2,), 0.5108))


def test_the_layers_state_dict_round_trips():
    torch.manual_seed(55)
    a, b = torchshifts.TemporalInterlace(4, 16, shift_div=2), torchshifts.TemporalInterlace(4, 16, shift_div=2)
    assert sorted(a.state_dict()) == ["offset_net.conv.bias", "offset_net.conv.weight", "offset_net.fc1.bias", "offset_net.fc1.weight",
                                      "offset_net.fc2.bias", "offset_net.fc2.weight", "weight_net.conv.bias", "weight_net.conv.weight"]
    x = torch.randn(8, 16, 3, 3)
    assert not torch.equal(a(x), b(x))
    b.load_state_dict(a.state_dict())
    assert torch.equal(a(x), b(x))
    assert a.extra_repr() == "n_segment=4, in_channels=16, shift_div=2, padding_method=zeros"


def test_a_fold_that_is_no_multiple_of_four_raises():
    for C, div in ((6, 1), (16, 8), (20, 2), (3, 1)):
        with pytest.raises(AssertionError, match="multiple of 4"):
            torchshifts.TemporalInterlace(4, C, shift_div=div)
    with pytest.raises(AssertionError, match="incorrect padding option"):
        torchshifts.TemporalInterlace(4, 8, padding="wrap")
    from torchshifts.modules import OffsetNet, TemporalInterlace, WeightNet   # noqa: F401  (exported from both packages)


# ---- the binding's surface --------------------------------------------------------------------------------------------------------
TIN_FWD = "(Tensor input, Tensor offsets, Tensor scales, int n_segment, int padding_mode, bool active_flag) -> Tensor"
TIN_BWD = ("(Tensor grad, Tensor offsets, Tensor scales, Tensor input, int n_segment, int padding_mode, bool active_flag)"
           " -> (Tensor, Tensor, Tensor)")
INTERLACE_SCHEMAS = {"temporal_interlace": TIN_FWD, "_temporal_interlace_forward": TIN_FWD, "_temporal_interlace_backward": TIN_BWD}
INTERLACE_KERNELS = {"temporal_interlace": COMPOSITE, "_temporal_interlace_forward": FLOAT, "_temporal_interlace_backward": FLOAT}


def test_the_surface_of_the_new_namespace():
    assert registered_ops("torchshifts_interlace") == sorted(INTERLACE_SCHEMAS)
    for op, schema in INTERLACE_SCHEMAS.items():
        name = "torchshifts_interlace::" + op
        assert str(torch._C._get_schema(name, "")) == name + schema
        assert tuple(k for k in KEYS if torch._C._dispatch_has_kernel_for_dispatch_key(name, k)) == INTERLACE_KERNELS[op], op


def test_the_existing_namespaces_keep_their_op_lists():
    assert registered_ops() == sorted(SCHEMAS)
    for namespace in ("torchshifts_per_clip", "torchshifts_inplace"):
        assert [namespace + "::" + op for op in registered_ops(namespace)] == sorted(n for n in LATER_SCHEMAS if n.startswith(namespace + "::"))


# ---- SHIFTND_INTERLACE at the C ABI, host side only: validation happens before any device work.  With NULL tensors an accepted geometry
# ends in INVALID_ARGUMENT (the tensors are refused) and its workspace query answers the plan's bytes; a refused problem answers 0.
def test_the_interlace_flag_host_side():
    from torchshifts import abi
    INVALID, UNSUPPORTED = -1, -2
    L = abi.lib()
    assert L.shiftnd_abi_version() == 5 and len(abi.EXPORTS) == 20
    assert abi.INTERLACE == 0x8000 and abi.problem(torch.zeros(2, 5, 3, 8), 0, 0, None, shift_dim0=True, interlace=True).dtype == 0x8200
    st = (ctypes.c_int64 * 5)(3 * 5 * 8, 8, 5 * 8, 1, 0)   # [N, C, T, M] = [2, 5, 3, 8] in memory order N, T, C, M
    nhwc = (ctypes.c_int64 * 5)(3 * 8 * 5, 1, 8 * 5, 5, 0)
    byref = ctypes.byref
    DIM0, IL = abi.SHIFT_DIM0, abi.INTERLACE

    def forward(p, x=None, out=None, s=st, w=None):
        return L.shiftnd_forward(byref(p), x, s, w, out, s, None)

    def backward(p, s=st):
        return L.shiftnd_backward(byref(p), None, s, None, s, None, None, s, None, None, 0, None)

    def workspace(p):
        return L.shiftnd_backward_workspace_bytes(byref(p))

    pool = (ctypes.c_int32 * 3)(2, 2, 1)
    for dt in (abi.F32, abi.F64, abi.F16, abi.BF16, abi.F16 | abi.WEIGHTS_F32, abi.BF16 | abi.WEIGHTS_F32):
        es = {abi.F32: 4, abi.F64: 8}.get(dt, 2)
        for active in (0, 1):
            ok = _problem(2, dt | DIM0 | IL, active=active)
            assert forward(ok) == INVALID and backward(ok) == INVALID                 # accepted: the NULL tensors are refused
            # both partial sets, a function of the geometry alone: chunks * N * C * (1 + 4 T) records of 24 bytes
            assert workspace(ok) == 2 * 5 * (1 + 4 * 3) * 24
            big = dict(sizes=(2, 5, 3, 5000, 1), borders=(0, 3, 0, 5000, 0, 1), active=active)
            assert workspace(_problem(2, dt | DIM0 | IL, **big)) == -(-5000 * es // 8192) * 2 * 5 * (1 + 4 * 3) * 24
            assert workspace(_problem(2, dt | DIM0 | IL, sizes=(0, 5, 3, 8, 1), active=active)) == 8   # an empty problem: sizeof(double)
            # the bit without SHIFT_DIM0: an unknown dtype bit on every entry point
            alone = _problem(2, dt | IL, active=active)
            assert forward(alone) == UNSUPPORTED and backward(alone) == UNSUPPORTED and workspace(alone) == 0
            assert L.shiftnd_forward_quantized(byref(alone), None, st, None, abi.I32, 0, 0, None, st, None) == UNSUPPORTED
            assert L.shiftnd_forward_pooled(byref(alone), pool, None, None, None, None) == UNSUPPORTED
            assert L.shiftnd_backward_pooled(byref(alone), pool, None, None, None, None, None, None, 0, None) == UNSUPPORTED
            # ... and on the quantized and the pooled entry points with SHIFT_DIM0 too
            assert L.shiftnd_forward_quantized(byref(ok), None, st, None, abi.I32, 0, 0, None, st, None) == UNSUPPORTED
            assert L.shiftnd_forward_pooled(byref(ok), pool, None, None, None, None) == UNSUPPORTED
            assert L.shiftnd_backward_pooled(byref(ok), pool, None, None, None, None, None, None, 0, None) == UNSUPPORTED
            # beside every other bit of the family
            for other in (abi.FRAMES, abi.PER_CLIP, abi.STREAM, abi.CLIP_FRAMES):
                both = _problem(2, dt | DIM0 | other | IL, active=active)
                for s in (st, nhwc):
                    assert forward(both, s=s) == INVALID and backward(both, s=s) == INVALID, hex(other)
                assert workspace(both) == 0, hex(other)
            # out == x: refused before the pointer is looked at (4096 is no allocation)
            assert forward(ok, x=ctypes.c_void_p(4096), out=ctypes.c_void_p(4096)) == INVALID
            # channels-last tensors: refused by their strides (pointers that are no allocation, never looked at)
            assert forward(ok, x=ctypes.c_void_p(4096), out=ctypes.c_void_p(8192), s=nhwc, w=ctypes.c_void_p(12288)) == INVALID
            # a cut window, ndim 1
            cut = _problem(2, dt | DIM0 | IL, borders=(1, 3, 0, 8, 0, 1), active=active)
            assert forward(cut) == INVALID and backward(cut) == INVALID and workspace(cut) == 0
            one = _problem(1, dt | DIM0 | IL, sizes=(2, 5, 24, 1, 1), borders=(0, 24, 0, 1, 0, 1), active=active)
            assert forward(one) == INVALID and backward(one) == INVALID and workspace(one) == 0
    # the x == NULL && grad_w == NULL form does not exist under the flag (here: on an accepted geometry, every other pointer NULL too)
    assert backward(_problem(2, abi.F32 | DIM0 | IL)) == INVALID
    # a quantized dtype, and WEIGHTS_F32 on a dtype that has no mixed form
    for dt in (abi.U8, abi.I8, abi.I32, abi.F32 | abi.WEIGHTS_F32):
        p = _problem(2, dt | DIM0 | IL)
        assert forward(p) == UNSUPPORTED and backward(p) == UNSUPPORTED and workspace(p) == 0
        assert L.shiftnd_forward_quantized(byref(p), None, st, None, abi.I32, 0, 0, None, st, None) == UNSUPPORTED
    # 0x800 stays unassigned: an unknown bit, with and without the new one
    for bits in (0x800, 0x800 | DIM0, 0x800 | DIM0 | IL, 0x800 | IL):
        p = _problem(2, abi.F32 | bits)
        assert forward(p) == UNSUPPORTED and backward(p) == UNSUPPORTED
    assert workspace(_problem(2, abi.F32 | 0x800 | DIM0 | IL)) == 0


def test_the_size_bounds_host_side():
    """N * T * C = 2^31 on both sides, and the tshift family's limit of 2^31 - 16 two-byte units.  Planes of one two-byte element: a
    plane is one unit, so planes < 2^31 - 16 is the tighter of the two there; 2^31 planes is beyond both, so the plane bound is
    also shown alone on the largest count the unit limit admits and the unit limit on both of its sides."""
    from torchshifts import abi
    L = abi.lib()
    DIM0, IL = abi.SHIFT_DIM0, abi.INTERLACE

    def workspace(N, C, T, M, dt=abi.F16):
        return L.shiftnd_backward_workspace_bytes(ctypes.byref(_problem(2, dt | DIM0 | IL, sizes=(N, C, T, M, 1), borders=(0, T, 0, M, 0, 1))))

    def forward(N, C, T, M, dt=abi.F16):
        st = (ctypes.c_int64 * 5)(T * C * M, M, C * M, 1, 0)
        p = _problem(2, dt | DIM0 | IL, sizes=(N, C, T, M, 1), borders=(0, T, 0, M, 0, 1))
        return L.shiftnd_forward(ctypes.byref(p), None, st, None, None, st, None)

    # N * T * C = 2^31: refused; one clip fewer (2^31 - 2^23 planes, as many two-byte units): accepted
    assert workspace(1 << 8, 1 << 15, 1 << 8, 1) == 0 and forward(1 << 8, 1 << 15, 1 << 8, 1) == -1
    below = ((1 << 8) - 1, 1 << 15, 1 << 8, 1)
    assert workspace(*below) == below[0] * below[1] * (1 + 4 * below[2]) * 24 and forward(*below) == -1   # (accepted; the NULL tensors)
    # ... also when T carries the product: N = 1, C = 2^15, T = 2^16
    assert workspace(1, 1 << 15, 1 << 16, 1) == 0 and workspace(1, (1 << 15) - 1, 1 << 16, 1) > 0
    # the unit limit, planes of two units: N * T * C * 2 + 16 < 2^31
    assert workspace(1, (1 << 15) - 1, 1 << 15, 2) > 0                   # 2^31 - 2^16 units
    assert workspace(1, 1 << 15, 1 << 15, 2) == 0                        # 2^31 units, 2^30 planes: the unit limit alone
    assert workspace(1, 1, (1 << 30) - 9, 2) > 0 and workspace(1, 1, (1 << 30) - 8, 2) == 0   # 2^31 - 18 and 2^31 - 16 units
    # four-byte elements count two units each
    assert workspace(1, 1, (1 << 29) - 5, 2, abi.F32) > 0 and workspace(1, 1, (1 << 29) - 4, 2, abi.F32) == 0
