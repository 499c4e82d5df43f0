"""Fixed shift + average pool on CPU tensors: torch.ops.torchshifts.shift{N}d_fixed_pool is the composed sequence there -- the
fixed shift, then ATen's avg_pool{N}d(kernel = stride = pool, ceil_mode=True) -- so the op and its autograd are compared bit for bit
with that sequence; the strided GroupedShift modules; the schemas; the refusals of shiftnd_backward_pooled's input-gradient-only
form that need no device.
"""
import ctypes

import numpy as np
import pytest
import torch

import torchshifts
from torchshifts import abi
from torchshifts.functional import (shift1d_fixed_func, shift1d_fixed_pool_func, shift2d_fixed_func, shift2d_fixed_pool_func,
                                    shift3d_fixed_func, shift3d_fixed_pool_func)

OPS = torch.ops.torchshifts
FIXED = {1: shift1d_fixed_func, 2: shift2d_fixed_func, 3: shift3d_fixed_func}
FUSED = {1: shift1d_fixed_pool_func, 2: shift2d_fixed_pool_func, 3: shift3d_fixed_pool_func}
POOLS = {1: torch.nn.functional.avg_pool1d, 2: torch.nn.functional.avg_pool2d, 3: torch.nn.functional.avg_pool3d}


def _table(rs, C, nd):
    s = rs.randint(-3, 4, size=(C, nd))
    s[0] = 0
    s[1] = 40          # larger than every axis
    s[2] = -5
    return torch.from_numpy(s.astype(np.int64))


@pytest.mark.parametrize("shape,pool", [((2, 9, 13, 20), 2), ((2, 9, 13, 20), 3), ((2, 8, 36), 2), ((2, 8, 36), 3), ((2, 8, 6, 7, 8), 2),
                                        ((2, 8, 6, 7, 8), (2, 3, 2))])
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_cpu_op_is_the_composed_sequence(shape, pool, dt):
    nd = len(shape) - 2
    rs = np.random.RandomState(7 + sum(shape))
    s = _table(rs, shape[1], nd)
    k = [pool] * nd if isinstance(pool, int) else list(pool)
    for pad in range(5):
        for cut in (None, torch.tensor([[1, 1]] * nd, dtype=torch.long)):
            x = torch.from_numpy(rs.uniform(-1, 1, size=shape)).to(dt)
            xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
            out = FUSED[nd](xa, s, pad, pool, cut)
            ref = POOLS[nd](FIXED[nd](xb, s, pad, cut), kernel_size=k, stride=k, ceil_mode=True)
            assert out.shape == ref.shape and torch.equal(out, ref), (shape, pool, pad)
            go = torch.from_numpy(rs.uniform(-1, 1, size=tuple(out.shape))).to(dt)
            out.backward(go)
            ref.backward(go)
            assert torch.equal(xa.grad, xb.grad), (shape, pool, pad)
            assert s.grad is None


def _packed_numels(fn):
    seen = []

    def pack(t):
        seen.append(t.numel())
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        fn()
    return seen


def test_the_node_saves_no_tensor_of_the_inputs_size():
    x = torch.randn(2, 9, 13, 20, requires_grad=True)
    s = _table(np.random.RandomState(0), 9, 2)
    cut = torch.tensor([[1, 1], [1, 1]])
    fused = _packed_numels(lambda: OPS.shift2d_fixed_pool(x, s, cut, [2, 2], 0))
    assert fused and max(fused) <= s.numel(), fused   # the table and the 6 borders
    composed = _packed_numels(lambda: torch.nn.functional.avg_pool2d(OPS.shift2d_fixed(x, s, cut, 0), 2, 2, ceil_mode=True))
    assert 2 * 9 * 11 * 18 in composed, composed   # what it is measured against: the pool keeps the full-size shift output


def test_backward_op_alone_and_double_backward_raises():
    rs = np.random.RandomState(3)
    s = _table(rs, 9, 2)
    x = torch.from_numpy(rs.uniform(-1, 1, size=(2, 9, 13, 20)).astype(np.float32)).requires_grad_(True)
    cut = torch.tensor([[1, 1], [1, 1]])
    out = OPS.shift2d_fixed_pool(x, s, cut, [2, 2], 3)
    go = torch.randn_like(out)
    gx, = torch.autograd.grad(out, x, go)
    b, _ = abi.check_borders([2, 9, 13, 20], [[1, 1], [1, 1]], 2)
    alone = OPS._shift2d_fixed_pool_backward(go, s, torch.tensor(b, dtype=torch.int32), [2, 9, 13, 20], [2, 2], 3)
    assert torch.equal(alone, gx)
    g = go.clone().requires_grad_(True)
    gi = OPS._shift2d_fixed_pool_backward(g, s, torch.tensor(b, dtype=torch.int32), [2, 9, 13, 20], [2, 2], 3)
    with pytest.raises(RuntimeError, match="double backwards"):
        gi.sum().backward()


@pytest.mark.parametrize("cls,shape", [(torchshifts.GroupedShift1d, (2, 9, 21)), (torchshifts.GroupedShift2d, (2, 9, 13, 20)),
                                       (torchshifts.GroupedShift3d, (2, 27, 6, 7, 8))])
@pytest.mark.parametrize("stride", [2, 3])
def test_module_with_a_stride_is_unchanged(cls, shape, stride):
    nd = len(shape) - 2
    m = cls(shape[1], padding="reflect", emulate_dw={"kernel_size": 3, "stride": stride, "padding": 0})
    assert sorted(m.state_dict().keys()) == ["shifts"] and list(m.parameters()) == []
    x = torch.randn(shape)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    out, none = m(xa)
    ref = POOLS[nd](FIXED[nd](xb, m.shifts, m.padding, m.cut_borders), kernel_size=[stride] * nd, stride=[stride] * nd, ceil_mode=True)
    assert none is None and torch.equal(out, ref)
    go = torch.randn_like(out)
    out.backward(go)
    ref.backward(go)
    assert torch.equal(xa.grad, xb.grad)


def test_from_shift_of_a_strided_module():
    torch.manual_seed(2)
    src = torchshifts.Shift2d(6, padding="symmetric", init_shift=3, sparsity_term=0, emulate_dw={"kernel_size": 3, "stride": 2, "padding": 0})
    frozen = torchshifts.GroupedShift2d.from_shift(src)
    x = torch.randn(2, 6, 13, 20)
    assert torch.equal(frozen(x)[0], src(x)[0])


def test_schemas():
    for nd in (1, 2, 3):
        fwd = getattr(OPS, "shift%dd_fixed_pool" % nd).default._schema
        bwd = getattr(OPS, "_shift%dd_fixed_pool_backward" % nd).default._schema
        assert str(fwd) == ("torchshifts::shift%dd_fixed_pool(Tensor input, Tensor shifts, Tensor borders, int[] pool, "
                            "int padding_mode) -> Tensor" % nd)
        assert str(bwd) == ("torchshifts::_shift%dd_fixed_pool_backward(Tensor grad, Tensor shifts, Tensor borders, "
                            "int[] input_size, int[] pool, int padding_mode) -> Tensor" % nd)


def test_exports_are_unchanged():
    assert len(abi.EXPORTS) == 20 and len(set(abi.EXPORTS)) == 20
    assert callable(abi.backward_pooled_input)


def test_refused_forms_need_no_device():
    """argument validation of shiftnd_backward_pooled's input-gradient-only form happens before any device work"""
    L = abi.lib()
    like = torch.empty(2, 3, 12, 16)
    pool = (ctypes.c_int32 * 2)(2, 2)
    one = ctypes.c_void_p(16)   # a non-NULL pointer nobody dereferences: the call is refused first
    active, sparse = abi.problem(like, 0, True, None), abi.problem(like, 0, False, None)
    call = lambda p, gp, x, w, gx, gw: L.shiftnd_backward_pooled(ctypes.byref(p), pool, gp, x, w, gx, gw, None, 0, None)
    assert call(active, one, None, one, one, None) == -1    # the NULL form of an active shift
    assert call(sparse, one, None, one, one, one) == -1     # only x NULL
    assert call(sparse, one, one, one, one, None) == -1     # only grad_w NULL
    assert call(sparse, None, None, one, one, None) == -1   # no grad_pooled
    assert call(sparse, one, None, None, one, None) == -1   # no table
    empty = abi.problem(torch.empty(0, 3, 12, 16), 0, True, None)
    assert call(empty, one, None, one, one, None) == -1     # ... of an empty problem too: the form does not exist


def test_quantized_input_raises():
    xq = torch.quantize_per_tensor(torch.randn(1, 4, 8, 8), 0.1, 0, torch.quint8)
    with pytest.raises(RuntimeError, match="quantized inputs are not supported"):
        OPS.shift2d_fixed_pool(xq, torch.zeros(4, 2, dtype=torch.int64), torch.Tensor(), [2, 2], 0)
