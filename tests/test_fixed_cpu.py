"""Fixed (grouped) shifts on CPU tensors: torch.ops.torchshifts.shift{N}d_fixed, its grad_x-only backward, the GroupedShift{N}d
modules -- every result against the C oracle, bit for bit (a sparse shift is a pure gather in both directions).

The oracle's grad_x of a sparse shift does not depend on x, so O.backward(go, s, x, ...)[0] with the real x is the reference
of the backward that never sees x.
"""
import itertools

import numpy as np
import pytest
import torch

import torchshifts
from torchshifts import abi
from torchshifts.functional import shift1d_fixed_func, shift2d_fixed_func, shift3d_fixed_func
from oracle import oracle as O

OPS = torch.ops.torchshifts
FUNCS = {1: shift1d_fixed_func, 2: shift2d_fixed_func, 3: shift3d_fixed_func}
SHAPES = {1: (2, 5, 13), 2: (2, 5, 7, 9), 3: (2, 4, 5, 6, 7)}
CUTS = {1: [[1, 2]], 2: [[1, 2], [0, 1]], 3: [[1, 2], [0, 1], [2, 0]]}


def _table(rs, C, nd, big):
    s = rs.randint(-3, 4, size=(C, nd))
    if big:
        s[0] = 40          # larger than every axis
        s[1] = -23
    return s.astype(np.int64)


def _run(x, s_t, pad, cut):
    nd = x.ndim - 2
    xt = torch.from_numpy(x.copy()).requires_grad_(True)
    b = None if cut is None else torch.tensor(cut, dtype=torch.long)
    out = FUNCS[nd](xt, s_t, pad, b)
    return xt, out


@pytest.mark.parametrize("nd", [1, 2, 3])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_op_matches_oracle_bit_exact(nd, dt):
    rs = np.random.RandomState(100 + nd)
    shape = SHAPES[nd]
    n = 0
    for pad, cut, big, sdt in itertools.product(range(5), (None, CUTS[nd]), (False, True), (torch.int32, torch.int64, torch.float32)):
        x = rs.uniform(-1, 1, size=shape).astype(dt)
        s = _table(rs, shape[1], nd, big)
        b = abi.default_borders(torch.from_numpy(x)) if cut is None else abi.check_borders(list(shape), cut, nd)[0]
        s_t = torch.from_numpy(s).to(sdt)
        xt, out = _run(x, s_t, pad, cut)
        go = rs.uniform(-1, 1, size=tuple(out.shape)).astype(dt)
        out.backward(torch.from_numpy(go))
        key = "nd%d %s pad%d cut%s big%d %s" % (nd, dt.__name__, pad, cut, big, sdt)
        assert np.array_equal(out.detach().numpy(), O.forward(x, s.astype(dt), pad, False, b)), "forward " + key
        assert np.array_equal(xt.grad.numpy(), O.backward(go, s.astype(dt), x, pad, False, b)[0]), "grad_x " + key
        assert s_t.grad is None
        n += 1
    assert n == 60


def test_float_table_rounds_half_to_even():
    rs = np.random.RandomState(5)
    x = rs.uniform(-1, 1, size=(2, 4, 6, 8)).astype(np.float32)
    s = np.array([[0.5, 1.5], [-0.5, -1.5], [2.5, 0.25], [-2.5, 1.75]], np.float32)
    xt, out = _run(x, torch.from_numpy(s), 3, None)
    go = rs.uniform(-1, 1, size=x.shape).astype(np.float32)
    out.backward(torch.from_numpy(go))
    assert np.array_equal(out.detach().numpy(), O.forward(x, s, 3, False))
    assert np.array_equal(xt.grad.numpy(), O.backward(go, s, x, 3, False)[0])


def test_backward_op_alone_and_double_backward_raises():
    rs = np.random.RandomState(6)
    x = rs.uniform(-1, 1, size=(2, 3, 8, 8)).astype(np.float32)
    s = _table(rs, 3, 2, False)
    b, new = abi.check_borders(list(x.shape), [[1, 1], [1, 1]], 2)
    go = rs.uniform(-1, 1, size=new).astype(np.float32)
    gx = OPS._shift2d_fixed_backward(torch.from_numpy(go), torch.from_numpy(s), torch.tensor(b, dtype=torch.int32), list(x.shape), 1)
    assert np.array_equal(gx.numpy(), O.backward(go, s.astype(np.float32), x, 1, False, b)[0])
    xt = torch.from_numpy(x).requires_grad_(True)
    out = shift2d_fixed_func(xt, torch.from_numpy(s), 1)
    seed = torch.ones_like(out, requires_grad=True)
    g, = torch.autograd.grad(out, xt, seed, create_graph=True)
    with pytest.raises(RuntimeError, match="double backwards"):
        g.sum().backward()


def _packed_numels(fn):
    seen = []

    def pack(t):
        seen.append(t.numel())
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        fn()
    return seen


def test_the_node_saves_no_input():
    x = torch.randn(2, 6, 10, 12, requires_grad=True)
    s = torch.randint(-2, 3, (6, 2))
    w = s.float().requires_grad_(True)
    fixed = _packed_numels(lambda: shift2d_fixed_func(x, s, 0))
    assert x.numel() not in fixed, fixed
    learnable = _packed_numels(lambda: OPS.shift2d(x, w, torch.Tensor(), 0, False))
    assert x.numel() in learnable, learnable   # what "saves no input" is measured against


def test_default_table_written_out():
    m = torchshifts.GroupedShift2d(20, kernel_size=3)
    expect = [[-1, -1], [-1, -1], [-1, 0], [-1, 0], [-1, 1], [-1, 1],
              [0, -1], [0, -1], [0, 0], [0, 0], [0, 1], [0, 1],
              [1, -1], [1, -1], [1, 0], [1, 0], [1, 1], [1, 1],
              [0, 0], [0, 0]]
    assert m.shifts.dtype == torch.int64 and m.shifts.tolist() == expect
    assert torchshifts.GroupedShift1d(7, kernel_size=3).shifts.tolist() == [[-1], [-1], [0], [0], [1], [1], [0]]
    assert torchshifts.GroupedShift3d(27, kernel_size=3).shifts[5].tolist() == [-1, 0, 1]
    assert torchshifts.GroupedShift2d(4, kernel_size=3).shifts.tolist() == [[0, 0]] * 4   # fewer channels than groups


def test_module_has_a_buffer_and_no_parameters():
    m = torchshifts.GroupedShift2d(20, shifts=torch.randint(-4, 5, (20, 2)))
    assert list(m.parameters()) == []
    sd = m.state_dict()
    assert list(sd.keys()) == ["shifts"]
    m2 = torchshifts.GroupedShift2d(20)
    assert not torch.equal(m2.shifts, m.shifts)
    m2.load_state_dict(sd)
    assert torch.equal(m2.shifts, m.shifts)
    x = torch.randn(2, 20, 9, 9)
    out, loss = m2(x)
    assert loss is None
    assert np.array_equal(out.numpy(), O.forward(x.numpy(), m.shifts.numpy().astype(np.float32), 0, False))


@pytest.mark.parametrize("emulate", [None, {"kernel_size": 3, "stride": 1, "padding": 0}, {"kernel_size": 3, "stride": 2, "padding": 0}])
@pytest.mark.parametrize("padding", ["zeros", "reflect"])
def test_from_shift_equals_the_source_module(emulate, padding):
    torch.manual_seed(3)
    src = torchshifts.Shift2d(6, padding=padding, init_shift=3, sparsity_term=0, emulate_dw=None if emulate is None else dict(emulate))
    with torch.no_grad():
        src.weight[0] = torch.tensor([0.5, -1.5])   # ties: half to even
        src.weight[1] = torch.tensor([2.5, 1.5])
    frozen = torchshifts.GroupedShift2d.from_shift(src)
    assert torch.equal(frozen.shifts, torch.round(src.weight.detach()).to(torch.int64))
    assert list(frozen.parameters()) == []
    x1 = torch.randn(2, 6, 11, 12, requires_grad=True)
    x2 = x1.detach().clone().requires_grad_(True)
    o1, _ = src(x1)
    o2, none = frozen(x2)
    assert none is None and o1.shape == o2.shape
    assert torch.equal(o1, o2)
    go = torch.randn_like(o1)
    o1.backward(go)
    o2.backward(go)
    assert torch.equal(x1.grad, x2.grad)


def test_emulate_dw_of_the_module_itself():
    m = torchshifts.GroupedShift2d(9, emulate_dw={"kernel_size": 3, "stride": 2, "padding": 0})
    assert m.cut_borders.tolist() == [[1, 1], [1, 1]] and m._pool_size == [2, 2]
    x = torch.randn(1, 9, 10, 10)
    out, _ = m(x)
    b, _ = abi.check_borders(list(x.shape), [[1, 1], [1, 1]], 2)
    shifted = torch.from_numpy(O.forward(x.numpy(), m.shifts.numpy().astype(np.float32), 0, False, b))
    assert torch.equal(out, torch.nn.functional.avg_pool2d(shifted, 2, 2, ceil_mode=True))


def test_from_shift_of_an_active_module_raises():
    with pytest.raises(ValueError):
        torchshifts.GroupedShift2d.from_shift(torchshifts.Shift2d(4, active_flag=True))


def test_the_existing_backward_op_still_returns_both_gradients():
    rs = np.random.RandomState(9)
    x = rs.uniform(-1, 1, size=(2, 3, 8, 10)).astype(np.float32)
    w = rs.uniform(-2, 2, size=(3, 2)).astype(np.float32)
    go = rs.uniform(-1, 1, size=x.shape).astype(np.float32)
    b = torch.tensor(abi.default_borders(torch.from_numpy(x)), dtype=torch.int32)
    gx_o, _ = O.backward(go, w, x, 0, False)
    _, gw_o = O.backward(go.astype(np.float64), w.astype(np.float64), x.astype(np.float64), 0, False)
    for requires in (True, False):
        wt = torch.from_numpy(w.copy()).requires_grad_(requires)
        gx, gw = OPS._shift2d_backward(torch.from_numpy(go), wt, torch.from_numpy(x), b, 0, False)
        assert gx is not None and gw is not None
        assert np.array_equal(gx.detach().numpy(), gx_o)
        assert np.abs(gw.detach().numpy() - gw_o).max() <= 1e-5 * np.abs(gw_o).max()
