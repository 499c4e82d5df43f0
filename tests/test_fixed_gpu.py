"""GPU: the input gradient of the sparse shift without the input -- shiftnd_backward's x == NULL && grad_w == NULL form
(abi.backward_input), the ops torch.ops.torchshifts.shift{N}d_fixed on HIP tensors and the GroupedShift modules.  Every result is
compared with the C oracle, bit for bit (pure gathers).  The oracle has float32 / float64 paths only: 16-bit gradients are drawn in
the 16-bit type, the oracle runs on the widened float32 copy and equality is required after narrowing (exact; |shift| <= 256).
"""
import ctypes

import numpy as np
import pytest
import torch

import torchshifts
from torchshifts import abi
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPS = torch.ops.torchshifts
TDT = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16, "bf16": torch.bfloat16}


def _draw(rs, shape, tdt):
    """values of the tensor dtype, as (host tensor of that dtype, numpy array the oracle takes)"""
    t = torch.from_numpy(rs.uniform(-1, 1, size=shape)).to(tdt)
    return t, (t.numpy() if tdt in (torch.float32, torch.float64) else t.float().numpy())


def _shifts(rs, C, nd, sizes):
    s = rs.randint(-3, 4, size=(C, nd)).astype(np.float64)
    s[0] = 0
    if C > 1:
        s[1] = [min(sz + 2, 256) for sz in sizes]   # beyond the axis
    if C > 2:
        s[2] = [-min(sz // 2, 256) for sz in sizes]
    return s


def _check(shape, cut, dt, pads, layout="contiguous", expect=None, seed=0):
    """abi.backward_input against the oracle for one tensor; returns the kernels that ran"""
    tdt = TDT[dt]
    nd = len(shape) - 2
    b, new = abi.check_borders(list(shape), cut, nd)
    rs = np.random.RandomState(seed + sum(shape))
    g_t, g_np = _draw(rs, new, tdt)
    s = _shifts(rs, shape[1], nd, new[2:])
    w_np = s.astype(g_np.dtype)
    gd = g_t.to(DEV)
    if layout == "channels_last":
        gd = gd.contiguous(memory_format=torch.channels_last if nd == 2 else torch.channels_last_3d)
    elif layout == "permuted":   # the last two dims swapped in memory: neither dense layout
        gd = gd.transpose(-1, -2).contiguous().transpose(-1, -2)
        assert not gd.is_contiguous()
    wd = torch.from_numpy(s).to(tdt).to(DEV)
    x_np = np.zeros(shape, g_np.dtype)   # (the oracle's grad_x of a sparse shift does not read it)
    ran = []
    for pad in pads:
        gx = abi.backward_input(gd, wd, shape, pad, b)
        ran.append(abi.last_kernel())
        ref = torch.from_numpy(O.backward(g_np, w_np, x_np, pad, False, b)[0]).to(tdt)
        assert torch.equal(gx.cpu(), ref), (shape, cut, dt, pad, layout, abi.last_kernel())
        if expect == "forward":
            assert "forward" in abi.last_kernel() and not abi.last_kernel().startswith("gradx"), abi.last_kernel()
        elif expect is not None:
            assert abi.last_kernel() == expect, (shape, cut, dt, pad, abi.last_kernel())
    return ran


def test_c2_like_tensor_no_cut_and_cut():
    for dt in ("f32", "bf16"):
        _check((8, 32, 224, 224), None, dt, (0, 3), expect="forward")
        _check((8, 32, 224, 224), [[1, 1], [1, 1]], dt, (0, 3), expect="gradx_embed")


@pytest.mark.parametrize("dt", ["f32", "f64", "f16", "bf16"])
def test_every_padding_and_element_width(dt):
    _check((2, 5, 24, 32), None, dt, range(5), expect="forward")
    _check((2, 5, 24, 32), [[1, 1], [1, 1]], dt, range(5), expect="gradx_embed")
    _check((2, 5, 24, 32), [[1, 2], [0, 1]], dt, range(5), expect="gradx_embed")
    _check((2, 5, 24, 32), [[0, 0], [3, 9]], dt, range(5), expect="gradx_embed")
    _check((3, 4, 40, 8), [[5, 0], [0, 3]], dt, range(5), expect="gradx_embed")      # rows of one to four pieces
    _check((1, 3, 1, 64), [[0, 0], [1, 1]], dt, range(5), expect="gradx_embed")      # a single row
    _check((2, 3, 6, 8, 16), [[1, 1], [1, 1], [1, 1]], dt, range(5), expect="gradx_embed")
    _check((2, 3, 6, 8, 16), [[2, 0], [0, 0], [0, 1]], dt, range(5), expect="gradx_embed")
    _check((2, 4, 4096), [[1, 2]], dt, range(5), expect="gradx_embed")
    _check((2, 4, 4096), None, dt, range(5), expect="forward")


@pytest.mark.parametrize("dt", ["f32", "f64", "f16", "bf16"])
def test_ragged_rows(dt):
    """rows of grad_x that are not whole 16-byte pieces: no cut -> the forward routes, a cut -> the element-wide kernel"""
    es = torch.empty(0, dtype=TDT[dt]).element_size()
    for shape in ((2, 3, 62, 62), (4, 8, 14, 14), (2, 3, 30, 61), (2, 3, 5, 9, 13), (2, 3, 5, 9, 62)):
        nd = len(shape) - 2
        _check(shape, None, dt, range(5), expect="forward")
        # (62 and 14 fp64 elements are whole pieces: the eligibility rule of gradx_embed, restated)
        _check(shape, [[1, 1]] * nd, dt, range(5), expect="gradx_embed" if (shape[-1] * es) % 16 == 0 else "gradx_gather")
    # ... and whole-piece rows of grad_x over a ragged window are the piece kernel's
    _check((2, 3, 16, 64), [[1, 1], [1, 2]], dt, range(5), expect="gradx_embed")


def test_1d_and_3d_routes():
    _check((4, 8, 4096), [[1, 1]], "f32", (0, 2), expect="gradx_embed")
    _check((4, 8, 4096), [[3, 0]], "f16", (1, 4), expect="gradx_embed")
    _check((4, 16, 16, 112, 112), [[1, 1], [1, 1], [1, 1]], "bf16", (0, 3), expect="gradx_embed")
    _check((4, 16, 16, 112, 112), None, "bf16", (0,), expect="forward")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_channels_last_and_permuted_gradients(dt):
    _check((2, 16, 32, 32), None, dt, range(5), layout="channels_last", expect="forward")
    _check((2, 16, 32, 32), [[1, 1], [1, 1]], dt, range(5), layout="channels_last", expect="gradx_gather")
    _check((2, 6, 32, 32), None, dt, range(5), layout="permuted", expect="forward")
    _check((2, 6, 32, 32), [[1, 1], [1, 1]], dt, range(5), layout="permuted", expect="gradx_gather")
    _check((2, 6, 4, 8, 16), [[1, 0], [1, 1], [0, 1]], dt, (0, 3), layout="channels_last", expect="gradx_gather")


def _guarded(shape, tdt):
    """a contiguous tensor of `shape` inside a larger buffer, 16-byte aligned, with 512 sentinel bytes on either side"""
    es = torch.empty(0, dtype=tdt).element_size()
    n = int(np.prod(shape))
    pad = 512 // es
    big = torch.full((n + 2 * pad,), 7.0, dtype=tdt, device=DEV)
    view = big[pad:pad + n].view(shape)
    view.fill_(3.0)
    assert view.data_ptr() % 16 == 0
    return big, view, pad


@pytest.mark.parametrize("dt", ["f32", "f64", "f16", "bf16"])
@pytest.mark.parametrize("shape,cut", [((2, 3, 14, 14), [[1, 1], [1, 1]]), ((2, 3, 9, 62), [[1, 2], [0, 1]]), ((1, 2, 5, 7, 13), [[1, 1], [1, 1], [1, 1]]),
                                       ((2, 3, 9, 64), [[1, 2], [1, 1]]), ((3, 5, 8, 24), [[0, 1], [3, 2]]), ((1, 2, 5, 7, 16), [[1, 1], [0, 1], [1, 0]]),
                                       ((2, 3, 21), [[2, 1]]), ((2, 3, 9, 62), None), ((2, 3, 9, 64), None)])
def test_nothing_is_written_outside_grad_x(shape, cut, dt):
    """sentinel bytes around grad_x survive every route and padding: rows that end in a partial 16-byte piece (the element-wide
    kernel and the forward routes) and rows of whole pieces (gradx_embed)"""
    tdt = TDT[dt]
    nd = len(shape) - 2
    b, new = abi.check_borders(list(shape), cut, nd)
    rs = np.random.RandomState(11 + sum(shape))
    g_t, g_np = _draw(rs, new, tdt)
    s = _shifts(rs, shape[1], nd, new[2:])
    wd = torch.from_numpy(s).to(tdt).to(DEV)
    for pad in range(5):
        big, gx, p = _guarded(shape, tdt)
        abi.backward_input(g_t.to(DEV), wd, shape, pad, b, grad_x=gx)
        torch.cuda.synchronize()
        assert bool((big[:p] == 7).all()) and bool((big[p + gx.numel():] == 7).all()), (shape, cut, dt, pad, abi.last_kernel())
        ref = torch.from_numpy(O.backward(g_np, s.astype(g_np.dtype), np.zeros(shape, g_np.dtype), pad, False, b)[0]).to(tdt)
        assert torch.equal(gx.cpu(), ref), (shape, cut, dt, pad, abi.last_kernel())


def _raw_backward(p, go, x, w, gx, gw, ws):
    ptr = lambda t: None if t is None else t.data_ptr()
    return abi.lib().shiftnd_backward(ctypes.byref(p), ptr(go), abi.strides5(gx if go is None else go), ptr(x), abi.strides5(gx), ptr(w), ptr(gx),
                                      abi.strides5(gx), ptr(gw), ptr(ws), ws.numel(), None)


def test_refused_argument_forms_launch_nothing():
    shape = (2, 4, 16, 16)
    x = torch.randn(shape, device=DEV)
    go = torch.randn(shape, device=DEV)
    w = torch.randint(-2, 3, (4, 2), device=DEV).float()
    gx = torch.full(shape, 5.0, device=DEV)
    gw = torch.empty_like(w)
    ws = abi.backward_workspace(x, 0, False)
    abi.forward(torch.randn(2, 4, 14, 14, device=DEV).contiguous(memory_format=torch.channels_last), w, 0, False)
    before = (abi.last_path(), abi.last_kernel())
    sparse, active = abi.problem(x, 0, False, None), abi.problem(x, 0, True, None)
    assert _raw_backward(active, go, None, w, gx, None, ws) == -1      # the NULL form of an active shift
    assert _raw_backward(sparse, go, None, w, gx, gw, ws) == -1        # only x NULL
    assert _raw_backward(sparse, go, x, w, gx, None, ws) == -1         # only grad_w NULL
    assert _raw_backward(active, go, x, w, gx, None, ws) == -1
    assert _raw_backward(sparse, None, None, w, gx, None, ws) == -1    # no grad_out
    assert (abi.last_path(), abi.last_kernel()) == before
    torch.cuda.synchronize()
    assert bool((gx == 5.0).all())
    # the whole-input window without room for the negated table: refused before any launch
    assert _raw_backward(sparse, go, None, w, gx, None, ws[:0]) == -3
    assert (abi.last_path(), abi.last_kernel()) == before
    assert _raw_backward(sparse, go, None, w, gx, None, ws[:w.numel() * 4]) == 0
    torch.cuda.synchronize()
    assert np.array_equal(gx.cpu().numpy(), O.backward(go.cpu().numpy(), w.cpu().numpy(), x.cpu().numpy(), 0, False)[0])


@pytest.mark.parametrize("cut", [None, [[1, 1], [1, 1]]])
def test_the_full_backward_did_not_move(cut):
    shape = (4, 8, 64, 64)
    b, new = abi.check_borders(list(shape), cut, 2)
    rs = np.random.RandomState(21)
    x = rs.uniform(-1, 1, size=shape).astype(np.float32)
    go = rs.uniform(-1, 1, size=new).astype(np.float32)
    w = rs.uniform(-3, 3, size=(8, 2)).astype(np.float32)
    xd, gd, wd = (torch.from_numpy(a).to(DEV) for a in (x, go, w))
    for pad in (0, 3):
        gx_in = abi.backward_input(gd, wd, shape, pad, b)
        gx, gw = abi.backward(gd, wd, xd, pad, False, b)
        assert "backward" in abi.last_kernel()
        gx_o, _ = O.backward(go, w, x, pad, False, b)
        _, gw64 = O.backward(go.astype(np.float64), w.astype(np.float64), x.astype(np.float64), pad, False, b)
        assert np.array_equal(gx.cpu().numpy(), gx_o) and np.array_equal(gx_in.cpu().numpy(), gx_o)
        assert np.abs(gw.cpu().numpy() - gw64).max() <= 1e-5 * np.abs(gw64).max()


@pytest.mark.parametrize("nd,shape,cut", [(1, (2, 6, 64), None), (1, (2, 6, 64), [[1, 2]]), (2, (2, 6, 24, 32), None), (2, (2, 6, 24, 32), [[1, 1], [1, 1]]),
                                          (2, (2, 6, 14, 14), [[1, 2], [0, 1]]), (3, (2, 4, 6, 8, 16), None), (3, (2, 4, 6, 8, 16), [[1, 1], [1, 1], [1, 1]])])
def test_fixed_ops_on_hip_tensors(nd, shape, cut):
    op = getattr(OPS, "shift%dd_fixed" % nd)
    for dt, sdt in (("f32", torch.int64), ("f64", torch.int32), ("bf16", torch.int64), ("f16", torch.float32)):
        tdt = TDT[dt]
        rs = np.random.RandomState(31 + sum(shape))
        b, new = abi.check_borders(list(shape), cut, nd)
        x_t, x_np = _draw(rs, shape, tdt)
        g_t, g_np = _draw(rs, new, tdt)
        s = _shifts(rs, shape[1], nd, new[2:])
        for pad in range(5):
            xt = x_t.to(DEV).requires_grad_(True)
            st = torch.from_numpy(s).to(sdt).to(DEV)
            out = op(xt, st, torch.Tensor() if cut is None else torch.tensor(cut, dtype=torch.long), pad)
            out.backward(g_t.to(DEV))
            assert xt.grad.is_contiguous() and st.grad is None
            w_np = s.astype(x_np.dtype)
            assert torch.equal(out.detach().cpu(), torch.from_numpy(O.forward(x_np, w_np, pad, False, b)).to(tdt)), (dt, pad)
            assert torch.equal(xt.grad.cpu(), torch.from_numpy(O.backward(g_np, w_np, x_np, pad, False, b)[0]).to(tdt)), (dt, pad)


def test_fixed_op_takes_a_channels_last_gradient():
    shape = (2, 16, 32, 32)
    rs = np.random.RandomState(41)
    x = rs.uniform(-1, 1, size=shape).astype(np.float32)
    s = _shifts(rs, 16, 2, shape[2:])
    for cut in (None, [[1, 1], [1, 1]]):
        b, new = abi.check_borders(list(shape), cut, 2)
        go = rs.uniform(-1, 1, size=new).astype(np.float32)
        xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
        out = OPS.shift2d_fixed(xt, torch.from_numpy(s).long().to(DEV), torch.Tensor() if cut is None else torch.tensor(cut), 3)
        out.backward(torch.from_numpy(go).to(DEV).contiguous(memory_format=torch.channels_last))
        assert xt.grad.is_contiguous()
        assert np.array_equal(xt.grad.cpu().numpy(), O.backward(go, s.astype(np.float32), x, 3, False, b)[0])


@pytest.mark.parametrize("cut", [None, [[1, 1], [1, 1]]])
def test_graph_capture_of_forward_and_backward(cut):
    shape = (4, 16, 56, 64)
    rs = np.random.RandomState(51)
    b, new = abi.check_borders(list(shape), cut, 2)
    s = _shifts(rs, 16, 2, new[2:])
    st = torch.from_numpy(s).long().to(DEV)
    bt = torch.Tensor() if cut is None else torch.tensor(cut, dtype=torch.long)
    x_static = torch.zeros(shape, device=DEV, requires_grad=True)
    g_static = torch.zeros(new, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture
        for _ in range(2):
            out = OPS.shift2d_fixed(x_static, st, bt, 0)
            gx, = torch.autograd.grad(out, x_static, g_static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_static = OPS.shift2d_fixed(x_static, st, bt, 0)
        gx_static, = torch.autograd.grad(out_static, x_static, g_static)
    for rep in range(2):
        x = rs.uniform(-1, 1, size=shape).astype(np.float32)
        go = rs.uniform(-1, 1, size=new).astype(np.float32)
        with torch.no_grad():
            x_static.copy_(torch.from_numpy(x))
            g_static.copy_(torch.from_numpy(go))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out_static.detach().cpu().numpy(), O.forward(x, s.astype(np.float32), 0, False, b))
        assert np.array_equal(gx_static.cpu().numpy(), O.backward(go, s.astype(np.float32), x, 0, False, b)[0])


def test_module_on_the_device_and_from_shift():
    torch.manual_seed(5)
    src = torchshifts.Shift2d(8, padding="reflect", init_shift=3, sparsity_term=0, emulate_dw={"kernel_size": 3, "stride": 2, "padding": 0}).to(DEV)
    frozen = torchshifts.GroupedShift2d.from_shift(src)
    assert frozen.shifts.is_cuda and list(frozen.parameters()) == []
    x = torch.randn(2, 8, 30, 32, device=DEV)
    out, none = frozen(x.clone().requires_grad_(True))
    b, _ = abi.check_borders(list(x.shape), [[1, 1], [1, 1]], 2)
    shifted = torch.from_numpy(O.forward(x.cpu().numpy(), frozen.shifts.cpu().numpy().astype(np.float32), 3, False, b))
    ref = torch.nn.functional.avg_pool2d(shifted, 2, 2, ceil_mode=True)
    assert none is None and torch.allclose(out.detach().cpu(), ref, rtol=0, atol=1e-6)   # (ATen's pool on two devices)
    m = torchshifts.GroupedShift2d(18).to(DEV)
    xt = x[:, :1].repeat(1, 18, 1, 1).requires_grad_(True)
    o, _ = m(xt)
    go = torch.randn_like(o)
    o.backward(go)
    w = m.shifts.cpu().numpy().astype(np.float32)
    assert np.array_equal(o.detach().cpu().numpy(), O.forward(xt.detach().cpu().numpy(), w, 0, False))
    assert np.array_equal(xt.grad.cpu().numpy(), O.backward(go.cpu().numpy(), w, xt.detach().cpu().numpy(), 0, False)[0])


def _chain_peak(layers, x):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    xt = x.requires_grad_(True)
    h = xt
    for m in layers:
        h, _ = m(h)
    h.backward(torch.ones_like(h))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    xt.grad = None
    return peak


def test_a_chain_of_fixed_layers_pins_no_activations():
    """forward + backward of 4 layers on an 8 x 64 x 224 x 224 fp32 tensor.  Each Shift2d node pins its input until the backward
    reaches it; of those 4 tensors the first is the caller's own, so a chain of GroupedShift2d is 3 activations lighter at the
    peak.  One is given away for allocator rounding and the small workspaces: at least 2 activations' bytes must be saved."""
    shape = (8, 64, 224, 224)
    act = int(np.prod(shape)) * 4
    learn = [torchshifts.Shift2d(64, sparsity_term=0).to(DEV) for _ in range(4)]
    for m in learn:
        m.weight.requires_grad_(False)   # frozen the only way there was
    fixed = [torchshifts.GroupedShift2d.from_shift(m) for m in learn]
    x = torch.randn(shape, device=DEV)
    p_learn = _chain_peak(learn, x.clone())
    p_fixed = _chain_peak(fixed, x.clone())
    print("peak bytes: frozen Shift2d chain %d, GroupedShift2d chain %d, activation %d" % (p_learn, p_fixed, act))
    assert p_learn - p_fixed >= 2 * act, (p_learn, p_fixed, act)
