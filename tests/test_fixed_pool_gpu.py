"""GPU: fixed shifts with a stride -- shiftnd_backward_pooled's x == NULL && grad_w == NULL form (abi.backward_pooled_input), the ops
torch.ops.torchshifts.shift{N}d_fixed_pool on HIP tensors and the strided GroupedShift modules.

The input gradient is a gather of the pooled gradient with one division in the compute type, so every grad_x is compared with the C
oracle bit for bit: O.backward_pooled(gp, w, zeros, pad, False, pool, b)[0].  The oracle has float32 / float64 paths only: 16-bit
gradients are drawn in the 16-bit type, O.avg_pool_backward runs on the widened copy (the fp32 division), the result is narrowed
once, and O.backward of that (a pure gather) must equal the kernel's output.
"""
import ctypes

import numpy as np
import pytest
import torch

import torchshifts
from torchshifts import abi
from torchshifts.functional import shift2d_fixed_func, shift3d_fixed_func
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPS = torch.ops.torchshifts
TDT = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16, "bf16": torch.bfloat16}
# grad_x rows of whole 16-byte pieces (contiguous tensors, aligned bases) run the piece kernel, everything else the element-wide one
PIECES, ELEMENTS = "gradx_embed_pool", "gradx_gather_pool"


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


def _pool_list(pool, nd):
    return [int(pool)] * nd if isinstance(pool, int) else [int(k) for k in pool]


def _pooled_shape(new, k):
    return list(new[:2]) + [-(-n // kk) for n, kk in zip(new[2:], k)]


def _reference(gp_np, w_np, shape, pad, k, b, new, tdt):
    """grad_x of the oracle, as a host tensor of the tensor dtype"""
    zeros = np.zeros(shape, gp_np.dtype)
    if tdt in (torch.float32, torch.float64):
        return torch.from_numpy(O.backward_pooled(gp_np, w_np, zeros, pad, False, k, b)[0])
    g = torch.from_numpy(O.avg_pool_backward(gp_np, k, new[2:])).to(tdt).float().numpy()   # divided in fp32, narrowed once
    return torch.from_numpy(O.backward(g, w_np, zeros, pad, False, b)[0]).to(tdt)


def _check(shape, pool, cut, dt, pads=range(5), expect=None, seed=0):
    tdt = TDT[dt]
    nd = len(shape) - 2
    k = _pool_list(pool, nd)
    b, new = abi.check_borders(list(shape), cut, nd)
    rs = np.random.RandomState(seed + sum(shape))
    gp_t, gp_np = _draw(rs, _pooled_shape(new, k), tdt)
    s = _shifts(rs, shape[1], nd, new[2:])
    w_np = s.astype(gp_np.dtype)
    gd, wd = gp_t.to(DEV), torch.from_numpy(s).to(tdt).to(DEV)
    if expect is None:
        es = torch.empty(0, dtype=tdt).element_size()
        expect = PIECES if (shape[-1] * es) % 16 == 0 else ELEMENTS
    for pad in pads:
        gx = abi.backward_pooled_input(gd, wd, shape, pad, k, b)
        assert abi.last_kernel() == expect, (shape, pool, cut, dt, pad, abi.last_kernel())
        ref = _reference(gp_np, w_np, shape, pad, k, b, new, tdt)
        assert torch.equal(gx.cpu(), ref), (shape, pool, cut, dt, pad, abi.last_kernel())


C11 = [[1, 1], [1, 1]]
WHOLE = [((2, 5, 24, 32), 2, C11), ((2, 5, 24, 32), 2, None),                    # ... and the whole-input window
         ((2, 3, 17, 24), 2, C11),                                               # an odd window: a partial last row, counts 2 and 1
         ((2, 4, 12, 24), (3, 2), [[1, 0], [2, 3]]),                             # counts that are no power of two
         ((1, 3, 9, 8), (4, 4), None), ((2, 3, 10, 12), (1, 2), None),
         ((2, 5, 24, 32), 1, C11),                                               # a pool of ones: the pooled kernels, counts of 1
         ((1, 3, 1, 64), (1, 2), [[0, 0], [1, 1]]),                              # a single row
         ((2, 4, 4096), 2, [[1, 1]]), ((3, 4, 36), 3, [[1, 2]]),
         ((2, 3, 6, 8, 16), 2, [[1, 1]] * 3), ((1, 4, 5, 6, 12), (2, 3, 2), [[0, 1], [1, 0], [0, 0]])]


@pytest.mark.parametrize("dt", ["f32", "f64", "f16", "bf16"])
def test_rows_of_whole_pieces(dt):
    """every padding and element width; the few 16-bit rows of this list that are no whole pieces (12 and 36 elements) are the
    element-wide kernel's, by the eligibility rule restated in _check"""
    ran = set()
    for shape, pool, cut in WHOLE:
        _check(shape, pool, cut, dt)
        ran.add(abi.last_kernel())
    assert PIECES in ran


def test_ragged_rows():
    _check((2, 3, 62, 62), 2, C11, "f32", expect=ELEMENTS)
    _check((4, 8, 14, 14), 2, C11, "f32", expect=ELEMENTS)
    _check((2, 3, 30, 61), 2, None, "bf16", expect=ELEMENTS)
    for dt in ("f32", "f16"):
        _check((2, 3, 5, 9, 13), 2, None, dt, expect=ELEMENTS)


@pytest.mark.parametrize("cut", [None, C11])
def test_null_form_and_full_form_agree(cut):
    """... and the full form did not move: its grad_x is the oracle's, its grad_w within the 1e-5 of the pooled tests"""
    shape = (4, 8, 64, 64)
    b, new = abi.check_borders(list(shape), cut, 2)
    rs = np.random.RandomState(21)
    x = rs.uniform(-1, 1, size=shape).astype(np.float32)
    gp = rs.uniform(-1, 1, size=_pooled_shape(new, [2, 2])).astype(np.float32)
    w = rs.uniform(-3, 3, size=(8, 2)).astype(np.float32)
    xd, gd, wd = (torch.from_numpy(a).to(DEV) for a in (x, gp, w))
    for pad in (0, 3):
        gx_in = abi.backward_pooled_input(gd, wd, shape, pad, 2, b)
        assert abi.last_kernel() == PIECES
        gx, gw = abi.backward_pooled(gd, wd, xd, pad, False, 2, b)
        assert "backward" in abi.last_kernel()
        gx_o, _ = O.backward_pooled(gp, w, x, pad, False, 2, b)
        _, gw64 = O.backward_pooled(gp.astype(np.float64), w.astype(np.float64), x.astype(np.float64), pad, False, 2, b)
        assert torch.equal(gx, gx_in)
        assert np.array_equal(gx.cpu().numpy(), gx_o) and np.array_equal(gx_in.cpu().numpy(), gx_o)
        assert np.abs(gw.cpu().numpy() - gw64).max() <= 1e-5 * np.abs(gw64).max()


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
@pytest.mark.parametrize("shape,cut", [((2, 3, 16, 32), C11), ((2, 3, 15, 15), None)])
def test_nothing_is_written_outside_grad_x(shape, cut, dt):
    tdt = TDT[dt]
    b, new = abi.check_borders(list(shape), cut, 2)
    rs = np.random.RandomState(11 + sum(shape))
    gp_t, gp_np = _draw(rs, _pooled_shape(new, [2, 2]), tdt)
    s = _shifts(rs, shape[1], 2, new[2:])
    wd = torch.from_numpy(s).to(tdt).to(DEV)
    for pad in range(5):
        big, gx, p = _guarded(shape, tdt)
        abi.backward_pooled_input(gp_t.to(DEV), wd, shape, pad, 2, b, grad_x=gx)
        torch.cuda.synchronize()
        assert bool((big[:p] == 7).all()) and bool((big[p + gx.numel():] == 7).all()), (shape, cut, dt, pad, abi.last_kernel())
        assert torch.equal(gx.cpu(), _reference(gp_np, s.astype(gp_np.dtype), shape, pad, [2, 2], b, new, tdt)), (shape, dt, pad)


def test_refused_argument_forms_launch_nothing():
    shape = (2, 4, 16, 16)
    x = torch.randn(shape, device=DEV)
    gp = torch.randn(2, 4, 8, 8, device=DEV)
    w = torch.randint(-2, 3, (4, 2), device=DEV).float()
    gx = torch.full(shape, 5.0, device=DEV)
    gw = torch.empty_like(w)
    ws = torch.empty(abi.backward_pooled_workspace_bytes(x, 0, False, 2), dtype=torch.uint8, device=DEV)
    pool = (ctypes.c_int32 * 2)(2, 2)
    ptr = lambda t: None if t is None else t.data_ptr()
    raw = lambda p, g, xx, gww: abi.lib().shiftnd_backward_pooled(ctypes.byref(p), pool, ptr(g), ptr(xx), ptr(w), ptr(gx), ptr(gww),
                                                                  ptr(ws), ws.numel(), None)
    abi.forward(torch.randn(2, 4, 14, 14, device=DEV).contiguous(memory_format=torch.channels_last), w, 0, False)
    before = (abi.last_path(), abi.last_kernel())
    sparse, active = abi.problem(x, 0, False, None), abi.problem(x, 0, True, None)
    assert raw(active, gp, None, None) == -1      # the NULL form of an active shift
    assert raw(sparse, gp, None, gw) == -1        # only x NULL
    assert raw(sparse, gp, x, None) == -1         # only grad_w NULL
    assert raw(sparse, None, None, None) == -1    # no grad_pooled
    assert (abi.last_path(), abi.last_kernel()) == before
    torch.cuda.synchronize()
    assert bool((gx == 5.0).all())
    assert raw(sparse, gp, None, None) == 0       # ... and the form itself, with a workspace it does not need
    torch.cuda.synchronize()
    assert np.array_equal(gx.cpu().numpy(), O.backward_pooled(gp.cpu().numpy(), w.cpu().numpy(), x.cpu().numpy(), 0, False, 2)[0])


@pytest.mark.parametrize("nd,shape,pool,cut", [(1, (3, 4, 36), 3, [[1, 2]]), (2, (2, 5, 24, 32), 2, C11), (2, (2, 5, 24, 32), 2, None),
                                               (3, (1, 4, 5, 6, 12), (2, 3, 2), [[0, 1], [1, 0], [0, 0]])])
def test_fixed_pool_ops_on_hip_tensors(nd, shape, pool, cut):
    """forward: fp32 / fp64 bit for bit (the fused forward sums in ATen's order), 16-bit within one ulp of the type as in
    tests/test_pooled_gpu.py; the input gradient bit for bit in every type"""
    op = getattr(OPS, "shift%dd_fixed_pool" % nd)
    k = _pool_list(pool, nd)
    for dt, sdt in (("f32", torch.int64), ("f64", torch.int32), ("bf16", torch.int64), ("f16", torch.float32)):
        tdt = TDT[dt]
        rs = np.random.RandomState(31 + sum(shape))
        b, new = abi.check_borders(list(shape), cut, nd)
        x_t, x_np = _draw(rs, shape, tdt)
        g_t, g_np = _draw(rs, _pooled_shape(new, k), tdt)
        s = _shifts(rs, shape[1], nd, new[2:])
        w_np = s.astype(x_np.dtype)
        eps = {"f32": 0.0, "f64": 0.0, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}[dt]
        for pad in range(5):
            xt = x_t.to(DEV).requires_grad_(True)
            st = torch.from_numpy(s).to(sdt).to(DEV)
            out = op(xt, st, torch.Tensor() if cut is None else torch.tensor(cut, dtype=torch.long), k, pad)
            out.backward(g_t.to(DEV))
            assert xt.grad.is_contiguous() and st.grad is None
            ref = O.forward_pooled(x_np, w_np, pad, False, k, b)
            err = np.abs(out.detach().double().cpu().numpy() - ref).max()
            assert err <= eps * max(1.0, np.abs(ref).max()), (dt, pad, err)
            assert torch.equal(xt.grad.cpu(), _reference(g_np, w_np, shape, pad, k, b, new, tdt)), (dt, pad)


def test_fixed_pool_op_takes_a_channels_last_gradient():
    shape = (2, 16, 32, 32)
    rs = np.random.RandomState(41)
    x = rs.uniform(-1, 1, size=shape).astype(np.float32)
    s = _shifts(rs, 16, 2, shape[2:])
    for cut in (None, C11):
        b, new = abi.check_borders(list(shape), cut, 2)
        gp = rs.uniform(-1, 1, size=_pooled_shape(new, [2, 2])).astype(np.float32)
        xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
        out = OPS.shift2d_fixed_pool(xt, torch.from_numpy(s).long().to(DEV), torch.Tensor() if cut is None else torch.tensor(cut), [2, 2], 3)
        out.backward(torch.from_numpy(gp).to(DEV).contiguous(memory_format=torch.channels_last))
        assert xt.grad.is_contiguous()
        assert np.array_equal(xt.grad.cpu().numpy(), O.backward_pooled(gp, s.astype(np.float32), x, 3, False, 2, b)[0])


@pytest.mark.parametrize("cut", [None, C11])
def test_graph_capture_of_forward_and_backward(cut):
    shape = (4, 16, 56, 64)
    rs = np.random.RandomState(51)
    b, new = abi.check_borders(list(shape), cut, 2)
    s = _shifts(rs, 16, 2, new[2:])
    st = torch.from_numpy(s).long().to(DEV)
    bt = torch.Tensor() if cut is None else torch.tensor(cut, dtype=torch.long)
    x_static = torch.zeros(shape, device=DEV, requires_grad=True)
    g_static = torch.zeros(_pooled_shape(new, [2, 2]), device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture
        for _ in range(2):
            out = OPS.shift2d_fixed_pool(x_static, st, bt, [2, 2], 0)
            gx, = torch.autograd.grad(out, x_static, g_static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_static = OPS.shift2d_fixed_pool(x_static, st, bt, [2, 2], 0)
        gx_static, = torch.autograd.grad(out_static, x_static, g_static)
    x = rs.uniform(-1, 1, size=shape).astype(np.float32)
    gp = rs.uniform(-1, 1, size=tuple(g_static.shape)).astype(np.float32)
    with torch.no_grad():
        x_static.copy_(torch.from_numpy(x))
        g_static.copy_(torch.from_numpy(gp))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out_static.detach().cpu().numpy(), O.forward_pooled(x, s.astype(np.float32), 0, False, 2, b))
    assert np.array_equal(gx_static.cpu().numpy(), O.backward_pooled(gp, s.astype(np.float32), x, 0, False, 2, b)[0])


class _Composed(torch.nn.Module):
    """the strided module as it was: shift{N}d_fixed, then ATen's pool, autograd through both"""

    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, x):
        m = self.m
        y = {2: shift2d_fixed_func, 3: shift3d_fixed_func}[m.dim](x, m.shifts, m.padding, m.cut_borders)
        pool = {2: torch.nn.functional.avg_pool2d, 3: torch.nn.functional.avg_pool3d}[m.dim]
        return pool(y, kernel_size=m._pool_size, stride=m._pool_size, ceil_mode=True), None


@pytest.mark.parametrize("cls,C,shape", [(torchshifts.GroupedShift2d, 9, (2, 9, 30, 32)), (torchshifts.GroupedShift3d, 27, (2, 27, 6, 10, 16))])
def test_strided_module_equals_the_composed_sequence(cls, C, shape):
    """stride 2: every count is a power of two, so the comparison does not depend on how ATen's GPU kernel divides"""
    m = cls(C, emulate_dw={"kernel_size": 3, "stride": 2, "padding": 0}).to(DEV)
    assert m._pool_size == [2] * m.dim and m.cut_borders is not None
    for tdt in (torch.float32, torch.bfloat16):
        x = torch.randn(shape, device=DEV).to(tdt)
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        out, none = m(xa)
        ref, _ = _Composed(m)(xb)
        go = torch.randn(out.shape, device=DEV).to(tdt)
        out.backward(go)
        ref.backward(go)
        assert none is None and out.shape == ref.shape
        assert torch.equal(xa.grad, xb.grad), tdt
        if tdt == torch.float32:
            assert torch.allclose(out.detach(), ref.detach(), rtol=0, atol=1e-6)


def test_from_shift_of_a_strided_shift2d():
    torch.manual_seed(5)
    src = torchshifts.Shift2d(8, padding="reflect", init_shift=3, sparsity_term=0, emulate_dw={"kernel_size": 3, "stride": 2, "padding": 0}).to(DEV)
    frozen = torchshifts.GroupedShift2d.from_shift(src)
    x = torch.randn(2, 8, 30, 32, device=DEV)
    assert torch.equal(frozen(x)[0], src(x)[0].detach())


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


def test_the_fused_op_allocates_no_full_size_intermediate():
    """forward + backward of one strided GroupedShift2d on an 8 x 64 x 224 x 224 fp32 tensor.  The composed sequence holds the
    full-size shift output for the pool's backward and then the full-size expanded gradient next to grad_x; the fused op holds
    grad_x alone.  padding = 1 keeps the window the whole input, so that intermediate is exactly one activation (with padding = 0
    it is the 222 x 222 window, 2 % less than the bound asks); the allocator counts 512-byte multiples, far below one activation."""
    shape = (8, 64, 224, 224)
    act = int(np.prod(shape)) * 4
    m = torchshifts.GroupedShift2d(64, emulate_dw={"kernel_size": 3, "stride": 2, "padding": 1}).to(DEV)
    x = torch.randn(shape, device=DEV)
    p_composed = _chain_peak([_Composed(m)], x.clone())
    p_fused = _chain_peak([m], x.clone())
    print("peak bytes: composed %d, fused %d, activation %d" % (p_composed, p_fused, act))
    assert p_composed - p_fused >= act, (p_composed, p_fused, act)
