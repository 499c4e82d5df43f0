"""Mixed precision through the operator library: torch.ops.torchshifts.shift{1,2,3}d and shift{1,2,3}d_pool on fp16 / bf16 HIP
tensors with fp32 weights -- what a Shift{N}d inside torch.autocast hands them.  weight.grad stays fp32, x.grad and the output keep
the tensor's dtype, the values are the C ABI's (tests/test_mixed_families_gpu.py and test_mixed_parity_gpu.py pin those);
channels-last and NDHWC inputs, device-resident borders under graph capture, an optimizer step under autocast (bf16, and fp16 with
a GradScaler); every other pair of types still raises "same type", and so does a mixed call on CPU tensors."""
import pytest
import torch

import torchshifts   # noqa: F401  (registers the ops)
from torchshifts import Shift2d

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPS = torch.ops.torchshifts
HALVES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "f16"]

# nd -> (shape, cut for the plain op)
SHAPES = {1: ((2, 3, 2048), [[1, 2]]), 2: ((2, 3, 18, 32), [[1, 1], [1, 1]]), 3: ((2, 3, 6, 8, 16), None)}


def _data(shape, tdt, seed):
    torch.manual_seed(seed)
    nd = len(shape) - 2
    x = torch.rand(shape, device=DEV).mul(2).sub(1).to(tdt)
    w = (torch.rand(shape[1], nd, device=DEV) * 2 - 1) * 2.7   # fp32, not representable in 16 bits
    assert w.dtype == torch.float32 and not torch.equal(w.to(tdt).float(), w)
    return x, w


@pytest.mark.parametrize("tdt", HALVES, ids=IDS)
@pytest.mark.parametrize("active", [False, True], ids=["sparse", "active"])
@pytest.mark.parametrize("nd", [1, 2, 3])
def test_shift_op_autograd(nd, active, tdt):
    from torchshifts import abi
    shape, cut = SHAPES[nd]
    x, w = _data(shape, tdt, 10 + nd)
    for pad in (0, 3):
        xt, wt = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        out = getattr(OPS, "shift%dd" % nd)(xt, wt, torch.Tensor() if cut is None else torch.tensor(cut, dtype=torch.long), pad, active)
        go = torch.rand(out.shape, device=DEV).to(tdt)
        out.backward(go)
        assert out.dtype == tdt and xt.grad.dtype == tdt and wt.grad.dtype == torch.float32
        b = abi.check_borders(list(shape), cut, nd)[0] if cut else None
        ref = abi.forward(x, w, pad, active, b)
        gx, gw = abi.backward(go, w, x, pad, active, b)
        assert torch.equal(out.detach(), ref), (nd, pad, active, tdt)
        assert torch.equal(xt.grad, gx) and torch.equal(wt.grad, gw), (nd, pad, active, tdt)


@pytest.mark.parametrize("tdt", HALVES, ids=IDS)
@pytest.mark.parametrize("active", [False, True], ids=["sparse", "active"])
@pytest.mark.parametrize("nd", [1, 2, 3])
def test_shift_pool_op_autograd(nd, active, tdt):
    from torchshifts import abi
    shape, _ = SHAPES[nd]
    x, w = _data(shape, tdt, 20 + nd)
    pool = [2] * nd
    for pad in (0, 2):
        xt, wt = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        out = getattr(OPS, "shift%dd_pool" % nd)(xt, wt, torch.Tensor(), pool, pad, active)
        gp = torch.rand(out.shape, device=DEV).to(tdt)
        out.backward(gp)
        assert out.dtype == tdt and xt.grad.dtype == tdt and wt.grad.dtype == torch.float32
        ref = abi.forward_pooled(x, w, pad, active, pool)        # (shapes the fused kernels serve in both directions)
        gx, gw = abi.backward_pooled(gp, w, x, pad, active, pool)
        assert torch.equal(out.detach(), ref), (nd, pad, active, tdt)
        assert torch.equal(xt.grad, gx) and torch.equal(wt.grad, gw), (nd, pad, active, tdt)


@pytest.mark.parametrize("tdt", HALVES, ids=IDS)
@pytest.mark.parametrize("active", [False, True], ids=["sparse", "active"])
@pytest.mark.parametrize("shape", [(2, 64, 9, 12), (1, 16, 4, 6, 8)], ids=["nhwc", "ndhwc"])
def test_channels_last_inputs(shape, active, tdt):
    """a channels-last / NDHWC input and gradient: the values of the contiguous call, weight.grad fp32"""
    nd = len(shape) - 2
    fmt = torch.channels_last if nd == 2 else torch.channels_last_3d
    x, w = _data(shape, tdt, 30 + nd)
    go = torch.rand(shape, device=DEV).to(tdt)
    op = getattr(OPS, "shift%dd" % nd)
    res = []
    for cl in (False, True):
        xt = (x.contiguous(memory_format=fmt) if cl else x.clone()).requires_grad_(True)
        wt = w.clone().requires_grad_(True)
        out = op(xt, wt, torch.Tensor(), 1, active)
        out.backward(go.contiguous(memory_format=fmt) if cl else go)
        assert wt.grad.dtype == torch.float32 and xt.grad.dtype == tdt and out.dtype == tdt
        res.append((out.detach(), xt.grad, wt.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), (shape, active, tdt)
    # (the two layouts may sum the weight gradient in different kernels: the fp32 bar between them)
    scale = res[0][2].abs().max().clamp_min(1e-30)
    assert float((res[0][2] - res[1][2]).abs().max() / scale) < 1e-5, (shape, active, tdt)


@pytest.mark.parametrize("tdt", HALVES, ids=IDS)
def test_graph_capture_with_device_borders(tdt):
    """forward + backward of a mixed call capture into a graph with device-resident whole-window borders (no D2H read, no sync), as
    tests/test_torch_ops_gpu.py::test_device_borders_stay_sync_free_and_capturable does for same-dtype calls"""
    x, w = _data((4, 8, 32, 32), tdt, 40)
    g = torch.rand(4, 8, 32, 32, device=DEV).to(tdt)
    bh = torch.tensor([0, 32, 0, 32, 0, 1], dtype=torch.int32)
    bd = bh.to(DEV)
    ref = OPS._shift2d_forward(x, w, bh, [4, 8, 32, 32], 3, True)
    gx_ref, gw_ref = OPS._shift2d_backward(g, w, x, bh, 3, True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):   # warm the allocator's pool of the capture stream
            OPS._shift2d_forward(x, w, bd, [4, 8, 32, 32], 3, True)
            OPS._shift2d_backward(g, w, x, bd, 3, True)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = OPS._shift2d_forward(x, w, bd, [4, 8, 32, 32], 3, True)
        gx, gw = OPS._shift2d_backward(g, w, x, bd, 3, True)
    graph.replay()
    torch.cuda.synchronize()
    assert gw.dtype == torch.float32 and gw_ref.dtype == torch.float32 and gx.dtype == tdt
    assert torch.equal(out, ref) and torch.equal(gx, gx_ref) and torch.equal(gw, gw_ref)


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Conv2d(8, 8, 1)
        self.shift = Shift2d(8, emulate_dw={'kernel_size': 3, 'stride': 2, 'padding': 0})
        self.b = torch.nn.Conv2d(8, 8, 1)

    def forward(self, x):
        y, loss = self.shift(self.a(x))
        return self.b(y), loss


@pytest.mark.parametrize("tdt", HALVES, ids=IDS)
def test_autocast_training_step(tdt):
    """Conv2d -> Shift2d(emulate_dw: cut 1 / 1, stride 2 -> the fused shift + pool) -> Conv2d under torch.autocast: one optimizer
    step (fp16: through a GradScaler); the loss is finite, shift.weight stays fp32 and moves"""
    torch.manual_seed(50)
    net = _Net().to(DEV)
    assert net.shift.weight.dtype == torch.float32
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    scaler = torch.amp.GradScaler("cuda", enabled=tdt == torch.float16)
    x = torch.rand(4, 8, 18, 34, device=DEV)
    before = net.shift.weight.detach().clone()
    with torch.autocast("cuda", dtype=tdt):
        y, reg = net(x)
        assert y.dtype == tdt
        loss = y.float().pow(2).mean() + reg
    assert bool(torch.isfinite(loss))
    scaler.scale(loss).backward()
    assert net.shift.weight.grad.dtype == torch.float32 and bool(torch.isfinite(net.shift.weight.grad).all())
    scaler.step(opt)
    scaler.update()
    assert net.shift.weight.dtype == torch.float32
    assert bool(torch.isfinite(net.shift.weight).all()) and not torch.equal(net.shift.weight.detach(), before)


REFUSED = [   # tensors, weights
    (torch.float32, torch.float64), (torch.float16, torch.float64), (torch.bfloat16, torch.float64),
    (torch.float16, torch.bfloat16), (torch.bfloat16, torch.float16), (torch.float32, torch.float16), (torch.float32, torch.bfloat16),
    (torch.float64, torch.float32),
]


@pytest.mark.parametrize("xdt,wdt", REFUSED, ids=lambda d: str(d).replace("torch.", ""))
def test_other_type_pairs_still_raise(xdt, wdt):
    x = torch.rand(2, 3, 8, 16, device=DEV).to(xdt)
    w = torch.rand(3, 2, device=DEV).to(wdt)
    b = torch.tensor([0, 8, 0, 16, 0, 1], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="same type"):
        OPS.shift2d(x, w, torch.Tensor(), 0, False)
    with pytest.raises(RuntimeError, match="same type"):
        OPS._shift2d_backward(x, w, x, b, 0, False)
    with pytest.raises(RuntimeError, match="same type"):
        OPS.shift2d_pool(x, w, torch.Tensor(), [2, 2], 0, False)
    with pytest.raises(RuntimeError, match="same type"):
        OPS._shift2d_pool_backward(x[:, :, :4, :8].contiguous(), w, x, b, [2, 2], 0, False)
    # the gradient and the saved input must still agree with each other
    with pytest.raises(RuntimeError, match="same type"):
        OPS._shift2d_backward(x.to(torch.float16), w.float(), x.to(torch.bfloat16), b, 0, False)


@pytest.mark.parametrize("tdt", HALVES, ids=IDS)
def test_cpu_mixed_call_still_raises(tdt):
    """the CPU key has no 16-bit kernels at all (like the reference), mixed or not"""
    x = torch.rand(2, 3, 8, 16).to(tdt)
    w = torch.rand(3, 2)
    with pytest.raises(RuntimeError):
        OPS.shift2d(x, w, torch.Tensor(), 0, False)
    with pytest.raises(RuntimeError):
        OPS.shift2d_pool(x, w, torch.Tensor(), [2, 2], 0, False)
