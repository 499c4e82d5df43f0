"""Exact-data and per-element parity of the fused shift + average pool kernels on fp16 / bf16 tensors (fp32 as a control),
through the C ABI (shiftnd_forward_pooled / shiftnd_backward_pooled), against the two-step sequence on widened values computed
with the CPU oracle alone.  Table, fixture, reference, route rules and assertion functions: tests/pooled16_cases.py (their own
self-checks, without a GPU: tests/test_pooled16_cases.py).

  exact data ........ the pooled output bit for bit on every case; with power-of-two window counts grad_x and grad_w == round(gw64)
                      bit for bit too (fp32: grad_w == the fp64 oracle's); 3-wide windows: backward under the bars of the random data
  random data ....... the sparse shift: pooled output and grad_x bit for bit; the interpolating shift: the pooled output within
                      avg_pool(ulp16(y) + FLOOR16) + 1.0001 ulp16(ref) per element, grad_x within 1 ulp (+ FLOOR16) per element;
                      grad_w per entry within 0.51 ulp16(gw64) + 1e-5 max|gw64|
  routes ............ the kernel name of every call against the host's eligibility rules restated in pooled16_cases.forward_route /
                      backward_route; every forward again under policy 2 (plane_pool_forward); every 2-D backward that
                      crop_backward<.., POOL> takes again on the band-walk kernels (policy 2 + knob 35 bit 6)

Every padding 0-4 and both shifts on every case."""
import numpy as np
import pytest
import torch

import pooled16_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWEEP = [(pad, active) for pad in range(5) for active in (0, 1)]


@pytest.fixture()
def abi():
    from torchshifts import abi as A
    assert torch.cuda.is_available(), "the gpu tests need an MI355X"
    A.set_path_policy(0)
    for k in (32, 34, 35):
        A.set_tuning(k, 0)
    yield A
    A.set_path_policy(0)
    for k in (32, 34, 35):
        A.set_tuning(k, 0)


def _dev(a, tdt):
    return torch.from_numpy(np.array(a)).to(tdt).to(DEV)   # (a copy: the shared references are read-only)


def _host(t):
    return t.float().cpu().numpy()


def _run_case(abi, ci, dt, kind, served, check=True):
    """every padding and shift of CASES[ci]: default routes (1-D long rows also under knobs 32 / 34 = 2), every forward again under
    policy 2, the crop_backward<.., POOL> cases again on the band-walk kernels.  `served`: the kernel names seen are added."""
    case = PC.CASES[ci]
    nd, shape, pool, cut, _ = case
    tdt = PC.DTYPES[dt]
    es = torch.finfo(tdt).bits // 8
    long_row = nd == 1 and shape[-1] >= PC.LONG_ROWS // 2   # (640 and longer: test_pooled_1d_rows' rows)
    for pad, active in SWEEP:
        what = (shape, pool, cut, dt, kind, pad, active)
        r = PC.reference(ci, dt, kind, pad, active) if check else dict(zip(("x", "w", "gp"), PC._inputs(ci, dt if kind == "random" else "", kind)),
                                                                       b=PC.geometry(case)[0])
        xd, wd, gpd, b = _dev(r["x"], tdt), _dev(r["w"], tdt), _dev(r["gp"], tdt), r["b"]

        def forward(route, tag):
            out = abi.forward_pooled(xd, wd, pad, active, pool, b)
            assert abi.last_kernel() == route, what + (tag, abi.last_kernel(), route)
            served.add(abi.last_kernel())
            if check:
                PC.check_forward(_host(out), r, case, active, kind, tdt, what + (tag, route))

        def backward(route, tag):
            if route == PC.NOT_SERVED:
                with pytest.raises(RuntimeError, match="not served"):
                    abi.backward_pooled(gpd, wd, xd, pad, active, pool, b)
                return
            gx, gw = abi.backward_pooled(gpd, wd, xd, pad, active, pool, b)
            name = abi.last_kernel()
            assert name in (route if isinstance(route, tuple) else (route,)), what + (tag, name, route)
            served.add(name)
            if check:
                PC.check_backward(_host(gx), _host(gw) if tdt != torch.float32 else gw.cpu().numpy(), r, case, active, kind, tdt,
                                  what + (tag, name))

        for knob in ((0, 2) if long_row else (0,)):
            try:
                abi.set_tuning(32, knob)
                abi.set_tuning(34, knob)
                forward(PC.forward_route(case, es, active, pad, knob34=knob), "knobs %d" % knob)
                route = PC.backward_route(case, es, active, pad, knob32=knob)
                backward(route, "knobs %d" % knob)
                if route == PC.NOT_SERVED and nd == 3:   # not fused by design: the band-walk kernels on request
                    abi.set_path_policy(2)
                    backward(PC.backward_route(case, es, active, pad, policy=2, knob32=knob), "policy 2")
            finally:
                abi.set_path_policy(0)
                abi.set_tuning(32, 0)
                abi.set_tuning(34, 0)
        try:
            abi.set_path_policy(2)
            forward(PC.forward_route(case, es, active, pad, policy=2), "policy 2")
            if nd == 2 and PC.backward_route(case, es, active, pad) == "crop_backward_pool":
                abi.set_tuning(35, 64)   # bit 6: plane_pool_backward keeps the band walk
                route = PC.backward_route(case, es, active, pad, policy=2, band_walk=True)
                assert route == PC.BAND_WALK
                backward(route, "policy 2, knob 35 = 64")
        finally:
            abi.set_tuning(35, 0)
            abi.set_path_policy(0)


@pytest.mark.parametrize("nd", [1, 2, 3])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_pooled_exact_data(abi, dt, nd):
    """dyadic inputs: every intermediate is exact, so the kernels must return the reference's bits whatever their evaluation order --
    indexing, window clipping, the divisor, the rounding and dropped partial sums all fail hard"""
    served = set()
    for ci, case in enumerate(PC.CASES):
        if case[0] == nd:
            _run_case(abi, ci, dt, "exact", served)
    assert served


@pytest.mark.parametrize("nd", [1, 2, 3])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_pooled_random_data(abi, dt, nd):
    """uniform inputs as test_pooled_gpu.py::test_pooled_16bit draws them, under per-element bars derived from the number formats"""
    served = set()
    for ci, case in enumerate(PC.CASES):
        if case[0] == nd:
            _run_case(abi, ci, dt, "random", served)
    assert served


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_pooled_16bit_served_set(abi, dt):
    """the 16-bit runs of the table (the same calls as above, routes only) reach every pooled kernel of the library: a route that
    silently moves shows up here as well as at its call"""
    served = set()
    for ci in range(len(PC.CASES)):
        _run_case(abi, ci, dt, "random", served, check=False)
    band = served & set(PC.BAND_WALK)
    print("served (%s):" % dt, sorted(served))
    assert band and served - band == PC.SERVED_16BIT, (sorted(served - band - PC.SERVED_16BIT), sorted(PC.SERVED_16BIT - served))
