"""Self-checks of the pooled 16-bit parity fixture (tests/pooled16_cases.py) that need no GPU: the exact-data claims hold on the
oracle for every case, padding and shift; the reference itself stays inside every bar; and the assertion functions the GPU tests
use reject references mutated the way a subtly wrong kernel would be."""
import numpy as np
import pytest
import torch

import pooled16_cases as PC
from oracle import oracle as O

T16 = (torch.float16, torch.bfloat16)
SWEEP = [(pad, active) for pad in range(5) for active in (0, 1)]


def _case(shape, pool):
    return next(i for i, c in enumerate(PC.CASES) if c[1] == shape and c[2] == pool)


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_fixture_holds(nd):
    for ci, case in enumerate(PC.CASES):
        if case[0] != nd:
            continue
        pool, pow2 = case[2], PC.pow2_counts(case)
        for pad, active in SWEEP:
            key = (case[1], pool, case[3], pad, active)
            r = PC.reference(ci, "f32", "exact", pad, active)
            x, w, gp, b = r["x"], r["w"], r["gp"], r["b"]
            # the oracle's fp32 and fp64 forward agree bit for bit (every tap exact)
            y64 = O.forward(x.astype(np.float64), w.astype(np.float64), pad, active, b)
            assert np.array_equal(r["y"].astype(np.float64), y64), key
            gx32, gw32 = O.backward(r["g"], w, x, pad, active, b)
            for tdt in T16:
                for name in ("x", "w", "gp", "y"):
                    assert PC.representable(r[name], tdt), key + (name, tdt)
                if pow2:   # the expanded gradient, grad_x and (in fp32) grad_w are exact too
                    assert PC.representable(r["g"], tdt) and PC.representable(gx32, tdt), key + (tdt,)
            if pow2:
                assert np.array_equal(gx32, r["gx_ref"]), key
                g64 = O.avg_pool_backward(gp.astype(np.float64), pool, r["y"].shape[2:])
                assert np.array_equal(r["g"].astype(np.float64), g64), key
                gx64, gw64 = O.backward(g64, w.astype(np.float64), x.astype(np.float64), pad, active, b)
                assert np.array_equal(gx32.astype(np.float64), gx64) and np.array_equal(gw32.astype(np.float64), gw64), key
                assert np.array_equal(gw64, r["gw64"]), key
            # the window sums are exact in fp32: one division, one narrowing (3-wide windows too)
            cnt = O._pool_counts(r["y"].shape[2:], r["ref"].shape[2:], list(pool))
            s64 = O.avg_pool(y64, pool) * cnt
            assert np.array_equal(s64.astype(np.float32).astype(np.float64), s64), key
            assert np.array_equal(O.avg_pool(r["y"], pool), (s64.astype(np.float32) / cnt.astype(np.float32))), key


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_reference_inside_every_bar(dt):
    """the fp32 oracle's own results, narrowed, pass every assertion of the GPU tests: no bar is tighter than the reference's error"""
    tdt = PC.DTYPES[dt]
    for ci, case in enumerate(PC.CASES):
        for pad, active in SWEEP:
            for kind in ("exact", "random"):
                r = PC.reference(ci, dt, kind, pad, active)
                what = (case[1], case[2], case[3], dt, kind, pad, active)
                gx32, gw32 = O.backward(r["g"], r["w"], r["x"], pad, active, r["b"])
                PC.check_forward(r["ref"], r, case, active, kind, tdt, what)
                PC.check_backward(PC.round16(gx32, tdt), PC.round16(gw32, tdt), r, case, active, kind, tdt, what)


def _windows_first_tap(y, pool):
    """a mask with the first element of every pooling window set"""
    m = np.zeros(y.shape, bool)
    m[(slice(None), slice(None)) + tuple(slice(0, None, k) for k in pool)] = True
    return m


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_checker_rejects_a_tap_off_by_two_ulps(dt):
    """(a) the sparse shift: one tap of every window 2 ulps off"""
    tdt = PC.DTYPES[dt]
    for ci in (_case((2, 3, 18, 32), (2, 2)), _case((1, 3, 16, 40), (3, 3)), _case((2, 3, 6, 8, 16), (2, 2, 2)), _case((2, 3, 2048), (2,))):
        case = PC.CASES[ci]
        for kind in ("exact", "random"):
            r = PC.reference(ci, dt, kind, 0, 0)
            y = r["y"] + np.where(_windows_first_tap(r["y"], case[2]), 2 * PC.ulp16(r["y"], tdt), 0.0).astype(np.float32)
            mutant = PC.round16(O.avg_pool(PC.round16(y, tdt), case[2]), tdt)
            with pytest.raises(AssertionError):
                PC.check_forward(mutant, r, case, 0, kind, tdt, ("mutation a",))


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("active", [0, 1])
def test_checker_rejects_full_count_at_a_ragged_edge(dt, active):
    """(b) the sum of a clipped window divided by the full window's count"""
    tdt = PC.DTYPES[dt]
    for ci in (_case((2, 3, 18, 32), (2, 2)), _case((1, 2, 7, 40), (2, 2)), _case((1, 3, 5, 7, 24), (2, 2, 2)), _case((1, 3, 640), (2,))):
        case = PC.CASES[ci]
        pool = case[2]
        for kind in ("exact", "random"):
            r = PC.reference(ci, dt, kind, 1, active)
            cnt = O._pool_counts(r["y"].shape[2:], r["ref"].shape[2:], list(pool)).astype(np.float32)
            if (2, 3, 18, 32) == case[1]:
                assert (cnt == cnt.max()).all()   # (whole windows only: nothing to mutate)
                continue
            mutant = PC.round16(O.avg_pool(r["y"], pool) * cnt / np.float32(np.prod(pool)), tdt)
            with pytest.raises(AssertionError):
                PC.check_forward(mutant, r, case, active, kind, tdt, ("mutation b",))


def _truncate16(a, tdt):
    """fp32 -> the 16-bit type by dropping bits (round toward zero)"""
    bits = np.ascontiguousarray(a, np.float32).view(np.uint32)
    if tdt == torch.bfloat16:
        return (bits & np.uint32(0xFFFF0000)).view(np.float32)
    t = torch.from_numpy(a.copy()).to(tdt)               # nearest; step back where that rounded away from zero
    back = t.float().numpy()
    away = np.abs(back) > np.abs(a)
    ti = t.view(torch.int16).numpy().copy()
    ti[away] -= 1                                        # (sign-magnitude: one code less is one step toward zero)
    return torch.from_numpy(ti).view(tdt).float().numpy()


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_checker_rejects_truncation(dt):
    """(c) the quotient truncated instead of rounded to nearest even.  On exact data the 3-wide windows round in both types; of the
    power-of-two windows' quotients fp16 holds all (9 bits) and bf16 all but those of magnitude >= 1/2 with an odd 9-bit numerator
    (the interpolating shift's: a few per case) -- what pins the rounding of those windows element by element is the sparse shift on
    random data, bit for bit."""
    tdt = PC.DTYPES[dt]
    rounds = 0
    for ci, case in enumerate(PC.CASES):
        for kind, active in (("exact", 0), ("exact", 1), ("random", 0)):
            r = PC.reference(ci, dt, kind, 3, active)
            mutant = _truncate16(O.avg_pool(r["y"], case[2]), tdt)
            assert PC.representable(mutant, tdt)
            if np.array_equal(mutant, r["ref"]):   # (nothing is rounded: nothing to reject)
                assert kind == "exact" and PC.pow2_counts(case), (case[1], case[2], kind, active)
                continue
            rounds += 1
            with pytest.raises(AssertionError):
                PC.check_forward(mutant, r, case, active, kind, tdt, ("mutation c",))
    assert rounds >= len(PC.CASES) + 2 * sum(not PC.pow2_counts(c) for c in PC.CASES)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_checker_rejects_a_dropped_row_in_grad_w(dt):
    """(d) one row of the gradient missing from one channel's grad_w sums"""
    tdt = PC.DTYPES[dt]
    for ci in (_case((2, 3, 18, 32), (2, 2)), _case((1, 2, 70, 64), (2, 2)), _case((2, 3, 6, 8, 16), (2, 2, 2)), _case((1, 3, 16, 40), (3, 3))):
        case = PC.CASES[ci]
        for kind in ("exact", "random"):
            for active in (0, 1):
                r = PC.reference(ci, dt, kind, 2, active)
                g = r["g"].copy()
                g[0, 1, ..., g.shape[-2] // 2, :] = 0          # channel 1 (not one of the special rows' zero-shift channel 0), a middle row
                _, gw = O.backward(g.astype(np.float64), r["w"].astype(np.float64), r["x"].astype(np.float64), 2, active, r["b"])
                assert not np.array_equal(gw, r["gw64"])
                gx = r["gx_ref"]
                with pytest.raises(AssertionError):
                    PC.check_backward(gx, PC.round16(gw.astype(np.float32), tdt), r, case, active, kind, tdt, ("mutation d",))


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_checker_rejects_grad_w_from_an_unrounded_gradient(dt):
    """(e) 3-wide windows: grad_w summed from the expanded gradient BEFORE it is narrowed (the specification narrows it, as ATen's
    avg_pool backward does).  The deviation is of the bar's own order -- the narrowing moves every gradient element by up to half a
    unit, their sum moves grad_w by about half a unit of ITS size, and the bar grants 0.51 -- so the per-entry bar catches it where
    an entry is smaller than its terms (cancellation), not in every single call (about half of them): on every 3-wide
    case somewhere in its sweep of paddings and shifts, on exact and on random data."""
    tdt = PC.DTYPES[dt]
    for ci, case in enumerate(PC.CASES):
        if PC.pow2_counts(case):
            continue
        for kind in ("exact", "random"):
            rejected = 0
            for pad, active in SWEEP:
                r = PC.reference(ci, dt, kind, pad, active)
                g = O.avg_pool_backward(r["gp"].astype(np.float64), case[2], r["y"].shape[2:])
                _, gw = O.backward(g, r["w"].astype(np.float64), r["x"].astype(np.float64), pad, active, r["b"])
                try:
                    PC.check_backward(r["gx_ref"], PC.round16(gw.astype(np.float32), tdt), r, case, active, kind, tdt, ("mutation e",))
                except AssertionError:
                    rejected += 1
            assert rejected >= 1, (case[1], case[2], kind, rejected)


def test_routes_cover_the_issue_list():
    """the route rules alone (host logic restated): the 16-bit runs of the table reach every pooled kernel"""
    served, band = set(), False
    for case in PC.CASES:
        for pad, active in SWEEP:
            long_row = case[0] == 1 and case[1][-1] >= PC.LONG_ROWS // 2
            for knob in ((0, 2) if long_row else (0,)):
                served.add(PC.forward_route(case, 2, active, pad, knob34=knob))
                bw = PC.backward_route(case, 2, active, pad, knob32=knob)
                band = band or bw == PC.BAND_WALK
                if bw not in (PC.BAND_WALK, PC.NOT_SERVED):
                    served.add(bw)
    assert served == PC.SERVED_16BIT and band
