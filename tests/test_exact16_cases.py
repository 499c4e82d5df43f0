"""Self-checks of the unpooled 16-bit parity fixtures (tests/exact16_cases.py) that need no GPU: the exact-data and probe claims hold
on the oracle for every case, padding and shift; the reference itself stays inside every bar; and the assertion functions the GPU
tests use reject references mutated the way a subtly wrong kernel would be."""
import numpy as np
import pytest
import torch

import exact16_cases as EC
from cases import gw16_tol, rel_err
from oracle import oracle as O

T16 = (torch.float16, torch.bfloat16)
TABLES = [(0, EC.CASES), (1, EC.CL_CASES)]
# the cases every mutation runs on: every 2-D case of the table, one 1-D and one 3-D
MUTATED = EC.group(2) + [next(i for i in EC.group(1) if EC.CASES[i][1] == (2, 4, 40)),
                         next(i for i in EC.group(3) if EC.CASES[i][1] == (2, 4, 5, 4, 112))]


@pytest.mark.parametrize("nd", [1, 2, 3])
@pytest.mark.parametrize("table", [0, 1])
def test_fixtures_hold(table, nd):
    """exact and probe data: the fp32 oracle equals the fp64 oracle bit for bit, out and grad_x are representable in fp16 and bf16,
    the probes' grad_w in bf16, and at least half of a case's probe grad_w entries are nonzero -- counted over the weight columns
    that are nonzero anywhere in the case's dense exact grad_w: the reference's gradient along a dim of size 1, and along the first
    dim of a volume whose second dim has size 1, is identically zero (1 x 4 x 2 x 1 x 8, 1 x 16 x 2 x 112 x 1)"""
    for ci in EC.group(nd, TABLES[table][1]):
        case = TABLES[table][1][ci]
        nonzero = entries = 0
        live = np.zeros(case[0], bool)
        for pad, active in EC.SWEEP:
            live |= (EC.reference(ci, "f32", "exact", pad, active, table)["calls"][0]["gw64"] != 0).any(axis=0)
        assert live.any(), case[1]
        for pad, active in EC.SWEEP:
            for kind in ("exact", "probe"):
                key = (case[1], case[2], kind, pad, active)
                r = EC.reference(ci, "f32", kind, pad, active, table)
                x, w = r["x"], r["w"]
                out64 = O.forward(x.astype(np.float64), w.astype(np.float64), pad, active, r["b"])
                assert np.array_equal(r["out"].astype(np.float64), out64), key
                assert len(r["calls"]) <= EC.MAX_PROBE_CALLS
                for c in r["calls"]:
                    assert np.array_equal(c["gx32"].astype(np.float64), c["gx64"]), key
                    assert np.array_equal(c["gw32"].astype(np.float64), c["gw64"]), key
                    for tdt in T16:
                        for name in ("x", "w", "out"):
                            assert EC.representable(r[name], tdt), key + (name, tdt)
                        assert EC.representable(c["g"], tdt) and EC.representable(c["gx32"], tdt), key + (tdt,)
                    if kind == "probe":
                        planes = np.abs(c["g"]).reshape(c["g"].shape[0], c["g"].shape[1], -1).sum(axis=2)
                        assert planes.max() == 1 and set(np.unique(c["g"])) <= {-1.0, 0.0, 1.0}, key
                        assert EC.representable(c["gw32"], torch.bfloat16), key
                        nonzero += int(np.count_nonzero(c["gw64"][:, live]))
                        entries += c["gw64"][:, live].size
        assert 2 * nonzero >= entries, (case[1], case[2], nonzero, entries)


def test_probes_keep_the_corners():
    for _, table in TABLES:
        for case in table:
            _, win = EC.geometry(case)
            hit = set()
            for g in EC.probe_gradients(case, 7):
                hit |= {tuple(p[2:]) for p in np.argwhere(g)}
            for corner in {tuple(c) for c in np.array(np.meshgrid(*[(0, o - 1) for o in win[2:]])).T.reshape(-1, len(win) - 2)}:
                assert corner in hit, (case[1], case[2], corner)


def test_the_drawn_channel_holds_a_tie():
    """mutation (c) below needs weights whose half-to-even and half-away roundings differ"""
    for ci in MUTATED:
        w = EC._inputs(0, ci, "", "exact")[1]
        assert np.any(np.rint(w) != np.sign(w) * np.floor(np.abs(w) + 0.5)), EC.CASES[ci][1]


def test_shapes_stay_small():
    for _, table in TABLES:
        for case in table:
            assert 2 * int(np.prod(case[1])) <= (1 << 20), case[1]


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("table", [0, 1])
def test_reference_inside_every_bar(table, dt):
    """the fp32 oracle's own results, narrowed, pass every assertion of the GPU tests: no bar is tighter than the reference's error"""
    tdt = EC.DTYPES[dt]
    for ci, case in enumerate(TABLES[table][1]):
        for pad, active in EC.SWEEP:
            for kind in ("exact", "probe") + (("random",) if dt != "f32" else ()):
                r = EC.reference(ci, dt, kind, pad, active, table)
                what = (case[1], case[2], dt, kind, pad, active)
                EC.check_forward(r["out"], r, active, kind, tdt, what)
                for c in r["calls"]:
                    gw = EC.round16(c["gw32"], tdt)
                    EC.check_backward(EC.round16(c["gx32"], tdt), gw, c, active, kind, tdt, what)


def _gw64(r, g, pad, active):
    return O.backward(g.astype(np.float64), r["w"].astype(np.float64), r["x"].astype(np.float64), pad, active, r["b"])[1]


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_checker_rejects_a_probe_not_counted(dt):
    """(a) grad_w summed without the probe element of one plane: wherever that element's tap is nonzero, the call is rejected -- in
    bf16 too, which a dense sum of 64 - 128 would not show"""
    tdt = EC.DTYPES[dt]
    for ci in MUTATED:
        case, calls, tried = EC.CASES[ci], 0, 0
        for pad, active in EC.SWEEP:
            r = EC.reference(ci, dt, "probe", pad, active)
            for c in r["calls"]:
                g = c["g"].copy()
                g[tuple(np.argwhere(g)[len(np.argwhere(g)) // 2])] = 0
                tried += 1
                gw = _gw64(r, g, pad, active)
                if np.array_equal(gw, c["gw64"]):   # (this element's taps are zero: a special weight that reads nothing)
                    continue
                calls += 1
                with pytest.raises(AssertionError):
                    EC.check_backward(c["gx"], EC.round16(gw.astype(np.float32), tdt), c, active, "probe", tdt, ("mutation a",))
        assert 2 * calls >= tried, (case[1], calls, tried)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_checker_rejects_grad_x_rolled_by_a_column(dt):
    """(b)"""
    tdt = EC.DTYPES[dt]
    for ci in MUTATED:
        for kind in ("exact", "probe", "random"):
            for pad, active in EC.SWEEP:
                r = EC.reference(ci, dt, kind, pad, active)
                c = r["calls"][0]
                gx = np.roll(c["gx"], 1, axis=-1)
                if np.array_equal(gx, c["gx"]):
                    assert kind == "probe", (EC.CASES[ci][1], kind, pad, active)   # (a probe call whose gradients all fall outside)
                    continue
                with pytest.raises(AssertionError):
                    EC.check_backward(gx, EC.round16(c["gw32"], tdt), c, active, kind, tdt, ("mutation b",))


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_checker_rejects_weights_rounded_half_away(dt):
    """(c) the sparse shift under weights rounded half away from zero instead of half to even: rejected by the forward and by grad_x
    wherever the two roundings give different results (under border padding a shift of 2 and of 3 along a dim of 3 both read the
    edge) -- under at least three of the five paddings of every case"""
    tdt = EC.DTYPES[dt]
    for ci in MUTATED:
        rejected = 0
        for pad in range(5):
            r = EC.reference(ci, dt, "exact", pad, 0)
            c = r["calls"][0]
            away = (np.sign(r["w"]) * np.floor(np.abs(r["w"]) + 0.5)).astype(np.float32)
            out = EC.round16(O.forward(r["x"], away, pad, 0, r["b"]), tdt)
            gx = EC.round16(O.backward(c["g"], away, r["x"], pad, 0, r["b"])[0], tdt)
            if np.array_equal(out, r["out"]) and np.array_equal(gx, c["gx"]):
                continue
            rejected += 1
            with pytest.raises(AssertionError):
                EC.check_forward(out, r, 0, "exact", tdt, ("mutation c",))
            with pytest.raises(AssertionError):
                EC.check_backward(gx, EC.round16(c["gw32"], tdt), c, 0, "exact", tdt, ("mutation c",))
        assert rejected >= 3, (EC.CASES[ci][1], rejected)


def _without_last_row(g):
    g = g.copy()
    if g.ndim == 3:
        g[..., -1] = 0     # (1-D: the last element of every row)
    else:
        g[..., -1, :] = 0
    return g


def test_checker_rejects_a_dropped_last_row_in_grad_w():
    """(d) the last row of the window left out of grad_w: rejected on the fp16 dense fixture in every call whose grad_w the row
    enters at all (under zeros padding its taps can all lie outside) -- at least half of a case's calls -- and by some probe call in
    bf16"""
    for ci in MUTATED:
        case, dense, probes = EC.CASES[ci], 0, 0
        for pad, active in EC.SWEEP:
            r = EC.reference(ci, "f16", "exact", pad, active)
            c = r["calls"][0]
            gw = _gw64(r, _without_last_row(c["g"]), pad, active)
            if not np.array_equal(gw, c["gw64"]):
                dense += 1
                with pytest.raises(AssertionError):
                    EC.check_backward(c["gx"], EC.round16(gw.astype(np.float32), torch.float16), c, active, "exact", torch.float16,
                                      ("mutation d",))
            r = EC.reference(ci, "bf16", "probe", pad, active)
            for c in r["calls"]:
                gw = _gw64(r, _without_last_row(c["g"]), pad, active)
                try:
                    EC.check_backward(c["gx"], EC.round16(gw.astype(np.float32), torch.bfloat16), c, active, "probe", torch.bfloat16,
                                      ("mutation d",))
                except AssertionError:
                    probes += 1
        assert 2 * dense >= len(EC.SWEEP) and probes >= 1, (case[1], dense, probes)


def test_the_old_bar_accepts_what_the_entry_bar_rejects():
    """(e) the gap, shown: on random bf16 data the smallest nonzero grad_w entry moved by 3 ulp16 of itself passes the bar of the
    existing tests, rel_err(gw, gw64) < gw16_tol(eps) -- relative to the LARGEST entry -- and fails assert_gw_entries.  It can pass
    the old bar only where 3.5 eps |entry| < 0.51 eps max|gw64|, and must fail the new one where 2.49 ulp16(entry) > 1e-5 max|gw64|:
    the calls with 2e-3 < |entry| / max|gw64| < 0.14 -- at least one per case."""
    tdt, eps = torch.bfloat16, torch.finfo(torch.bfloat16).eps
    for ci in MUTATED:
        shown = 0
        for pad, active in EC.SWEEP:
            r = EC.reference(ci, "bf16", "random", pad, active)
            c = r["calls"][0]
            gw64 = c["gw64"]
            mag = np.where(gw64 == 0, np.inf, np.abs(gw64))
            at = np.unravel_index(np.argmin(mag), mag.shape)
            if not 2e-3 < mag[at] / np.abs(gw64).max() < 0.14:
                continue
            gw = EC.round16(gw64.astype(np.float32), tdt).astype(np.float64)
            gw[at] = EC.round16(np.array([gw[at] + 3 * float(EC.ulp16(gw[at], tdt))], np.float32), tdt)[0]   # (narrowed: a value a kernel could return)
            assert rel_err(gw, gw64) < gw16_tol(eps), (EC.CASES[ci][1], pad, active)
            with pytest.raises(AssertionError):
                EC.check_backward(c["gx"], gw, c, active, "random", tdt, ("mutation e",))
            shown += 1
        assert shown >= 1, EC.CASES[ci][1]


def test_every_case_names_its_kernels():
    for case in EC.CASES:
        for d in "fb":
            for pad, active in EC.SWEEP:
                assert EC.expected(case, d, active, pad), (case[1], d, active, pad)
