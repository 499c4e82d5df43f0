"""Self-checks of the shift ladder (tests/shift_ladder.py) and of the tables tests/test_shift_ladder_gpu.py runs -- no GPU needed.

  rungs ............ every rung is finite, below 2^40 + 2049 and exact in its weight dtype; every table of every family deals every
                     rung of its ladder; only the two rows of the coverage exception use the reduced ladder; under zeros padding
                     every near rung stands in a row whose reference output keeps elements
  index map ........ oracle_infer_index == shift_ladder.index_ref (Python integers) at every effective shift of every ladder, for
                     every dim length of the tables, under every padding
  teeth ............ for every family and every wrong preparation of shift_ladder.MUTANTS that can differ on it at all, some dealt row
                     under some padding gives another expectation than the oracle's
  CPU backend ...... torch.ops.torchshifts on CPU tensors agrees with the oracle on the full ladder"""
import itertools

import numpy as np
import pytest
import torch

import shift_ladder as SL
import test_shift_ladder_gpu as G
from cases import rel_err
from oracle import oracle as O
from test_cpu_backend import _run

FAMILIES = G.families()
WDTYPES = ("float16", "bfloat16", "float32", "float64")


def _lengths():
    return sorted({n for f in FAMILIES for n in f.shape[2:]})


def test_rungs_are_exact_in_their_dtype():
    for n, pad, dt, active, nd, reduced in itertools.product(_lengths(), range(5), WDTYPES, (False, True), (1, 3), (False, True)):
        ladder = SL.rungs(n, pad, dt, active, nd, reduced)
        assert ladder and len(set(map(repr, ladder))) == len(ladder), (n, pad, dt, active)
        t = torch.tensor(ladder, dtype=torch.float64)
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) <= SL.LIMIT
        assert torch.equal(t.to(SL.TORCH_DTYPES[dt]).double(), t), (n, pad, dt, active)
        if not reduced:
            assert any(v == 0 and np.signbit(v) for v in ladder) and any(abs(v) >= 2048 for v in ladder)
            if dt in ("float32", "float64"):
                assert {2.0 ** 30, -(2.0 ** 30 + 128), 2.0 ** 40, 2.0 ** 31 + 256} <= set(ladder)
            if dt == "bfloat16":
                assert {2.0 ** 30, 2.0 ** 40, 258.0} <= set(ladder)
            if dt == "float16":
                assert {2050.0, 65504.0, -65504.0} <= set(ladder)
    for n, pad, (name, zps) in itertools.product(_lengths(), range(5), SL.ZERO_POINTS.items()):
        for zp in zps:
            lo, hi = SL.INT_RANGE[name]
            assert all(lo <= r + zp <= hi for r in SL.int_rungs(n, pad, name, zp))
    for sign in (1, -1):
        shifts = [int(v) - sign * SL.EXTREME_ZERO_POINT for t in SL.int32_extreme_tables([3], 5, 2, sign) for v in t[:, 0]]
        assert max(abs(s) for s in shifts) >= 2 ** 32 - 2 and all(s * sign <= 0 for s in shifts)


def test_every_table_deals_every_rung():
    """each dim of each family meets every rung of its ladder under every padding"""
    for f in FAMILIES:
        if f.ladders is None:
            continue
        for pad in range(5):
            dealt = np.concatenate(f.shifts(pad))
            for d, ladder in enumerate(f.ladders(pad)):
                seen = {repr(float(v)) for v in dealt[:, d]}
                missing = [v for v in ladder if repr(float(v)) not in seen]
                assert not missing, (f.id, pad, d, missing)


def test_only_the_two_large_rows_use_the_exception():
    assert sorted(f.name for f in FAMILIES if f.exception) == ["forward-step_gather_forward", "forward-sweep_active_forward"]
    for f in FAMILIES:
        if f.table == "A" and not f.quantized:
            entry = [e for e in G.FAMILY_ROUTES if G.entry_id(e) == f.name][0]
            for pad in range(5):
                full = [SL.rungs(n, pad, f.wdtype, f.active, len(f.shape) - 2) for n in f.shape[2:]]
                assert (f.ladders(pad) == full) == (not f.exception or pad == entry[5]), (f.id, pad)


def _slice_forward(f, x1, row, c, pad, borders):
    """the oracle's forward of one (n, c) slice under one row of shifts"""
    if f.quantized:
        return O.forward_q(x1, np.rint(row).astype(np.int64).reshape(1, -1), 0, G.X_ZERO_POINT, pad, borders)
    return O.forward(x1, np.asarray(row, np.float64).reshape(1, -1), pad, f.active, borders)


def _family_data(f):
    """the family's input (table A: what the GPU test feeds the kernel) as the fp64 / integer array the self-checks gather from"""
    if f.data is not None:
        x = f.data()
    elif f.quantized:
        x = G.quantized_data(np.random.RandomState(5), f.shape, torch.int8, G.X_ZERO_POINT)
    else:
        x = SL.dyadic(np.random.RandomState(5), f.shape)
    return x if f.quantized else x.astype(np.float64)


def _borders(f):
    return None if f.cut is None else O.check_borders(list(f.shape), f.cut, len(f.shape) - 2)[0]


def test_zeros_padding_keeps_every_near_rung_observable():
    """under zeros padding a rung that empties one dim fills the whole channel: every near rung must stand in a row whose reference
    output (the oracle on that channel; large problems: of the first sample) holds something else than the fill"""
    for f in FAMILIES:
        sizes = f.shape[2:]
        x, borders = _family_data(f), _borders(f)
        fill = G.X_ZERO_POINT if f.quantized else 0
        seen = [set() for _ in sizes]
        win = SL.windows(sizes, f.cut)
        for table in f.shifts(0):
            for c, row in enumerate(table):
                if not all(SL.is_near(v, n, f.active, lo, hi) for v, (n, lo, hi) in zip(row, win)):
                    continue
                some = slice(0, 1 if x[0, 0].size > 1 << 14 else None)    # (small problems: every sample, so that a blend that cancels
                out = _slice_forward(f, x[some, c:c + 1], row, c, 0, borders)   # on the one surviving element does not hide the row)
                if (out != fill).any():
                    for d, v in enumerate(row):
                        seen[d].add(repr(float(v)))
        for d, n in enumerate(sizes):
            near = {repr(float(v)) for t in f.shifts(0) for v in t[:, d] if SL.is_near(v, n, f.active, *win[d][1:])}
            assert near <= seen[d], (f.id, d, sorted(near - seen[d]))


def _index_ref_np(i, n, pad):
    """shift_ladder.index_ref on an int64 array (|i| stays below 2^41: nothing overflows); numpy's // and % floor like Python's"""
    if pad == 1:
        return np.clip(i, 0, n - 1)
    if pad == 2:
        return i % n
    if pad in (3, 4):
        p = n - 1 if pad == 3 else n
        q, r = i // p, i % p
        return np.where(q % 2 == 0, r, n - 1 - r)
    return np.where((i > n - 1) | (i < 0), -1, i)


EXACT_POSITIONS = 1024   # dims up to this length: shift_ladder.index_ref itself, in Python integers, at every position


def test_oracle_index_map_equals_the_integer_restatement():
    """every rung, position and padding, for every dim length of the tables.  Per length and padding ONE call of the oracle's integer
    forward on the row 0, 1, .., len - 1 returns the oracle's map at every position p under every effective shift s of every ladder
    (sparse and interpolating, every weight dtype, every integer table, the ends of int32 under the extreme zero points; s - 1 too:
    the interpolating shift's second tap, coordinate p + 1).  It must equal index_ref(p - s): in Python integers at every position
    of dims up to 1024 elements; for longer dims through the int64 restatement above, which is itself held to the Python-integer
    index_ref at 600 coordinates around either end of the row and every 97th between, for every shift.  oracle_infer_index is also
    called directly on those coordinates."""
    compared = 0
    for n in _lengths():
        if n == 1:
            continue
        row = np.arange(n, dtype=np.int32)
        for pad in range(5):
            shifts = {SL.effective(v, active) for dt in WDTYPES for active in (False, True) for v in SL.rungs(n, pad, dt, active)}
            shifts |= {int(r) for name, zps in SL.ZERO_POINTS.items() for zp in zps for r in SL.int_rungs(n, pad, name, zp)}
            shifts |= {2 ** 32 - 1, -(2 ** 32 - 1), 2 ** 32 - 2}
            shifts = sorted(shifts | {s - 1 for s in shifts})
            x = np.ascontiguousarray(np.broadcast_to(row, (1, len(shifts), n)))
            got = O.forward_q(x, np.array(shifts, np.int64).reshape(-1, 1), 0, -1, pad)[0].astype(np.int64)
            some = sorted(set(range(min(n, 300))) | set(range(max(0, n - 300), n)) | set(range(0, n, 97)))
            for c, s in enumerate(shifts):
                if n <= EXACT_POSITIONS:
                    want = np.array([max(SL.index_ref(p - s, n, pad), -1) for p in range(n)], np.int64)
                else:
                    want = _index_ref_np(np.arange(n, dtype=np.int64) - s, n, pad)
                    for p in some:
                        assert want[p] == max(SL.index_ref(p - s, n, pad), -1), (n, pad, s, p)
                assert np.array_equal(got[c], want), (n, pad, s, np.flatnonzero(got[c] != want)[:4].tolist())
                for p in (0, 1, n // 2, n - 1, n):
                    assert O.infer_index(p - s, n, pad) == SL.index_ref(p - s, n, pad), (n, pad, s, p)
                compared += n
    print("index map: %d coordinates compared" % compared)


def test_most_channels_get_the_exact_grad_w_check():
    """the gate of shift_ladder.exact_gw_channels decides which channels' grad_w is compared bit for bit on the GPU: per family with a
    weight gradient (table A's backward rows on the data the GPU test feeds them, table B's learnable rows) at least half of the
    dealt channel rows pass it under every padding, and the shares are printed"""
    for f in FAMILIES:
        learnable = f.table == "B" and f.name.split("-")[0] in ("tshift", "per_clip", "frames")
        if not (learnable or (f.table == "A" and f.name.startswith("backward-"))):
            continue
        if f.table == "A":
            entry = [e for e in G.FAMILY_ROUTES if G.entry_id(e) == f.name][0]
            x, g = G.entry_data(entry)
        else:
            rs = np.random.RandomState(7)
            x, g = SL.dyadic(rs, f.shape), SL.dyadic(rs, f.shape)
        shares = []
        for pad in range(5):
            passed = [SL.exact_gw_channels(g, x, t) for t in f.shifts(pad)]
            shares.append(float(np.mean(np.concatenate(passed))))
        print("%-60s exact grad_w rows per padding: %s" % (f.id, " ".join("%.2f" % v for v in shares)))
        assert min(shares) >= 0.5, (f.id, shares)


def _candidate(name, row, sizes, pad, f):
    """a cheap necessary condition for mutant `name` to differ from the right preparation on this row"""
    _, prep, src = SL.MUTANTS[name]
    for v, n in zip(row, sizes):
        s, frac = SL.prepare(float(v), n, pad, f.active, f.wdtype)
        if prep is not None and n > 1 and prep(float(v), n, pad, f.active, f.wdtype) != (s, frac):
            return True
        if name == "c" and n > 1 and pad >= 3 and s < 0 and abs(int(np.fmod(s, SL.map_period(n, pad)))) >= n - 1:
            return True     # (C's remainder keeps the sign: p + |c| leaves the one period the two folds cover)
        if name == "d" and n > 1 and abs(s) > 3:
            return True
        if name == "g" and n == 1 and pad == 0 and (s != 0 or frac != 0):
            return all(SL.is_near(u, m, f.active, lo, hi) for u, (m, lo, hi) in zip(row, SL.windows(sizes, f.cut)))
    return False


def _has_teeth(f, name, x, borders):
    """-> (padding, row) of the first dealt row whose expectation under the mutant differs from the right one's -- which must be the
    oracle's --, or None"""
    sizes = f.shape[2:]
    fill = G.X_ZERO_POINT if f.quantized else 0
    for pad in range(5):
        tried = 0
        for table in f.shifts(pad):
            for c, row in enumerate(table):
                if tried >= 12 or not _candidate(name, row, sizes, pad, f):
                    continue
                tried += 1
                xc = x[:1, c]
                right = SL.expect_channel(xc, row, pad, f.active, borders, f.wdtype, None, fill)
                wrong = SL.expect_channel(xc, row, pad, f.active, borders, f.wdtype, name, fill)
                if not np.array_equal(right, wrong):
                    assert np.array_equal(right, _slice_forward(f, x[:1, c:c + 1], row, c, pad, borders)[:, 0]), (f.id, name, pad, row)
                    return pad, [float(v) for v in row]
    return None


def test_the_ladder_has_teeth_for_every_family():
    matrix, toothless = [], []
    for f in FAMILIES:
        sizes = f.shape[2:]
        x, borders = _family_data(f), _borders(f)
        dealt = np.concatenate([t for pad in range(5) for t in f.shifts(pad)]) if f.quantized else None
        marks = []
        for name in sorted(SL.MUTANTS):
            applies = SL.applicable(name, sizes, f.wdtype, f.active, dealt)
            if not applies:
                marks.append("-")
                continue
            found = _has_teeth(f, name, x, borders)
            marks.append("x" if found else "MISSING")
            if not found:
                toothless.append((f.id, name, SL.MUTANTS[name][0]))
        matrix.append((f.id, marks))
    print("mutant applicability (x: some dealt row tells it from the oracle, -: cannot differ on this family)")
    print("%-78s %s" % ("family", "  ".join(sorted(SL.MUTANTS))))
    for fid, marks in matrix:
        print("%-78s %s" % (fid, "  ".join(marks)))
    assert not toothless, toothless


CPU_SHAPES = {1: (2, 3, 7), 2: (2, 3, 5, 6), 3: (1, 2, 3, 4, 5)}


@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("nd", [1, 2, 3])
def test_cpu_backend_on_the_full_ladder(nd, dt):
    """torch.ops.torchshifts.shift{N}d on CPU tensors (csrc/torch_cpu_backend.cpp): out and grad_x bit for bit, grad_w by
    tests/test_cpu_backend.py's bar (1e-5 / 1e-12 of the largest entry against the fp64 evaluation)"""
    shape = CPU_SHAPES[nd]
    ndt = np.dtype(dt).type
    rs = np.random.RandomState(nd)
    x, g = SL.dyadic(rs, shape).astype(ndt), SL.dyadic(rs, shape).astype(ndt)
    calls = 0
    for pad, active in itertools.product(range(5), (False, True)):
        for table in SL.tables(shape[2:], shape[1], pad, dt, active):
            w = table.astype(ndt)
            out, gx, gw = _run(x, w, pad, active, None, g)
            what = (shape, dt, pad, active, table.tolist())
            assert np.array_equal(out, O.forward(x, w, pad, active)), what + ("out",)
            gx_o, _ = O.backward(g, w, x, pad, active)
            gw64 = O.backward(g.astype(np.float64), table, x.astype(np.float64), pad, active)[1]
            assert np.array_equal(gx, gx_o), what + ("grad_x",)
            assert rel_err(gw, gw64) < (1e-5 if dt == "float32" else 1e-12), what + ("grad_w", rel_err(gw, gw64))
            calls += 1
    print("%d calls" % calls)
