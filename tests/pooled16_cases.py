"""Case table, exact-data fixture, two-step reference, route rules and assertion functions of the pooled 16-bit parity tests
(tests/test_pooled16_gpu.py on the GPU, tests/test_pooled16_cases.py for the self-checks that need none).

The specification of the fused shift + average pool on fp16 / bf16 tensors is the module's two-step sequence on widened values:
the shift's output narrowed to the storage type, the window summed in fp32 in ATen's plane, row, column order, divided once and
narrowed once; backward: the pooled gradient divided by the window count and narrowed (what ATen's avg_pool
backward returns), then the plain shift backward.

EXACT DATA.  x and grad_pooled are multiples of 1/8 with |k| <= 7, the weights lie on a grid of quarters (1-D, 2-D) or halves
(3-D) and are narrowed to bf16 (which fp16 holds too), so every tap of the interpolation, every window sum, every expanded gradient
over a window of 2^n elements, grad_x and every partial sum of grad_w is exact in fp32 -- and the shifted tensor, the expanded gradient
and grad_x are representable in fp16 and in bf16.  A correct kernel therefore returns round16(fp32(sum) / fp32(count)), the exact
grad_x and round16(grad_w) bit for bit, whatever its evaluation order or fma use.  tests/test_pooled16_cases.py checks these claims
on the oracle for every case, padding and shift.
"""
import functools

import numpy as np
import torch

from oracle import oracle as O
from test_step_gpu import FLOOR16   # 8 fp32 ulps of the operands' unit scale: results that cancel to almost nothing

PIECE = 16   # bytes

# nd, shape, pool, cut (rows [left, right] per dim, as check_borders takes them; None: the whole input), note
CASES = [
    # 2-D, 2 x 2 windows
    (2, (2, 3, 18, 32), (2, 2), None, "odd number of pooled rows"),
    (2, (2, 3, 20, 24), (2, 2), [[1, 1], [1, 1]], "window 18 x 22, P = 9 x 11: pooled rows and planes at 2-byte boundaries"),
    (2, (1, 2, 7, 40), (2, 2), [[0, 0], [1, 0]], "window 7 x 39: ragged last window row and column"),
    (2, (2, 2, 9, 8), (2, 2), None, "rows of one piece"),
    (2, (2, 3, 11, 30), (2, 2), None, "input rows that are not whole pieces"),
    (2, (1, 2, 70, 64), (2, 2), [[1, 1], [1, 1]], "several steps per plane"),
    (2, (2, 2, 6, 16), (2, 2), [[0, 0], [7, 8]], "a one-column window"),
    # 2-D, other windows
    (2, (2, 3, 13, 24), (3, 2), [[1, 0], [0, 3]], "3 x 2 windows over a cut"),
    (2, (1, 3, 16, 40), (3, 3), [[1, 1], [1, 1]], "3 x 3 windows, cut 1 / 1"),
    (2, (2, 2, 12, 16), (1, 2), None, "a row window"),
    (2, (1, 2, 9, 16), (4, 4), None, "4 x 4 windows, ragged rows of windows"),
    # 3-D
    (3, (2, 3, 6, 8, 16), (2, 2, 2), None, "whole windows"),
    (3, (1, 3, 5, 7, 24), (2, 2, 2), None, "ragged planes and rows"),
    (3, (2, 3, 6, 9, 16), (2, 2, 2), [[1, 1], [1, 1], [1, 1]], "window 4 x 7 x 14: P2 = 7"),
    (3, (1, 2, 5, 8, 24), (2, 2, 2), [[1, 0], [0, 1], [2, 2]], "one-sided cuts, a left cut of 2"),
    (3, (1, 2, 5, 8, 24), (2, 2, 2), [[0, 0], [0, 0], [3, 0]], "odd width and a left cut of more than 2"),
    (3, (1, 2, 4, 6, 16), (1, 2, 2), None, "windows of one plane"),
    (3, (1, 2, 4, 6, 16), (3, 2, 2), None, "windows of three planes"),
    (3, (1, 3, 2, 1, 8), (2, 2, 2), None, "one row per plane"),
    # 1-D
    (1, (2, 3, 2048), (2,), None, "long rows"),
    (1, (2, 2, 1032), (2,), [[1, 1]], "long rows, cut 1 / 1"),
    (1, (1, 3, 640), (2,), [[0, 3]], "a 637-wide window"),
    (1, (2, 3, 40), (2,), None, "short rows: the plane kernels"),
    (1, (2, 3, 40), (3,), None, "short rows, windows of 3: the plane kernels"),
]
LONG_ROWS = 128 * PIECE // 2   # elements of a 1-D row from which these cases also run under knobs 32 / 34 = 2 (as test_pooled_1d_rows does)

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def group(nd):
    return [c for c in CASES if c[0] == nd]


def geometry(case):
    """-> (borders: 6 ints, window sizes [O...], pooled sizes [P...])"""
    nd, shape, pool, cut, _ = case
    b, new = O.check_borders(list(shape), cut, nd)
    win = list(new[2:])
    return b, win, [-(-o // k) for o, k in zip(win, pool)]


def pow2_counts(case):
    """every clipped window count is a power of two: dividing by it is exact"""
    _, win, pooled = geometry(case)
    cnt = O._pool_counts(win, pooled, list(case[2]))
    return bool(np.all((cnt & (cnt - 1)) == 0))


def round16(a, tdt):
    """fp32 array -> the storage type (round to nearest even) -> fp32; the identity for fp32"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if tdt == torch.float32:
        return a
    return torch.from_numpy(a).to(tdt).float().numpy()


def representable(a, tdt):
    a = np.asarray(a)
    return bool(np.array_equal(round16(a.astype(np.float32), tdt).astype(a.dtype), a))


def ulp16(v, tdt):
    """one unit in the last place of `tdt` at v, as tests/test_hip_parity.py::_ulp_close takes it: clamp(|v|, tiny) * eps"""
    fi = torch.finfo(tdt)
    return np.maximum(np.abs(np.asarray(v, np.float64)), fi.tiny) * fi.eps


def exact_data(rs, nd, shape, pooled_shape, turn=0):
    """-> x[shape], w[C, nd], grad_pooled[pooled_shape] (fp32): the dyadic inputs of the module docstring.  The usual special
    weights -- 0; the dim's size + 1 + one grid step (everything out of range); minus half the size -- go to the channels before the
    last, one per dim and rotated from dim to dim and channel to channel (`turn` rotates them from case to case), so that with the
    two or three channels of CASES every special meets every padding while the last channel keeps a drawn fractional shift in every
    dim.  The weights are narrowed to bf16: 41.25 stays, 2049.25 becomes 2048 -- still on the grid, still beyond the row."""
    x = (rs.randint(-7, 8, size=shape) / 8.0).astype(np.float32)
    gp = (rs.randint(-7, 8, size=pooled_shape) / 8.0).astype(np.float32)
    grid = 4.0 if nd <= 2 else 2.0
    C = shape[1]
    w = rs.randint(-int(3.5 * grid), int(3.5 * grid) + 1, size=(C, nd)) / grid
    sizes = np.array(shape[2:], np.float64)
    special = [np.zeros(nd), sizes + 1 + 1 / grid, -sizes / 2]
    for r in range(min(C - 1, 3)):
        for d in range(nd):
            w[r, d] = special[(r + d + turn) % 3][d]
    w[C - 1] += np.where(w[C - 1] == np.rint(w[C - 1]), 1 / grid, 0.0)   # (the drawn channel interpolates in every dim)
    w = round16(w.astype(np.float32), torch.bfloat16)
    assert np.array_equal(w * grid, np.rint(w * grid))
    return x, w, gp


def random_data(rs, nd, shape, pooled_shape, tdt):
    """as tests/test_pooled_gpu.py::test_pooled_16bit draws them: uniform(-1, 1) tensors and uniform(-2.6, 2.6) weights, narrowed"""
    x = round16(rs.uniform(-1, 1, size=shape), tdt)
    w = round16(rs.uniform(-2.6, 2.6, size=(shape[1], nd)), tdt)
    gp = round16(rs.uniform(-1, 1, size=pooled_shape), tdt)
    return x, w, gp


def two_step_reference(x, w, gp, pad, active, pool, b, tdt):
    """the module's sequence on widened values, through oracle.oracle only -> y, ref, g, gx_ref (fp32 arrays holding values of
    `tdt`), gw64 (fp64, unrounded, from the SAME narrowed g)"""
    y = round16(O.forward(x, w, pad, active, b), tdt)
    ref = round16(O.avg_pool(y, pool), tdt)
    g = round16(O.avg_pool_backward(gp, pool, y.shape[2:]), tdt)
    gx_ref = round16(O.backward(g, w, x, pad, active, b)[0], tdt)
    _, gw64 = O.backward(g.astype(np.float64), w.astype(np.float64), x.astype(np.float64), pad, active, b)
    return y, ref, g, gx_ref, gw64


@functools.lru_cache(maxsize=None)
def reference(ci, dt, kind, pad, active):
    """the inputs and the two-step reference of CASES[ci] -- computed once, shared by every test that needs them and never written
    to.  kind: "exact" (the same inputs for every dtype) or "random" (narrowed to the dtype).
    -> dict(x, w, gp, y, ref, g, gx_ref, gw64, b)"""
    case = CASES[ci]
    nd, shape, pool, _, _ = case
    tdt = DTYPES[dt]
    b, _, pooled = geometry(case)
    x, w, gp = _inputs(ci, dt if kind == "random" else "", kind)
    y, ref, g, gx_ref, gw64 = two_step_reference(x, w, gp, pad, active, pool, b, tdt)
    r = dict(x=x, w=w, gp=gp, y=y, ref=ref, g=g, gx_ref=gx_ref, gw64=gw64, b=b)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _inputs(ci, dt, kind):
    nd, shape, pool, _, _ = CASES[ci]
    _, _, pooled = geometry(CASES[ci])
    pshape = tuple(shape[:2]) + tuple(pooled)
    if kind == "exact":
        return exact_data(np.random.RandomState(100 + ci), nd, shape, pshape, turn=ci)
    return random_data(np.random.RandomState(200 + ci), nd, shape, pshape, DTYPES[dt])


# ---------------------------------------------------------------------------------------------------------------------
# assertion functions: numpy arrays of widened values in, AssertionError out.  Shared by the GPU tests (on what the kernels return)
# and by the CPU self-checks (on the reference itself, and on mutated references, which they must reject).
# ---------------------------------------------------------------------------------------------------------------------
def assert_bits(got, ref, what):
    """bit for bit (torch.equal on the widened values)"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = got != ref
    assert not bad.any(), (what, "%d of %d differ" % (int(bad.sum()), bad.size), "first at", tuple(np.argwhere(bad)[0]),
                           float(got[bad][0]), float(ref[bad][0]))


def assert_ulp_close(got, ref, tdt, floor, what):
    """tests/test_hip_parity.py::_ulp_close on arrays: |got - ref| <= 1.0001 ulp16(ref) + floor, per element"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    over = np.abs(got - ref) - (ulp16(ref, tdt) * 1.0001 + floor)
    assert not (over > 0).any() and not np.isnan(got).any(), (what, "%d of %d beyond 1 ulp" % (int((over > 0).sum()), over.size),
                                                               "worst excess", float(np.nanmax(over)))


def assert_pooled_interp(out, y, ref, pool, tdt, what):
    """the interpolating shift's pooled forward, per element: |out - ref| <= avg_pool(ulp16(y) + FLOOR16) + 1.0001 ulp16(ref).
    Each tap may differ from the oracle's by the 1 ulp (+ FLOOR16) the suite grants 16-bit interpolation everywhere; their mean
    passes through the pool; the two narrowed results then differ by at most one more unit."""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    bound = O.avg_pool(ulp16(y, tdt) + FLOOR16, pool) + 1.0001 * ulp16(ref, tdt)
    over = np.abs(out - ref) - bound
    assert not (over > 0).any() and not np.isnan(out).any(), (what, "%d of %d beyond the bound" % (int((over > 0).sum()), over.size),
                                                               "worst excess", float(np.nanmax(over)))


def assert_gw_entries(gw, gw64, tdt, what):
    """grad_w per entry: |gw - gw64| <= 0.51 ulp16(gw64) + 1e-5 max|gw64| -- one narrowing at the entry's OWN magnitude (cases.gw16_tol)
    plus the project's fp32 accumulation bar; the largest entry does not lend its rounding allowance to the small ones"""
    gw, gw64 = np.asarray(gw, np.float64), np.asarray(gw64, np.float64)
    assert gw.shape == gw64.shape, (what, gw.shape, gw64.shape)
    bound = 0.51 * ulp16(gw64, tdt) + 1e-5 * np.abs(gw64).max()
    over = np.abs(gw - gw64) - bound
    assert not (over > 0).any() and not np.isnan(gw).any(), (what, "entries beyond the bound", np.argwhere(over > 0).tolist(),
                                                              "got", gw[over > 0].tolist(), "want", gw64[over > 0].tolist())


def check_forward(out, r, case, active, kind, tdt, what):
    """item 2 (exact data: bit for bit on every case) / item 3 (random data: the sparse shift bit for bit, interpolation per element)"""
    if kind == "exact" or not active or tdt == torch.float32:
        assert_bits(out, r["ref"], what + ("forward",))
    else:
        assert_pooled_interp(out, r["y"], r["ref"], case[2], tdt, what + ("forward",))


def check_backward(gx, gw, r, case, active, kind, tdt, what):
    """item 2 on exact data with power-of-two window counts: grad_x and grad_w == round(gw64) bit for bit (fp32: grad_w == gw64).
    Otherwise (random data; exact data under 3-wide windows, whose expanded gradient is rounded) the bounds of item 3: the sparse
    shift's grad_x bit for bit (a copy of the narrowed gradient), the interpolating shift's within 1 ulp (+ FLOOR16), grad_w per
    entry.  fp32 (the control): grad_x bit for bit as everywhere in the suite, grad_w within 1e-5 of the largest entry."""
    if kind == "exact" and pow2_counts(case):
        assert_bits(gx, r["gx_ref"], what + ("grad_x",))
        assert_bits(gw, round16(r["gw64"].astype(np.float32), tdt), what + ("grad_w",))
        if tdt == torch.float32:
            assert np.array_equal(np.asarray(gw, np.float64), r["gw64"]), what + ("grad_w vs fp64",)
        return
    if not active or tdt == torch.float32:
        assert_bits(gx, r["gx_ref"], what + ("grad_x",))
    else:
        assert_ulp_close(gx, r["gx_ref"], tdt, FLOOR16, what + ("grad_x",))
    if tdt == torch.float32:
        err = np.abs(np.asarray(gw, np.float64) - r["gw64"]).max() / max(np.abs(r["gw64"]).max(), 1e-30)
        assert err < 1e-5, what + ("grad_w", err)
    else:
        assert_gw_entries(gw, r["gw64"], tdt, what + ("grad_w",))


# ---------------------------------------------------------------------------------------------------------------------
# routes: which kernel serves a case, restated from the host's eligibility rules (csrc/shiftnd_api.hip: shiftnd_forward_pooled /
# backward_pooled_planned, and the *_eligible functions they call) for the small dense aligned tensors of CASES
# ---------------------------------------------------------------------------------------------------------------------
NOT_SERVED = "not served"
BAND_WALK = ("plane_backward_pool", "plane_backward_lds_pool")   # (which of the two: the plane family's own LDS plan)


def forward_route(case, es, active, pad, policy=0, knob34=0):
    nd, shape, pool, cut, _ = case
    _, O_, P = geometry(case)
    S = list(shape[2:])
    whole = (S[-1] * es) % PIECE == 0          # source rows of whole 16-byte pieces
    if policy != 0:
        return "plane_pool_forward"             # (policy 2: the per-channel plane kernel, every shape)
    # walk_forward_pooled_eligible: 3-D, interpolating, windows (K0, K1 <= 2, 2), no cut, at least two planes, rows of whole pieces;
    # a window's two rows live in one workgroup (at least two rows per step)
    if nd == 3 and active and cut is None and pool[2] == 2 and pool[1] in (1, 2) and S[0] >= 2 and whole and S[2] * es // PIECE <= 128:
        if pool[1] == 1 or min(256 // (S[2] * es // PIECE) - 1, S[1]) >= 2:
            return "walk_forward_pool"
    # step_forward_pooled_eligible: 2-D, 2 x 2 windows of any width; 16-bit tensors: the sparse shift only; 4-byte: both (dims >= 2)
    if nd == 2 and tuple(pool) == (2, 2) and (not active or (es >= 4 and min(S) >= 2)):
        return "step_gather_forward_pool"
    # span_forward_pooled3_eligible: 3-D, 2 x 2 x 2 windows, cut or not, every dim of volume and window >= 2, rows of whole pieces
    if nd == 3 and tuple(pool) == (2, 2, 2) and min(S) >= 2 and min(O_) >= 2 and whole and 3 * (S[2] * es // PIECE) <= 256:
        return "crop_forward3_pool"
    # span_forward_pooled_eligible: 1-D, windows of 2, rows of whole pieces, at least 128 output chunks (knob 34 = 2: any)
    if nd == 1 and pool[0] == 2 and whole and S[0] >= 2 and (knob34 >= 2 or (O_[0] * es + PIECE - 1) // PIECE >= 128):
        return "row_forward_pool"
    return "plane_pool_forward"


def backward_route(case, es, active, pad, policy=0, knob32=0, band_walk=False):
    """-> a kernel name, BAND_WALK (either of the two) or NOT_SERVED.  band_walk: knob 35 bit 6 (plane_pool_backward keeps the
    band-walk kernels instead of handing windows / the interpolating shift to crop_backward<.., POOL>)"""
    nd, shape, pool, cut, _ = case
    _, O_, P = geometry(case)
    b, _, _ = geometry(case)
    S = list(shape[2:])
    whole = (S[-1] * es) % PIECE == 0
    L2 = b[2 * (nd - 1)]                       # the window's first column
    if not whole:
        return NOT_SERVED                       # (plane_pool_backward_eligible and every fused form: x rows of whole pieces)
    # span_geometry_ok(pooled): windows of 2 in every dim, pooled rows of at least half a piece
    span_geo = all(k == 2 for k in pool) and P[-1] >= max(1, 8 // es) and not (pad == 0 and O_[-1] == 1)
    if nd == 3:
        # walk_backward_pooled_eligible: windows (K0, K1, 2), both shifts, at least two planes; a cut: zeros padding, a window of
        # at least 2 x 2 x 2 that begins at most two columns into the rows and has an even width
        cwalk = cut is not None and pad == 0 and min(O_) >= 2 and L2 <= 2 and O_[2] % 2 == 0
        if policy == 0 and pool[2] == 2 and S[0] >= 2 and (cut is None or cwalk):
            return "walk_backward_crop_pool" if cut is not None else "walk_backward_pool"
        # span_backward_pooled_eligible, 3-D: cut volumes, 2 x 2 x 2 windows, every dim of volume and window >= 2 (crop_backward3<.., POOL>)
        crop3 = cut is not None and span_geo and min(S) >= 2 and min(O_) >= 2
        if crop3:
            return "crop_backward3_pool"        # (policy 0: shiftnd_backward_pooled; policy 2: plane_pool_backward hands it over)
        if active and policy != 2:
            return NOT_SERVED                   # (slower than avg_pool backward + the shift's backward: not fused)
        if policy == 0 and cut is not None and min(S) >= 2 and min(O_) >= 2:
            return NOT_SERVED                   # (a cut volume crop_backward3 serves unpooled: the op composes the two)
        return BAND_WALK
    # step_backward_pooled_eligible: 2-D, the sparse shift, no cut, any window
    if nd == 2 and not active and cut is None:
        return "step_backward_pool"
    if not band_walk:
        if nd == 2 and span_geo:
            return "crop_backward_pool"         # windows and the interpolating shift, 2 x 2
        if nd == 1 and span_geo and (S[0] * es // PIECE >= 128 or knob32 == 2):   # (short rows: the per-channel kernels, as unpooled)
            return "row_backward_pool"
    return BAND_WALK


SERVED_16BIT = {"step_gather_forward_pool", "plane_pool_forward", "walk_forward_pool", "crop_forward3_pool", "row_forward_pool",
                "step_backward_pool", "crop_backward_pool", "walk_backward_pool", "walk_backward_crop_pool", "crop_backward3_pool",
                "row_backward_pool"}   # ... and plane_backward_pool and / or plane_backward_lds_pool (BAND_WALK)
