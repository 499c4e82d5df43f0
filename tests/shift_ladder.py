"""The shift ladder: the weights at which a kernel's shift preparation can go wrong -- far shifts, the edges of every magnitude-dependent
branch, rounding ties and negative fractions -- dealt into [C, nd] tables for every kernel family (tests/test_shift_ladder_gpu.py on
the GPU, tests/test_shift_ladder_cases.py for the self-checks that need none).  Nothing here touches a GPU.

A shift weight is rounded (rint: the sparse shift; floor: the interpolating shift), converted to int64, reduced to one period of the
padding's index map and folded.  The ladder holds, with both signs:

  near / branch edges   0, -0.0, 1, 2, 3, 4 (csrc/shiftnd_cl_tiled.hip: the LDS ring serves |shift| <= kR = 3, the rest is gathered "far"),
                        6, 7 (the six-dword window of csrc/shiftnd_walk*.hip and shiftnd_step.hip), 8, 9 (csrc/shiftnd_qpool.hip: cs2 in
                        [-8, 8]), len - 1, len, len + 1, len + 2 (zeros / border clamp to +-(len + 1): shiftnd_common.hpp canon_shift)
  periods               P - 1, P, P + 1, 2P, 3P + 1, 1000 P + 1 with P = map_period(len, pad) (len where the map has no period)
  far                   10^6 + 3, 2^24 - 1, 2^24 + 2 (fp32's integer grid ends), 2^30 - 128, 2^30, 2^30 + 128 (canon_shift goes from
                        32-bit to 64-bit arithmetic at 2^30 inclusive, shiftnd_step.hpp canon_of at 2^30 strict), 2^31 + 256 (int32),
                        2^33 + 2048, 2^40 -- and 2^24 + 1, 2^31 + 1, 2^40 + 1, which only fp64 holds
  ties                  +-0.5, +-1.5, +-2.5, len + 0.5, 2^22 + 0.5 (the sparse shift rounds half to even)
  fractions             every integer rung below 64 plus 0.25, 0.5, 0.75 (3-D: 0.5), negative bases included (-3 + 0.25 -> floor -3);
                        -2^-20 and 2^22 + 0.5 for fp32 / fp64, 1 + 2^-30 for fp64

Each rung is kept only if the weight dtype represents it exactly (`representable`): that is the whole per-type filter.  No rung is
NaN, infinite or beyond 2^40 + 2049, so float -> int64 is defined everywhere.

`index_ref` restates the five padding maps in Python integers, `expect_channel` a channel's forward on top of it, and MUTANTS are the
wrong preparations the ladder must tell from the right one (the teeth test of tests/test_shift_ladder_cases.py)."""
import functools
import math

import numpy as np
import torch

TORCH_DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32, "float64": torch.float64}
LIMIT = 2 ** 40 + 2049
FAR = [10 ** 6 + 3, 2 ** 24 - 1, 2 ** 24 + 2, 2 ** 30 - 128, 2 ** 30, 2 ** 30 + 128, 2 ** 31 + 256, 2 ** 33 + 2048, 2 ** 40,
       2 ** 24 + 1, 2 ** 31 + 1, 2 ** 40 + 1,     # odd: fp64 only
       2048, 2050, 65504,                         # fp16's integer grid and its largest value
       256, 258]                                  # bf16's integer grid
RING = [0, 1, 2, 3, 4, 6, 7, 8, 9]
REDUCED_FAR = [2 ** 30, 2 ** 30 + 128, 2 ** 40]


def map_period(length, pad):
    """csrc/shiftnd_common.hpp map_period"""
    return {2: length, 3: 2 * (length - 1), 4: 2 * length}.get(pad, 0)


def representable(v, wdtype):
    """`wdtype` (a name of TORCH_DTYPES) holds the value v exactly"""
    if not math.isfinite(v) or abs(v) > LIMIT:
        return False
    try:
        return float(torch.tensor(float(v), dtype=torch.float64).to(TORCH_DTYPES[wdtype]).double()) == float(v) and float(v) == v
    except (OverflowError, RuntimeError):
        return False


def _both_signs(values):
    out = []
    for v in values:
        for s in (v, -v):
            if not any(s == o and math.copysign(1, s) == math.copysign(1, o) for o in out):
                out.append(s)
    return out


def integer_rungs(length, pad):
    """the integer rungs of one dim, unsigned and unfiltered: (near, periods, far)"""
    P = map_period(length, pad) or length
    near = RING + [length - 1, length, length + 1, length + 2]
    periods = [P - 1, P, P + 1, 2 * P, 3 * P + 1, 1000 * P + 1]
    return near, periods, list(FAR)


@functools.lru_cache(maxsize=None)
def _rungs(length, pad, wdtype, active, nd, reduced):
    near, periods, far = integer_rungs(length, pad)
    P = map_period(length, pad) or length
    if reduced:
        ints = [0, 3, 4, length + 1, P, P + 1, 1000 * P + 1] + REDUCED_FAR
    else:
        ints = near + periods + far
    ints = [float(v) for v in ints if v >= 0]
    values = _both_signs(ints)       # (0 and -0.0 are two rungs)
    steps = (0.5,) if nd == 3 else (0.25, 0.5, 0.75)
    if reduced:
        values += [-3 + steps[0]] if active else [-2.5]
    elif not active:
        values += _both_signs([0.5, 1.5, 2.5, length + 0.5, 2 ** 22 + 0.5])
    else:
        for r in _both_signs([v for v in ints if v < 64]):
            values += [r + f for f in steps]    # (-3 + 0.25: floor -3)
        if wdtype in ("float32", "float64"):    # (16-bit tensors would not stay exact under such fractions)
            values += [-2.0 ** -20, 2 ** 22 + 0.5, -(2 ** 22 + 0.5), 1 + 2.0 ** -30]
    out = []
    for v in values:
        if representable(v, wdtype) and not any(v == o and math.copysign(1, v) == math.copysign(1, o) for o in out):
            out.append(v)
    return tuple(out)


def rungs(length, pad, wdtype, active, nd=2, reduced=False):
    """the shift values of one dim of `length` under padding `pad` for weights of dtype `wdtype` (a name): the sparse shift's ladder
    (ties) or the interpolating shift's (fractions: quarters, halves in 3-D).  reduced: the short ladder of the coverage exception"""
    return list(_rungs(int(length), int(pad), wdtype, bool(active), int(nd), bool(reduced)))


def effective(v, active):
    """the integer shift a correct kernel derives from the weight v"""
    return int(math.floor(v)) if active else int(np.rint(v))


def is_near(v, length, active, lo=0, hi=None):
    """under zeros padding this rung leaves some coordinate of the window [lo, hi) of a dim of `length` on a tap inside the dim with
    a weight above zero (a size-1 dim ignores its shift)"""
    if length == 1:
        return True
    hi = length if hi is None else hi
    s = effective(v, active)
    frac = v - s if active else 0.0
    first = max(lo, s) < min(hi, length + s)                  # some i in [lo, hi) with 0 <= i - s < length
    second = max(lo, s - 1) < min(hi, length + s - 1)         # ... with 0 <= i - s + 1 < length
    return (first and frac < 1) or (second and frac > 0)


def _stride(k, n):
    s = (1, 3, 7)[k]
    while math.gcd(s, n) != 1:
        s += 1
    return s


@functools.lru_cache(maxsize=None)
def _rows(rungs_per_dim, lengths, active):
    nd = len(rungs_per_dim)
    rows = []

    def rotate(ladders, count, start=0):
        for r in range(start, start + count):
            yield [ladders[d][(r * _stride(d, len(ladders[d]))) % len(ladders[d])] for d in range(nd)]

    if lengths is None:
        return tuple(tuple(row) for row in rotate(rungs_per_dim, max(len(l) for l in rungs_per_dim)))
    near = [tuple(v for v in rungs_per_dim[d] if is_near(v, *lengths[d][:1], active, *lengths[d][1:])) for d in range(nd)]
    far = [tuple(v for v in rungs_per_dim[d] if not is_near(v, *lengths[d][:1], active, *lengths[d][1:])) for d in range(nd)]
    at = 0
    for d in range(nd):
        for f, row in zip(far[d], rotate(near, len(far[d]), at)):
            row[d] = f
            rows.append(tuple(row))
        at += len(far[d])
    rows += [tuple(row) for row in rotate(near, max(len(l) for l in near))]
    return tuple(rows)


def rows(rungs_per_dim, lengths=None, active=False):
    """every row the tables of one problem hold, in order.  Each dim rotates through its ladder with a stride of its own (1, 3, 7,
    moved to the next value coprime with the ladder's size), for as many rows as the longest ladder has rungs.  With `lengths` (zeros
    padding, where a rung that empties one dim fills the whole channel; an entry is the dim's length or (length, window start, window
    end)): first one row per emptying rung, the other dims on near
    rungs, then the near rungs of all dims rotating -- so every near rung stands in a row that keeps elements"""
    geometry = None if lengths is None else tuple((g,) if np.isscalar(g) else tuple(g) for g in lengths)
    return [list(r) for r in _rows(tuple(tuple(l) for l in rungs_per_dim), geometry, bool(active))]


def n_calls(rungs_per_dim, C, lengths=None, active=False):
    return -(-len(rows(rungs_per_dim, lengths, active)) // C)


def deal(rungs_per_dim, C, call, lengths=None, active=False):
    """-> the [C, nd] float64 table of call number `call` (the last call wraps round to the first rows)"""
    all_rows = rows(rungs_per_dim, lengths, active)
    assert 0 <= call < n_calls(rungs_per_dim, C, lengths, active)
    return np.array([all_rows[(call * C + c) % len(all_rows)] for c in range(C)], np.float64).reshape(C, len(rungs_per_dim))


def windows(sizes, cut):
    """-> per dim (length, window start, window end) for a cut of rows [left, right] per dim (None: the whole input)"""
    return [(n, 0, n) if cut is None else (n, int(cut[d][0]), n - int(cut[d][1])) for d, n in enumerate(sizes)]


def tables(sizes, C, pad, wdtype, active, reduced=False, cut=None):
    """-> the list of [C, nd] tables of a problem with spatial `sizes` (and the window `cut` leaves) under `pad`"""
    nd = len(sizes)
    ladders = [rungs(s, pad, wdtype, active, nd, reduced) for s in sizes]
    lengths = windows(sizes, cut) if pad == 0 else None
    return [deal(ladders, C, k, lengths, active) for k in range(n_calls(ladders, C, lengths, active))]


# -- integer tables ---------------------------------------------------------------------------------------------------------------
INT_RANGE = {"uint8": (0, 255), "int8": (-128, 127), "int32": (-2 ** 31, 2 ** 31 - 1)}
ZERO_POINTS = {"uint8": (0, 128, 255), "int8": (0,), "int32": (0,)}


def int_rungs(length, pad, table_dtype, zero_point):
    """the integer rungs r of one dim that an entry r + zero_point of `table_dtype` holds"""
    near, periods, far = integer_rungs(length, pad)
    lo, hi = INT_RANGE[table_dtype]
    pool = near + periods + (far + [2 ** 31 - 1, 2 ** 31 - 2] if table_dtype == "int32" else [])
    out = []
    for r in _both_signs(pool):
        r = int(r)
        if lo <= r + zero_point <= hi and abs(r) <= 2 ** 31 - 1 and r not in out:
            out.append(r)
    return out


def int_tables(sizes, C, pad, table_dtype, zero_point, cut=None):
    """-> the list of [C, nd] int64 tables of ENTRIES (shift + zero_point) of a quantized problem"""
    ladders = [int_rungs(s, pad, table_dtype, zero_point) for s in sizes]
    lengths = windows(sizes, cut) if pad == 0 else None
    return [np.rint(deal(ladders, C, k, lengths, False)).astype(np.int64) + zero_point
            for k in range(n_calls(ladders, C, lengths, False))]


EXTREME_ZERO_POINT = 2 ** 31 - 1


def int32_extreme_tables(sizes, C, pad, sign):
    """int32 tables under the zero point sign * (2^31 - 1): entry - zero_point passes -+2^32.  The shifts all have the sign opposite
    to the zero point's: every rung of the integer ladder the entries hold, and the two entries at the far end of int32"""
    zp = sign * EXTREME_ZERO_POINT
    ladders = []
    for s in sizes:
        near, periods, far = integer_rungs(s, pad)
        mags = sorted({int(v) for v in near + periods + far if v <= 2 ** 31 - 1} | {2 ** 32 - 2, 2 ** 32 - 1})
        ladders.append([-sign * m for m in mags if INT_RANGE["int32"][0] <= -sign * m + zp <= INT_RANGE["int32"][1]])
    lengths = list(sizes) if pad == 0 else None
    return [np.rint(deal(ladders, C, k, lengths, False)).astype(np.int64) + zp for k in range(n_calls(ladders, C, lengths, False))]


# -- the index maps in Python integers --------------------------------------------------------------------------------------------
def index_ref(i, n, pad):
    """source index of coordinate i in a dim of n elements: zeros (-1, or a negative i itself: "outside"), border, periodic,
    reflect, symmetric"""
    if pad == 1:
        return min(max(i, 0), n - 1)
    if pad == 2:
        return i % n
    if pad in (3, 4):
        p = n - 1 if pad == 3 else n
        q, r = divmod(i, p)
        return r if q % 2 == 0 else n - 1 - r
    return -1 if i > n - 1 else i


def prepare(w, n, pad, active, wdtype):
    """weight -> (integer shift, fraction): rint for the sparse shift, floor for the interpolating one"""
    s = effective(w, active)
    return s, (w - s if active else 0.0)


def source(p, s, n, pad):
    """the element of a dim of n that coordinate p reads under shift s (negative: outside); a size-1 dim ignores its shift"""
    return 0 if n == 1 else index_ref(p - s, n, pad)


def _fold_once(idx, n, pad):
    """csrc/shiftnd_common.hpp fold_index: at most two conditional folds, right for idx within one period of [0, n)"""
    if pad == 2:
        idx += n if idx < 0 else 0
        return idx - n if idx >= n else idx
    if pad == 3:
        idx = -idx if idx < 0 else idx
        return 2 * (n - 1) - idx if idx > n - 1 else idx
    idx = -idx - 1 if idx < 0 else idx
    return 2 * n - 1 - idx if idx >= n else idx


def _mut_int32(w, n, pad, active, wdtype):
    s, f = prepare(w, n, pad, active, wdtype)
    return (s + 2 ** 31) % 2 ** 32 - 2 ** 31, f


def _mut_clamp(w, n, pad, active, wdtype):
    s, f = prepare(w, n, pad, active, wdtype)
    return (max(-(n + 1), min(n + 1, s)) if pad >= 2 else s), f


def _mut_c_remainder(p, s, n, pad):
    if n == 1 or pad < 2:
        return source(p, s, n, pad)
    P = map_period(n, pad)
    c = int(math.fmod(s, P))          # C's %: the sign of s
    r = _fold_once(p - c, n, pad)
    return r if 0 <= r < n else -1


def _mut_far_fill(p, s, n, pad):
    return -1 if (n > 1 and abs(s) > 3) else source(p, s, n, pad)


def _mut_half_away(w, n, pad, active, wdtype):
    if active:
        return prepare(w, n, pad, active, wdtype)
    return int(math.copysign(math.floor(abs(w) + 0.5), w)), 0.0


def _mut_through_fp32(w, n, pad, active, wdtype):
    return prepare(float(np.float32(w)), n, pad, active, wdtype)


def _mut_size1(p, s, n, pad):
    if n != 1:
        return source(p, s, n, pad)
    return (0 if p - s == 0 else -1) if pad == 0 else 0


def _mut_trunc(w, n, pad, active, wdtype):
    if not active:
        return prepare(w, n, pad, active, wdtype)
    s = int(math.trunc(w))
    return s, w - s


# name -> (what it models, prepare or None, source or None)
MUTANTS = {
    "a": ("the shift truncated to int32", _mut_int32, None),
    "b": ("the shift clamped to +-(len + 1) under paddings 2-4", _mut_clamp, None),
    "c": ("C's truncating % on negative shifts, then the two-fold index", None, _mut_c_remainder),
    "d": ("|shift| > 3 treated as fill", None, _mut_far_fill),
    "e": ("ties rounded half away from zero", _mut_half_away, None),
    "f": ("an fp64 weight passed through fp32", _mut_through_fp32, None),
    "g": ("the shift applied on a size-1 dim", None, _mut_size1),
    "h": ("floor replaced by truncation toward zero", _mut_trunc, None),
}


def max_shift(wdtype):
    """the largest |shift| a float weight type can carry on this ladder"""
    return min(LIMIT, int(min(torch.finfo(TORCH_DTYPES[wdtype]).max, LIMIT)))


def applicable(name, sizes, wdtype, active, dealt=None):
    """whether mutant `name` can differ from the right preparation on a family at all -- from the family's shape and weight type;
    a quantized family passes `dealt`, the integer shifts its tables carry as [rows, nd] (entry - zero point: a uint8 table under
    zero point 0 holds no negative shift, one under 255 no positive one)"""
    big = [n for n in sizes if n > 1]
    quantized = dealt is not None
    top = int(np.abs(dealt).max()) if quantized else max_shift(wdtype)
    if name == "a":
        return bool(big) and top >= 2 ** 31
    if name == "b":
        return any(n + 1 < top for n in big)
    if name == "c":    # a negative shift beyond one dim's length (reflect / symmetric fold it twice)
        if quantized:
            return any(n > 1 and (np.asarray(dealt)[:, d] < -n - 1).any() for d, n in enumerate(sizes))
        return any(n + 1 < top for n in big)
    if name == "d":
        return bool(big) and top > 3
    if name == "e":
        return bool(big) and not active and not quantized
    if name == "f":
        return bool(big) and wdtype == "float64"
    if name == "g":
        return any(n == 1 for n in sizes)
    if name == "h":
        return bool(big) and bool(active) and not quantized
    raise KeyError(name)


def channel_maps(row, sizes, window, pad, active, wdtype, mutant=None):
    """-> per dim (fraction, [source indices per tap: one array over the window's coordinates each])"""
    _, prep, src = MUTANTS[mutant] if mutant else (None, None, None)
    prep, src = prep or prepare, src or source
    maps = []
    for d, n in enumerate(sizes):
        s, frac = prep(float(row[d]), n, pad, active, wdtype)
        lo, hi = window[d]
        taps = [np.array([src(p + q, s, n, pad) for p in range(lo, hi)], np.int64) for q in ((0, 1) if active else (0,))]
        maps.append((frac, taps))
    return maps


def expect_channel(xc, row, pad, active, borders=None, wdtype="float64", mutant=None, fill=0):
    """one channel's forward, xc[N, S...] -> [N, O...], from index_ref (or a mutant's preparation): the corners gathered in
    Python-integer index arithmetic, combined in the oracle's order (dim 0 innermost; v1 * (1 - d) + v2 * d)"""
    sizes = list(xc.shape[1:])
    nd = len(sizes)
    window = [(0, n) for n in sizes] if borders is None else [(int(borders[2 * d]), int(borders[2 * d + 1])) for d in range(nd)]
    maps = channel_maps(row, sizes, window, pad, active, wdtype, mutant)

    def corner(q):
        idx = [maps[d][1][(q >> d) & 1] for d in range(nd)]
        v = xc[(slice(None),) + np.ix_(*[np.clip(i, 0, n - 1) for i, n in zip(idx, sizes)])]
        valid = np.ones([len(i) for i in idx], bool)
        for d, (i, n) in enumerate(zip(idx, sizes)):
            valid &= ((i >= 0) & (i < n)).reshape([-1 if k == d else 1 for k in range(nd)])
        return np.where(valid[None], v, np.asarray(fill, xc.dtype))

    if not active:
        return corner(0)
    level = [corner(q) for q in range(1 << nd)]
    for d in range(nd):
        t = xc.dtype.type(maps[d][0])
        level = [level[2 * k] * (1 - t) + level[2 * k + 1] * t for k in range(len(level) // 2)]
    return level[0]


def maps_differ(row, sizes, window, pad, active, wdtype, mutant):
    a = channel_maps(row, sizes, window, pad, active, wdtype)
    b = channel_maps(row, sizes, window, pad, active, wdtype, mutant)
    return any(fa != fb or any(not np.array_equal(ta, tb) for ta, tb in zip(ma, mb)) for (fa, ma), (fb, mb) in zip(a, b))


# -- data and the gradient bound --------------------------------------------------------------------------------------------------
def dyadic(rs, shape):
    """multiples of 1/8 with 1 <= |k| <= 7 (tests/pooled16_cases.py exact_data's grid without the zero: under zeros padding an
    element that survives a shift never looks like fill)"""
    k = rs.randint(1, 8, size=shape) * (2 * rs.randint(0, 2, size=shape) - 1)
    return (k / 8.0).astype(np.float32)


def fraction_bits(w):
    """per entry of a weight table: the bits of its fraction w - floor(w) -- 0 (an integer), 1 (a half), 2 (a quarter) -- or -1 where
    the fraction lies off the exact-data grid"""
    f = np.asarray(w, np.float64)
    f = f - np.floor(f)
    return np.where(f == 0, 0, np.where(2 * f == np.rint(2 * f), 1, np.where(4 * f == np.rint(4 * f), 2, -1)))


def exact_gw_channels(g, x, w):
    """per channel: every partial sum of grad_w is exact in fp32, in any order.  A term of grad_w[d] is g (a multiple of 2^-3) times
    a difference of two taps (2^-3) blended by the fractions of the OTHER dims, so it is a multiple of 2^-u with u = 6 + the fraction
    bits of the other dims (at most 2^-8 on the quarters of 1-D / 2-D and the halves of 3-D tables), and its magnitude is at most
    |g| (|xa| + |xb|) <= |g| 2 max|x|.  The gate is sum |g| * 2 max|x| * 2^u < 2^24 with u taken for the dim whose others carry
    the most bits: the issue's sum |g| (|xa| + |xb|) * 2^8 < 2^24 with the taps bounded by the channel's largest |x| and 2^8
    replaced by the unit the row's own fractions give (never above 2^8), which admits the integer and one-fraction rows of channels
    too large for the blanket 2^8."""
    axes = tuple(a for a in range(x.ndim) if a != 1)
    bits = fraction_bits(w)
    on_grid = np.all(bits >= 0, axis=1)
    u = 6 + np.where(on_grid, bits.sum(axis=1) - bits.min(axis=1), 0)
    bound = np.abs(g).astype(np.float64).sum(axis=axes) * 2 * np.abs(x).astype(np.float64).max(axis=axes) * 2.0 ** u
    return on_grid & (u <= 8) & (bound < 2 ** 24)
