"""Every kernel family under the shift ladder (tests/shift_ladder.py): far shifts, the edges of each magnitude-dependent branch,
rounding ties, negative fractions and size-1 dims, against the CPU oracle on widened values.

  table A   one test per row of test_routing_gpu.FAMILY_ROUTES: the row's shape, dtype, cut, layout and shift kind under all five
            paddings; the pinned kernel name at the row's own padding, the name that ran (printed) at the others
  table B   the temporal family (length = T)
  table C   the input-free backward and the pooled kernels

Only the weight table comes from the ladder.  x and the gradients are multiples of 1/8 with |k| <= 7 (pooled16_cases.exact_data's
grid), quantized tensors random integers without the zero point's value.  Every output buffer starts as NaN (0xA5 bytes for integer
tensors): an element no kernel wrote fails.

out and grad_x: bit for bit.  grad_w: bit-equal to the fp64 oracle's sum (narrowed once for 16-bit tensors) in every channel where
shift_ladder.exact_gw_channels holds -- every partial sum is then exact in fp32 in any order --, elsewhere the suite's bars (1e-5 /
1e-12 of the largest entry for fp32 / fp64, pooled16_cases.assert_gw_entries for 16-bit); a channel whose reference grad_w is zero
comes back zero."""
import concurrent.futures
import zlib

import numpy as np
import pytest
import torch

import shift_ladder as SL
from cases import rel_err
from oracle import oracle as O
from pooled16_cases import assert_bits, assert_gw_entries, round16
from test_exact16_gpu import abi   # noqa: F401  (the fixture: path policy 0 and default knobs before and after)
from test_routing_gpu import FAMILY_ROUTES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
X_ZERO_POINT = 3
EXCEPTION_ELEMENTS = 1 << 19

# what the runs of this process saw: table -> {"calls": n, "names": {kernel names}, "other": {(pinned, padding, name that ran)}}
LOG = {t: {"calls": 0, "names": set(), "other": set()} for t in "ABC"}
DONE = set()
_POOL = concurrent.futures.ThreadPoolExecutor(max_workers=8)   # the oracle's calls run side by side (ctypes drops the GIL)


def entry_id(e):
    return "%s-%s" % (e[0], e[1])


def uses_exception(entry):
    """the coverage exception: more than 2^19 elements and at most two channels -> the reduced ladder at the non-pinned paddings"""
    shape = entry[3]
    return int(np.prod(shape)) > EXCEPTION_ELEMENTS and shape[1] <= 2


def entry_tables(entry, pad):
    """-> the weight tables of a FAMILY_ROUTES row under `pad`: float [C, nd] arrays, or (zero point, entries) for quantized rows"""
    kind, _, dt, shape, cut, epad, active, _ = entry
    sizes, C = list(shape[2:]), shape[1]
    if kind == "forward_quantized":
        return [(zp, t) for zp in SL.ZERO_POINTS["uint8"] for t in SL.int_tables(sizes, C, pad, "uint8", zp, cut)]
    return SL.tables(sizes, C, pad, dt, bool(active), reduced=uses_exception(entry) and pad != epad, cut=cut)


def _seed(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def quantized_data(rs, shape, tdt, zero_point):
    """random integers without the zero point's value (tests/test_qtemporal_gpu.py::_data)"""
    if tdt == torch.int32:
        x = rs.randint(-1000, 1000, size=shape)
    else:
        info = torch.iinfo(tdt)
        x = rs.randint(info.min, info.max + 1, size=shape)
    x[x == zero_point] = zero_point + 1
    return x.astype({torch.int8: np.int8, torch.uint8: np.uint8, torch.int32: np.int32}[tdt])


def check_grad_w(gw, gw64, g, x, w, tdt, what):
    """gw: widened values (fp64 as it is) of the kernel's grad_w; gw64: the fp64 oracle's on the widened inputs"""
    gw = np.asarray(gw)
    assert not np.isnan(gw).any(), what + ("grad_w entries left unwritten",)
    exact = SL.exact_gw_channels(g, x, w)
    want = gw64 if tdt == torch.float64 else round16(gw64.astype(np.float32), tdt)
    assert_bits(gw[exact], want[exact], what + ("grad_w, exact channels",))
    zero = np.all(gw64 == 0, axis=tuple(range(1, gw64.ndim)))
    assert not gw[zero].any(), what + ("grad_w of channels whose reference is zero", gw[zero].tolist())
    if tdt in (torch.float32, torch.float64):
        err = rel_err(gw, gw64)
        assert err < (1e-5 if tdt == torch.float32 else 1e-12), what + ("grad_w", err)
    else:
        assert_gw_entries(gw, gw64, tdt, what + ("grad_w",))


def host(t, tdt):
    """widened values of a device tensor: fp32 for the 16-bit types, fp32 and fp64 as they are"""
    return t.float().cpu().numpy() if tdt in (torch.float16, torch.bfloat16) else t.cpu().numpy()


def _np_dtype(tdt):
    return np.float64 if tdt == torch.float64 else np.float32


def _lowered_shape(A, entry):
    """the two rows of the coverage exception run with the smallest N at which the pinned kernel is still the one that runs"""
    kind, kernel, dt, shape, cut, epad, active, cl = entry
    if not uses_exception(entry):
        return tuple(shape)
    tdt = getattr(torch, dt)
    n = 1
    while n < shape[0]:
        s = (n,) + tuple(shape[1:])
        A.forward(torch.zeros(s, dtype=tdt, device=DEV), torch.zeros(shape[1], len(shape) - 2, dtype=tdt, device=DEV), epad, active)
        if A.last_kernel() == kernel:
            return s
        n *= 2
    return tuple(shape)


def entry_data(entry, shape=None):
    """-> x, gradient (None for a quantized row) of a FAMILY_ROUTES row as numpy arrays, for `shape` (the row's, or with N lowered)"""
    kind, kernel, dt, eshape, cut, _, _, _ = entry
    shape = tuple(eshape if shape is None else shape)
    tdt = getattr(torch, dt)
    rs = np.random.RandomState(_seed(kernel + kind))
    if kind == "forward_quantized":
        return quantized_data(rs, shape, tdt, X_ZERO_POINT), None
    _, new = O.check_borders(list(shape), cut, len(shape) - 2) if cut else (None, list(shape))
    ndt = _np_dtype(tdt)
    return SL.dyadic(rs, shape).astype(ndt), SL.dyadic(rs, tuple(new)).astype(ndt)


def run_entry(A, entry, check=True, first_only=False):
    """one row of table A under every padding and every table of its ladder"""
    kind, kernel, dt, shape, cut, epad, active, cl = entry
    tdt = getattr(torch, dt)
    shape = _lowered_shape(A, entry) if kind == "forward" else tuple(shape)
    nd = len(shape) - 2
    b, new = A.check_borders(list(shape), cut, nd) if cut else (None, list(shape))
    ob = None if b is None else list(b)
    log = LOG["A"]
    to_dev = (lambda t: A.to_channels_last(t)) if cl else (lambda t: t)

    x, g = entry_data(entry, shape)
    if kind == "forward_quantized":
        xd = to_dev(torch.from_numpy(x).to(DEV))
    else:
        ndt = _np_dtype(tdt)
        xd, gd = to_dev(torch.from_numpy(x).to(tdt).to(DEV)), to_dev(torch.from_numpy(g).to(tdt).to(DEV))
        x64, g64 = x.astype(np.float64), g.astype(np.float64)

    def reference(pad, table):
        if kind == "forward_quantized":
            zp, entries = table
            return O.forward_q(x, entries, zp, X_ZERO_POINT, pad, ob)
        w = table.astype(ndt)
        if kind == "forward":
            return round16(O.forward(x, w, pad, active, ob), tdt) if tdt != torch.float64 else O.forward(x, w, pad, active, ob)
        gx, gw = O.backward(g, w, x, pad, active, ob)
        if tdt != torch.float64:
            gx, gw = round16(gx, tdt), O.backward(g64, table, x64, pad, active, ob)[1]
        return gx, gw

    for pad in range(5):
        tabs = entry_tables(entry, pad)   # (the row's own shape decides the coverage exception, whatever N the run uses)
        if first_only:
            tabs = tabs[:1]
        refs = _POOL.map(lambda t: reference(pad, t), tabs) if check else [None] * len(tabs)
        for k, (table, ref) in enumerate(zip(tabs, refs)):
            what = (entry_id(entry), "padding %d" % pad, "table %d" % k, np.asarray(table[1] if kind == "forward_quantized" else table).tolist())
            if kind == "forward_quantized":
                zp, entries = table
                out = torch.empty(new, dtype=tdt, device=DEV)
                out.view(-1).view(torch.uint8).fill_(0xA5)
                out = to_dev(out)
                A.forward_quantized(xd, torch.from_numpy(entries.astype(np.uint8)).to(DEV), zp, X_ZERO_POINT, pad, b, out=out)
                got = [out.cpu().numpy()]
                ref = [ref]
            elif kind == "forward":
                out = A.forward(xd, torch.from_numpy(table).to(tdt).to(DEV), pad, active, b, out=torch.full_like(gd, float("nan")))
                got = [host(out, tdt)]
                ref = [ref]
            else:
                wd = torch.from_numpy(table).to(tdt).to(DEV)
                gx, gw = A.backward(gd, wd, xd, pad, active, b, grad_x=torch.full_like(xd, float("nan")),
                                    grad_w=torch.full_like(wd, float("nan")))
                got = [host(gx, tdt), host(gw, tdt)]
            name = A.last_kernel()
            log["calls"] += 1
            log["names"].add(name)
            if pad == epad:
                assert name == kernel, what + (name,)
            elif name != kernel:
                log["other"].add((kernel, pad, name))
            if not check:
                continue
            assert_bits(got[0], ref[0], what + (name, "out" if kind != "backward" else "grad_x"))
            if kind == "backward":
                check_grad_w(got[1], ref[1], g, x, table, tdt, what + (name,))
    DONE.add(("A", entry_id(entry)))


@pytest.mark.parametrize("entry", FAMILY_ROUTES, ids=entry_id)
def test_table_a(abi, entry):   # noqa: F811
    run_entry(abi, entry)
    print("other paddings:", sorted(o for o in LOG["A"]["other"] if o[0] == entry[1]))


# -- table B: the temporal family (length = T) ------------------------------------------------------------------------------------------
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
DTNAME = {F16: "float16", BF16: "bfloat16", F32: "float32", F64: "float64"}
_TSHIFT = [((2, 3, 5, 8), F16, 0), ((2, 3, 5, 49), F32, 0), ((1, 9, 3, 16), F32, 0), ((2, 3, 5, 2), F64, 0)]     # (N, T, C, M)
# (N, T, M, C): the two smallest whole and ragged cases of tests/test_tshift_cl_gpu.py, and the smallest 16-bit one of each
_FRAMES = [((2, 3, 5, 2), F64, 0), ((2, 3, 5, 4), F32, 0), ((2, 3, 5, 8), F16, 0), ((2, 3, 4, 3), F64, 0), ((2, 3, 5, 3), F32, 0),
           ((2, 3, 5, 5), F16, 0)]
TEMPORAL = [("tshift", c) for c in _TSHIFT] + [("per_clip", c) for c in _TSHIFT] + [("frames", c) for c in _FRAMES]
# (N, T, C, M), dtype, offset, kernel: the smallest case of each form of tests/test_temporal_gpu.py, and a 16-bit one of each
SEGMENT = [((2, 3, 5, 2), F64, 0, "segment_forward"), ((2, 3, 5, 8), F16, 0, "segment_forward"),
           ((2, 3, 4, 3), F64, 0, "segment_forward_ragged"), ((2, 3, 5, 49), F16, 0, "segment_forward_ragged")]
QSEGMENT = [((2, 3, 5, 16), torch.uint8, "segment_forward"), ((2, 3, 5, 49), torch.int8, "segment_forward_ragged"),
            ((2, 3, 5, 4), torch.int32, "segment_forward"), ((2, 3, 5, 3), torch.int32, "segment_forward_ragged")]
TABLE_B_NAMES = {"tshift_forward", "tshift_backward", "tshift_forward_ragged", "tshift_backward_ragged", "frames_forward",
                 "frames_forward_ragged", "frames_active_forward", "frames_active_forward_ragged", "frames_backward",
                 "frames_backward_ragged", "segment_forward", "segment_forward_ragged"}


def temporal_id(row):
    family, (shape, dt, off) = row
    return "%s-%s-%s" % (family, "x".join(map(str, shape)), DTNAME[dt])


def temporal_geometry(row):
    """-> T, the number of channels, the rows of a weight table"""
    family, (shape, _, _) = row
    C = shape[3] if family == "frames" else shape[2]
    return shape[1], C, (shape[0] * C if family == "per_clip" else C)


def run_temporal(row, check=True, first_only=False):
    import test_per_clip_gpu as PCLIP
    import test_tshift_cl_gpu as TCL
    import test_tshift_gpu as TS
    family, (shape, dt, off) = row
    mod = TCL if family == "frames" else TS
    N = shape[0]
    T, C, slots = temporal_geometry(row)
    rs = np.random.RandomState(_seed(temporal_id(row)))
    x, go = SL.dyadic(rs, shape).astype(np.float64), SL.dyadic(rs, shape).astype(np.float64)
    log = LOG["B"]
    for pad in range(5):
        for active in (0, 1):
            tabs = SL.tables([T], slots, pad, DTNAME[dt], bool(active))
            for k, table in enumerate(tabs[:1] if first_only else tabs):
                what = (temporal_id(row), "padding %d" % pad, "active %d" % active, "table %d" % k, table[:, 0].tolist())
                w = table[:, 0]
                if family == "per_clip":
                    w = w.reshape(N, C)
                    out, gx, gw, kf, kb = PCLIP._run_per_clip(shape, dt, off, x, go, w, pad, active)
                elif family == "tshift":
                    out, gx, gw, kf, kb = TS._run(shape, dt, off, x, go, w, pad, active)
                else:
                    out, gx, gw = TCL._run(shape, dt, off, x, go, w, pad, active)     # (asserts the names itself)
                    kf, kb = TCL._names(shape, dt, off, active)
                if family != "frames":
                    assert (kf, kb) == ((TS.FWD, TS.BWD) if TS._whole(shape, dt, off) else (TS.FWD_R, TS.BWD_R)), what + (kf, kb)
                log["calls"] += 2
                log["names"] |= {kf, kb}
                if not check:
                    continue
                clips = [slice(n, n + 1) for n in range(N)] if family == "per_clip" else [slice(0, N)]
                for n, clip in enumerate(clips):
                    wn = w[n] if family == "per_clip" else w
                    want_out, want_gx, gw64 = mod._reference(x[clip], go[clip], wn, pad, active, dt)
                    assert_bits(mod._wide(out)[clip], want_out, what + (kf, "out", n))
                    assert_bits(mod._wide(gx)[clip], want_gx, what + (kb, "grad_x", n))
                    got_gw = mod._wide(gw)[n] if family == "per_clip" else mod._wide(gw)
                    check_grad_w(got_gw.reshape(C, 1), gw64.reshape(C, 1), mod._lines(go[clip]), mod._lines(x[clip]), wn.reshape(C, 1), dt,
                                 what + (kb, n))
    DONE.add(("B", temporal_id(row)))


@pytest.mark.parametrize("row", TEMPORAL, ids=temporal_id)
def test_table_b_learnable(abi, row):   # noqa: F811
    """tshift_* (per channel and per clip) and frames_*: forward and backward, both shift kinds"""
    run_temporal(row)


def segment_id(case):
    return "%s-%s" % ("x".join(map(str, case[0])), str(case[1]).split(".")[-1])


def run_segment(A, case, check=True, first_only=False):
    """the segment-major sparse forward and its input gradient under a [C, 2] table whose first column holds the ladder"""
    import test_temporal_gpu as TG
    shape, dt, off, kernel = case
    N, T, C, M = shape
    ndt = _np_dtype(dt)
    rs = np.random.RandomState(_seed(segment_id(case)))
    x, go = SL.dyadic(rs, shape).astype(ndt), SL.dyadic(rs, shape).astype(ndt)
    xd, gd = TG._buffer(shape, dt, off), TG._buffer(shape, dt, off)
    xd.copy_(torch.from_numpy(x).to(dt))
    gd.copy_(torch.from_numpy(go).to(dt))
    xc, gc = np.ascontiguousarray(x.transpose(0, 2, 1, 3)), np.ascontiguousarray(go.transpose(0, 2, 1, 3))
    log = LOG["B"]
    for pad in range(5):
        tabs = SL.tables([T], C, pad, DTNAME[dt], False)
        for k, table in enumerate(tabs[:1] if first_only else tabs):
            what = (segment_id(case), "padding %d" % pad, "table %d" % k, table[:, 0].tolist())
            w = np.zeros((C, 2), ndt)
            w[:, 0] = table[:, 0]
            wd = torch.from_numpy(w).to(dt).to(DEV)
            out, gx = TG._buffer(shape, dt, off, fill=0xA5), TG._buffer(shape, dt, off, fill=0xA5)
            A.forward(TG._view(xd), wd, pad, 0, out=TG._view(out))
            names = [A.last_kernel()]
            A.backward_input(TG._view(gd), wd, (N, C, T, M), pad, grad_x=TG._view(gx))
            names.append(A.last_kernel())
            log["calls"] += 2
            log["names"] |= set(names)
            assert names == [kernel, kernel], what + tuple(names)
            if check:
                assert_bits(TG._np(TG._view(out)), O.forward(xc, w, pad, False), what + ("out",))
                assert_bits(TG._np(TG._view(gx)), O.backward(gc, w, xc, pad, False)[0], what + ("grad_x",))
    DONE.add(("B", segment_id(case)))


@pytest.mark.parametrize("case", SEGMENT, ids=segment_id)
def test_table_b_segment(abi, case):   # noqa: F811
    run_segment(abi, case)


def qsegment_plans(T, C, pad):
    """-> [(table dtype, zero point, [entries [C, 1] ...])]: uint8, int8 and int32 tables, and the two int32 tables whose zero point
    is +-(2^31 - 1)"""
    plans = [(name, zp, SL.int_tables([T], C, pad, name, zp)) for name in ("uint8", "int8", "int32") for zp in SL.ZERO_POINTS[name]]
    plans += [("int32", sign * SL.EXTREME_ZERO_POINT, SL.int32_extreme_tables([T], C, pad, sign)) for sign in (1, -1)]
    return plans


def run_qsegment(A, case, check=True, first_only=False):
    import test_qtemporal_gpu as QT
    shape, dt, kernel = case
    N, T, C, M = shape
    rs = np.random.RandomState(_seed(segment_id(case)))
    x_np = QT._data(rs, shape, dt)
    xv = x_np.transpose(0, 2, 1, 3)
    x = QT._buffer(shape, dt, 0)
    x.copy_(torch.from_numpy(x_np))
    log = LOG["B"]
    for pad in range(5):
        for name, zp, tabs in qsegment_plans(T, C, pad):
            for k, entries in enumerate(tabs[:1] if first_only else tabs):
                what = (segment_id(case), "padding %d" % pad, name, "zero point %d" % zp, "table %d" % k, entries[:, 0].tolist())
                w = np.zeros((C, 2), np.int64) + zp
                w[:, 0] = entries[:, 0]
                wq = w.astype(getattr(np, name))
                assert np.array_equal(wq.astype(np.int64), w), what
                out = QT._buffer(shape, dt, 0, fill=0xA5)
                # (the zero points at either end of int32 are served like every other: entry - zero_point in 64 bits)
                A.forward_quantized(QT._view(x), torch.from_numpy(wq).to(DEV), zp, QT.ZP[dt], pad, out=QT._view(out))
                log["calls"] += 1
                log["names"].add(A.last_kernel())
                assert A.last_kernel() == kernel, what + (A.last_kernel(),)
                if check:
                    got, want = QT._view(out).cpu().numpy(), O.forward_q(xv, w, zp, QT.ZP[dt], pad)
                    assert np.array_equal(got, want), what + ("%d differ" % int((got != want).sum()),)
    DONE.add(("B", "q" + segment_id(case)))


@pytest.mark.parametrize("case", QSEGMENT, ids=segment_id)
def test_table_b_quantized_segment(abi, case):   # noqa: F811
    run_qsegment(abi, case)


# (N, T, C, spatial), dtype, offset, kernel, channels-last: tests/test_temporal_inplace_gpu.py's cases -- 16-byte, 2-byte and 1-byte
# pieces, all 16 frame slots, a channels-last table that mixes pieces, both layouts quantized
INPLACE = [((2, 4, 8, (4, 4)), F32, 0, "frames_inplace", False), ((2, 3, 5, (7, 7)), F16, 0, "frames_inplace_ragged", False),
           ((1, 16, 4, (2, 2)), F32, 0, "frames_inplace", False), ((2, 4, 5, (7, 7)), torch.uint8, 0, "frames_inplace_ragged", False),
           ((2, 4, 16, (3, 3)), F16, 0, "frames_inplace", True), ((2, 4, 3, (3, 3)), torch.uint8, 0, "frames_inplace_ragged", True)]
TABLE_B_NAMES |= {"frames_inplace", "frames_inplace_ragged"}


def inplace_id(case):
    (N, T, C, sp), dt, _, _, cl = case
    return "N%d-T%d-C%d-%s-%s-%s" % (N, T, C, "x".join(map(str, sp)), str(dt).split(".")[-1], "channels_last" if cl else "contiguous")


def inplace_tables(case, pad):
    """-> the [C] tables (torch) of an in-place case: the sparse ladder as the float table the call hands over (fp32 for 16-bit
    tensors), the int32 ladder for quantized tensors"""
    (_, T, C, _), dt = case[:2]
    if not dt.is_floating_point:
        return [torch.from_numpy(t[:, 0].copy()) for t in SL.int_tables([T], C, pad, "int32", 0)]
    return [torch.from_numpy(t[:, 0].copy()) for t in SL.tables([T], C, pad, "float64" if dt == F64 else "float32", False)]


def run_inplace(A, case, first_only=False):
    """against inplace_cases.reference computed from a clone (test_temporal_inplace_gpu._check: kernel name, bits, painted guards)"""
    import test_temporal_inplace_gpu as TI
    geom, dt, off, kernel, cl = case
    rs = np.random.RandomState(_seed(inplace_id(case)))
    for pad in range(5):
        tabs = inplace_tables(case, pad)
        for table in (tabs[:1] if first_only else tabs):
            TI._check(geom, dt, off, kernel, cl, table, pad, rs)
            LOG["B"]["calls"] += 1
            LOG["B"]["names"].add(A.last_kernel())
    DONE.add(("B", inplace_id(case)))


@pytest.mark.parametrize("case", INPLACE, ids=inplace_id)
def test_table_b_inplace(abi, case):   # noqa: F811
    run_inplace(abi, case)


# -- table C: the input gradient without the input ---------------------------------------------------------------------------------------
# shape, cut, dtype, the unpooled kernel, the pooled kernel (2 x 2 windows): rows of whole 16-byte pieces and ragged rows (tests/test_fixed_gpu.py)
INPUT_FREE = [((2, 5, 24, 32), [[1, 1], [1, 1]], dt, "gradx_embed", "gradx_embed_pool") for dt in (F32, BF16)] + \
             [((4, 8, 14, 14), [[1, 1], [1, 1]], dt, "gradx_gather", "gradx_gather_pool") for dt in (F32, BF16)]
TABLE_C_NAMES = {"gradx_embed", "gradx_gather", "gradx_embed_pool", "gradx_gather_pool", "step_gather_forward_pool", "plane_pool_forward",
                 "walk_forward_pool", "crop_forward3_pool", "row_forward_pool", "step_backward_pool", "crop_backward_pool",
                 "walk_backward_pool", "walk_backward_crop_pool", "crop_backward3_pool", "row_backward_pool"}   # (pooled16_cases.SERVED_16BIT)


def input_free_id(case):
    return "%s-%s" % ("x".join(map(str, case[0])), DTNAME[case[2]])


def run_input_free(A, case, check=True, first_only=False):
    shape, cut, dt, kernel, pooled_kernel = case
    nd, C = len(shape) - 2, shape[1]
    b, new = A.check_borders(list(shape), cut, nd)
    pool = [2] * nd
    pshape = list(new[:2]) + [-(-o // 2) for o in new[2:]]
    rs = np.random.RandomState(_seed(input_free_id(case)))
    g, gp = SL.dyadic(rs, tuple(new)), SL.dyadic(rs, tuple(pshape))
    gd, gpd = torch.from_numpy(g).to(dt).to(DEV), torch.from_numpy(gp).to(dt).to(DEV)
    x0 = np.zeros(shape, np.float32)
    expanded = round16(O.avg_pool_backward(gp, pool, new[2:]), dt)      # (dyadic over windows of 2^n elements: exact)
    log = LOG["C"]
    for pad in range(5):
        tabs = SL.tables(list(shape[2:]), C, pad, DTNAME[dt], False, cut=cut)
        for k, table in enumerate(tabs[:1] if first_only else tabs):
            what = (input_free_id(case), "padding %d" % pad, "table %d" % k, table.tolist())
            w = table.astype(np.float32)
            wd = torch.from_numpy(w).to(dt).to(DEV)
            gx = A.backward_input(gd, wd, shape, pad, b, grad_x=torch.full(shape, float("nan"), dtype=dt, device=DEV))
            names = [A.last_kernel()]
            gxp = A.backward_pooled_input(gpd, wd, shape, pad, pool, b, grad_x=torch.full(shape, float("nan"), dtype=dt, device=DEV))
            names.append(A.last_kernel())
            log["calls"] += 2
            log["names"] |= set(names)
            assert names == [kernel, pooled_kernel], what + tuple(names)
            if check:
                assert_bits(host(gx, dt), round16(O.backward(g, w, x0, pad, False, b)[0], dt), what + (kernel, "grad_x"))
                assert_bits(host(gxp, dt), round16(O.backward(expanded, w, x0, pad, False, b)[0], dt), what + (pooled_kernel, "grad_x"))
    DONE.add(("C", input_free_id(case)))


@pytest.mark.parametrize("case", INPUT_FREE, ids=input_free_id)
def test_table_c_input_free(abi, case):   # noqa: F811
    run_input_free(abi, case)


# -- table C: the fused shift + average pool on 16-bit tensors (tests/pooled16_cases.py's cases, routes and rules) ---------------------------
import pooled16_cases as PC   # noqa: E402


def pooled_id(row):
    ci, dt = row
    return "case%d-%s" % (ci, dt)


POOLED = [(ci, dt) for ci in range(len(PC.CASES)) for dt in ("f16", "bf16")]


def run_pooled(A, row, check=True, first_only=False):
    """shiftnd_forward_pooled / shiftnd_backward_pooled on the default route: the kernel PC.forward_route / PC.backward_route name,
    compared by PC.check_forward / PC.check_backward on exact data (bit for bit where every window count is a power of two)"""
    ci, dt = row
    case = PC.CASES[ci]
    nd, shape, pool, cut, _ = case
    tdt = PC.DTYPES[dt]
    b, _, pooled = PC.geometry(case)
    rs = np.random.RandomState(_seed(pooled_id(row)))
    x, gp = SL.dyadic(rs, shape), SL.dyadic(rs, tuple(shape[:2]) + tuple(pooled))
    xd, gpd = torch.from_numpy(x).to(tdt).to(DEV), torch.from_numpy(gp).to(tdt).to(DEV)
    log = LOG["C"]
    for pad in range(5):
        for active in (0, 1):
            tabs = SL.tables(list(shape[2:]), shape[1], pad, DTNAME[tdt], bool(active), cut=cut)
            fwd, bwd = PC.forward_route(case, 2, active, pad), PC.backward_route(case, 2, active, pad)
            for k, table in enumerate(tabs[:1] if first_only else tabs):
                what = (shape, pool, cut, dt, "padding %d" % pad, "active %d" % active, "table %d" % k, table.tolist())
                w = table.astype(np.float32)
                wd = torch.from_numpy(w).to(tdt).to(DEV)
                r = None
                if check:
                    y, ref, g, gx_ref, gw64 = PC.two_step_reference(x, w, gp, pad, active, pool, b, tdt)
                    r = dict(y=y, ref=ref, g=g, gx_ref=gx_ref, gw64=gw64)
                out = A.forward_pooled(xd, wd, pad, active, pool, b, out=torch.full(list(shape[:2]) + pooled, float("nan"), dtype=tdt, device=DEV))
                assert A.last_kernel() == fwd, what + (A.last_kernel(), fwd)
                log["calls"] += 1
                log["names"].add(fwd)
                if check:
                    PC.check_forward(host(out, tdt), r, case, active, "exact", tdt, what + (fwd,))
                if bwd == PC.NOT_SERVED:
                    with pytest.raises(RuntimeError, match="not served"):
                        A.backward_pooled(gpd, wd, xd, pad, active, pool, b)
                    continue
                gx, gw = A.backward_pooled(gpd, wd, xd, pad, active, pool, b, grad_x=torch.full_like(xd, float("nan")),
                                           grad_w=torch.full_like(wd, float("nan")))
                name = A.last_kernel()
                assert name in (bwd if isinstance(bwd, tuple) else (bwd,)), what + (name, bwd)
                log["calls"] += 1
                log["names"].add(name)
                if check:
                    PC.check_backward(host(gx, tdt), host(gw, tdt), r, case, active, "exact", tdt, what + (name,))
    DONE.add(("C", pooled_id(row)))


@pytest.mark.parametrize("row", POOLED, ids=pooled_id)
def test_table_c_pooled16(abi, row):   # noqa: F811
    run_pooled(abi, row)


# -- table C: the quantized shift + average pool (csrc/shiftnd_qpool.hip) ---------------------------------------------------------------------
# The smallest case of test_pooled_gpu.CASES + QCASES that reaches each kernel of test_redzone_gpu.QPOOL_NAMES with the knobs untouched:
# nd, shape, pool, cut, the kernel under zeros padding, the kernel under paddings 1-4.  qpool_band_fast serves zeros padding only
# (qband_plan: `fast`), so its two cases fall to the plane and the band kernel elsewhere; its pads hold column shifts in [-8, 8]
# (rungs 8 and 9).  uint8 weight tables under zero point 128 (test_pooled_gpu.quantized_pool_references' own): shifts -128 .. 127.
QPOOL = [(2, (1, 3, 9, 8), (4, 4), None, "qpool_forward", "qpool_forward"),
         (2, (2, 3, 9, 4), (2, 2), [[1, 1], [1, 1]], "qpool_plane_forward", "qpool_plane_forward"),
         (2, (2, 3, 24, 56), (1, 2), None, "qpool_band_fast", "qpool_plane_forward"),
         (2, (2, 2, 300, 36), (1, 2), None, "qpool_band_fast", "qpool_band_forward")]
QPOOL_W_ZERO_POINT = 128
QPOOL_ROWS = [(k, pad) for k in range(len(QPOOL)) for pad in range(5)]
TABLE_C_NAMES |= {"qpool_forward", "qpool_plane_forward", "qpool_band_forward", "qpool_band_fast"}


def qpool_id(row):
    k, pad = row
    return "%s-%s-padding%d" % ("x".join(map(str, QPOOL[k][1])), QPOOL[k][4 if pad == 0 else 5], pad)


def qpool_tables(k, pad):
    nd, shape, pool, cut = QPOOL[k][:4]
    return SL.int_tables(list(shape[2:]), shape[1], pad, "uint8", QPOOL_W_ZERO_POINT, cut)


def run_qpool(A, row, check=True, first_only=False):
    """shiftnd_forward_quantized_pooled, both requant forms, against test_pooled_gpu.quantized_pool_references; uint8 tensors, and
    int8 too where the case is small"""
    import test_pooled_gpu as TP
    k, pad = row
    nd, shape, pool, cut, zeros_kernel, other_kernel = QPOOL[k]
    kernel = zeros_kernel if pad == 0 else other_kernel
    b, new = A.check_borders(list(shape), cut, nd)
    pshape = list(new[:2]) + [-(-new[2 + r] // pool[r]) for r in range(nd)]
    tabs = qpool_tables(k, pad)
    log = LOG["C"]
    for tdt, zp in ((torch.uint8, 7), (torch.int8, -9))[:2 if int(np.prod(shape)) < 10000 else 1]:
        rs = np.random.RandomState(_seed(qpool_id(row) + str(tdt)))
        xq = quantized_data(rs, shape, tdt, zp)
        xd = torch.from_numpy(xq).to(DEV)
        for t, entries in enumerate(tabs[:1] if first_only else tabs):
            what = (qpool_id(row), str(tdt), "table %d" % t, (entries - QPOOL_W_ZERO_POINT).tolist())
            wq = entries.astype(np.uint8)
            refs = TP.quantized_pool_references(xq, wq, zp, pad, pool, b, new) if check else (None, None)
            for requant, ref in zip((A.REQUANT_ZP_INSIDE, A.REQUANT_ZP_OUTSIDE), refs):
                out = torch.empty(pshape, dtype=tdt, device=DEV)
                out.view(-1).view(torch.uint8).fill_(0xA5)
                A.forward_quantized_pooled(xd, torch.from_numpy(wq).to(DEV), QPOOL_W_ZERO_POINT, zp, pad, pool, b, out=out, requant=requant)
                log["calls"] += 1
                log["names"].add(A.last_kernel())
                assert A.last_kernel() == kernel, what + (A.last_kernel(),)
                if check:
                    got = out.cpu().numpy()
                    assert np.array_equal(got, ref), what + (kernel, "requant %d" % requant, "%d differ" % int((got != ref).sum()))
    DONE.add(("C", qpool_id(row)))


@pytest.mark.parametrize("row", QPOOL_ROWS, ids=qpool_id)
def test_table_c_quantized_pool(abi, row):   # noqa: F811
    run_qpool(abi, row)


# -- every problem of the tables, for the self-checks that need no GPU (tests/test_shift_ladder_cases.py) ----------------------------------
class Family:
    """one problem of tables A-C as the oracle sees it: shape [N, C, S...], cut, the weights' dtype name, shift kind, and per padding
    the tables of SHIFTS ([C, nd] float64; quantized: entry - zero point) with the rungs each table's dtype can hold"""

    def __init__(self, table, name, shape, cut, wdtype, active, quantized, shifts, ladders, data=None, exception=False):
        self.table, self.name, self.shape, self.cut, self.wdtype = table, name, tuple(shape), cut, wdtype
        self.active, self.quantized, self.shifts, self.ladders, self.data, self.exception = active, quantized, shifts, ladders, data, exception

    @property
    def id(self):
        return "%s-%s-%s" % (self.table, self.name, "active" if self.active else "sparse")


def families():
    out = []
    for e in FAMILY_ROUTES:
        kind, kernel, dt, shape, cut, epad, active, _ = e
        sizes = list(shape[2:])
        if kind == "forward_quantized":
            shifts = (lambda pad, e=e: [t - zp for zp, t in entry_tables(e, pad)])
            ladders = (lambda pad, sizes=sizes: [sorted({r for zp in SL.ZERO_POINTS["uint8"] for r in SL.int_rungs(n, pad, "uint8", zp)})
                                                 for n in sizes])
            out.append(Family("A", entry_id(e), shape, cut, "uint8", False, True, shifts, ladders, lambda e=e: entry_data(e)[0]))
        else:
            shifts = (lambda pad, e=e: entry_tables(e, pad))
            ladders = (lambda pad, e=e, sizes=sizes: [SL.rungs(n, pad, e[2], bool(e[6]), len(sizes), uses_exception(e) and pad != e[5])
                                                      for n in sizes])
            out.append(Family("A", entry_id(e), shape, cut, dt, bool(active), False, shifts, ladders, lambda e=e: entry_data(e)[0],
                              exception=uses_exception(e)))
    for row in TEMPORAL:
        family, (shape, dt, _) = row
        T, C, slots = temporal_geometry(row)
        lines = int(np.prod(shape)) // (T * slots)
        for active in (False, True):
            out.append(Family("B", temporal_id(row), (lines, slots, T), None, DTNAME[dt], active, False,
                              lambda pad, T=T, slots=slots, dt=dt, active=active: SL.tables([T], slots, pad, DTNAME[dt], active),
                              lambda pad, T=T, dt=dt, active=active: [SL.rungs(T, pad, DTNAME[dt], active, 1)]))
    for shape, dt, _, kernel in SEGMENT:
        N, T, C, M = shape
        out.append(Family("B", kernel + "-" + segment_id((shape, dt)), (N * M, C, T), None, DTNAME[dt], False, False,
                          lambda pad, T=T, C=C, dt=dt: SL.tables([T], C, pad, DTNAME[dt], False),
                          lambda pad, T=T, dt=dt: [SL.rungs(T, pad, DTNAME[dt], False, 1)]))
    for shape, dt, kernel in QSEGMENT:
        N, T, C, M = shape
        for plan in range(7):
            name = qsegment_plans(T, C, 0)[plan][0]
            out.append(Family("B", "quantized-%s-%s-plan%d" % (kernel, segment_id((shape, dt)), plan), (N * M, C, T), None, name, False, True,
                              lambda pad, T=T, C=C, plan=plan: [t - qsegment_plans(T, C, pad)[plan][1] for t in qsegment_plans(T, C, pad)[plan][2]],
                              None))
    for case in INPLACE:
        (N, T, C, sp), dt = case[:2]
        quantized = not dt.is_floating_point
        out.append(Family("B", case[3] + "-" + inplace_id(case), (N * int(np.prod(sp)), C, T), None,
                          "int32" if quantized else ("float64" if dt == F64 else "float32"), False, quantized,
                          lambda pad, case=case: [t.double().numpy().reshape(-1, 1) for t in inplace_tables(case, pad)],
                          (lambda pad, T=T: [SL.int_rungs(T, pad, "int32", 0)]) if quantized else
                          (lambda pad, T=T, dt=dt: [SL.rungs(T, pad, "float64" if dt == F64 else "float32", False, 1)])))
    for case in INPUT_FREE:
        shape, cut, dt = case[:3]
        out.append(Family("C", case[3] + "-" + input_free_id(case), shape, cut, DTNAME[dt], False, False,
                          lambda pad, shape=shape, dt=dt, cut=cut: SL.tables(list(shape[2:]), shape[1], pad, DTNAME[dt], False, cut=cut),
                          lambda pad, shape=shape, dt=dt: [SL.rungs(n, pad, DTNAME[dt], False, len(shape) - 2) for n in shape[2:]]))
    for k, (nd, shape, pool, cut, zeros_kernel, other_kernel) in enumerate(QPOOL):
        out.append(Family("C", "quantized-pool-%s-%s" % ("x".join(map(str, shape)), zeros_kernel), shape, cut, "uint8", False, True,
                          lambda pad, k=k: [t - QPOOL_W_ZERO_POINT for t in qpool_tables(k, pad)],
                          lambda pad, shape=shape: [SL.int_rungs(n, pad, "uint8", QPOOL_W_ZERO_POINT) for n in shape[2:]]))
    for ci, dt in POOLED:
        nd, shape, pool, cut, _ = PC.CASES[ci]
        name = DTNAME[PC.DTYPES[dt]]
        for active in (False, True):
            out.append(Family("C", "pooled-" + pooled_id((ci, dt)), shape, cut, name, active, False,
                              lambda pad, shape=shape, name=name, active=active, cut=cut: SL.tables(list(shape[2:]), shape[1], pad, name, active, cut=cut),
                              lambda pad, shape=shape, name=name, active=active: [SL.rungs(n, pad, name, active, len(shape) - 2) for n in shape[2:]]))
    return out


def test_served_set(abi):   # noqa: F811
    """the union of the kernel names reached contains every name of the tables; rows this process has not run yet run their first
    table per padding here (routes only)"""
    for entry in FAMILY_ROUTES:
        if ("A", entry_id(entry)) not in DONE:
            run_entry(abi, entry, check=False, first_only=True)
    for row in TEMPORAL:
        if ("B", temporal_id(row)) not in DONE:
            run_temporal(row, check=False, first_only=True)
    for case in SEGMENT:
        if ("B", segment_id(case)) not in DONE:
            run_segment(abi, case, check=False, first_only=True)
    for case in QSEGMENT:
        if ("B", "q" + segment_id(case)) not in DONE:
            run_qsegment(abi, case, check=False, first_only=True)
    for case in INPLACE:
        if ("B", inplace_id(case)) not in DONE:
            run_inplace(abi, case, first_only=True)
    for case in INPUT_FREE:
        if ("C", input_free_id(case)) not in DONE:
            run_input_free(abi, case, check=False, first_only=True)
    for row in QPOOL_ROWS:
        if ("C", qpool_id(row)) not in DONE:
            run_qpool(abi, row, check=False, first_only=True)
    for row in POOLED:
        if ("C", pooled_id(row)) not in DONE:
            run_pooled(abi, row, check=False, first_only=True)
    for t in sorted(LOG):
        print("table %s: %d calls, %d kernels" % (t, LOG[t]["calls"], len(LOG[t]["names"])))
        print("  names:", sorted(LOG[t]["names"]))
        print("  at other paddings:", sorted(LOG[t]["other"]))
    for t, want in (("A", {e[1] for e in FAMILY_ROUTES}), ("B", TABLE_B_NAMES), ("C", TABLE_C_NAMES)):
        assert want <= LOG[t]["names"], (t, sorted(want - LOG[t]["names"]))
