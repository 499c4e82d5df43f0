"""Every kernel family under guard: inputs (x, the gradient, the weight table) and outputs (out, grad_x, grad_w, the workspace) all lie
between painted red zones (tests/redzone.py; its own self-checks: tests/test_redzone_cases.py), under both patterns.  After every call:
every red zone intact, every input unchanged, every output equal to the expectation, the two patterns' outputs byte-identical.

  a  unpooled ........ exact16_cases.CASES and CL_CASES on the dense exact fixture, f16 / bf16 / f32 / f64, against EC.reference
  b  pooled .......... pooled16_cases.CASES, f16 / bf16 / f32, against PC.reference where it is bit-determined (the forward; the
                       backward under power-of-two window counts), else against the same call on plain fresh tensors; rows that are
                       not served raise as they do unguarded and launch nothing
  c  quantized pool .. test_pooled_gpu.CASES + QCASES, int8 / uint8, both requant forms, against that module's numpy restatement
  d  families ........ every row of test_routing_gpu.FAMILY_ROUTES, random data drawn as there, against the same call on plain tensors
  e  grad_x only ..... backward_input / backward_pooled_input on the sparse calls of a / b, against the full form's grad_x
  f  placement ....... the zeros- and reflect-padding calls of a / b / e with every buffer 16 bytes into its 512-byte line, and with
                       the weight table alone one element in (2- and 4-byte tables): the same kernel, the same bits
  transposes ......... shiftnd_transpose, element sizes 1 / 2 / 4 / 8, both directions

Every padding 0-4 and both shifts; knobs and policy at their defaults; workspaces of exactly the bytes the size functions return.
The runs are memoised per (family, table, dtype, placement): test_served_set asserts over the names they reached (and runs what the
session has not run yet)."""
import collections
import ctypes
import itertools

import numpy as np
import pytest
import torch

import exact16_cases as EC
import pooled16_cases as PC
import redzone as RZ
import test_pooled_gpu as TP
from test_routing_gpu import FAMILY_ROUTES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = dict(EC.DTYPES, f64=torch.float64)    # (EC.DTYPES itself stays as the exact16 modules use it)
KNOBS = {**EC.KNOB_DEFAULTS, 34: 0, 36: 0}
VARIANT_PADS = (0, 3)                            # zeros and reflect
PLACEMENTS = ("base", "off16", "table")
REFLECT_SWEEP = [(pad, active) for pad in VARIANT_PADS for active in (0, 1)]

DONE, SEEN, CALLS, NAMES = set(), set(), collections.Counter(), {}
SEEN_BY = collections.defaultdict(set)   # table (a - f of the module docstring) -> kernel names


def _reset(A):
    A.set_path_policy(0)
    for k, v in KNOBS.items():
        A.set_tuning(k, v)


@pytest.fixture()
def abi():
    from torchshifts import abi as A
    assert torch.cuda.is_available(), "the gpu tests need an MI355X"
    _reset(A)
    yield A
    _reset(A)


def T(a, tdt):
    return torch.from_numpy(np.array(a)).to(tdt)   # (a copy: the shared references are read-only)


def es_of(tdt):
    return torch.empty(0, dtype=tdt).element_size()


def offsets(placement, tdt):
    """-> (offset_bytes of every tensor and of the workspace, offset_bytes of the weight table)"""
    return {"base": (0, 0), "off16": (16, 16), "table": (0, es_of(tdt))}[placement]


def sweep_of(placement):
    return EC.SWEEP if placement == "base" else REFLECT_SWEEP


def guard(table, call, inputs, outputs, expect, what, raises=None):
    name = RZ.run_guarded(call, inputs, outputs, expect, what, raises=raises)
    CALLS[table] += 1
    if name is not None:
        SEEN.add(name)
        SEEN_BY[table].add(name)
    return name


def same_kernel_as_base(key, placement, name, what):
    """the placement variants must run the kernel the 512-aligned call ran (the host checks no alignment above 16 bytes)"""
    if placement == "base":
        NAMES[key] = name
    else:
        assert NAMES[key] == name, what + ("kernel at offset 0", NAMES[key], "here", name)


def workspace(abi, x, pad, active, b, off, pool=None):
    p = abi.problem(x, pad, active, b)
    if pool is None:
        n = int(abi.lib().shiftnd_backward_workspace_bytes(ctypes.byref(p)))
    else:
        n = int(abi.lib().shiftnd_backward_pooled_workspace_bytes(ctypes.byref(p), abi._pool_arg(pool, p.ndim)))
    return RZ.Guarded((n,), torch.uint8, DEV, offset_bytes=off)


def gw_expect(gw64, tdt):
    """round16(gw64); fp32: gw64 itself, which the fixture makes exact in fp32 (exact16_cases.check_backward); fp64: gw64"""
    if tdt == torch.float64:
        return T(gw64, tdt)
    if tdt == torch.float32:
        assert np.array_equal(gw64.astype(np.float32).astype(np.float64), gw64)
    return T(EC.round16(gw64.astype(np.float32), tdt), tdt)


# ---------------------------------------------------------------------------------------------------------------------
# a, e, f: unpooled
# ---------------------------------------------------------------------------------------------------------------------
def run_unpooled(abi, table, nd, dt, placement):
    if placement != "base":
        run(abi, ("unpooled", table, nd, dt, "base"))
    tdt = DTYPES[dt]
    rdt = "f32" if dt == "f64" else dt        # (the dyadic fixture is exact in fp32: the fp64 expectation is the fp32 one, widened)
    cases = (EC.CASES, EC.CL_CASES)[table]
    layout = ("contiguous", "channels_last")[table]
    off, woff = offsets(placement, tdt)
    for ci in EC.group(nd, cases):
        case = cases[ci]
        shape, cut = case[1], case[2]
        x, w, grads = EC._inputs(table, ci, "", "exact")
        b, win = EC.geometry(case)
        X, OUT, GX = (RZ.Guarded(s, tdt, DEV, layout, off) for s in (shape, win, shape))
        GXI = RZ.Guarded(shape, tdt, DEV, "contiguous", off)      # (the input-gradient-only form returns contiguous tensors)
        W, GW = (RZ.Guarded(w.shape, tdt, DEV, offset_bytes=woff) for _ in range(2))
        gforms = [(layout, RZ.Guarded(win, tdt, DEV, layout, off))]
        if table == 1:
            gforms.append(("contiguous", RZ.Guarded(win, tdt, DEV, "contiguous", off)))
        xin, win_, gin = ("x", X, T(x, tdt)), ("w", W, T(w, tdt)), T(grads[0], tdt)
        for pad, active in sweep_of(placement):
            what = ("unpooled", ("contiguous", "channels-last")[table], shape, cut, dt, placement, pad, active)
            r = EC.reference(ci, rdt, "exact", pad, active, table)
            key = (table, ci, dt, pad, active)

            def forward():
                abi.forward(X.t, W.t, pad, active, b, out=OUT.t)
                return abi.last_kernel()

            name = guard("a" if placement == "base" else "f", forward, [xin, win_], [("out", OUT)], [T(r["out"], tdt)], what + ("forward",))
            same_kernel_as_base(key + ("f",), placement, name, what)
            if es_of(tdt) == 2:
                want = EC.cl_expected(case, "f", active) if table else EC.expected(case, "f", active, pad)
                assert name == want, what + ("forward", name, want)
            WS = workspace(abi, X.t, pad, active, b, off)
            call = r["calls"][0]
            for glayout, G in gforms:

                def backward():
                    abi.backward(G.t, W.t, X.t, pad, active, b, grad_x=GX.t, grad_w=GW.t, workspace=WS.t)
                    return abi.last_kernel()

                name = guard("a" if placement == "base" else "f", backward, [("grad_out", G, gin), xin, win_],
                             [("grad_x", GX), ("grad_w", GW), ("workspace", WS)], [T(call["gx"], tdt), gw_expect(call["gw64"], tdt), None],
                             what + ("backward", glayout))
                same_kernel_as_base(key + ("b", glayout), placement, name, what)
                if es_of(tdt) == 2:
                    want = EC.cl_expected(case, "b", active, glayout == layout) if table else EC.expected(case, "b", active, pad)
                    assert name == want, what + ("backward", glayout, name, want)
                if active:
                    continue

                # e: the input gradient alone -- no x, no grad_w -- is the full form's grad_x
                def backward_input():
                    abi.backward_input(G.t, W.t, shape, pad, b, grad_x=GXI.t, workspace=WS.t)
                    return abi.last_kernel()

                name = guard("e" if placement == "base" else "f", backward_input, [("grad_out", G, gin), win_],
                             [("grad_x", GXI), ("workspace", WS)], [T(call["gx"], tdt), None], what + ("backward_input", glayout))
                same_kernel_as_base(key + ("i", glayout), placement, name, what)


# ---------------------------------------------------------------------------------------------------------------------
# b, e, f: pooled
# ---------------------------------------------------------------------------------------------------------------------
def run_pooled(abi, nd, dt, placement):
    if placement != "base":
        run(abi, ("pooled", nd, dt, "base"))
    tdt = DTYPES[dt]
    es = es_of(tdt)
    off, woff = offsets(placement, tdt)
    for ci, case in enumerate(PC.CASES):
        if case[0] != nd:
            continue
        _, shape, pool, cut, _ = case
        b, _, pooled = PC.geometry(case)
        pshape = tuple(shape[:2]) + tuple(pooled)
        X, GX, GXI = (RZ.Guarded(shape, tdt, DEV, offset_bytes=off) for _ in range(3))
        OUT, GP = (RZ.Guarded(pshape, tdt, DEV, offset_bytes=off) for _ in range(2))
        W, GW = (RZ.Guarded((shape[1], nd), tdt, DEV, offset_bytes=woff) for _ in range(2))
        exact = PC.pow2_counts(case)
        for pad, active in sweep_of(placement):
            what = ("pooled", shape, pool, cut, dt, placement, pad, active)
            r = PC.reference(ci, dt, "exact", pad, active)
            xin, win_, gin = ("x", X, T(r["x"], tdt)), ("w", W, T(r["w"], tdt)), ("grad_pooled", GP, T(r["gp"], tdt))
            key = (ci, dt, pad, active)

            def forward():
                abi.forward_pooled(X.t, W.t, pad, active, pool, b, out=OUT.t)
                return abi.last_kernel()

            name = guard("b" if placement == "base" else "f", forward, [xin, win_], [("out", OUT)], [T(r["ref"], tdt)], what + ("forward",))
            same_kernel_as_base(key + ("f",), placement, name, what)
            want = PC.forward_route(case, es, active, pad)
            assert name == want, what + ("forward", name, want)

            route = PC.backward_route(case, es, active, pad)
            WS = workspace(abi, X.t, pad, active, b, off, pool)

            def backward():
                abi.backward_pooled(GP.t, W.t, X.t, pad, active, pool, b, grad_x=GX.t, grad_w=GW.t, workspace=WS.t)
                return abi.last_kernel()

            outs = [("grad_x", GX), ("grad_w", GW), ("workspace", WS)]
            gx_full = None
            if route == PC.NOT_SERVED:   # raises as it does unguarded; nothing is launched
                guard("b" if placement == "base" else "f", backward, [gin, xin, win_], outs, [None] * 3, what + ("backward",), raises="not served")
            else:
                if exact:
                    gx_full, gw_full = T(r["gx_ref"], tdt), gw_expect(r["gw64"], tdt)
                else:   # 3-wide windows round the expanded gradient: the same call on plain fresh tensors (grad_w is deterministic)
                    gx_full, gw_full = abi.backward_pooled(gin[2].to(DEV), win_[2].to(DEV), xin[2].to(DEV), pad, active, pool, b)
                    plain = abi.last_kernel()
                name = guard("b" if placement == "base" else "f", backward, [gin, xin, win_], outs, [gx_full, gw_full, None], what + ("backward",))
                same_kernel_as_base(key + ("b",), placement, name, what)
                assert name in (route if isinstance(route, tuple) else (route,)), what + ("backward", name, route)
                assert exact or name == plain, what + ("backward", name, "on plain tensors", plain)
            if active:
                continue
            # e: the input gradient alone is the full form's grad_x (where the full form is not served: the exact reference's)
            if gx_full is None:
                assert exact, what
                gx_full = T(r["gx_ref"], tdt)

            def backward_input():
                abi.backward_pooled_input(GP.t, W.t, shape, pad, pool, b, grad_x=GXI.t)
                return abi.last_kernel()

            name = guard("e" if placement == "base" else "f", backward_input, [gin, win_], [("grad_x", GXI)], [gx_full], what + ("backward_pooled_input",))
            same_kernel_as_base(key + ("i",), placement, name, what)
            assert name == ("gradx_embed_pool" if (shape[-1] * es) % 16 == 0 else "gradx_gather_pool"), what + (name,)


# ---------------------------------------------------------------------------------------------------------------------
# c: quantized pooled
# ---------------------------------------------------------------------------------------------------------------------
QPOOL = TP.CASES + TP.QCASES
QPOOL_PARTS = 4
QPOOL_NAMES = ("qpool_forward", "qpool_plane_forward", "qpool_band_forward", "qpool_band_fast")
_QFIX = {}


def qpool_fixture(dt):
    """the inputs of every case, drawn in the table's order from the seed test_pooled_gpu uses"""
    if dt not in _QFIX:
        rs = np.random.RandomState(21)
        _QFIX[dt] = [TP.quantized_pool_inputs(rs, nd, shape, np.dtype(dt).type) for nd, shape, _, _ in QPOOL]
    return _QFIX[dt]


def run_qpool(abi, dt, part):
    tdt = {"int8": torch.int8, "uint8": torch.uint8}[dt]
    fixture = qpool_fixture(dt)
    for i in range(part, len(QPOOL), QPOOL_PARTS):
        nd, shape, pool, crop = QPOOL[i]
        xq, wq, zp = fixture[i]
        b, new = abi.check_borders(list(shape), crop, nd)
        pshape = list(new[:2]) + [-(-new[2 + r] // pool[r]) for r in range(nd)]
        X, OUT, W = RZ.Guarded(shape, tdt, DEV), RZ.Guarded(pshape, tdt, DEV), RZ.Guarded(wq.shape, torch.uint8, DEV)
        for pad in range(5):
            refs = TP.quantized_pool_references(xq, wq, zp, pad, pool, b, new)
            for requant, ref in zip((abi.REQUANT_ZP_INSIDE, abi.REQUANT_ZP_OUTSIDE), refs):

                def forward():
                    abi.forward_quantized_pooled(X.t, W.t, 128, zp, pad, pool, b, out=OUT.t, requant=requant)
                    return abi.last_kernel()

                name = guard("c", forward, [("xq", X, torch.from_numpy(xq)), ("wq", W, torch.from_numpy(wq))], [("out", OUT)],
                             [torch.from_numpy(ref)], ("quantized pool", shape, pool, crop, dt, pad, requant))
                assert name in QPOOL_NAMES, name


# ---------------------------------------------------------------------------------------------------------------------
# d: one default-routed problem per kernel family
# ---------------------------------------------------------------------------------------------------------------------
def run_family(abi, index):
    entry = FAMILY_ROUTES[index]
    kind, kernel, dt, shape, cut, pad, active, cl = entry
    tdt = getattr(torch, dt)
    nd = len(shape) - 2
    layout = "channels_last" if cl else "contiguous"
    b, new = abi.check_borders(list(shape), cut, nd) if cut else (None, list(shape))
    torch.manual_seed(1)   # drawn as test_routing_gpu.test_every_family_has_a_default_route draws them
    if kind == "forward_quantized":
        if tdt == torch.int32:
            xq = torch.randint(-1000, 1000, shape, dtype=tdt, device=DEV)
        else:
            info = torch.iinfo(tdt)
            xq = torch.randint(info.min, info.max + 1, shape, dtype=tdt, device=DEV)
        wq = torch.randint(118, 139, (shape[1], nd), dtype=torch.uint8, device=DEV)
        xp, op = xq, None
        if cl:
            xp, op = abi.to_channels_last(xq), abi.to_channels_last(torch.empty(new, dtype=tdt, device=DEV))
        plain = abi.forward_quantized(xp, wq, 128, 3, pad, b, out=op)
        assert abi.last_kernel() == kernel, (entry, abi.last_kernel())
        X, OUT, W = RZ.Guarded(shape, tdt, DEV, layout), RZ.Guarded(new, tdt, DEV, layout), RZ.Guarded(wq.shape, torch.uint8, DEV)

        def forward_quantized():
            abi.forward_quantized(X.t, W.t, 128, 3, pad, b, out=OUT.t)
            return abi.last_kernel()

        name = guard("d", forward_quantized, [("xq", X, xq), ("wq", W, wq)], [("out", OUT)], [plain], ("family",) + entry)
        assert name == kernel, (entry, name)
        return
    x = torch.rand(shape, device=DEV).to(tdt)
    go = torch.rand(new, device=DEV).to(tdt)
    w = ((torch.rand(shape[1], nd, device=DEV) * 2 - 1) * 4).to(tdt)
    xp, gp, op, gxp = x, go, None, None
    if cl:
        xp, gp = abi.to_channels_last(x), abi.to_channels_last(go)
        op, gxp = torch.empty_like(gp), torch.empty_like(xp)
    X, W = RZ.Guarded(shape, tdt, DEV, layout), RZ.Guarded(w.shape, tdt, DEV)
    if kind == "forward":
        plain = abi.forward(xp, w, pad, active, b, out=op)
        assert abi.last_kernel() == kernel, (entry, abi.last_kernel())
        OUT = RZ.Guarded(new, tdt, DEV, layout)

        def forward():
            abi.forward(X.t, W.t, pad, active, b, out=OUT.t)
            return abi.last_kernel()

        name = guard("d", forward, [("x", X, x), ("w", W, w)], [("out", OUT)], [plain], ("family",) + entry)
    else:
        gx_plain, gw_plain = abi.backward(gp, w, xp, pad, active, b, grad_x=gxp)
        assert abi.last_kernel() == kernel, (entry, abi.last_kernel())
        G, GX, GW = RZ.Guarded(new, tdt, DEV, layout), RZ.Guarded(shape, tdt, DEV, layout), RZ.Guarded(w.shape, tdt, DEV)
        WS = workspace(abi, X.t, pad, active, b, 0)

        def backward():
            abi.backward(G.t, W.t, X.t, pad, active, b, grad_x=GX.t, grad_w=GW.t, workspace=WS.t)
            return abi.last_kernel()

        name = guard("d", backward, [("grad_out", G, go), ("x", X, x), ("w", W, w)], [("grad_x", GX), ("grad_w", GW), ("workspace", WS)],
                     [gx_plain, gw_plain, None], ("family",) + entry)
    assert name == kernel, (entry, name)


RUNNERS = {"unpooled": run_unpooled, "pooled": run_pooled, "qpool": run_qpool, "family": run_family}
GROUPS = ([("unpooled", 0, nd, dt, pl) for pl in PLACEMENTS for dt in DTYPES for nd in (1, 2, 3) if pl != "table" or dt != "f64"]
          + [("unpooled", 1, nd, dt, pl) for pl in PLACEMENTS for dt in DTYPES for nd in (2, 3) if pl != "table" or dt != "f64"]
          + [("pooled", nd, dt, pl) for pl in PLACEMENTS for dt in PC.DTYPES for nd in (1, 2, 3)]
          + [("qpool", dt, part) for dt in ("int8", "uint8") for part in range(QPOOL_PARTS)]
          + [("family", i) for i in range(len(FAMILY_ROUTES))])


def run(abi, key):
    """each group once per session"""
    if key not in DONE:
        RUNNERS[key[0]](abi, *key[1:])
        DONE.add(key)


def _id(key):
    if key[0] == "family":
        return "family-%s-%s" % FAMILY_ROUTES[key[1]][:2]
    return "-".join(str(k) for k in key)


@pytest.mark.parametrize("key", GROUPS, ids=_id)
def test_guarded(abi, key):
    run(abi, key)


def test_served_set(abi):
    """the union of the kernel names reached under guard holds every family the tables name (no name is struck)"""
    for key in GROUPS:
        run(abi, key)
    print("calls under guard, every red zone intact:", dict(sorted(CALLS.items())))
    for table in sorted(SEEN_BY):
        print("kernels reached under guard, table %s (%d):" % (table, len(SEEN_BY[table])), sorted(SEEN_BY[table]))
    print("kernels reached under guard (%d):" % len(SEEN), sorted(SEEN))
    want = set(EC.SERVED_BACKWARD) | set(EC.SERVED_FORWARD) | set(EC.CL_SERVED) | set(PC.SERVED_16BIT) | set(QPOOL_NAMES)
    want |= {e[1] for e in FAMILY_ROUTES}
    want |= {"gradx_embed", "gradx_gather", "gradx_embed_pool", "gradx_gather_pool"}   # (test_fixed_gpu.py / test_fixed_pool_gpu.py)
    assert want <= SEEN, sorted(want - SEEN)
    for names in EC.SERVED_BACKWARD_ANY + EC.SERVED_FORWARD_ANY + [PC.BAND_WALK]:
        assert SEEN & set(names), names


# ---------------------------------------------------------------------------------------------------------------------
# shiftnd_transpose: what every channels-last op call goes through
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_transpose_guarded(abi, es):
    """[batch, rows, cols] -> [batch, cols, rows] of `es`-byte elements: the vector path (both sides multiples of 16 bytes), both
    scalar edges, tiles that are partial in either direction; bit for bit src.permute(0, 2, 1).contiguous(), in both directions"""
    tdt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[es]
    gen = torch.Generator().manual_seed(es)
    lo, hi = (0, 256) if es == 1 else (-2 ** (8 * es - 2), 2 ** (8 * es - 2))
    for batch, rows, cols in itertools.product((1, 3), (1, 7, 16, 33, 64, 70), (1, 4, 16, 31, 64, 72)):
        m = torch.randint(lo, hi, (batch, rows, cols), dtype=tdt, generator=gen)   # the source as it lies in memory
        for direction in ("to_contiguous", "to_channels_last"):
            # to_contiguous: [N, C = cols, P = rows] channels-last -> contiguous; to_channels_last: [N, C = rows, P = cols] the other way
            shape = (batch, cols, rows, 1) if direction == "to_contiguous" else (batch, rows, cols, 1)
            layouts = ("channels_last", "contiguous") if direction == "to_contiguous" else ("contiguous", "channels_last")
            SRC, DST = RZ.Guarded(shape, tdt, DEV, layouts[0]), RZ.Guarded(shape, tdt, DEV, layouts[1])
            value = (m.permute(0, 2, 1) if direction == "to_contiguous" else m).reshape(shape)   # the same elements, as the logical tensor

            def transpose():
                getattr(abi, direction)(SRC.t, out=DST.t)
                return "shiftnd_transpose"

            what = ("transpose", direction, es, batch, rows, cols)
            RZ.run_guarded(transpose, [("src", SRC, value)], [("dst", DST)], [value], what)
            assert torch.equal(SRC.interior_bytes().cpu().view(tdt).view(batch, rows, cols), m), what
            assert torch.equal(DST.interior_bytes().cpu().view(tdt).view(batch, cols, rows), m.permute(0, 2, 1).contiguous()), what


# ---------------------------------------------------------------------------------------------------------------------
# the harness itself on device memory (its full self-checks run on CPU tensors: tests/test_redzone_cases.py)
# ---------------------------------------------------------------------------------------------------------------------
def test_the_harness_sees_device_writes_and_leaks(abi):
    """device "kernels" made of torch ops, every access inside the test's own allocation: one element stored past `out`, a store into
    the input, and the element after the input entering the result through 0 * (the NaN pattern alone) and through max (the finite
    pattern alone) are each rejected"""
    from test_redzone_cases import _beyond
    shape = (2, 3, 7, 11)
    value = torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(shape) / 8
    X, OUT = RZ.Guarded(shape, torch.float16, DEV), RZ.Guarded(shape, torch.float16, DEV)

    def run(mutation, patterns=RZ.PATTERNS):
        def kernel():
            out = X.t * 2
            if mutation == "0 *":
                out = out + 0 * _beyond(X)
            if mutation == "max":
                out = torch.fmax(out, _beyond(X))
            OUT.t.copy_(out)
            if mutation == "past out":
                _beyond(OUT)[0] = 1.0
            if mutation == "input":
                X.t[1, 2, 6, 10] = 0.0
            return "device_ops"

        return RZ.run_guarded(kernel, [("x", X, value)], [("out", OUT)], [(value * 2).half()], ("harness", mutation), patterns=patterns)

    assert run(None) == "device_ops"
    with pytest.raises(AssertionError, match=r"red zone of 'out' written: 2 bytes, first at offset %d" % OUT.nbytes):
        run("past out")
    with pytest.raises(AssertionError, match="input written"):
        run("input")
    assert run("0 *", (0x7B,)) == "device_ops" and run("max", (0xFF,)) == "device_ops"
    with pytest.raises(AssertionError, match="pattern 0xFF"):
        run("0 *")
    with pytest.raises(AssertionError, match="pattern 0x7B"):
        run("max")
