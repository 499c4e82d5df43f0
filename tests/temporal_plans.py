"""The launch plans of the three channels-last temporal kernels, restated in plain Python, and the case table built on them
(tests/test_temporal_plans_cases.py checks both without a GPU; tests/test_temporal_plans_gpu.py runs the cases).

frames_forward (csrc/shiftnd_frames.hip), frames_active_forward and frames_backward (csrc/shiftnd_frames_learn.hip) each choose the
rows of a workgroup -- and with them the trip counts of their row loops -- from thresholds on the grid.  Shapes with a handful of
frames see one plan only: one batch per workgroup, one row step, one row per fp64 sum.  The functions here return, for a problem
(N, T, M, C, element size, base offset in elements), what the host code plans and what the kernel then does with it, so that a
case can be placed in a regime by arithmetic and a test can say in which workgroup, batch or step a wrong element lies.

A buffer is (N, T, M, C): N clips of T frames of M pixel rows of C channels, the base `off` elements past a 16-byte-aligned
allocation.  R = C * es bytes per row; the piece is piece_bytes() of R and the bases; P pieces per row; rps rows per step.

CASES: (regime, kernel, (N, T, M, C), dtype, offset, table kind, bytes of one tensor) -- every regime of REGIMES holds for at least one case; a case is
the smallest (in bytes of one tensor) that search() finds for its regime over its candidate grid; `python tests/temporal_plans.py`
prints the search's answer beside every row.  Table kinds are those of tests/test_tshift_cl_gpu.py::_weights -- "specials" (random
quarters: pieces of several elements are mixed), "pieces" (constant inside every 16-byte piece: every piece uniform), "runs" (TSM-like
runs: uniform but for a boundary inside a piece) -- with "clip-" in front for a per-clip [N, C] table whose rows all differ.
"""
import numpy as np

# ---- the constants of the two files (tests/test_temporal_plans_cases.py reads them from the sources' text) -----------------------
K_THREADS = 256                # kThreads, csrc/shiftnd_common.hpp
FRAMES = {"kInFlight": 8, "kMinRowGroups": 8, "kMaxRowGroups": 16, "kWantWorkgroups": 6144}          # csrc/shiftnd_frames.hip
LEARN = {"kFwdInFlight": 4, "kWantWorkgroups": 6144, "kMaxRowSteps": 8, "kWantGroups": 2048}         # csrc/shiftnd_frames_learn.hip
ES = {"u8": 1, "i8": 1, "i32": 4, "f16": 2, "bf16": 2, "f32": 4, "f64": 8}

MIB = 1 << 20
CASE_CAP, TOTAL_CAP = 256 * MIB, 2048 * MIB      # the largest tensor of a case; the sum over the table


def cdiv(a, b):
    return (a + b - 1) // b


def piece(C, es, off):
    """piece_bytes (csrc/shiftnd_temporal.hpp) of a row of C * es bytes at bases off * es bytes past a 16-byte boundary, and what
    make_params / frames_forward derive from it (shiftnd_frames.hip: q.unit_log2 .. q.rps; shiftnd_frames_learn.hip: make_params)
    -> unit bytes, P pieces per row, elements per piece, span = min(P, 256), rps = 256 / span"""
    bits = (C * es) | 16 | (off * es)
    unit = bits & -bits
    P = C * es // unit
    span = min(P, K_THREADS)
    return dict(unit=unit, P=P, epp=unit // es, span=span, rps=K_THREADS // span)


def _split(M, chunks0, batch_rows):
    """rows_per_wg = the even split rounded up to whole batches; chunks = the workgroups that then hold rows"""
    rows_per_wg = cdiv(cdiv(M, chunks0), batch_rows) * batch_rows
    return rows_per_wg, cdiv(M, rows_per_wg)


def _walk(p, M, in_flight):
    """what the workgroups of one frame (or clip) do: the first one and the last one.  batches: trips of the uniform-piece loop
    `r += rps * in_flight` of the thread with rl = 0; iterations: trips of the row loop `r += rps`; tail: rows of the last batch"""
    rows, rps = min(p["rows_per_wg"], M), p["rps"]
    last = M - (p["chunks"] - 1) * p["rows_per_wg"]
    p.update(rows=rows, batches=cdiv(rows, rps * in_flight), iterations=cdiv(rows, rps),
             last_rows=last, last_batches=cdiv(last, rps * in_flight), last_iterations=cdiv(last, rps),
             last_tail=last - (cdiv(last, rps * in_flight) - 1) * rps * in_flight,
             column_trips=cdiv(p["P"], K_THREADS))
    return p


def forward_plan(N, T, M, C, es, off=0):
    """frames_forward(const Geometry &...) in csrc/shiftnd_frames.hip, from `const int64_t frames = g.N * q.T` to `q.chunks = ...`,
    and the loops of frames_body"""
    k = FRAMES
    p = piece(C, es, off)
    frames, step_rows = N * T, p["rps"]
    fewest = cdiv(M, step_rows * k["kMaxRowGroups"])
    most = cdiv(M, step_rows * k["kMinRowGroups"])
    wanted = cdiv(k["kWantWorkgroups"], frames)
    chunks0 = max(fewest, min(most, wanted))
    decided = "most" if wanted >= most else ("fewest" if wanted <= fewest else "wanted")   # (a tie is the bound's: the regimes ask strictly)
    p["rows_per_wg"], p["chunks"] = _split(M, chunks0, step_rows * k["kInFlight"])
    p.update(fewest=fewest, most=most, wanted=wanted, decided=decided, workgroups=frames * p["chunks"])
    return _walk(p, M, k["kInFlight"])


def active_forward_plan(N, T, M, C, es, off=0):
    """frames_active_forward(const Geometry &...) in csrc/shiftnd_frames_learn.hip, from `const int64_t frames = g.N * q.T` to
    `q.chunks = ...`, and the loops of forward_body.  No `fewest`: nothing bounds the batches of a workgroup"""
    k = LEARN
    p = piece(C, es, off)
    frames, batch_rows = N * T, p["rps"] * k["kFwdInFlight"]
    most = cdiv(M, batch_rows)
    wanted = cdiv(k["kWantWorkgroups"], frames)
    p["rows_per_wg"], p["chunks"] = _split(M, min(most, wanted), batch_rows)
    p.update(fewest=None, most=most, wanted=wanted, decided="most" if most <= wanted else "wanted", workgroups=frames * p["chunks"])
    return _walk(p, M, k["kFwdInFlight"])


def backward_plan(N, T, M, C, es, off=0):
    """backward_rows_per_wg / backward_chunks / frames_backward_workspace in csrc/shiftnd_frames_learn.hip -- the plan is made from
    the geometry alone, as if the pieces were 16 bytes (plan_rps) -- and the row loop `r += rps` of backward_body under the kernel's
    own rps.  groups = N * chunks partial records of C * 3 doubles: workspace_bytes"""
    k = LEARN
    p = piece(C, es, off)
    pieces = cdiv(C * es, 16)
    plan_rps = K_THREADS // pieces if pieces < K_THREADS else 1
    steps = k["kMaxRowSteps"]
    while steps > 1 and N * cdiv(M, plan_rps * steps) < k["kWantGroups"]:
        steps //= 2
    p["rows_per_wg"] = plan_rps * steps
    p["chunks"] = cdiv(M, p["rows_per_wg"])
    p.update(plan_rps=plan_rps, steps=steps, workgroups=N * p["chunks"], workspace_bytes=N * p["chunks"] * C * 24)
    return _walk(p, M, 1)


PLANS = {"frames_forward": forward_plan, "frames_active_forward": active_forward_plan, "frames_backward": backward_plan}
IN_FLIGHT = {"frames_forward": FRAMES["kInFlight"], "frames_active_forward": LEARN["kFwdInFlight"], "frames_backward": 1}


def plan_of(case):
    regime, kernel, (N, T, M, C), dt, off, table = case[:6]
    return PLANS[kernel](N, T, M, C, ES[dt], off)


def nbytes(case):
    N, T, M, C = case[2]
    return N * T * M * C * ES[case[3]]


def locate(kernel, shape, es, off, flat):
    """a flat element index of the (N, T, M, C) buffer -> text: (n, t, row, channel) and the workgroup, batch or step that wrote it"""
    N, T, M, C = shape
    n, t, row, c = np.unravel_index(int(flat), shape)
    p = PLANS[kernel](N, T, M, C, es, off)
    chunk, r = divmod(int(row), p["rows_per_wg"])
    per = p["rps"] * IN_FLIGHT[kernel]
    wg = (n * p["chunks"] + chunk) if kernel == "frames_backward" else ((n * T + t) * p["chunks"] + chunk)
    return ("(n, t, row, channel) = (%d, %d, %d, %d): workgroup %d (chunk %d of %d, rows_per_wg %d), row %d of the workgroup -- uniform path: "
            "batch %d, slot %d; row loop: step %d; thread row %d, piece %d (%d-byte pieces, rps %d)"
            % (n, t, row, c, wg, chunk, p["chunks"], p["rows_per_wg"], r, r // per, (r % per) // p["rps"], r // p["rps"], r % p["rps"],
               c // p["epp"], p["unit"], p["rps"]))


# ---- the tables ------------------------------------------------------------------------------------------------------------
def table_of(case, pad, seed=0):
    """the table of a case under a padding, float64 on quarters, from tests/test_tshift_cl_gpu.py::_weights: [C], or for the "clip-"
    kinds [N, C] -- row n: turn pad + n and a quarter of n mod (4 T + 5) on top of every channel, so that neighbouring rows differ
    and a uniform piece stays uniform"""
    import torch
    from test_tshift_cl_gpu import _weights
    regime, kernel, (N, T, M, C), dt, off, table = case[:6]
    tdt = {"u8": torch.uint8, "f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "f64": torch.float64}[dt]
    rs = np.random.RandomState(7000 + 10 * seed + pad)
    if not table.startswith("clip-"):
        return np.asarray(_weights(rs, C, T, pad, table=table, dt=tdt), np.float64)
    rows = np.stack([np.asarray(_weights(rs, C, T, pad + n, table=table[5:], dt=tdt), np.float64) for n in range(N)])
    rows += (np.arange(N) % (4 * T + 5)).reshape(N, 1) * 0.25      # a whole row moves: uniform pieces stay uniform, neighbours differ
    return rows


def source_frames(w, T, pad, active):
    """the source frames of the forward under weights w [..., C] for t = 0 .. T-1 -> int array [..., C, T, taps] (-1: a fill);
    taps: floor(w) and floor(w) + 1 (interpolating) or rint(w) (sparse).  The padding map is the oracle's (bigindex_cases.fold)"""
    import torch
    from bigindex_cases import fold
    w = torch.as_tensor(np.asarray(w, np.float64))
    iw = (torch.floor(w) if active else torch.round(w)).to(torch.int64)
    taps = []
    for q in range(2 if active else 1):
        idx, ok = fold(torch.arange(T).view(*([1] * w.dim()), T) - iw.unsqueeze(-1) + q, T, pad)
        taps.append(torch.where(ok, idx, torch.full_like(idx, -1)))
    return torch.stack(taps, -1).numpy()


def mixed_pieces(case, pad, active):
    """how many pieces of a row (of the first clip's row of the table) hold elements with different source frames, of how many"""
    p = plan_of(case)
    T, C = case[2][1], case[2][3]
    w = table_of(case, pad)
    src = source_frames(w if w.ndim == 1 else w[0], T, pad, active).reshape(C // p["epp"], p["epp"], -1)
    return int((src != src[:, :1]).any(axis=(1, 2)).sum()), C // p["epp"]


# ---- the regimes: name -> (kernel, predicate on (plan, table kind)) -------------------------------------------------------------
def _uniform(t):
    return t.replace("clip-", "") in ("pieces", "runs")


def _mixed(p, t):
    return t.replace("clip-", "") == "specials" and p["epp"] > 1


def _partial(p):
    return p["chunks"] > 1 and p["last_rows"] < p["rows_per_wg"]


FF, FA, FB = "frames_forward", "frames_active_forward", "frames_backward"
REGIMES = {
    # frames_forward
    "ff-two-full-batches": (FF, lambda p, t: _uniform(t) and p["batches"] == 2 and p["rows"] == 2 * p["rps"] * FRAMES["kInFlight"]),
    "ff-second-batch-under-rps": (FF, lambda p, t: _uniform(t) and p["last_batches"] == 2 and p["last_tail"] < p["rps"]),
    "ff-wanted-decides": (FF, lambda p, t: p["decided"] == "wanted" and p["fewest"] < p["wanted"] < p["most"]),
    "ff-fewest-decides": (FF, lambda p, t: p["wanted"] < p["fewest"] and p["batches"] == 2),      # (strictly: no tie with `wanted`)
    "ff-long-rows-several-chunks": (FF, lambda p, t: p["P"] > 256 and p["chunks"] > 1),
    "ff-odd-pieces-two-batches": (FF, lambda p, t: _uniform(t) and 256 % p["P"] != 0 and p["P"] < 256 and p["batches"] == 2),
    "ff-two-batches-1-byte": (FF, lambda p, t: _uniform(t) and p["unit"] == 1 and p["batches"] == 2),
    "ff-two-batches-2-byte": (FF, lambda p, t: _uniform(t) and p["unit"] == 2 and p["batches"] == 2),
    "ff-two-batches-4-byte": (FF, lambda p, t: _uniform(t) and p["unit"] == 4 and p["batches"] == 2),
    "ff-two-batches-8-byte": (FF, lambda p, t: _uniform(t) and p["unit"] == 8 and p["batches"] == 2),
    "ff-two-batches-16-byte": (FF, lambda p, t: _uniform(t) and p["unit"] == 16 and p["batches"] == 2),
    "ff-mixed-several-steps": (FF, lambda p, t: _mixed(p, t) and p["rows_per_wg"] > p["rps"] and p["iterations"] > 8),
    # frames_active_forward
    "fa-one-batch-uniform": (FA, lambda p, t: t == "pieces" and p["batches"] == 1 and p["chunks"] > 1),
    "fa-one-batch-uniform-runs": (FA, lambda p, t: t == "runs" and p["batches"] == 1 and p["chunks"] > 1),
    "fa-two-batches-uniform-pieces": (FA, lambda p, t: t == "pieces" and p["batches"] == 2),
    "fa-two-batches-uniform-runs": (FA, lambda p, t: t == "runs" and p["batches"] == 2),
    "fa-three-batches-uniform-pieces": (FA, lambda p, t: t == "pieces" and p["batches"] >= 3),
    "fa-three-batches-uniform-runs": (FA, lambda p, t: t == "runs" and p["batches"] >= 3),
    "fa-one-batch-mixed": (FA, lambda p, t: _mixed(p, t) and p["batches"] == 1 and p["chunks"] > 1),
    "fa-two-batches-mixed": (FA, lambda p, t: _mixed(p, t) and p["batches"] == 2),
    "fa-three-batches-mixed": (FA, lambda p, t: _mixed(p, t) and p["batches"] >= 3),
    "fa-wanted-partial-last-chunk": (FA, lambda p, t: p["decided"] == "wanted" and p["wanted"] < p["most"] and _partial(p)),
    "fa-ragged-two-batches": (FA, lambda p, t: p["unit"] < 16 and p["batches"] >= 2),
    # the unsuffixed kernel -- 16-byte pieces of 2 to 8 elements, what 64-channel models run -- past its first batch
    "fa-whole-two-batches-uniform": (FA, lambda p, t: _uniform(t) and p["unit"] == 16 and p["epp"] > 1 and p["batches"] >= 2),
    "fa-whole-two-batches-mixed": (FA, lambda p, t: _mixed(p, t) and p["unit"] == 16 and p["batches"] >= 2),
    # frames_backward
    "fb-steps-1-partial": (FB, lambda p, t: p["steps"] == 1 and _partial(p) and p["iterations"] == 1),
    "fb-steps-2-partial": (FB, lambda p, t: p["steps"] == 2 and _partial(p) and p["iterations"] == 2),
    "fb-steps-4-partial": (FB, lambda p, t: p["steps"] == 4 and _partial(p) and p["iterations"] == 4),
    "fb-steps-8-partial": (FB, lambda p, t: p["steps"] == 8 and _partial(p) and p["iterations"] == 8),
    "fb-whole-steps-4-partial": (FB, lambda p, t: p["unit"] == 16 and p["epp"] > 1 and p["steps"] == 4 and _partial(p) and p["iterations"] == 4),
    "fb-whole-steps-8-partial": (FB, lambda p, t: p["unit"] == 16 and p["epp"] > 1 and p["steps"] == 8 and _partial(p) and p["iterations"] == 8),
    "fb-ragged-rps-2-byte": (FB, lambda p, t: p["rps"] != p["plan_rps"] and p["iterations"] >= 2 and p["unit"] == 2),
    "fb-ragged-rps-4-byte": (FB, lambda p, t: p["rps"] != p["plan_rps"] and p["iterations"] >= 2 and p["unit"] == 4),
    "fb-ragged-rps-8-byte": (FB, lambda p, t: p["rps"] != p["plan_rps"] and p["iterations"] >= 2 and p["unit"] == 8),
    "fb-ragged-rps-steps": (FB, lambda p, t: p["rps"] != p["plan_rps"] and p["steps"] > 1 and p["iterations"] > p["steps"]),
    "fb-long-rows-steps": (FB, lambda p, t: p["P"] > 256 and p["steps"] > 1),
    "fb-channel-table-records": (FB, lambda p, t: not t.startswith("clip-") and p["chunks"] > 1 and p["N"] > 1),
    "fb-clip-table-records": (FB, lambda p, t: t.startswith("clip-") and p["chunks"] > 1 and p["N"] > 1),
    "fb-clip-table-steps": (FB, lambda p, t: t.startswith("clip-") and p["chunks"] > 1 and p["steps"] > 1),
}

# (regime, kernel, (N, T, M, C), dtype, offset, table kind, bytes of one tensor)
CASES = [
    ("ff-two-full-batches", FF, (128, 2, 1921, 24), "u8", 1, "pieces", 11802624),
    ("ff-second-batch-under-rps", FF, (615, 2, 401, 24), "u8", 1, "pieces", 11837520),
    ("ff-wanted-decides", FF, (128, 2, 1921, 24), "u8", 1, "pieces", 11802624),
    ("ff-fewest-decides", FF, (128, 2, 3841, 24), "u8", 1, "pieces", 23599104),
    ("ff-long-rows-several-chunks", FF, (1, 2, 9, 2056), "f16", 0, "pieces", 74016),
    ("ff-odd-pieces-two-batches", FF, (128, 2, 1921, 24), "u8", 1, "pieces", 11802624),
    ("ff-two-batches-1-byte", FF, (128, 2, 1921, 24), "u8", 1, "pieces", 11802624),
    ("ff-two-batches-2-byte", FF, (384, 2, 641, 24), "f16", 1, "pieces", 23629824),
    ("ff-two-batches-4-byte", FF, (384, 2, 2689, 6), "f32", 1, "pieces", 49563648),
    ("ff-two-batches-8-byte", FF, (384, 2, 5441, 24), "u8", 0, "pieces", 100288512),
    ("ff-two-batches-16-byte", FF, (384, 2, 5441, 48), "u8", 0, "pieces", 200577024),
    ("ff-mixed-several-steps", FF, (384, 2, 16385, 2), "u8", 0, "specials", 25167360),
    ("fa-one-batch-uniform", FA, (1, 2, 41, 24), "f16", 1, "pieces", 3936),
    ("fa-one-batch-uniform-runs", FA, (1, 2, 41, 24), "f16", 1, "runs", 3936),
    ("fa-two-batches-uniform-pieces", FA, (256, 2, 481, 24), "f16", 1, "pieces", 11821056),
    ("fa-two-batches-uniform-runs", FA, (256, 2, 481, 24), "f16", 1, "runs", 11821056),
    ("fa-three-batches-uniform-pieces", FA, (384, 2, 641, 24), "f16", 1, "pieces", 23629824),
    ("fa-three-batches-uniform-runs", FA, (384, 2, 641, 24), "f16", 1, "runs", 23629824),
    ("fa-one-batch-mixed", FA, (1, 2, 341, 6), "f16", 0, "specials", 8184),
    ("fa-two-batches-mixed", FA, (256, 2, 4081, 6), "f16", 0, "specials", 25073664),
    ("fa-three-batches-mixed", FA, (384, 2, 5441, 6), "f16", 0, "specials", 50144256),
    ("fa-wanted-partial-last-chunk", FA, (256, 2, 481, 24), "f16", 1, "pieces", 11821056),
    ("fa-ragged-two-batches", FA, (256, 2, 481, 24), "f16", 1, "pieces", 11821056),
    ("fa-whole-two-batches-uniform", FA, (256, 2, 4081, 24), "f16", 0, "runs", 100294656),
    ("fa-whole-two-batches-mixed", FA, (256, 2, 4081, 24), "f16", 0, "specials", 100294656),
    ("fb-steps-1-partial", FB, (1, 2, 257, 2), "f16", 0, "pieces", 2056),
    ("fb-steps-2-partial", FB, (1024, 2, 513, 2), "f16", 0, "pieces", 4202496),
    ("fb-steps-4-partial", FB, (1024, 2, 1025, 2), "f16", 0, "pieces", 8396800),
    ("fb-steps-8-partial", FB, (1024, 2, 2049, 2), "f16", 0, "pieces", 16785408),
    ("fb-whole-steps-4-partial", FB, (1024, 2, 341, 24), "f16", 0, "specials", 33521664),
    ("fb-whole-steps-8-partial", FB, (1024, 2, 681, 24), "f16", 0, "pieces", 66945024),
    ("fb-ragged-rps-2-byte", FB, (1, 2, 129, 2), "f16", 1, "pieces", 1032),
    ("fb-ragged-rps-4-byte", FB, (1, 2, 86, 6), "f16", 0, "pieces", 2064),
    ("fb-ragged-rps-8-byte", FB, (1, 2, 86, 12), "f16", 0, "pieces", 4128),
    ("fb-ragged-rps-steps", FB, (1024, 2, 513, 2), "f16", 1, "pieces", 4202496),
    ("fb-long-rows-steps", FB, (1024, 2, 3, 2056), "f16", 0, "pieces", 25264128),
    ("fb-channel-table-records", FB, (2, 2, 257, 2), "f16", 0, "pieces", 4112),
    ("fb-clip-table-records", FB, (2, 2, 257, 2), "f16", 0, "clip-specials", 4112),
    ("fb-clip-table-steps", FB, (1024, 2, 513, 2), "f16", 0, "clip-specials", 4202496),
    # beside the smallest: the ragged shape of four row-loop trips (T = 3, 2-byte pieces, rps 51 under a plan of 256), the mixed path of
    # the backward with two steps, and a per-clip table under the two forwards' second batch
    ("fb-ragged-rps-2-byte", FB, (2, 3, 196, 5), "f16", 0, "specials", 11760),
    ("fb-steps-2-partial", FB, (1024, 2, 65, 64), "bf16", 0, "specials", 17039360),
    ("ff-two-batches-2-byte", FF, (384, 2, 641, 24), "f16", 1, "clip-pieces", 23629824),
    ("fa-two-batches-mixed", FA, (256, 2, 4081, 6), "f16", 0, "clip-specials", 25073664),
    # ... and the 64-channel rows of 8 whole pieces: one workgroup per frame with two batches, four row steps of the backward
    ("fa-whole-two-batches-uniform", FA, (3072, 2, 129, 64), "f16", 0, "pieces", 101449728),     # (the batched loop is the uniform path's)
    ("fa-whole-two-batches-mixed", FA, (3072, 2, 129, 64), "f16", 0, "specials", 101449728),
    ("fb-whole-steps-4-partial", FB, (1024, 2, 129, 64), "bf16", 0, "specials", 33816576),
]


def unique_cases():
    """the cases the GPU test runs: CASES without the rows that differ in the regime's name only"""
    seen, out = set(), []
    for c in CASES:
        if c[1:6] not in seen:
            seen.add(c[1:6])
            out.append(c)
    return out


def holds(regime, case):
    kernel, pred = REGIMES[regime]
    if case[1] != kernel:
        return False
    p = plan_of(case)
    p["N"] = case[2][0]
    return bool(pred(p, case[5]))


# ---- the fuzz's generator (tests/test_fuzz_temporal_gpu.py) ---------------------------------------------------------------------
# family -> (layout, dtypes): "segment" buffers are (N, T, C, M), "frames" buffers (N, T, M, C)
FUZZ_FAMILIES = [
    ("tshift", "segment", ("f16", "bf16", "f32", "f64")),
    ("per_clip", "segment", ("f16", "bf16", "f32", "f64")),
    ("interlace", "segment", ("f16", "bf16", "f32", "f64")),
    ("learnable_cl", "frames", ("f16", "bf16", "f32", "f64")),
    ("fixed_cl", "frames", ("f16", "bf16", "f32", "f64")),
    ("per_clip_cl", "frames", ("f16", "bf16", "f32", "f64")),
    ("quantized_segment", "segment", ("u8", "i8", "i32")),
    ("quantized_cl", "frames", ("u8", "i8", "i32")),
    ("inplace_segment", "segment", ("f16", "bf16", "f32", "f64", "u8", "i8", "i32")),
    ("inplace_cl", "frames", ("f16", "bf16", "f32", "f64", "u8", "i8", "i32")),
]
FUZZ_BYTES = 1 << 20                       # the largest tensor of a case
FAST_BYTES = (16, 32, 48, 80, 160, 4096, 4112, 8192)      # the fastest dim: around 16, multiples of 16 and 8192, P = 3, 5, 10, 256, 257
SLOW_SIZES = (2, 3, 5, 7, 16, 33, 52, 86, 130, 257, 300, 515)   # the other dim (pixel rows of a frame, or channels): row loops that iterate


def draw_case(rs, n):
    """case n of a run: the families in turn; every second visit of a family is aligned (the fastest dim in whole 16-byte pieces, no
    offset: the kernels' unsuffixed forms), the others ragged (a fastest dim one or two elements off a multiple of 16 bytes, or a
    base one element off).  -> dict(family, layout, dt, N, T, C, M, off, pad, active, table)"""
    family, layout, dts = FUZZ_FAMILIES[n % len(FUZZ_FAMILIES)]
    aligned = (n // len(FUZZ_FAMILIES)) % 2 == 0
    dt = dts[rs.randint(len(dts))]
    es = ES[dt]
    fast_bytes = FAST_BYTES[rs.randint(len(FAST_BYTES))]
    off = 0
    if not aligned:
        if rs.randint(3) == 0:
            off = 1
        else:
            fast_bytes += int(rs.choice([-2, -1, 1, 2])) * es
    fast = max(2, fast_bytes // es)
    if aligned and (fast * es) % 16:
        fast = cdiv(fast * es, 16) * 16 // es
    slow = int(SLOW_SIZES[rs.randint(len(SLOW_SIZES))])
    T = int(rs.randint(1, 17 if family.startswith("inplace") else 18))
    least_T = 2 if family == "quantized_segment" else 1  # (the segment route takes clips of two frames and more)
    T = max(T, least_T)
    N = int(rs.randint(1, 5))
    while N * T * fast * slow * es > FUZZ_BYTES:          # the slow dim first, then the clips and the frames
        if slow > 2:
            slow = max(2, slow // 2)
        elif N > 1:
            N -= 1
        else:
            T = max(least_T, T // 2)
    C, M = (slow, fast) if layout == "segment" else (fast, slow)
    table = ("specials", "pieces", "runs")[rs.randint(3)]
    return dict(family=family, layout=layout, dt=dt, N=N, T=T, C=C, M=M, off=off, pad=int(rs.randint(5)), active=int(rs.randint(2)),
                table=table, aligned=aligned)


FUZZ_SEEDS = (0, 1, 2)
FUZZ_COUNT = 6 * len(FUZZ_FAMILIES)        # cases per seed: six visits of every family, three aligned and three ragged


def fuzz_cases(seed, count=FUZZ_COUNT):
    """the cases of a seed: case n is drawn from a generator of its own, so the list does not depend on what a runner draws"""
    return [draw_case(np.random.RandomState(100003 * (seed + 1) + n), n) for n in range(count)]


def fuzz_kernels(case):
    """the names shiftnd_last_kernel() gives a case: the forward's and (learnable families) the backward's.  The unsuffixed form runs
    where the fastest dim is whole 16-byte pieces and the bases are aligned (piece() == 16), *_ragged elsewhere"""
    es = ES[case["dt"]]
    fast = case["M"] if case["layout"] == "segment" else case["C"]
    tail = "" if piece(fast, es, case["off"])["unit"] == 16 else "_ragged"
    family = case["family"]
    if family in ("tshift", "per_clip"):
        return ("tshift_forward" + tail, "tshift_backward" + tail)
    if family == "interlace":
        return ("tinterlace_forward" + tail, "tinterlace_backward" + tail)
    if family in ("learnable_cl", "per_clip_cl"):
        return (("frames_active_forward" if case["active"] else "frames_forward") + tail, "frames_backward" + tail)
    if family in ("fixed_cl", "quantized_cl"):
        return ("frames_forward" + tail,)
    if family == "quantized_segment":
        return ("segment_forward" + tail,)
    return ("frames_inplace" + tail,)


FUZZ_MUST_SEE = ("tshift_forward", "tshift_forward_ragged", "tshift_backward", "tshift_backward_ragged",
                 "tinterlace_forward", "tinterlace_forward_ragged", "tinterlace_backward", "tinterlace_backward_ragged",
                 "frames_forward", "frames_forward_ragged", "frames_active_forward", "frames_active_forward_ragged",
                 "frames_backward", "frames_backward_ragged", "segment_forward", "frames_inplace", "frames_inplace_ragged")


# ---- the search ------------------------------------------------------------------------------------------------------------
ROWS = [(1, "u8"), (2, "u8"), (3, "u8"), (4, "u8"), (8, "u8"), (16, "u8"), (24, "u8"), (48, "u8"),
        (2, "f16"), (3, "f16"), (4, "f16"), (5, "f16"), (6, "f16"), (8, "f16"), (12, "f16"), (24, "f16"), (40, "f16"), (64, "f16"),
        (2056, "f16"), (2112, "f16"), (3, "f32"), (4, "f32"), (6, "f32"), (12, "f32"), (3, "f64"), (2, "f64")]


def candidates(kernel, rows=ROWS, T=2, offs=(0, 1)):
    """the grid the search walks: rows (C, dtype), both offsets, N around the frame and group counts at which a threshold moves, M
    around the multiples of the row steps"""
    float_only = kernel != FF
    ns = {1, 2, 3}
    for want in (LEARN["kWantGroups"], FRAMES["kWantWorkgroups"]):
        for f in range(1, 9):
            for d in (-1, 0, 1):
                ns.add(max(1, cdiv(want, f * T) + d))
                ns.add(max(1, cdiv(want, f) + d))
    for C, dt in rows:
        if float_only and dt == "u8":
            continue
        for off in offs:
            es = ES[dt]
            pc = piece(C, es, off)
            plan_rps = max(1, K_THREADS // cdiv(C * es, 16))
            ms = set()
            for base in {pc["rps"], plan_rps}:
                for k in list(range(1, 34)) + [40, 48, 64]:
                    for d in (-1, 0, 1):
                        ms.add(k * base + d)
            for M in sorted(m for m in ms if m >= 2):
                for N in sorted(ns):
                    if N * T * M * C * es <= CASE_CAP:
                        yield (N, T, M, C), dt, off


def search(regime, table, **kw):
    """the smallest case (bytes of one tensor, then N) of the grid in the regime"""
    kernel = REGIMES[regime][0]
    best = None
    for shape, dt, off in candidates(kernel, **kw):
        case = (regime, kernel, shape, dt, off, table)
        key = (nbytes(case), shape[0])
        if (best is None or key < best[0]) and holds(regime, case):
            best = (key, case)
    return best and best[1]


if __name__ == "__main__":
    for c in CASES:
        found = search(c[0], c[5])
        print("%-34s %-22s %-22s %-5s off %d %-14s %10d bytes | search: %s %s off %d, %d bytes"
              % (c[:2] + (c[2],) + c[3:6] + (nbytes(c),) + (found[2], found[3], found[4], nbytes(found))))
    print("total", sum(nbytes(c) for c in CASES))
