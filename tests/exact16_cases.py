"""Case table, fixtures, reference, alternates and assertion functions of the exact-data and single-tap parity tests of the unpooled
16-bit kernels (tests/test_exact16_gpu.py and tests/test_exact16_cl_gpu.py on the GPU, tests/test_exact16_cases.py for the
self-checks that need none).  The machinery is tests/pooled16_cases.py's; nothing of it is copied.

The specification of shiftnd_forward / shiftnd_backward on fp16 / bf16 tensors is the oracle on widened values, narrowed once:
out = round16(forward), grad_x = round16(backward's), grad_w = round16(the fp64 sums).

EXACT DATA (pooled16_cases.exact_data with the window's shape in the pooled shape's place).  x and the gradient are multiples of 1/8
with |k| <= 7, the weights lie on quarters (1-D, 2-D) or halves (3-D): every tap, grad_x and every partial sum of grad_w is exact in
fp32, out and grad_x are representable in fp16 and bf16 -- a correct kernel returns out, grad_x and round16(grad_w) bit for bit,
whatever its evaluation order.  bf16's unit is 0.5 at 64 - 128, so one dropped term of a dense grad_w may round away; hence the

PROBE DATA.  x and w as above, the gradient zero but for one +-1 per (n, c) plane, at positions from the product over the window's
dims of {0, 1, 7, 8, O-9, O-8, O-2, O-1, O//2} (the 16-byte piece boundaries of 2-byte elements and both ends).  grad_w is then a sum of at most N taps on a
1/32 grid -- representable in bf16 -- and shows bit for bit whether that one position was counted once with the right corner weights.

tests/test_exact16_cases.py checks these claims on the oracle for every case, padding and shift.
"""
import functools
import itertools

import numpy as np
import torch

from oracle import oracle as O
from pooled16_cases import (DTYPES, assert_bits, assert_gw_entries, assert_ulp_close, exact_data, random_data, representable,  # noqa: F401
                            round16, ulp16)
from test_step_gpu import FLOOR16   # 8 fp32 ulps of the operands' unit scale: results that cancel to almost nothing

SWEEP = [(pad, active) for pad in range(5) for active in (0, 1)]
MAX_PROBE_CALLS = 12


def _per_pad(zeros, other):
    """an expected kernel that depends on the padding: `zeros` under padding 0, `other` under 1-4"""
    return (zeros, other, other, other, other)


# ---------------------------------------------------------------------------------------------------------------------
# The case table, contiguous tensors.  Per row: nd, shape, cut (rows [left, right] per dim as check_borders takes them; None: the
# whole input), note, and the kernel shiftnd_last_kernel() names under the default route for 2-byte elements:
#   bs / ba  shiftnd_backward, sparse / interpolating shift;  fs / fa  shiftnd_forward, sparse / interpolating shift
# -- a name, or five names (one per padding) where the host's rule reads the padding.  Each name cites the eligibility function that
# decides it (csrc/shiftnd_api.hip: forward_common / backward_planned walk them in the order given there).
#
# The rules the rows cite (es = 2; a piece = 16 bytes = 8 elements; kThreads = 256), in the order the host asks them:
#  backward_planned (csrc/shiftnd_api.hip):
#  [B1] sweep_backward_eligible && !plane_backward_eligible (shiftnd_plane.hip: S + O + 6 index-map entries beyond kMaxMapEntries,
#       or x rows that are not whole pieces) -> sweep_backward
#  [B2] !span_backward_eligible && (ragged_rows || cropped) && flat_backward_eligible (shiftnd_flat.hip flat_common_ok: 1-D / 2-D)
#       -> flat_backward
#  [B3] plane_backward_eligible -> plane_backward() (shiftnd_plane.hip), which asks in this order
#       (a) walk16_backward_eligible (shiftnd_walk.hip): walk16_geometry_ok -- 3-D, S0 >= 2, rows of whole pieces, no cut -- ->
#           walk_backward16 / walk_backward16_sparse; walk16_crop_geometry_ok -- a cut under zeros padding, every window dim >= 2,
#           the window at most two columns in, an even width -- -> walk_backward16_crop / _crop_sparse
#       (b) step_backward_eligible (shiftnd_step.hip step_backward_core): 2-D, no cut, rows of whole pieces, at most kThreads pieces
#           per row -> step_backward
#       (c) span_backward_eligible (shiftnd_span.hip; span_geometry_ok): 3-D cut volumes, every dim of volume and window >= 2 ->
#           crop_backward3; 2-D cut windows on x rows of whole pieces -> crop_backward; 1-D rows of at least 128 pieces -> row_backward
#       (d) slide_backward_eligible (shiftnd_slide.hip) -> slide_backward
#       (e) its own per-channel kernel -> plane_backward
#  [B4] small_backward_eligible (shiftnd_small.hip small_plan: 3-D, no cut, a volume of at most 16 KiB) -> small_plane_backward
#  [B5] plane_ragged_backward_eligible (shiftnd_plane.hip: 3-D, ragged rows) -> plane_backward_ragged
#  forward_common (csrc/shiftnd_api.hip):
#  [F1] step_forward_eligible (shiftnd_step_fwd.hip): the sparse shift, 2-D; 2-byte elements: zeros padding and output planes of at
#       least 16 KiB -> step_gather_forward_small   (no row of this table: every plane is smaller)
#  [F2] cropped && walk16_forward_eligible (shiftnd_walk.hip: crop_ok -- zeros padding, a 3-D cut volume, every window dim >= 2, an even
#       width) -> walk_forward16_crop / walk_forward16_crop_sparse
#  [F3] !step_forward_lds_eligible && span_forward_eligible (shiftnd_span.hip): crop_forward3_ok (3-D cut volumes, an even window
#       width) -> crop_*_forward3; crop_rows_forward_ok (2-D cut windows whose planes are not whole pieces, at least kThreads / 2
#       chunks per step) -> crop_*_forward_rows; crop_forward_ok && cropped (2-D windows whose planes are whole pieces) ->
#       crop_*_forward; 1-D source rows of whole pieces with at least 128 output chunks -> row_*_forward
#  [F4] ragged_rows && flat_forward_eligible (shiftnd_flat.hip) -> flat_gather_forward / flat_active_forward
#  [F5] walk16_forward_eligible (walk16_geometry_ok: 3-D interpolating, S0 >= 2, rows of whole pieces, no cut) -> walk_forward16
#  [F6] step_forward_lds_eligible (shiftnd_step_fwd.hip): 2-D, source and output rows of whole pieces, at most kThreads per row; the
#       interpolating shift -> step_active_forward; the sparse shift on output planes of at least 4 KiB -> step_gather_forward_lds
#  [F7] plane_forward_eligible (shiftnd_plane.hip; the interpolating shift: output rows of whole pieces) -> plane_forward():
#       slide_forward_eligible (shiftnd_slide.hip) -> slide_forward, else plane_active_forward; the sparse shift:
#       lds_gather_wanted -> plane_gather_forward_lds, else plane_gather_forward
#  [F8] cropped && flat_forward_eligible (what no chunk kernel took) -> flat_active_forward
#  [F9] small_forward_eligible (shiftnd_small.hip small_plan, as [B4]) -> small_plane_forward;
#       plane_ragged_forward_eligible (shiftnd_plane.hip) -> plane_active_forward_ragged
# ---------------------------------------------------------------------------------------------------------------------
CASES = []


def _case(nd, shape, cut, note, **routes):
    CASES.append((nd, tuple(shape), cut, note, routes))


# 2-D
_case(2, (2, 4, 18, 32), None, "rows of whole pieces (4); planes of 1152 bytes",
      bs="step_backward", ba="step_backward",            # [B3b]
      fs="plane_gather_forward_lds",                      # [F7]: below [F6]'s 4 KiB
      fa="step_active_forward")                           # [F6]
_case(2, (1, 4, 70, 64), None, "several steps per plane: partial sums from more than one workgroup (rows of 8 pieces, 32 rows per step)",
      bs="step_backward", ba="step_backward",            # [B3b]
      fs="step_gather_forward_lds",                       # [F6]: a plane of 8960 bytes
      fa="step_active_forward")                           # [F6]
_case(2, (2, 4, 9, 8), None, "rows of one piece",
      bs="step_backward", ba="step_backward", fs="plane_gather_forward_lds", fa="step_active_forward")   # [B3b], [F7], [F6]
_case(2, (3, 4, 1, 24), None, "a single row",
      bs="step_backward", ba="step_backward", fs="plane_gather_forward_lds", fa="step_active_forward")   # [B3b], [F7], [F6]
_case(2, (1, 4, 3, 2048), None, "rows of 256 chunks: the one-step family's limit (kThreads pieces per row)",
      bs="step_backward", ba="step_backward",            # [B3b]
      fs="step_gather_forward_lds", fa="step_active_forward")   # [F6]: a plane of 12 KiB
_case(2, (1, 4, 3, 2056), None, "rows of 257 chunks: beyond [B3b] and [F6]; [B3c] takes cut windows only, so the per-channel kernels",
      bs="plane_backward", ba="plane_backward",          # [B3e]
      fs="plane_gather_forward", fa="plane_active_forward")     # [F7]
_case(2, (2, 4, 20, 24), [[1, 1], [1, 1]], "window 18 x 22: output planes of 792 bytes, not whole pieces; 18 rows of 3 chunks do not "
      "fill half a workgroup, so crop_rows_forward_ok refuses (the next row reaches it)",
      bs="crop_backward", ba="crop_backward",            # [B3c]
      fs="plane_gather_forward",                          # [F7]
      fa="flat_active_forward")                           # [F8]: [F7] wants output rows of whole pieces
_case(2, (2, 4, 45, 24), [[1, 1], [1, 1]], "the row above moved by the least that reaches crop_*_forward3<.., ND = 2>: window 43 x 22, "
      "43 rows of 3 chunks = 129 >= kThreads / 2, planes of 1892 bytes",
      bs="crop_backward", ba="crop_backward",            # [B3c]
      fs="crop_gather_forward_rows", fa="crop_active_forward_rows")   # [F3] crop_rows_forward_ok
_case(2, (1, 4, 7, 112), [[1, 0], [2, 2]], "the route census' smallest cut shape: window 6 x 108, planes of 1296 bytes = 81 pieces",
      bs="crop_backward", ba="crop_backward",            # [B3c]
      fs="crop_gather_forward", fa="crop_active_forward")       # [F3] crop_forward_ok
_case(2, (2, 4, 7, 11), None, "ragged rows",
      bs="flat_backward", ba="flat_backward", fs="flat_gather_forward", fa="flat_active_forward")   # [B2], [F4]
_case(2, (3, 4, 112, 3), None, "ragged rows shorter than a piece",
      bs="flat_backward", ba="flat_backward", fs="flat_gather_forward", fa="flat_active_forward")   # [B2], [F4]
_case(2, (2, 4, 16, 62), [[1, 2], [0, 1]], "ragged rows under a window 13 x 61 (an odd width: span_geometry_ok's rag_ok refuses)",
      bs="flat_backward", ba="flat_backward", fs="flat_gather_forward", fa="flat_active_forward")   # [B2], [F4]
# 3-D
_case(3, (2, 4, 5, 4, 112), None, "the walk; the special weights go beyond the +-6 the five-dword window covers",
      bs="walk_backward16_sparse", ba="walk_backward16",  # [B3a]
      fs="plane_gather_forward_lds",                      # [F7]: [F6] wants planes of 4 KiB for the sparse shift (here 896 bytes)
      fa="walk_forward16")                                # [F5]
_case(3, (1, 4, 6, 7, 200), None, "the walk, rows of 25 pieces",
      bs="walk_backward16_sparse", ba="walk_backward16", fs="plane_gather_forward_lds", fa="walk_forward16")   # [B3a], [F7], [F5]
_case(3, (2, 4, 6, 9, 16), [[1, 1], [1, 1], [1, 1]], "window 4 x 7 x 14: the walk with the window inside under zeros padding only",
      bs=_per_pad("walk_backward16_crop_sparse", "crop_backward3"), ba=_per_pad("walk_backward16_crop", "crop_backward3"),   # [B3a] / [B3c]
      fs=_per_pad("walk_forward16_crop_sparse", "crop_gather_forward3"), fa=_per_pad("walk_forward16_crop", "crop_active_forward3"))  # [F2] / [F3]
_case(3, (1, 4, 5, 8, 24), [[0, 0], [0, 0], [3, 0]], "window 5 x 8 x 21: a left cut above 2 and an odd width -- not the cropped walk, "
      "and not crop_forward3_ok (an even width)",
      bs="crop_backward3", ba="crop_backward3",          # [B3c]
      fs="plane_gather_forward",                          # [F7]
      fa="plane_active_forward_ragged")                   # [F9]: [F7] wants output rows of whole pieces
_case(3, (1, 4, 1, 2, 200), None, "one plane: S0 = 1 is neither the walk's nor crop_backward3's",
      bs="slide_backward", ba="slide_backward",          # [B3d]
      fs="plane_gather_forward_lds", fa="slide_forward")        # [F7]
_case(3, (1, 4, 4, 7, 30), None, "ragged volume of 1680 bytes",
      bs="small_plane_backward", ba="small_plane_backward",     # [B4]
      fs="plane_gather_forward", fa="small_plane_forward")      # [F7], [F9]
_case(3, (1, 4, 16, 28, 28), None, "ragged volume of 25088 bytes, beyond small_plan's 16 KiB",
      bs="plane_backward_ragged", ba="plane_backward_ragged",   # [B5]
      fs="plane_gather_forward", fa="plane_active_forward_ragged")   # [F7], [F9]
_case(3, (1, 4, 2, 1, 8), None, "one row per plane, two planes: still the walk (S0 >= 2, S1 >= 1)",
      bs="walk_backward16_sparse", ba="walk_backward16", fs="plane_gather_forward_lds", fa="walk_forward16")   # [B3a], [F7], [F5]
# 1-D
_case(1, (2, 4, 2048), None, "long rows: 256 pieces",
      bs="row_backward", ba="row_backward", fs="row_gather_forward", fa="row_active_forward")   # [B3c], [F3]
_case(1, (2, 4, 1032), [[1, 1]], "a 1030-wide window on rows of 129 pieces: 128 whole output chunks",
      bs="row_backward", ba="row_backward", fs="row_gather_forward", fa="row_active_forward")   # [B3c], [F3]
_case(1, (2, 4, 40), None, "short rows of whole pieces: below [B3c]'s and [F3]'s 128 pieces",
      bs="plane_backward", ba="plane_backward", fs="plane_gather_forward_lds", fa="plane_active_forward")   # [B3e], [F7]
_case(1, (1, 4, 45), None, "ragged short rows",
      bs="flat_backward", ba="flat_backward", fs="flat_gather_forward", fa="flat_active_forward")   # [B2], [F4]
_case(1, (2, 4, 16384), None, "index maps beyond LDS: 2 x 16384 + 6 entries",
      bs="sweep_backward", ba="sweep_backward",          # [B1]
      fs="row_gather_forward", fa="row_active_forward")         # [F3]

# channels-last tensors (tests/test_exact16_cl_gpu.py): nd, shape, cut, note
CL_CASES = [
    (2, (1, 64, 32, 31), None, "odd rows of channel vectors"),
    (2, (3, 64, 7, 9), None, "a plane smaller than a band"),
    (2, (2, 64, 16, 14), [[1, 1], [1, 1]], "window 14 x 12"),
    (3, (2, 16, 4, 8, 19), None, "NDHWC, two lane groups of channels"),
    (3, (1, 16, 2, 112, 1), None, "NDHWC, rows of one element"),
]



def cl_expected(case, direction, active, grad_channels_last=True):
    """the kernel that serves a row of CL_CASES as it lies (2-byte elements, pixel lines of C * 2 bytes = whole 16-byte pieces):
    cl_tiled_forward_eligible / cl_tiled_backward_eligible (csrc/shiftnd_cl_tiled.hip: 2-D, rows > 3 resp. >= 5, a window in the
    last two dims) and cl_tiled3_backward_eligible (csrc/shiftnd_cl_tiled3.hip: NDHWC); the incoming gradient may be channels-last
    like the rest or NCHW / NCDHW-contiguous (the *_nchw_grad / *_ncdhw_grad forms)"""
    tail = "_3d" if case[0] == 3 else ""
    if direction == "f":
        return ("cl_tiled_active_forward" if active else "cl_tiled_forward") + tail
    return "cl_tiled_backward" + tail + ("" if grad_channels_last else ("_ncdhw_grad" if case[0] == 3 else "_nchw_grad"))


# what policy 4 (the channel-fastest kernels or fail) reaches with the tiled kernels switched off (knobs 20 = 0, 23 = 1):
# cl_forward_eligible / cl_backward_eligible (csrc/shiftnd_cl.hip)
CL_PLAIN = {"f0": "cl_gather_forward", "f1": "cl_active_forward", "b0": "cl_backward", "b1": "cl_backward"}
CL_SERVED = {"cl_tiled_backward", "cl_tiled_backward_nchw_grad", "cl_tiled_active_forward", "cl_tiled_backward_3d",
             "cl_tiled_backward_3d_ncdhw_grad", "cl_tiled_active_forward_3d", "cl_backward", "cl_active_forward"}

# "results never depend on the knobs": every case again, on the dense exact fixture, under each of these.  ("policy", v) sets the
# path policy, (knob, v) a tuning knob.  Knob 12: the values tests/test_slide_gpu.py uses (3: 2-D and 3-D problems slide; 0: none).
ALTERNATES = [("policy", 1), ("policy", 2), ("policy", 3), (32, 1), (27, 1), (24, 0), (12, 3), (12, 0),
              (35, 128), (35, 256), (35, 1024), (35, 2048), (38, 1), (38, 2)]
KNOB_DEFAULTS = {32: 0, 27: 0, 24: 1, 12: -1, 35: 0, 38: 0, 20: 1, 21: 0, 23: 0}   # (csrc/shiftnd_api.hip: kKnobDefault)

# the kernels the 16-bit runs of the table (default routes + alternates) must reach
SERVED_BACKWARD = {"step_backward", "crop_backward", "crop_backward3", "row_backward", "flat_backward", "walk_backward16",
                   "walk_backward16_sparse", "walk_backward16_crop", "walk_backward16_crop_sparse", "slide_backward",
                   "small_plane_backward", "band_plane_backward", "plane_backward_ragged", "sweep_backward", "strided_backward"}
SERVED_BACKWARD_ANY = [("plane_backward", "plane_backward_lds")]
SERVED_FORWARD = {"step_active_forward", "row_active_forward", "flat_active_forward", "walk_forward16", "walk_forward16_crop",
                  "slide_forward", "small_plane_forward", "band_plane_forward", "plane_active_forward", "plane_active_forward_ragged",
                  "sweep_active_forward", "strided_active_forward"}
SERVED_FORWARD_ANY = [("crop_active_forward", "crop_active_forward3", "crop_active_forward_rows")]


def group(nd, table=None):
    return [i for i, c in enumerate(CASES if table is None else table) if c[0] == nd]


def expected(case, direction, active, pad):
    """the kernel the table names for this call: direction "b" / "f" """
    name = case[4][direction + ("a" if active else "s")]
    return name if isinstance(name, str) else name[pad]


def geometry(case):
    """-> (borders: 6 ints, window shape [N, C, O...])"""
    nd, shape, cut = case[:3]
    b, new = O.check_borders(list(shape), cut, nd)
    return b, tuple(new)


def probe_gradients(case, seed):
    """-> a list of at most MAX_PROBE_CALLS gradients of the window's shape (fp32), each zero but for at most one +-1 per (n, c) plane.
    Positions: the product over the window's dims of {0, 1, 7, 8, O-9, O-8, O-2, O-1, O//2} (inside the window), shuffled with a fixed
    seed and dealt N * C per call (a call the list does not fill goes on from the list's head, so that every plane of every call
    holds its element); when there are more than MAX_PROBE_CALLS * N * C, all 2^nd corners stay and the rest is sampled."""
    _, win = geometry(case)
    N, C, dims = win[0], win[1], win[2:]
    coords = [sorted({v for v in (0, 1, 7, 8, o - 9, o - 8, o - 2, o - 1, o // 2) if 0 <= v < o}) for o in dims]
    positions = list(itertools.product(*coords))
    rs = np.random.RandomState(seed)
    room = MAX_PROBE_CALLS * N * C
    if len(positions) > room:
        corners = sorted(set(itertools.product(*[(0, o - 1) for o in dims])))
        rest = [p for p in positions if p not in set(corners)]
        keep = rs.choice(len(rest), room - len(corners), replace=False)
        positions = corners + [rest[i] for i in sorted(keep)]
    order = rs.permutation(len(positions))
    grads = []
    for at in range(0, len(order), N * C):
        g = np.zeros(win, np.float32)
        dealt = [order[(at + i) % len(order)] for i in range(N * C)]
        for slot, pi in enumerate(dealt):
            g[(slot // C, slot % C) + positions[pi]] = 1.0 if rs.randint(0, 2) else -1.0
        grads.append(g)
    return grads


@functools.lru_cache(maxsize=None)
def _inputs(table, ci, dt, kind):
    """-> x, w, [gradients]: one dense gradient for "exact" / "random", the probe calls' for "probe" """
    case = (CASES, CL_CASES)[table][ci]
    nd, shape = case[0], case[1]
    _, win = geometry(case)
    seed = 1000 * table + ci
    if kind == "random":
        x, w, g = random_data(np.random.RandomState(200 + seed), nd, shape, win, DTYPES[dt])
        return x, w, [g]
    x, w, g = exact_data(np.random.RandomState(100 + seed), nd, shape, win, turn=ci)
    if nd >= 2 or ci % 2 == 0:
        # the sparse shift rounds half to even: one dim of the drawn channel sits on a tie whose two roundings differ (the dim and the
        # tie rotate from case to case; the other dims keep their drawn quarters / halves; of the 1-D cases every other one)
        w[shape[1] - 1, ci % nd] = TIES[ci % len(TIES)]
    return x, w, ([g] if kind == "exact" else probe_gradients(case, 300 + seed))


TIES = (0.5, -2.5, -0.5, 2.5)   # rint: 0, -2, -0, 2; half away from zero: 1, -3, -1, 3


@functools.lru_cache(maxsize=None)
def _oracle(table, ci, dkey, kind, pad, active):
    """the oracle's results on the inputs of _inputs(table, ci, dkey, kind): the fp32 forward, and per gradient the fp32 backward and
    the fp64 backward of the widened inputs"""
    case = (CASES, CL_CASES)[table][ci]
    b, _ = geometry(case)
    x, w, grads = _inputs(table, ci, dkey, kind)
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    calls = []
    for g in grads:
        gx32, gw32 = O.backward(g, w, x, pad, active, b)
        gx64, gw64 = O.backward(g.astype(np.float64), w64, x64, pad, active, b)
        calls.append(dict(g=g, gx32=gx32, gw32=gw32, gx64=gx64, gw64=gw64))
    return O.forward(x, w, pad, active, b), calls


@functools.lru_cache(maxsize=None)
def reference(ci, dt, kind, pad, active, table=0):
    """the inputs and the oracle's results of CASES[ci] (table 1: CL_CASES) -- computed once, shared by every test that needs them and
    never written to.  kind: "exact", "probe" (the same inputs for every dtype) or "random" (narrowed to the dtype).
    -> dict(x, w, b, out, calls = [dict(g, gx, gw64, and the unrounded gx32, gw32, gx64), ...]): out = round16(O.forward(..)),
    gx = round16(O.backward(..)[0]), gw64 from the fp64 oracle on the widened inputs"""
    tdt = DTYPES[dt]
    case = (CASES, CL_CASES)[table][ci]
    dkey = dt if kind == "random" else ""
    x, w, _ = _inputs(table, ci, dkey, kind)
    out32, calls = _oracle(table, ci, dkey, kind, pad, active)
    r = dict(x=x, w=w, b=geometry(case)[0], out=round16(out32, tdt), calls=[dict(c, gx=round16(c["gx32"], tdt)) for c in calls])
    for v in [r["x"], r["w"], r["out"]] + [a for c in r["calls"] for a in c.values()]:
        v.setflags(write=False)
    return r


# ---------------------------------------------------------------------------------------------------------------------
# assertion functions: numpy arrays of widened values in, AssertionError out.  Shared by the GPU tests (on what the kernels return)
# and by the CPU self-checks (on the reference itself, and on mutated references, which they must reject).
# ---------------------------------------------------------------------------------------------------------------------
def check_forward(out, r, active, kind, tdt, what):
    """exact / probe data, the sparse shift (a copy) and fp32: bit for bit.  The interpolating shift on random 16-bit data: 1 ulp
    (+ FLOOR16) per element"""
    if kind != "random" or not active or tdt == torch.float32:
        assert_bits(out, r["out"], what + ("forward",))
    else:
        assert_ulp_close(out, r["out"], tdt, FLOOR16, what + ("forward",))


def check_backward(gx, gw, call, active, kind, tdt, what):
    """exact / probe data: grad_x and grad_w == round16(gw64) bit for bit (fp32: grad_w == gw64).  Random data: the sparse shift's
    grad_x bit for bit, the interpolating shift's within 1 ulp (+ FLOOR16), grad_w per entry (fp32: 1e-5 of the largest entry)"""
    if kind != "random":
        assert_bits(gx, call["gx"], what + ("grad_x",))
        assert_bits(gw, round16(call["gw64"].astype(np.float32), tdt), what + ("grad_w",))
        if tdt == torch.float32:
            assert np.array_equal(np.asarray(gw, np.float64), call["gw64"]), what + ("grad_w vs fp64",)
        return
    if not active or tdt == torch.float32:
        assert_bits(gx, call["gx"], what + ("grad_x",))
    else:
        assert_ulp_close(gx, call["gx"], tdt, FLOOR16, what + ("grad_x",))
    if tdt == torch.float32:
        err = np.abs(np.asarray(gw, np.float64) - call["gw64"]).max() / max(np.abs(call["gw64"]).max(), 1e-30)
        assert err < 1e-5, what + ("grad_w", err)
    else:
        assert_gw_entries(gw, call["gw64"], tdt, what + ("grad_w",))
