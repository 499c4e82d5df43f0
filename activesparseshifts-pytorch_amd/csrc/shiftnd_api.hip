// shiftnd_api.hip -- the C ABI declared in include/shiftnd_hip.h: argument validation, geometry
// normalisation and kernel-family selection.  No torch types, no allocation, no synchronisation.
#include <string.h>

#include <algorithm>
#include <array>

#include "shiftnd_common.hpp"
#include "shiftnd_launch.hpp"

using namespace shiftnd;

namespace {

thread_local int g_last_path = SHIFTND_PATH_NONE;
thread_local const char *g_last_kernel = "";
thread_local int g_cl3 = 0;     // knob 23: the direct NDHWC backward (shiftnd_cl_tiled3.hip) 0 automatic / 1 never / 2 whenever eligible
thread_local int g_policy = 0;  // 0 auto, 1 force strided, 2 plane kernels (or fail), 3 sweep kernels (or fail)

bool is_float_dtype(int dt) { return dt >= SHIFTND_F32 && dt <= SHIFTND_BF16; }
bool is_quant_dtype(int dt) { return dt >= SHIFTND_I8 && dt <= SHIFTND_I32; }

// Mixed precision (SHIFTND_WEIGHTS_F32 on p->dtype): fp32 weights and grad_w with fp16 / bf16 tensors.  `q` becomes the problem
// with the tensors' plain dtype -- all the routing below sees -- and `wkind` the element type of the weights (and of grad_w): q.dtype
// without the flag.  The flag on any other dtype is SHIFTND_ERR_UNSUPPORTED_DTYPE.
int split_dtype(const shiftnd_problem *p, shiftnd_problem &q, int &wkind) {
    q = *p;
    q.dtype = p->dtype & ~SHIFTND_WEIGHTS_F32;
    wkind = q.dtype;
    if (!(p->dtype & SHIFTND_WEIGHTS_F32)) return SHIFTND_OK;
    if (q.dtype != SHIFTND_F16 && q.dtype != SHIFTND_BF16) return SHIFTND_ERR_UNSUPPORTED_DTYPE;
    wkind = SHIFTND_F32;
    return SHIFTND_OK;
}

// Build the normalised 3-dim geometry: real spatial dim r (0..nd-1 = H, W, D) becomes normalised
// dim r + 3 - nd, so the innermost (contiguous) dim is always index 2 and leading dims have size 1.
int build_geometry(const shiftnd_problem *p, const int64_t *xs, const int64_t *os, const int64_t *gs, Geometry &g) {
    if (!p || p->ndim < 1 || p->ndim > 3 || p->padding_mode < 0 || p->padding_mode > 4) return SHIFTND_ERR_INVALID_ARGUMENT;
    memset(&g, 0, sizeof(g));
    g.nd = p->ndim;
    g.pad = p->padding_mode;
    g.active = p->active ? 1 : 0;
    g.N = p->sizes[0];
    g.C = p->sizes[1];
    if (g.N < 0 || g.C < 0) return SHIFTND_ERR_INVALID_ARGUMENT;
    const int lead = 3 - p->ndim;
    for (int d = 0; d < 3; ++d) {
        g.S[d] = 1;
        g.O[d] = 1;
        g.L[d] = 0;
        g.wcol[d] = -1;
    }
    g.xs[0] = xs[0];
    g.xs[1] = xs[1];
    g.os[0] = os[0];
    g.os[1] = os[1];
    if (gs) {
        g.gs[0] = gs[0];
        g.gs[1] = gs[1];
    }
    for (int r = 0; r < p->ndim; ++r) {
        const int d = r + lead;
        const int64_t size = p->sizes[2 + r];
        const int64_t l = p->borders[2 * r], rr = p->borders[2 * r + 1];
        if (size < 0) return SHIFTND_ERR_INVALID_ARGUMENT;
        if (size > 0 && (l < 0 || rr > size || rr <= l)) return SHIFTND_ERR_INVALID_ARGUMENT;
        g.S[d] = size;
        g.L[d] = l;
        g.O[d] = size > 0 ? rr - l : 0;
        g.wcol[d] = r;
        g.xs[2 + d] = xs[2 + r];
        g.os[2 + d] = os[2 + r];
        if (gs) g.gs[2 + d] = gs[2 + r];
    }
    return SHIFTND_OK;
}

thread_local int g_flat = 0;   // knob 27 (mirrors shiftnd_flat.hip's): 2 = the flat-stream kernels whenever eligible

// rows of the INPUT that are not whole 16-byte pieces: what the chunk kernels (step_*, crop_*, row_*: input rows of whole pieces, any
// window) do not take -- the flat-stream kernels' automatic share
bool ragged_rows(const Geometry &g, int dtype) {
    const int es = dtype_size(dtype);
    return (g.S[2] * es) % 16 != 0;
}

// ---------------------------------------------------------------------------------------------
// The tuning knobs (shiftnd_set_tuning) live in thread-local arrays next to the kernels they shape; this file keeps a
// thread-local shadow of every value so that a call can be planned under the DEFAULT knobs whatever the calling thread
// has set: shiftnd_backward_workspace_bytes returns the larger of the default plan's and the calling thread's plan's
// bytes, and a backward whose plan (under the calling thread's knobs) needs more than it was given runs under the
// default plan instead -- sizing on one thread and running on another can never end in WORKSPACE_TOO_SMALL.
// ---------------------------------------------------------------------------------------------
constexpr int kKnobs = 40;
constexpr std::array<int, kKnobs> kKnobDefault = {
    0, 128 * 1024, 4, 2, 1, 0, 1, 0,   //  0..7   plane kernels (g_tune)
    4, 512, 2, 256,                    //  8..11  sweep kernels
    -1, 0, 16, 0,                      // 12..15  sliding-window kernels
    1, 0, 0, 0,                        // 16..19  one-byte small-plane kernel
    1, 0, 1,                           // 20..22  LDS-tiled channels-last kernels
    0,                                 // 23      direct NDHWC backward
    1, 0, 0,                           // 24..26  small-plane / row-band kernels
    0,                                 // 27      flat-stream kernels
    1, 0, 0, 0,                        // 28..31  one-byte row kernel (31 unused)
    0, 0, 0, 0,                        // 32..35  one-step kernels
    0, 0,                              // 36..37  quantized pool
    0, 0};                             // 38      planes per workgroup of the walk kernels (39 unused)
thread_local std::array<int, kKnobs> g_knob = kKnobDefault;

void apply_knob(int knob, int value) {
    if (knob == 27) { g_flat = value; flat_set_tuning(value); }   // 27: the flat-stream kernels 0 automatic (ragged rows) / 1 never / 2 whenever eligible
    else if (knob >= 38) step_set_tuning(4 + knob - 38, value);  // 38: planes per workgroup of the walk kernels
    else if (knob >= 36) qpool_set_tuning(knob - 36, value);  // 36: quantized pool 0 automatic / 1 the element-per-thread kernel only
    else if (knob >= 32) step_set_tuning(knob - 32, value);  // 32: one-step backward 0 automatic / 1 never / 2 whenever eligible
    else if (knob >= 28) rows_set_tuning(knob - 28, value);  // 28: element sizes served (bit 0: 1 byte, bit 1: 2 bytes), 29: rows per band, 30: workgroups
    else if (knob >= 24) small_set_tuning(knob - 24, value);  // 24: small-plane kernels on / off, 25: planes per round, 26: rounds per workgroup
    else if (knob == 23) g_cl3 = value;
    else if (knob >= 20) cl_tiled_set_tuning(knob - 20, value);  // 20: LDS-tiled channels-last forward on / off, 21: rows per band
    else if (knob >= 16) bytes_set_tuning(knob - 16, value);  // 16: 1-byte small-plane kernel on / off, 17: planes per workgroup
    else if (knob >= 12) slide_set_tuning(knob - 12, value);  // 12: which problems slide, 13: workgroups wanted, 14: min rows per band
    else if (knob >= 8) sweep_set_tuning(knob - 8, value);  // 8/9: sweep forward K / max threads, 10/11: sweep backward
    else plane_set_tuning(knob, value);
}

bool knobs_touched() {
    for (int k = 0; k < kKnobs; ++k)
        if (g_knob[k] != kKnobDefault[k]) return true;
    return false;
}

// the default knobs for the lifetime of the object (this thread only), the thread's own back afterwards
struct DefaultKnobs {
    DefaultKnobs() {
        for (int k = 0; k < kKnobs; ++k)
            if (g_knob[k] != kKnobDefault[k]) apply_knob(k, kKnobDefault[k]);
    }
    ~DefaultKnobs() {
        for (int k = 0; k < kKnobs; ++k)
            if (g_knob[k] != kKnobDefault[k]) apply_knob(k, g_knob[k]);
    }
    DefaultKnobs(const DefaultKnobs &) = delete;
    DefaultKnobs &operator=(const DefaultKnobs &) = delete;
};

bool empty_geometry(const Geometry &g) { return g.N == 0 || g.C == 0 || g.S[0] * g.S[1] * g.S[2] == 0; }
bool empty_problem(const Geometry &g) { return empty_geometry(g) || g.O[0] * g.O[1] * g.O[2] == 0; }   // ... or its window is

int finish(int rc) {
    if (rc != SHIFTND_OK) return rc;
    return hipGetLastError() == hipSuccess ? SHIFTND_OK : SHIFTND_ERR_LAUNCH_FAILED;
}

int forward_common(const shiftnd_problem *p, const void *x, const int64_t *xs, const void *w, int wkind, int64_t wzp,
                   uint64_t fill, void *out, const int64_t *os, void *stream) {
    Geometry g;
    const int rc = build_geometry(p, xs, os, nullptr, g);
    if (rc != SHIFTND_OK) return rc;
    if (empty_problem(g)) {
        g_last_path = SHIFTND_PATH_EMPTY;
        return SHIFTND_OK;
    }
    if (!x || !w || !out) return SHIFTND_ERR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool can_sweep = sweep_forward_eligible(g, p->dtype, x, out);
    const bool can_plane = plane_forward_eligible(g, p->dtype, x, out);
    if ((g_policy == 2 && !can_plane) || (g_policy == 3 && !can_sweep)) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (g_policy != 4) {
        // automatic choice: the sweep kernels for planes of >= 32 KiB (their per-wave prologue is amortised over
        // several rows); small planes (e.g. 56x56 int8 = 3 KiB) go to the plane kernels, which walk many planes
        // of one channel per workgroup (measured on C4: 0.13 ms vs 0.33 ms)
        const int64_t out_plane_bytes = g.O[0] * g.O[1] * g.O[2] * dtype_size(p->dtype);
        // (interpolating problems keep the LDS-staged plane kernels whenever those take them: see DESIGN 3.14)
        const bool interpolating = g.active && p->dtype <= SHIFTND_BF16;
        const bool prefer_sweep = (out_plane_bytes >= 32 * 1024 && !interpolating && !(can_plane && plane_forward_lds_gather(g, p->dtype, x, out))) || !can_plane;
        if (g_policy == 0 && g_flat == 2 && wkind <= SHIFTND_BF16 && flat_forward_eligible(g, p->dtype, x, out)) {   // (knob 27 = 2: tests)
            g_last_path = SHIFTND_PATH_PLANE;
            return finish(flat_forward(g, p->dtype, x, w, wkind, out, st));
        }
        // 2-D sparse shift / quantized forward as a linear sweep of one-step workgroups
        if (g_policy == 0 && (g.nd == 2 || wkind <= SHIFTND_BF16) && step_forward_eligible(g, p->dtype, x, out)) {
            g_last_path = SHIFTND_PATH_SWEEP;
            return finish(step_forward(g, p->dtype, x, w, wkind, wzp, fill, out, st));
        }
        // cropped windows with ragged rows, 1-D rows of any length, ragged source rows (float tensors): one-step workgroups over
        // row spans -- what the aligned one-step forwards below do not take
        // cropped 16-bit volumes under zeros padding, interpolating: the walk through the planes with the window inside (round 6)
        if (g_policy == 0 && wkind <= SHIFTND_BF16 && cropped(g) && walk16_forward_eligible(g, p->dtype, x, out)) {
            g_last_path = SHIFTND_PATH_PLANE;
            return finish(walk16_forward(g, p->dtype, x, w, wkind, out, st));
        }
        if (g_policy == 0 && wkind <= SHIFTND_BF16 && !step_forward_lds_eligible(g, p->dtype, x, out) && span_forward_eligible(g, p->dtype, x, out)) {
            g_last_path = SHIFTND_PATH_PLANE;
            return finish(span_forward(g, p->dtype, x, w, wkind, out, st));
        }
        // rows that are not whole 16-byte pieces (14 x 14, 62 x 62, 222 x 222 ...; float tensors): one-step workgroups over the
        // tensor's flat chunk stream
        if (g_policy == 0 && wkind <= SHIFTND_BF16 && ragged_rows(g, p->dtype) && flat_forward_eligible(g, p->dtype, x, out)) {
            g_last_path = SHIFTND_PATH_PLANE;
            return finish(flat_forward(g, p->dtype, x, w, wkind, out, st));
        }
        // 1-byte (and, knob 28, 2-byte) rows of whole 16-byte pieces beyond the byte kernel's small planes: rows through LDS
        if (g_policy == 0 && !bytes_forward_eligible(g, p->dtype, x, out) && rows_forward_eligible(g, p->dtype, x, out)) {
            g_last_path = SHIFTND_PATH_PLANE;
            return finish(rows_forward(g, p->dtype, x, w, wkind, wzp, fill, out, st));
        }
        // rows that are not whole 16-byte pieces, planes above 16 KiB: the chunk kernels would move them element by
        // element (shiftnd_small.hip)
        if (g_policy == 0 && out_plane_bytes > 16 * 1024 && band_gather_forward_eligible(g, p->dtype)) {
            g_last_path = SHIFTND_PATH_PLANE;
            return finish(band_gather_forward(g, p->dtype, x, w, wkind, wzp, fill, out, st));
        }
        // 2-D sparse shift of 4- / 8-byte elements on planes of >= 32 KiB: the linear sweep of one-step workgroups
        // 3-D interpolating forward: a walk through the planes (one new plane per step, the other carried in registers)
        if (g_policy == 0 && wkind <= SHIFTND_BF16 && walk16_forward_eligible(g, p->dtype, x, out)) {
            g_last_path = SHIFTND_PATH_PLANE;
            return finish(walk16_forward(g, p->dtype, x, w, wkind, out, st));
        }
        if (g_policy == 0 && wkind <= SHIFTND_BF16 && walk_forward_eligible(g, p->dtype, x, out)) {
            g_last_path = SHIFTND_PATH_PLANE;
            return finish(walk_forward(g, p->dtype, x, w, wkind, out, st));
        }
        if (g_policy == 0 && wkind <= SHIFTND_BF16 && step_forward_lds_eligible(g, p->dtype, x, out)) {
            g_last_path = SHIFTND_PATH_PLANE;  // (LDS-staged, like the per-channel kernels it supersedes)
            return finish(step_forward_lds(g, p->dtype, x, w, wkind, fill, out, st));
        }
        if (can_sweep && (g_policy == 3 || (g_policy == 0 && prefer_sweep))) {
            g_last_path = SHIFTND_PATH_SWEEP;
            return finish(sweep_forward(g, p->dtype, x, w, wkind, wzp, fill, out, st));
        }
        if (can_plane && g_policy != 1) {
            g_last_path = SHIFTND_PATH_PLANE;
            return finish(plane_forward(g, p->dtype, x, w, wkind, wzp, fill, out, st));
        }
    }
    // windows no chunk kernel took (output planes that are not a whole number of 16-byte pieces): the flat chunk stream before the
    // one-thread-per-element kernels
    if (g_policy == 0 && wkind <= SHIFTND_BF16 && cropped(g) && flat_forward_eligible(g, p->dtype, x, out)) {
        g_last_path = SHIFTND_PATH_PLANE;
        return finish(flat_forward(g, p->dtype, x, w, wkind, out, st));
    }
    if (g_policy == 0 && small_forward_eligible(g, p->dtype)) {  // interpolating, rows not whole 16-byte pieces, small planes
        g_last_path = SHIFTND_PATH_PLANE;
        return finish(small_forward(g, p->dtype, x, w, wkind, out, st));
    }
    if (g_policy == 0 && wkind <= SHIFTND_BF16 && plane_ragged_forward_eligible(g, p->dtype, x, out)) {  // ... larger 3-D volumes: narrow chunks
        g_last_path = SHIFTND_PATH_PLANE;
        return finish(plane_ragged_forward(g, p->dtype, x, w, wkind, out, st));
    }
    if ((g_policy == 0 || g_policy == 4) && cl_tiled_forward_eligible(g, p->dtype, x, out)) {  // channels-last in, LDS-tiled
        g_last_path = SHIFTND_PATH_CL;
        return finish(cl_tiled_forward(g, p->dtype, x, w, wkind, wzp, fill, out, st));
    }
    if (g_policy == 4 && !cl_forward_eligible(g)) return SHIFTND_ERR_INVALID_ARGUMENT;
    if ((g_policy == 0 && cl_forward_preferred(g)) || g_policy == 4) {  // channels-last tensors: channel-fastest kernels
        g_last_path = SHIFTND_PATH_CL;
        return finish(cl_forward(g, p->dtype, x, w, wkind, wzp, fill, out, st));
    }
    // segment-major tensors (memory order N, S0, C, S1, S2: a temporal shift of [N*T, C, H, W]): plane copies at stream rate
    // instead of one element per thread; quantized tensors with their zero point as the fill
    if (g_policy == 0 && segment_forward_eligible(g, p->dtype, x, out)) {
        g_last_path = SHIFTND_PATH_PLANE;
        return finish(segment_forward(g, p->dtype, x, w, wkind, wzp, fill, out, st));
    }
    g_last_path = SHIFTND_PATH_STRIDED;
    return finish(strided_forward(g, p->dtype, x, w, wkind, wzp, fill, out, st));
}

// ---- SHIFTND_SHIFT_DIM0: the learnable temporal shift (shiftnd_tshift.hip).  `weights` / `grad_w` are [C] arrays and the shift acts
// on spatial dim 0 of dense segment-major tensors; the forward's sparse shift also takes dense channels-last tensors (the fixed
// temporal shift of an NHWC tensor, shiftnd_frames.hip), and so does shiftnd_forward_quantized.  No routing and no fallback: the call
// is served by the kernels of its layout or refused before anything is launched.
// SHIFTND_PER_CLIP beside the flag: `weights` / `grad_w` are [N, C] arrays, one row per clip -- the tshift kernels on segment-major
// tensors alone, out of place (tshift_forward_call / tshift_backward_call); every other form under the flag refuses the bit.
// SHIFTND_FRAMES beside the flag: the same problem on dense channels-last tensors, all of them (shiftnd_frames_learn.hip; the sparse
// forward is frames_forward).  The explicit bit takes every such call to the frame kernels -- also tensors that the segment-major
// layout describes as well -- or refuses it.
// SHIFTND_CLIP_FRAMES beside the flag: both at once under a bit of its own -- dense channels-last tensors, all of them, and [N, C]
// arrays; the frame kernels under a row stride (FramesParams::wrow), out of place, or the call is refused.  SHIFTND_FRAMES |
// SHIFTND_PER_CLIP stays refused, and so is the new bit beside either of them.
// -> the problem without the flag bits in `q`, the weights' type in `wkind`, whether the table is per clip ([N, C]: SHIFTND_PER_CLIP or
// SHIFTND_CLIP_FRAMES) and whether the frame kernels alone serve the call (SHIFTND_FRAMES or SHIFTND_CLIP_FRAMES)
int tshift_problem(const shiftnd_problem *p, shiftnd_problem &q, int &wkind, bool &per_clip, bool &frames) {
    shiftnd_problem r = *p;
    r.dtype = p->dtype & ~(SHIFTND_SHIFT_DIM0 | SHIFTND_PER_CLIP | SHIFTND_FRAMES | SHIFTND_CLIP_FRAMES);
    const bool clip_frames = (p->dtype & SHIFTND_CLIP_FRAMES) != 0;
    per_clip = (p->dtype & SHIFTND_PER_CLIP) != 0;
    frames = (p->dtype & SHIFTND_FRAMES) != 0;
    if (split_dtype(&r, q, wkind) != SHIFTND_OK || !is_float_dtype(q.dtype)) return SHIFTND_ERR_UNSUPPORTED_DTYPE;
    if (frames && per_clip) return SHIFTND_ERR_INVALID_ARGUMENT;   // (under SHIFTND_FRAMES the frame kernels take a [C] table alone)
    if (clip_frames && (frames || per_clip)) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (clip_frames) per_clip = frames = true;
    return SHIFTND_OK;
}

// the bound SHIFTND_PER_CLIP adds to tshift_geometry_ok's: the [N, C] table is indexed in 32 bits.  (Today N * S0 * C < 2^31 implies
// it; it is stated on its own because the kernels' table index and the reduction's entry count rest on it.)  SHIFTND_CLIP_FRAMES adds
// it to frames_learn_geometry_ok's, which does not imply it: the reduction counts the N * C entries in an int.
bool per_clip_table_ok(const Geometry &g) { return g.N * g.C < (1LL << 31); }   // (both factors are below 2^31 here: no overflow)

// the sizes a backward under the flag is served at, and its workspace: the two points where the workspace query and the backward
// call tell the layouts apart together
bool tshift_backward_sizes_ok(const Geometry &g, int dtype, bool per_clip, bool frames) {
    return (frames ? frames_learn_geometry_ok(g, dtype) : tshift_geometry_ok(g, dtype)) && (!per_clip || per_clip_table_ok(g));
}
size_t tshift_backward_workspace_for(const Geometry &g, int dtype, bool frames) {
    return frames ? frames_backward_workspace(g, dtype) : tshift_backward_workspace(g, dtype);
}

// ---- SHIFTND_SHIFT_DIM0 with out == x: the fixed temporal shift IN PLACE (shiftnd_inplace.hip).  `q`: the problem with its plain
// dtype, p->active as the caller gave it.  Served -- both dense layouts, at most 16 frames per clip, the sparse shift, the whole
// window, x and out under the same strides -- or refused before anything is launched: the out-of-place kernels would race.
int inplace_call(const shiftnd_problem &q, void *x, const int64_t *xs, const int64_t *os, const void *w, int wkind, int64_t wzp,
                 uint64_t fill, void *stream) {
    Geometry g;
    const int rc = build_geometry(&q, xs, os, nullptr, g);
    if (rc != SHIFTND_OK) return rc;
    for (int i = 0; i < 5; ++i)
        if (g.xs[i] != g.os[i]) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (!inplace_geometry_ok(g, q.dtype)) return SHIFTND_ERR_INVALID_ARGUMENT;   // (active, a cut window, S0 > 16, the sizes)
    if (empty_problem(g)) {
        g_last_path = SHIFTND_PATH_EMPTY;
        return SHIFTND_OK;
    }
    if (!w) return SHIFTND_ERR_INVALID_ARGUMENT;
    const int layout = inplace_layout(g, q.dtype, x, g.xs);
    if (layout == 0) return SHIFTND_ERR_INVALID_ARGUMENT;
    g_last_path = layout == 1 ? SHIFTND_PATH_PLANE : SHIFTND_PATH_CL;
    return finish(inplace_forward(g, q.dtype, layout, x, w, wkind, wzp, fill, static_cast<hipStream_t>(stream)));
}

// ---- SHIFTND_SHIFT_DIM0 | SHIFTND_STREAM: one step of the ONLINE temporal shift (shiftnd_stream.hip).  `q`: the problem with its
// plain dtype, p->active as the caller gave it; `flags`: the caller's dtype bits.  sizes {B, C, D, spatial...}; `state` (the entry
// points' x) carries the slot stride in the S0 place, `frame` (their out) is read and written too, its S0 stride is not looked at.
// Served -- both dense layouts, at most 15 slots, paddings 0 and 1 (the initial state IS the padding: no other mode can be
// causal), the whole window -- or refused before anything is launched.
int stream_call(const shiftnd_problem &q, int flags, void *state, const int64_t *xs, void *frame, const int64_t *os, const void *w,
                int wkind, int64_t wzp, void *stream) {
    if (flags & (SHIFTND_FRAMES | SHIFTND_PER_CLIP | SHIFTND_CLIP_FRAMES)) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (q.active || q.padding_mode > 1) return SHIFTND_ERR_INVALID_ARGUMENT;
    Geometry g;
    const int rc = build_geometry(&q, xs, os, nullptr, g);
    if (rc != SHIFTND_OK) return rc;
    if (!stream_geometry_ok(g, q.dtype)) return SHIFTND_ERR_INVALID_ARGUMENT;   // (a cut window, more than 15 slots, the sizes)
    if (empty_problem(g)) {   // (no slots: every shift clamps to 0)
        g_last_path = SHIFTND_PATH_EMPTY;
        return SHIFTND_OK;
    }
    if (!state || !frame || !w) return SHIFTND_ERR_INVALID_ARGUMENT;
    const int layout = stream_layout(g, q.dtype, state, g.xs, frame, g.os);
    if (layout == 0) return SHIFTND_ERR_INVALID_ARGUMENT;
    g_last_path = layout == 1 ? SHIFTND_PATH_PLANE : SHIFTND_PATH_CL;
    return finish(stream_forward(g, q.dtype, layout, state, frame, w, wkind, wzp, static_cast<hipStream_t>(stream)));
}

int tshift_forward_call(const shiftnd_problem *p, const void *x, const int64_t *xs, const void *w, void *out, const int64_t *os,
                        void *stream) {
    if (p->dtype & SHIFTND_STREAM) {   // the online step: x is the state, read AND written (the header says so)
        shiftnd_problem r = *p, q;
        int wkind;
        r.dtype = p->dtype & ~(SHIFTND_SHIFT_DIM0 | SHIFTND_STREAM | SHIFTND_FRAMES | SHIFTND_PER_CLIP | SHIFTND_CLIP_FRAMES);
        if (split_dtype(&r, q, wkind) != SHIFTND_OK || !is_float_dtype(q.dtype)) return SHIFTND_ERR_UNSUPPORTED_DTYPE;
        return stream_call(q, p->dtype, const_cast<void *>(x), xs, out, os, w, wkind, 0, stream);
    }
    if (out && out == x) {   // in place: its own kernel, or refused (SHIFTND_FRAMES asks for kernels that have no such form)
        shiftnd_problem q;
        int wkind;
        bool per_clip, frames;
        if (p->dtype & SHIFTND_FRAMES) return SHIFTND_ERR_INVALID_ARGUMENT;
        const int rc = tshift_problem(p, q, wkind, per_clip, frames);
        if (rc == SHIFTND_OK && per_clip) return SHIFTND_ERR_INVALID_ARGUMENT;   // (the in-place kernel takes a [C] table alone; SHIFTND_CLIP_FRAMES too)
        return rc != SHIFTND_OK ? rc : inplace_call(q, out, xs, os, w, wkind, 0, 0ull, stream);
    }
    shiftnd_problem q;
    int wkind;
    bool per_clip, frames;
    int rc = tshift_problem(p, q, wkind, per_clip, frames);
    if (rc != SHIFTND_OK) return rc;
    Geometry g;
    rc = build_geometry(&q, xs, os, nullptr, g);
    if (rc != SHIFTND_OK) return rc;
    // without SHIFTND_FRAMES two layouts are served: segment-major (the tshift kernels, sparse and interpolating) and, for the sparse
    // shift, channels-last (shiftnd_frames.hip: frames_geometry_ok refuses `active`).  A tensor both describe (planes or channels of
    // size 1) stays with the tshift kernels.  A per-clip table: the tshift kernels alone.  With the bit: the frame kernels alone (and
    // under SHIFTND_CLIP_FRAMES the frame kernels alone with a per-clip table)
    const bool segment_sizes = !frames && tshift_geometry_ok(g, q.dtype) && (!per_clip || per_clip_table_ok(g));
    const bool frames_sizes = frames ? frames_learn_geometry_ok(g, q.dtype) && (!per_clip || per_clip_table_ok(g))
                                     : !per_clip && frames_geometry_ok(g, q.dtype);
    if (!segment_sizes && !frames_sizes) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (empty_geometry(g)) {   // (empty_problem's answer: every *_geometry_ok above refuses a cut window)
        g_last_path = SHIFTND_PATH_EMPTY;
        return SHIFTND_OK;
    }
    if (!x || !w || !out) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (segment_sizes && tshift_tensor_ok(g, q.dtype, x, g.xs) && tshift_tensor_ok(g, q.dtype, out, g.os)) {
        g_last_path = SHIFTND_PATH_PLANE;
        return finish(tshift_forward(g, q.dtype, x, w, wkind, per_clip, out, static_cast<hipStream_t>(stream)));
    }
    if (frames_sizes && frames_tensor_ok(g, q.dtype, x, g.xs) && frames_tensor_ok(g, q.dtype, out, g.os)) {
        g_last_path = SHIFTND_PATH_CL;
        if (g.active) return finish(frames_active_forward(g, q.dtype, x, w, wkind, per_clip, out, static_cast<hipStream_t>(stream)));   // (SHIFTND_FRAMES / SHIFTND_CLIP_FRAMES only)
        return finish(frames_forward(g, q.dtype, x, w, wkind, 0, 0ull, per_clip, out, static_cast<hipStream_t>(stream)));
    }
    return SHIFTND_ERR_INVALID_ARGUMENT;
}

// shiftnd_forward_quantized under the flag: the channels-last layout alone (I8 / U8 / I32 tensors, an integer [C] table)
int frames_quantized_call(const shiftnd_problem *p, const void *x, const int64_t *xs, const void *wq, int wq_dtype, int64_t wzp,
                          uint64_t fill, void *out, const int64_t *os, void *stream) {
    shiftnd_problem q = *p;
    q.dtype = p->dtype & ~SHIFTND_SHIFT_DIM0;
    q.active = 0;
    Geometry g;
    const int rc = build_geometry(&q, xs, os, nullptr, g);
    if (rc != SHIFTND_OK) return rc;
    if (!frames_geometry_ok(g, q.dtype)) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (empty_problem(g)) {
        g_last_path = SHIFTND_PATH_EMPTY;
        return SHIFTND_OK;
    }
    if (!x || !wq || !out) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (!frames_tensor_ok(g, q.dtype, x, g.xs) || !frames_tensor_ok(g, q.dtype, out, g.os)) return SHIFTND_ERR_INVALID_ARGUMENT;
    g_last_path = SHIFTND_PATH_CL;
    return finish(frames_forward(g, q.dtype, x, wq, wq_dtype, wzp, fill, false, out, static_cast<hipStream_t>(stream)));
}

// shiftnd_forward_quantized under the flag with an fp32 table: the quantized INTERPOLATING temporal shift (shiftnd_tshift_quant.hip) --
// I8 / U8 / I32 segment-major tensors, out of place, p->active == 1, the whole window, `wq` the fp32 [C] table (w_zero_point 0).  Served
// by its one kernel or refused before anything is launched: no other flag bit, no channels-last view; p->active == 0 stays an
// unsupported table type (the sparse shift is the integer table's call).  With SHIFTND_FRAMES beside the flag (and no further bit)
// the same call on dense channels-last tensors, served by frames_forward_quantized (shiftnd_frames_quant.hip) or
// refused: segment-major tensors have no route under the pair
int tshift_quantized_call(const shiftnd_problem *p, const void *x, const int64_t *xs, const void *wq, int64_t wzp, int64_t xzp, void *out,
                          const int64_t *os, void *stream) {
    const int flags = SHIFTND_WEIGHTS_F32 | SHIFTND_SHIFT_DIM0 | SHIFTND_FRAMES | SHIFTND_PER_CLIP | SHIFTND_STREAM | SHIFTND_CLIP_FRAMES |
                      SHIFTND_INTERLACE | SHIFTND_INTERLACE_FRAMES;
    shiftnd_problem q = *p;
    q.dtype = p->dtype & ~flags;
    if (!is_quant_dtype(q.dtype)) return SHIFTND_ERR_UNSUPPORTED_DTYPE;   // (the flag with a float dtype: no quantized dtype)
    // the sparse shift has no float table: what such a call was answered before this form existed (tests/test_temporal_cl_cpu.py pins it)
    if (!p->active) return SHIFTND_ERR_UNSUPPORTED_DTYPE;
    // SHIFTND_FRAMES beside the flag: the same problem on dense channels-last tensors, both of them (shiftnd_frames_quant.hip).  The
    // explicit bit is required -- channels-last views under the flag alone stay refused -- and takes every such call to that kernel
    const bool frames = (p->dtype & flags) == (SHIFTND_SHIFT_DIM0 | SHIFTND_FRAMES);
    if (((p->dtype & flags) != SHIFTND_SHIFT_DIM0 && !frames) || wzp != 0) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (out && out == x) return SHIFTND_ERR_INVALID_ARGUMENT;   // (x and out are __restrict__: there is no in-place form)
    Geometry g;
    const int rc = build_geometry(&q, xs, os, nullptr, g);
    if (rc != SHIFTND_OK) return rc;
    if (!(frames ? frames_quantized_geometry_ok(g, q.dtype, xzp) : tshift_quantized_geometry_ok(g, q.dtype, xzp)))
        return SHIFTND_ERR_INVALID_ARGUMENT;   // (a cut window, ndim 1, the sizes, the zero point)
    if (empty_geometry(g)) {
        g_last_path = SHIFTND_PATH_EMPTY;
        return SHIFTND_OK;
    }
    if (!x || !wq || !out || !aligned_to(wq, sizeof(float))) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (frames) {
        if (!frames_tensor_ok(g, q.dtype, x, g.xs) || !frames_tensor_ok(g, q.dtype, out, g.os)) return SHIFTND_ERR_INVALID_ARGUMENT;
        g_last_path = SHIFTND_PATH_CL;
        return finish(frames_quantized_forward(g, q.dtype, x, wq, xzp, out, static_cast<hipStream_t>(stream)));
    }
    if (!tshift_tensor_ok(g, q.dtype, x, g.xs) || !tshift_tensor_ok(g, q.dtype, out, g.os)) return SHIFTND_ERR_INVALID_ARGUMENT;
    g_last_path = SHIFTND_PATH_PLANE;
    return finish(tshift_quantized_forward(g, q.dtype, x, wq, xzp, out, static_cast<hipStream_t>(stream)));
}

// shiftnd_forward_quantized under the flag with an fp32 table and SHIFTND_PER_CLIP or SHIFTND_INTERLACE beside it: the quantized
// per-clip temporal shift (`wq` the fp32 [N, C] table) and quantized temporal interlacing (`wq` the packed fp32 table, N * C offsets
// followed by N * S0 * C scales), shiftnd_interlace_quant.hip -- I8 / U8 / I32 segment-major tensors, out of place, the
// whole window, p->active 0 or 1 (the sparse shift rounds the offset half to even and still applies the scale), w_zero_point 0.
// Served by its one kernel or refused before anything is launched: exactly one of the two bits and no further one, no channels-last
// view
int interlace_quantized_call(const shiftnd_problem *p, const void *x, const int64_t *xs, const void *wq, int64_t wzp, int64_t xzp,
                             void *out, const int64_t *os, void *stream) {
    const int flags = SHIFTND_WEIGHTS_F32 | SHIFTND_SHIFT_DIM0 | SHIFTND_FRAMES | SHIFTND_PER_CLIP | SHIFTND_STREAM | SHIFTND_CLIP_FRAMES |
                      SHIFTND_INTERLACE | SHIFTND_INTERLACE_FRAMES;
    shiftnd_problem q = *p;
    q.dtype = p->dtype & ~flags;
    if (!is_quant_dtype(q.dtype)) return SHIFTND_ERR_UNSUPPORTED_DTYPE;   // (the bits with a float dtype: no quantized dtype)
    const int bits = p->dtype & flags;
    const bool scaled = bits == (SHIFTND_SHIFT_DIM0 | SHIFTND_INTERLACE);
    if ((!scaled && bits != (SHIFTND_SHIFT_DIM0 | SHIFTND_PER_CLIP)) || wzp != 0) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (out && out == x) return SHIFTND_ERR_INVALID_ARGUMENT;   // (x and out are __restrict__: there is no in-place form)
    Geometry g;
    const int rc = build_geometry(&q, xs, os, nullptr, g);
    if (rc != SHIFTND_OK) return rc;
    // a cut window, ndim 1, the sizes (N * S0 * C < 2^31 bounds the offsets' and the scales' index), the zero point
    if (!tshift_quantized_geometry_ok(g, q.dtype, xzp) || !per_clip_table_ok(g)) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (empty_geometry(g)) {
        g_last_path = SHIFTND_PATH_EMPTY;
        return SHIFTND_OK;
    }
    if (!x || !wq || !out || !aligned_to(wq, sizeof(float))) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (!tshift_tensor_ok(g, q.dtype, x, g.xs) || !tshift_tensor_ok(g, q.dtype, out, g.os)) return SHIFTND_ERR_INVALID_ARGUMENT;
    g_last_path = SHIFTND_PATH_PLANE;
    return finish(tinterlace_quantized_forward(g, q.dtype, x, wq, scaled, xzp, out, static_cast<hipStream_t>(stream)));
}

// the backward under the flag, both layouts: `frames` (SHIFTND_FRAMES) picks the sizes, the tensor check, the workspace and the kernels
int tshift_backward_call(const shiftnd_problem *p, const void *go, const int64_t *gos, const void *x, const int64_t *xs, const void *w,
                         void *gx, const int64_t *gxs, void *gw, void *workspace, size_t workspace_bytes, void *stream) {
    shiftnd_problem q;
    int wkind;
    bool per_clip, frames;
    int rc = tshift_problem(p, q, wkind, per_clip, frames);
    if (rc != SHIFTND_OK) return rc;
    if (!x || !xs || !gw) return SHIFTND_ERR_INVALID_ARGUMENT;   // (the x == NULL form does not exist under the flag)
    Geometry g;
    rc = build_geometry(&q, xs, gos, gxs, g);
    if (rc != SHIFTND_OK) return rc;
    if (!tshift_backward_sizes_ok(g, q.dtype, per_clip, frames)) return SHIFTND_ERR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (empty_geometry(g)) {
        g_last_path = SHIFTND_PATH_EMPTY;
        const size_t entries = static_cast<size_t>(per_clip ? g.N * g.C : g.C);
        if (entries > 0 && hipMemsetAsync(gw, 0, entries * dtype_size(wkind), st) != hipSuccess) return SHIFTND_ERR_LAUNCH_FAILED;
        return SHIFTND_OK;
    }
    if (!go || !w || !gx || !workspace) return SHIFTND_ERR_INVALID_ARGUMENT;
    const auto tensor_ok = [&](const void *t, const int64_t *strides) {
        return frames ? frames_tensor_ok(g, q.dtype, t, strides) : tshift_tensor_ok(g, q.dtype, t, strides);
    };
    if (!tensor_ok(go, g.os) || !tensor_ok(x, g.xs) || !tensor_ok(gx, g.gs)) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (tshift_backward_workspace_for(g, q.dtype, frames) > workspace_bytes) return SHIFTND_ERR_WORKSPACE_TOO_SMALL;
    g_last_path = frames ? SHIFTND_PATH_CL : SHIFTND_PATH_PLANE;
    if (frames) return finish(frames_backward(g, q.dtype, go, x, w, wkind, per_clip, gx, gw, workspace, st));
    return finish(tshift_backward(g, q.dtype, go, x, w, wkind, per_clip, gx, gw, workspace, st));
}

// ---- SHIFTND_SHIFT_DIM0 | SHIFTND_INTERLACE: temporal interlacing (shiftnd_interlace.hip) -- the per-clip shift times a scale per
// (n, t, c) plane.  `weights` / `grad_w` are ONE packed array each, [N, C] offsets followed by [N, S0, C] scales.  Segment-major
// tensors alone, out of place, under the geometry and limits of SHIFTND_PER_CLIP; served by its own kernels or refused before
// anything is launched.  No other form under SHIFTND_SHIFT_DIM0 combines with the bit.
// -> the problem without the flag bits in `q`, the weights' type in `wkind`
int interlace_problem(const shiftnd_problem *p, shiftnd_problem &q, int &wkind) {
    constexpr int others = SHIFTND_FRAMES | SHIFTND_PER_CLIP | SHIFTND_STREAM | SHIFTND_CLIP_FRAMES;
    shiftnd_problem r = *p;
    r.dtype = p->dtype & ~(SHIFTND_SHIFT_DIM0 | SHIFTND_INTERLACE | others);
    if (split_dtype(&r, q, wkind) != SHIFTND_OK || !is_float_dtype(q.dtype)) return SHIFTND_ERR_UNSUPPORTED_DTYPE;
    return (p->dtype & others) ? SHIFTND_ERR_INVALID_ARGUMENT : SHIFTND_OK;
}

// tshift_geometry_ok's sizes, the [N, C] offsets indexed in 32 bits, and N * S0 * C < 2^31: the scales' index and the entry count of
// their reduction.  (tshift_geometry_ok implies the last two today; they are stated because the kernels rest on them.)
bool interlace_sizes_ok(const Geometry &g, int dtype) {
    if (!tshift_geometry_ok(g, dtype) || !per_clip_table_ok(g)) return false;
    return g.N * g.S[3 - g.nd] * g.C < (1LL << 31);   // (N * S0 and C are below 2^31 here: no overflow)
}

int interlace_forward_call(const shiftnd_problem *p, const void *x, const int64_t *xs, const void *w, void *out, const int64_t *os,
                           void *stream) {
    shiftnd_problem q;
    int wkind;
    int rc = interlace_problem(p, q, wkind);
    if (rc != SHIFTND_OK) return rc;
    if (out && out == x) return SHIFTND_ERR_INVALID_ARGUMENT;   // (the in-place form takes a [C] table alone)
    Geometry g;
    rc = build_geometry(&q, xs, os, nullptr, g);
    if (rc != SHIFTND_OK) return rc;
    if (!interlace_sizes_ok(g, q.dtype)) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (empty_geometry(g)) {
        g_last_path = SHIFTND_PATH_EMPTY;
        return SHIFTND_OK;
    }
    if (!x || !w || !out) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (!tshift_tensor_ok(g, q.dtype, x, g.xs) || !tshift_tensor_ok(g, q.dtype, out, g.os)) return SHIFTND_ERR_INVALID_ARGUMENT;
    g_last_path = SHIFTND_PATH_PLANE;
    return finish(tinterlace_forward(g, q.dtype, x, w, wkind, out, static_cast<hipStream_t>(stream)));
}

int interlace_backward_call(const shiftnd_problem *p, const void *go, const int64_t *gos, const void *x, const int64_t *xs,
                            const void *w, void *gx, const int64_t *gxs, void *gw, void *workspace, size_t workspace_bytes,
                            void *stream) {
    shiftnd_problem q;
    int wkind;
    int rc = interlace_problem(p, q, wkind);
    if (rc != SHIFTND_OK) return rc;
    if (!x || !xs || !gw) return SHIFTND_ERR_INVALID_ARGUMENT;   // (the x == NULL form does not exist under the flag)
    Geometry g;
    rc = build_geometry(&q, xs, gos, gxs, g);
    if (rc != SHIFTND_OK) return rc;
    if (!interlace_sizes_ok(g, q.dtype)) return SHIFTND_ERR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (empty_geometry(g)) {
        g_last_path = SHIFTND_PATH_EMPTY;
        const size_t entries = static_cast<size_t>(g.N * g.C * (1 + g.S[3 - g.nd]));   // offsets and scales
        if (entries > 0 && hipMemsetAsync(gw, 0, entries * dtype_size(wkind), st) != hipSuccess) return SHIFTND_ERR_LAUNCH_FAILED;
        return SHIFTND_OK;
    }
    if (!go || !w || !gx || !workspace) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (!tshift_tensor_ok(g, q.dtype, go, g.os) || !tshift_tensor_ok(g, q.dtype, x, g.xs) || !tshift_tensor_ok(g, q.dtype, gx, g.gs))
        return SHIFTND_ERR_INVALID_ARGUMENT;
    if (tinterlace_backward_workspace(g, q.dtype) > workspace_bytes) return SHIFTND_ERR_WORKSPACE_TOO_SMALL;
    g_last_path = SHIFTND_PATH_PLANE;
    return finish(tinterlace_backward(g, q.dtype, go, x, w, wkind, gx, gw, workspace, st));
}

size_t interlace_workspace_bytes(const shiftnd_problem *p) {
    const int64_t unit[5] = {0, 0, 0, 0, 0};
    shiftnd_problem q;
    int wkind;
    Geometry g;
    if (interlace_problem(p, q, wkind) != SHIFTND_OK || build_geometry(&q, unit, unit, unit, g) != SHIFTND_OK) return 0;
    if (!interlace_sizes_ok(g, q.dtype)) return 0;
    return empty_geometry(g) ? sizeof(double) : tinterlace_backward_workspace(g, q.dtype);
}

// ---- SHIFTND_SHIFT_DIM0 | SHIFTND_INTERLACE_FRAMES: temporal interlacing of dense channels-last tensors, all of them
// (shiftnd_interlace_frames.hip) -- SHIFTND_INTERLACE's problem and packed table on SHIFTND_FRAMES' layout, out of place; served by its
// own kernels or refused before anything is launched.  No other bit of the family combines with it, SHIFTND_INTERLACE included.
// -> the problem without the flag bits in `q`, the weights' type in `wkind`
int interlace_frames_problem(const shiftnd_problem *p, shiftnd_problem &q, int &wkind) {
    constexpr int others = SHIFTND_FRAMES | SHIFTND_PER_CLIP | SHIFTND_STREAM | SHIFTND_CLIP_FRAMES | SHIFTND_INTERLACE;
    shiftnd_problem r = *p;
    r.dtype = p->dtype & ~(SHIFTND_SHIFT_DIM0 | SHIFTND_INTERLACE_FRAMES | others);
    if (split_dtype(&r, q, wkind) != SHIFTND_OK || !is_float_dtype(q.dtype)) return SHIFTND_ERR_UNSUPPORTED_DTYPE;
    return (p->dtype & others) ? SHIFTND_ERR_INVALID_ARGUMENT : SHIFTND_OK;
}

int interlace_frames_forward_call(const shiftnd_problem *p, const void *x, const int64_t *xs, const void *w, void *out,
                                  const int64_t *os, void *stream) {
    shiftnd_problem q;
    int wkind;
    int rc = interlace_frames_problem(p, q, wkind);
    if (rc != SHIFTND_OK) return rc;
    if (out && out == x) return SHIFTND_ERR_INVALID_ARGUMENT;   // (no in-place form)
    Geometry g;
    rc = build_geometry(&q, xs, os, nullptr, g);
    if (rc != SHIFTND_OK) return rc;
    if (!frames_interlace_geometry_ok(g, q.dtype)) return SHIFTND_ERR_INVALID_ARGUMENT;   // (ndim 1, a cut window, the sizes)
    if (empty_geometry(g)) {
        g_last_path = SHIFTND_PATH_EMPTY;
        return SHIFTND_OK;
    }
    if (!x || !w || !out) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (!frames_tensor_ok(g, q.dtype, x, g.xs) || !frames_tensor_ok(g, q.dtype, out, g.os)) return SHIFTND_ERR_INVALID_ARGUMENT;
    g_last_path = SHIFTND_PATH_CL;
    return finish(frames_interlace_forward(g, q.dtype, x, w, wkind, out, static_cast<hipStream_t>(stream)));
}

int interlace_frames_backward_call(const shiftnd_problem *p, const void *go, const int64_t *gos, const void *x, const int64_t *xs,
                                   const void *w, void *gx, const int64_t *gxs, void *gw, void *workspace, size_t workspace_bytes,
                                   void *stream) {
    shiftnd_problem q;
    int wkind;
    int rc = interlace_frames_problem(p, q, wkind);
    if (rc != SHIFTND_OK) return rc;
    if (!x || !xs || !gw) return SHIFTND_ERR_INVALID_ARGUMENT;   // (the x == NULL form does not exist under the flag)
    Geometry g;
    rc = build_geometry(&q, xs, gos, gxs, g);
    if (rc != SHIFTND_OK) return rc;
    if (!frames_interlace_geometry_ok(g, q.dtype)) return SHIFTND_ERR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (empty_geometry(g)) {
        g_last_path = SHIFTND_PATH_EMPTY;
        const size_t entries = static_cast<size_t>(g.N * g.C * (1 + g.S[3 - g.nd]));   // offsets and scales
        if (entries > 0 && hipMemsetAsync(gw, 0, entries * dtype_size(wkind), st) != hipSuccess) return SHIFTND_ERR_LAUNCH_FAILED;
        return SHIFTND_OK;
    }
    if (!go || !w || !gx || !workspace) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (!frames_tensor_ok(g, q.dtype, go, g.os) || !frames_tensor_ok(g, q.dtype, x, g.xs) || !frames_tensor_ok(g, q.dtype, gx, g.gs))
        return SHIFTND_ERR_INVALID_ARGUMENT;
    if (frames_interlace_backward_workspace(g, q.dtype) > workspace_bytes) return SHIFTND_ERR_WORKSPACE_TOO_SMALL;
    g_last_path = SHIFTND_PATH_CL;
    return finish(frames_interlace_backward(g, q.dtype, go, x, w, wkind, gx, gw, workspace, st));
}

size_t interlace_frames_workspace_bytes(const shiftnd_problem *p) {
    const int64_t unit[5] = {0, 0, 0, 0, 0};
    shiftnd_problem q;
    int wkind;
    Geometry g;
    if (interlace_frames_problem(p, q, wkind) != SHIFTND_OK || build_geometry(&q, unit, unit, unit, g) != SHIFTND_OK) return 0;
    if (!frames_interlace_geometry_ok(g, q.dtype)) return 0;
    return empty_geometry(g) ? sizeof(double) : frames_interlace_backward_workspace(g, q.dtype);
}

}  // namespace

namespace shiftnd {
void note_kernel(const char *name) { g_last_kernel = name; }
const char *last_kernel() { return g_last_kernel; }
}  // namespace shiftnd

extern "C" {

const char *shiftnd_last_kernel(void) { return g_last_kernel; }

int shiftnd_abi_version(void) { return SHIFTND_ABI_VERSION; }

const char *shiftnd_status_string(int status) {
    switch (status) {
    case SHIFTND_OK: return "ok";
    case SHIFTND_ERR_INVALID_ARGUMENT: return "invalid argument";
    case SHIFTND_ERR_UNSUPPORTED_DTYPE: return "unsupported dtype";
    case SHIFTND_ERR_WORKSPACE_TOO_SMALL: return "workspace too small";
    case SHIFTND_ERR_LAUNCH_FAILED: return "kernel launch failed";
    case SHIFTND_ERR_TOO_LARGE: return "problem too large";
    case SHIFTND_ERR_NOT_FUSED: return "geometry not served by the fused kernels";
    default: return "unknown status";
    }
}

int shiftnd_last_path(void) { return g_last_path; }

void shiftnd_set_path_policy(int policy) { g_policy = policy; }

void shiftnd_set_tuning(int knob, int value) {
    if (knob < 0 || knob >= kKnobs) return;
    g_knob[knob] = value;
    apply_knob(knob, value);
}

int shiftnd_debug_map(int64_t p, int64_t shift, int64_t len, int padding_mode) {
    return sweep_debug_map(p, shift, len, padding_mode);
}

// check_borders, ops/shifts.cpp:93-135 (host arithmetic only)
int shiftnd_check_borders(const int64_t *sizes, int nsizes, const int32_t *user, int ndim, int32_t borders[6],
                          int64_t *new_sizes) {
    if (!sizes || !borders || !new_sizes || ndim < 1 || nsizes < ndim + 1) return SHIFTND_ERR_INVALID_ARGUMENT;
    const int shift = ((ndim + 1) == nsizes) ? 1 : 2;
    const int hdim = 3;
    const int dims = ndim < hdim ? ndim : hdim;
    if (shift + dims > nsizes) return SHIFTND_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < hdim; ++i) {
        borders[2 * i] = 0;
        borders[2 * i + 1] = (i + 1 > ndim) ? 1 : static_cast<int32_t>(sizes[i + shift]);
    }
    if (user) {
        for (int i = 0; i < dims; ++i) {
            const int32_t size = static_cast<int32_t>(sizes[i + shift]);
            int32_t l = user[2 * i];
            int32_t r = borders[2 * i + 1] - user[2 * i + 1];
            if (r - l < 1) r = l + 1;          // degenerate window -> one element wide
            if (l == size) { l = size - 1; r = l + 1; }
            if (r == 0) { l = 0; r = 1; }
            if (l < 0) l = 0;
            if (r > size) r = size;
            borders[2 * i] = l;
            borders[2 * i + 1] = r;
        }
    }
    for (int i = 0; i < shift; ++i) new_sizes[i] = sizes[i];
    for (int i = 0; i < dims; ++i) new_sizes[i + shift] = static_cast<int64_t>(borders[2 * i + 1] - borders[2 * i]);
    return SHIFTND_OK;
}

int shiftnd_forward_serves_channels_last(const shiftnd_problem *p, const void *x, const int64_t x_strides[5], const void *out,
                                         const int64_t out_strides[5]) {
    if (!p || !x_strides || !out_strides || g_policy != 0) return 0;
    shiftnd_problem q;
    int wkind;
    if (split_dtype(p, q, wkind) != SHIFTND_OK) return 0;
    p = &q;   // (the weights' type changes no route: the same answer with and without SHIFTND_WEIGHTS_F32)
    Geometry g;
    if (build_geometry(p, x_strides, out_strides, nullptr, g) != SHIFTND_OK || empty_problem(g)) return 0;
    // 16-bit interpolation: one layout change + the contiguous kernel is faster than the tiled kernel (N16 C256 224x224
    // bf16 through the op: 0.30 vs 0.54 ms; tools/cl_op_bench.py), so the answer is no although shiftnd_forward would
    // take a channels-last tensor
    if (g.active && (p->dtype == SHIFTND_F16 || p->dtype == SHIFTND_BF16)) return 0;
    // NDHWC (round 4): the tiled kernel stages element by element.  N8 C128 16x112x112 (tools/cl3d_bench.py): fp32 0.42 ms to an
    // NDHWC output, 0.49 to NCDHW, against 0.57 ms for the layout change + the contiguous kernel (+ a transpose back when the format
    // is kept); bf16 0.29 / 0.36 against 0.29 -- so 2-byte elements to an NCDHW output keep the layout change
    if (g.nd == 3 && !(g.os[1] == 1 && g.C > 1) && dtype_size(p->dtype) != 4) return 0;
    // ... and the interpolating NDHWC kernel (plane blend at staging time, fp32 ring) only wins for fp32 to an NDHWC output: 0.56 ms
    // against 0.59 + a transpose back (to NCDHW 0.61 against 0.59; bf16 0.49 - 0.52 against 0.29)
    if (g.nd == 3 && g.active && !(g.os[1] == 1 && g.C > 1)) return 0;
    return cl_tiled_forward_eligible(g, p->dtype, x, out) ? 1 : 0;
}

int shiftnd_backward_serves_channels_last(const shiftnd_problem *p, const void *grad_out, const int64_t grad_out_strides[5],
                                          const void *x, const int64_t x_strides[5], const void *grad_x,
                                          const int64_t grad_x_strides[5]) {
    if (!p || !grad_out_strides || !x_strides || !grad_x_strides || g_policy != 0) return 0;
    shiftnd_problem q;
    int wkind;
    if (split_dtype(p, q, wkind) != SHIFTND_OK || !is_float_dtype(q.dtype)) return 0;
    p = &q;
    Geometry g;
    if (build_geometry(p, x_strides, grad_out_strides, grad_x_strides, g) != SHIFTND_OK) return 0;
    if (empty_geometry(g)) return 0;
    if (g.nd == 3) {
        // NDHWC (round 5): shiftnd_cl_tiled3.hip serves such tensors as they lie (what a C-ABI caller gets: 1.2 - 1.5 ms on N8 C128
        // 16x112x112 fp32 where the channel-fastest kernels took 21 - 36 ms), but the op's route -- shiftnd_transpose of the saved
        // input, the walk kernels, shiftnd_transpose of grad_x back -- measures 1.04 ms (bf16 0.53 against 1.0 - 1.4;
        // tools/cl3d_bench.py): the answer stays no unless knob 23 asks for the direct kernel
        if (g_cl3 != 2) return 0;
        return cl_tiled3_backward_eligible(g, p->dtype, grad_out, x, grad_x) ? 1 : 0;
    }
    if (g.active && (p->dtype == SHIFTND_F16 || p->dtype == SHIFTND_BF16)) return 0;  // (0.56 vs 0.66 ms: see above)
    return cl_tiled_backward_eligible(g, p->dtype, grad_out, x, grad_x) ? 1 : 0;
}

int shiftnd_forward(const shiftnd_problem *p, const void *x, const int64_t x_strides[5], const void *weights, void *out,
                    const int64_t out_strides[5], void *stream) {
    if (!p || !x_strides || !out_strides) return SHIFTND_ERR_INVALID_ARGUMENT;
    if ((p->dtype & SHIFTND_SHIFT_DIM0) && (p->dtype & SHIFTND_INTERLACE_FRAMES))   // (first: beside SHIFTND_INTERLACE it is this family's refusal)
        return interlace_frames_forward_call(p, x, x_strides, weights, out, out_strides, stream);
    if ((p->dtype & SHIFTND_SHIFT_DIM0) && (p->dtype & SHIFTND_INTERLACE))   // (the bit alone is an unknown dtype bit, below)
        return interlace_forward_call(p, x, x_strides, weights, out, out_strides, stream);
    if (p->dtype & SHIFTND_SHIFT_DIM0) return tshift_forward_call(p, x, x_strides, weights, out, out_strides, stream);
    shiftnd_problem q;
    int wkind;
    if (split_dtype(p, q, wkind) != SHIFTND_OK || !is_float_dtype(q.dtype)) return SHIFTND_ERR_UNSUPPORTED_DTYPE;
    return forward_common(&q, x, x_strides, weights, wkind, 0, 0ull, out, out_strides, stream);
}

int shiftnd_forward_quantized(const shiftnd_problem *p, const void *x, const int64_t x_strides[5], const void *wq,
                              int32_t wq_dtype, int64_t w_zero_point, int64_t x_zero_point, void *out,
                              const int64_t out_strides[5], void *stream) {
    if (!p || !x_strides || !out_strides) return SHIFTND_ERR_INVALID_ARGUMENT;
    // an fp32 table under the flag: the quantized interpolating temporal shift, or its refusal (without the flag a float table
    // stays an unsupported dtype, below)
    // ... with SHIFTND_PER_CLIP or SHIFTND_INTERLACE beside the flag: the quantized per-clip shift / quantized temporal interlacing
    if ((p->dtype & SHIFTND_SHIFT_DIM0) && wq_dtype == SHIFTND_F32 && (p->dtype & (SHIFTND_PER_CLIP | SHIFTND_INTERLACE)))
        return interlace_quantized_call(p, x, x_strides, wq, w_zero_point, x_zero_point, out, out_strides, stream);
    if ((p->dtype & SHIFTND_SHIFT_DIM0) && wq_dtype == SHIFTND_F32)
        return tshift_quantized_call(p, x, x_strides, wq, w_zero_point, x_zero_point, out, out_strides, stream);
    // the online step (SHIFTND_STREAM beside the flag; alone it is an unknown dtype bit): SHIFTND_FRAMES / SHIFTND_PER_CLIP beside it
    // are its own refusal, not an unknown dtype
    const bool online = (p->dtype & SHIFTND_SHIFT_DIM0) && (p->dtype & SHIFTND_STREAM);
    const int dtype = p->dtype & ~(online ? SHIFTND_SHIFT_DIM0 | SHIFTND_STREAM | SHIFTND_FRAMES | SHIFTND_PER_CLIP : SHIFTND_SHIFT_DIM0);   // (the flag with a float dtype or with SHIFTND_WEIGHTS_F32: no quantized dtype; SHIFTND_CLIP_FRAMES is left in: none either)
    if (!is_quant_dtype(dtype) || !is_quant_dtype(wq_dtype)) return SHIFTND_ERR_UNSUPPORTED_DTYPE;
    shiftnd_problem q = *p;
    if (online) {   // x is the state, read AND written; the state's initial bytes are the padding, so x_zero_point is not used
        q.dtype = dtype;
        return stream_call(q, p->dtype, const_cast<void *>(x), x_strides, out, out_strides, wq, wq_dtype, w_zero_point, stream);
    }
    q.active = 0;
    // fill value = input zero point, as the element type's bit pattern
    uint64_t fill = 0;
    if (dtype == SHIFTND_I8) fill = static_cast<uint8_t>(static_cast<int8_t>(x_zero_point));
    else if (dtype == SHIFTND_U8) fill = static_cast<uint8_t>(x_zero_point);
    else fill = static_cast<uint32_t>(static_cast<int32_t>(x_zero_point));
    if ((p->dtype & SHIFTND_SHIFT_DIM0) && out && out == x) {   // in place: both dense layouts
        q.dtype = dtype;
        q.active = p->active;
        return inplace_call(q, out, x_strides, out_strides, wq, wq_dtype, w_zero_point, fill, stream);
    }
    if (p->dtype & SHIFTND_SHIFT_DIM0)
        return frames_quantized_call(p, x, x_strides, wq, wq_dtype, w_zero_point, fill, out, out_strides, stream);
    return forward_common(&q, x, x_strides, wq, wq_dtype, w_zero_point, fill, out, out_strides, stream);
}

// bytes of partial-sum records the backward families can need for this geometry under the calling thread's knobs
static size_t backward_workspace_now(const Geometry &g, int dtype) {
    size_t m = strided_backward_workspace(g);
    m = std::max(m, plane_backward_workspace(g, dtype));
    m = std::max(m, sweep_backward_workspace(g, dtype));
    m = std::max(m, cl_backward_workspace(g));
    m = std::max(m, cl_tiled_backward_workspace(g));
    m = std::max(m, small_backward_workspace(g, dtype));
    m = std::max(m, cl_tiled3_backward_workspace(g));
    m = std::max(m, flat_backward_workspace(g));
    m = std::max(m, plane_ragged_backward_workspace(g, dtype));
    return m;
}

size_t shiftnd_backward_workspace_bytes(const shiftnd_problem *p) {
    if (!p) return 0;
    shiftnd_problem q;
    int wkind;
    // every entry point refuses the bit alone, so the answer is 0.  (The path below would not give it: it looks at the geometry and sizes
    // the families' plans whatever unknown bits the dtype carries -- 0x800 on F32 answers 512 bytes there, an answer a test pins)
    if ((p->dtype & (SHIFTND_PER_CLIP | SHIFTND_CLIP_FRAMES | SHIFTND_INTERLACE | SHIFTND_INTERLACE_FRAMES)) && !(p->dtype & SHIFTND_SHIFT_DIM0)) return 0;
    if (p->dtype & SHIFTND_INTERLACE_FRAMES) return interlace_frames_workspace_bytes(p);   // both partial sets of shiftnd_interlace_frames.hip, or 0 for a refused problem
    if (p->dtype & SHIFTND_INTERLACE) return interlace_workspace_bytes(p);   // both partial sets of shiftnd_interlace.hip, or 0 for a refused problem
    if (p->dtype & SHIFTND_STREAM) return 0;   // (alone an unknown bit like the one above; beside the flag the online step: no backward, no workspace)
    if (p->dtype & SHIFTND_SHIFT_DIM0) {   // the walk's plan alone (SHIFTND_FRAMES: the channels-last walk's): no other family runs under the flag, no knob shapes it
        const int64_t unit[5] = {0, 0, 0, 0, 0};
        Geometry g;
        bool per_clip, frames;   // (a per-clip table re-indexes the same records: the same bytes with and without SHIFTND_PER_CLIP)
        if (tshift_problem(p, q, wkind, per_clip, frames) != SHIFTND_OK || build_geometry(&q, unit, unit, unit, g) != SHIFTND_OK) return 0;
        if (!tshift_backward_sizes_ok(g, q.dtype, per_clip, frames)) return 0;
        return empty_geometry(g) ? sizeof(double) : tshift_backward_workspace_for(g, q.dtype, frames);
    }
    if (split_dtype(p, q, wkind) != SHIFTND_OK) return 0;
    p = &q;   // (the records are fp64 whatever the weights are: the same bytes with and without SHIFTND_WEIGHTS_F32)
    // the layout of the partial-sum buffer depends only on the geometry: evaluate every family's plan
    const int64_t unit[5] = {0, 0, 0, 0, 0};
    Geometry g;
    if (build_geometry(p, unit, unit, unit, g) != SHIFTND_OK) return 0;
    if (empty_geometry(g)) return sizeof(double);
    size_t m = backward_workspace_now(g, p->dtype);
    if (knobs_touched()) {   // ... and under the default knobs: what a run on any thread can fall back to
        DefaultKnobs scope;
        m = std::max(m, backward_workspace_now(g, p->dtype));
    }
    return m;
}

static int backward_planned(const shiftnd_problem *p, const void *grad_out, const int64_t grad_out_strides[5], const void *x,
                            const int64_t x_strides[5], const void *weights, void *grad_x, const int64_t grad_x_strides[5],
                            void *grad_w, void *workspace, size_t workspace_bytes, void *stream);

int shiftnd_backward(const shiftnd_problem *p, const void *grad_out, const int64_t grad_out_strides[5], const void *x,
                     const int64_t x_strides[5], const void *weights, void *grad_x, const int64_t grad_x_strides[5],
                     void *grad_w, void *workspace, size_t workspace_bytes, void *stream) {
    if (p && (p->dtype & SHIFTND_SHIFT_DIM0) && (p->dtype & SHIFTND_INTERLACE_FRAMES)) {
        if (!grad_out_strides || !grad_x_strides) return SHIFTND_ERR_INVALID_ARGUMENT;
        return interlace_frames_backward_call(p, grad_out, grad_out_strides, x, x_strides, weights, grad_x, grad_x_strides, grad_w,
                                              workspace, workspace_bytes, stream);
    }
    if (p && (p->dtype & SHIFTND_SHIFT_DIM0) && (p->dtype & SHIFTND_INTERLACE)) {
        if (!grad_out_strides || !grad_x_strides) return SHIFTND_ERR_INVALID_ARGUMENT;
        return interlace_backward_call(p, grad_out, grad_out_strides, x, x_strides, weights, grad_x, grad_x_strides, grad_w, workspace,
                                       workspace_bytes, stream);
    }
    if (p && (p->dtype & SHIFTND_SHIFT_DIM0)) {
        if (p->dtype & SHIFTND_STREAM) return SHIFTND_ERR_INVALID_ARGUMENT;   // (the online step is an inference call: no backward)
        if (!grad_out_strides || !grad_x_strides) return SHIFTND_ERR_INVALID_ARGUMENT;
        return tshift_backward_call(p, grad_out, grad_out_strides, x, x_strides, weights, grad_x, grad_x_strides, grad_w, workspace,
                                    workspace_bytes, stream);
    }
    int rc = backward_planned(p, grad_out, grad_out_strides, x, x_strides, weights, grad_x, grad_x_strides, grad_w, workspace,
                              workspace_bytes, stream);
    if (rc == SHIFTND_ERR_WORKSPACE_TOO_SMALL && knobs_touched()) {
        // (nothing was launched.)  This thread's knobs plan more partial records than the caller sized for -- e.g. sized on
        // a thread with the default knobs: run the default plan, which shiftnd_backward_workspace_bytes always covers
        DefaultKnobs scope;
        rc = backward_planned(p, grad_out, grad_out_strides, x, x_strides, weights, grad_x, grad_x_strides, grad_w, workspace,
                              workspace_bytes, stream);
    }
    return rc;
}

static int backward_planned(const shiftnd_problem *p, const void *grad_out, const int64_t grad_out_strides[5], const void *x,
                            const int64_t x_strides[5], const void *weights, void *grad_x, const int64_t grad_x_strides[5],
                            void *grad_w, void *workspace, size_t workspace_bytes, void *stream) {
    // x == NULL && grad_w == NULL: the input gradient only (the sparse shift's grad_x is a gather of grad_out; shiftnd_gradx.hip)
    const bool input_only = !x && !grad_w;
    if (!p || !grad_out_strides || !grad_x_strides || (!x_strides && !input_only)) return SHIFTND_ERR_INVALID_ARGUMENT;
    shiftnd_problem q;
    int wkind;   // element type of `weights` and `grad_w`
    if (split_dtype(p, q, wkind) != SHIFTND_OK || !is_float_dtype(q.dtype)) return SHIFTND_ERR_UNSUPPORTED_DTYPE;
    // (the fixed ops convert their integer table to the tensors' type themselves: the x == NULL form takes no fp32 table)
    if (input_only && wkind != q.dtype) return SHIFTND_ERR_INVALID_ARGUMENT;
    p = &q;
    Geometry g;
    const int rc = build_geometry(p, x_strides ? x_strides : grad_x_strides, grad_out_strides, grad_x_strides, g);
    if (rc != SHIFTND_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (empty_geometry(g)) {
        // nothing to differentiate; grad_w (if any channels) is all zeros (zeros_like, shifts_cpu.cpp:247)
        g_last_path = SHIFTND_PATH_EMPTY;
        if (g.C > 0 && grad_w)
            if (hipMemsetAsync(grad_w, 0, static_cast<size_t>(g.C) * g.nd * dtype_size(wkind), st) != hipSuccess)
                return SHIFTND_ERR_LAUNCH_FAILED;
        return SHIFTND_OK;
    }
    if (input_only) {
        if (p->active || !grad_out || !weights || !grad_x) return SHIFTND_ERR_INVALID_ARGUMENT;
        if (!cropped(g)) {
            // the window is the whole input: grad_x = sparse forward of grad_out under -w (rint is odd-symmetric), on whichever
            // forward route serves this tensor; the negated table lives in the caller's workspace
            if (!workspace || gradx_negate_workspace(g, p->dtype) > workspace_bytes) return SHIFTND_ERR_WORKSPACE_TOO_SMALL;
            const int nrc = gradx_negate_weights(g, p->dtype, weights, workspace, st);
            if (nrc != SHIFTND_OK) return nrc;
            return forward_common(p, grad_out, grad_out_strides, workspace, p->dtype, 0, 0ull, grad_x, grad_x_strides, stream);
        }
        if (g_policy == 0 && gradx_embed_eligible(g, p->dtype, grad_out, grad_x)) {
            g_last_path = SHIFTND_PATH_PLANE;
            return finish(gradx_embed(g, p->dtype, grad_out, weights, grad_x, st));
        }
        g_last_path = SHIFTND_PATH_STRIDED;
        return finish(gradx_gather(g, p->dtype, grad_out, weights, grad_x, st));
    }
    if (!grad_out || !x || !weights || !grad_x || !grad_w || !workspace) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (g_policy == 0 && g_flat == 2 && flat_backward_eligible(g, p->dtype, grad_out, x, grad_x)) {   // (knob 27 = 2: tests)
        if (flat_backward_workspace(g) > workspace_bytes) return SHIFTND_ERR_WORKSPACE_TOO_SMALL;
        g_last_path = SHIFTND_PATH_PLANE;
        return finish(flat_backward(g, p->dtype, grad_out, x, weights, wkind, grad_x, grad_w, workspace, st));
    }
    const bool can_sweep = sweep_backward_eligible(g, p->dtype, grad_out, x, grad_x);
    const bool can_plane = plane_backward_eligible(g, p->dtype, grad_out, x, grad_x);
    if ((g_policy == 2 && !can_plane) || (g_policy == 3 && !can_sweep)) return SHIFTND_ERR_INVALID_ARGUMENT;
    // automatic choice: the per-plane kernels (faster for the backward pass); the sweep kernels take over
    // when the index maps do not fit in LDS
    if (can_sweep && (g_policy == 3 || (g_policy == 0 && !can_plane))) {
        if (sweep_backward_workspace(g, p->dtype) > workspace_bytes) return SHIFTND_ERR_WORKSPACE_TOO_SMALL;
        g_last_path = SHIFTND_PATH_SWEEP;
        return finish(sweep_backward(g, p->dtype, grad_out, x, weights, wkind, grad_x, grad_w, workspace, st));
    }
    // ragged rows of 4- / 8-byte elements on planes with rows of at least 8 chunks: the row-relative crop_backward (shiftnd_span.hip, XRAG)
    if (g_policy == 0 && g_flat != 2 && ragged_rows(g, p->dtype) && span_backward_eligible(g, p->dtype, grad_out, x, grad_x)) {
        if (span_backward_workspace(g, p->dtype) > workspace_bytes) return SHIFTND_ERR_WORKSPACE_TOO_SMALL;
        g_last_path = SHIFTND_PATH_PLANE;
        return finish(span_backward(g, p->dtype, grad_out, x, weights, wkind, grad_x, grad_w, workspace, st));
    }
    // ragged input rows -- and windows crop_backward does not take: the flat chunk stream.  (Ragged rows of 4- / 8-byte elements on
    // planes large enough for the row-relative crop_backward: that one, through plane_backward below.)
    if (g_policy == 0 && !span_backward_eligible(g, p->dtype, grad_out, x, grad_x) && (ragged_rows(g, p->dtype) || cropped(g)) &&
        flat_backward_eligible(g, p->dtype, grad_out, x, grad_x)) {
        if (flat_backward_workspace(g) > workspace_bytes) return SHIFTND_ERR_WORKSPACE_TOO_SMALL;
        g_last_path = SHIFTND_PATH_PLANE;
        return finish(flat_backward(g, p->dtype, grad_out, x, weights, wkind, grad_x, grad_w, workspace, st));
    }
    if (can_plane && g_policy != 1 && g_policy != 4) {
        if (plane_backward_workspace(g, p->dtype) > workspace_bytes) return SHIFTND_ERR_WORKSPACE_TOO_SMALL;
        g_last_path = SHIFTND_PATH_PLANE;
        return finish(plane_backward(g, p->dtype, grad_out, x, weights, wkind, grad_x, grad_w, workspace, st));
    }
    if (g_policy == 0 && small_backward_eligible(g, p->dtype)) {  // rows not whole 16-byte pieces, small planes
        if (small_backward_workspace(g, p->dtype) > workspace_bytes) return SHIFTND_ERR_WORKSPACE_TOO_SMALL;
        g_last_path = SHIFTND_PATH_PLANE;
        return finish(small_backward(g, p->dtype, grad_out, x, weights, wkind, grad_x, grad_w, workspace, st));
    }
    // 3-D volumes with ragged rows beyond the small-plane kernels (16 x 28 x 28 bf16, 8 x 56 x 62 fp32 ...): the direct-load plane
    // kernels with 4- / 8-byte chunks instead of the one-thread-per-element fallback
    if (g_policy == 0 && plane_ragged_backward_eligible(g, p->dtype, grad_out, x, grad_x)) {
        if (plane_ragged_backward_workspace(g, p->dtype) > workspace_bytes) return SHIFTND_ERR_WORKSPACE_TOO_SMALL;
        g_last_path = SHIFTND_PATH_PLANE;
        return finish(plane_ragged_backward(g, p->dtype, grad_out, x, weights, wkind, grad_x, grad_w, workspace, st));
    }
    if ((g_policy == 0 || g_policy == 4) && cl_tiled_backward_eligible(g, p->dtype, grad_out, x, grad_x)) {  // all channels-last: LDS-tiled
        if (cl_tiled_backward_workspace(g) > workspace_bytes) return SHIFTND_ERR_WORKSPACE_TOO_SMALL;
        g_last_path = SHIFTND_PATH_CL;
        return finish(cl_tiled_backward(g, p->dtype, grad_out, x, weights, wkind, grad_x, grad_w, workspace, st));
    }
    if ((g_policy == 0 || g_policy == 4) && g_cl3 != 1 && cl_tiled3_backward_eligible(g, p->dtype, grad_out, x, grad_x)) {  // NDHWC: LDS-tiled, one plane per workgroup
        if (cl_tiled3_backward_workspace(g) > workspace_bytes) return SHIFTND_ERR_WORKSPACE_TOO_SMALL;
        g_last_path = SHIFTND_PATH_CL;
        return finish(cl_tiled3_backward(g, p->dtype, grad_out, x, weights, wkind, grad_x, grad_w, workspace, st));
    }
    if (g_policy == 4 && !cl_backward_eligible(g, p->dtype)) return SHIFTND_ERR_INVALID_ARGUMENT;
    if ((g_policy == 0 && cl_backward_preferred(g, p->dtype)) || g_policy == 4) {
        if (cl_backward_workspace(g) > workspace_bytes) return SHIFTND_ERR_WORKSPACE_TOO_SMALL;
        g_last_path = SHIFTND_PATH_CL;
        return finish(cl_backward(g, p->dtype, grad_out, x, weights, wkind, grad_x, grad_w, workspace, st));
    }
    if (strided_backward_workspace(g) > workspace_bytes) return SHIFTND_ERR_WORKSPACE_TOO_SMALL;
    g_last_path = SHIFTND_PATH_STRIDED;
    return finish(strided_backward(g, p->dtype, grad_out, x, weights, wkind, grad_x, grad_w, workspace, st));
}

// ---- layout change ---------------------------------------------------------------------------------------------
int shiftnd_transpose(const void *src, void *dst, int64_t batch, int64_t rows, int64_t cols, int32_t element_bytes,
                      void *stream) {
    if (batch < 0 || rows < 0 || cols < 0) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (batch == 0 || rows == 0 || cols == 0) return SHIFTND_OK;
    if (!src || !dst) return SHIFTND_ERR_INVALID_ARGUMENT;
    return finish(transpose_planes(src, dst, batch, rows, cols, element_bytes, static_cast<hipStream_t>(stream)));
}

// ---- fused shift + average pool ----------------------------------------------------------------------------
// (p: the problem with the tensors' plain dtype -- split_dtype() has run)
static int pooled_geometry(const shiftnd_problem *p, const int32_t *pool, Geometry &g, bool quantized_too = false) {
    if (!p || !pool) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (!is_float_dtype(p->dtype) && !(quantized_too && is_quant_dtype(p->dtype))) return SHIFTND_ERR_UNSUPPORTED_DTYPE;
    const int64_t unit[5] = {0, 0, 0, 0, 0};
    const int rc = build_geometry(p, unit, unit, unit, g);
    if (rc != SHIFTND_OK) return rc;
    const int lead = 3 - p->ndim;
    for (int d = 0; d < 3; ++d) g.K[d] = 1;
    for (int r = 0; r < p->ndim; ++r) {
        if (pool[r] < 1) return SHIFTND_ERR_INVALID_ARGUMENT;
        g.K[r + lead] = pool[r];
    }
    for (int d = 0; d < 3; ++d) g.P[d] = (g.O[d] + g.K[d] - 1) / g.K[d];
    // contiguous tensors: element strides in normalised order N, C, d0, d1, inner
    auto fill = [&](int64_t *st, const int64_t *sz) {
        st[4] = 1;
        st[3] = sz[2];
        st[2] = sz[2] * sz[1];
        st[1] = sz[2] * sz[1] * sz[0];
        st[0] = st[1] * g.C;
    };
    fill(g.xs, g.S);
    fill(g.gs, g.S);
    fill(g.os, g.P);
    return SHIFTND_OK;
}

size_t shiftnd_backward_pooled_workspace_bytes(const shiftnd_problem *p, const int32_t *pool) {
    // the pooled backward plans its launch with the pool in the geometry (more, shorter workgroups than the plain
    // backward of the same tensor can need more partial-sum groups)
    shiftnd_problem q;
    int wkind;
    if (!p || split_dtype(p, q, wkind) != SHIFTND_OK) return 0;
    p = &q;   // (as shiftnd_backward_workspace_bytes: the same bytes with and without SHIFTND_WEIGHTS_F32)
    Geometry g;
    if (pooled_geometry(p, pool, g) != SHIFTND_OK) return 0;
    if (empty_geometry(g)) return sizeof(double);
    size_t m = plane_backward_workspace(g, p->dtype);
    if (knobs_touched()) {   // (as shiftnd_backward_workspace_bytes)
        DefaultKnobs scope;
        m = std::max(m, plane_backward_workspace(g, p->dtype));
    }
    return m;
}

int shiftnd_pooled_sizes(const shiftnd_problem *p, const int32_t *pool, int64_t pooled_spatial[3]) {
    if (!p) return SHIFTND_ERR_INVALID_ARGUMENT;
    shiftnd_problem q;
    int wkind;
    if (split_dtype(p, q, wkind) != SHIFTND_OK) return SHIFTND_ERR_UNSUPPORTED_DTYPE;
    p = &q;
    Geometry g;
    const int rc = pooled_geometry(p, pool, g, true);  // (the sizes do not depend on the element type)
    if (rc != SHIFTND_OK) return rc;
    if (!pooled_spatial) return SHIFTND_ERR_INVALID_ARGUMENT;
    const int lead = 3 - p->ndim;
    for (int r = 0; r < 3; ++r) pooled_spatial[r] = r < p->ndim ? g.P[r + lead] : 1;
    return SHIFTND_OK;
}

int shiftnd_forward_pooled(const shiftnd_problem *p, const int32_t *pool, const void *x, const void *weights, void *out,
                           void *stream) {
    if (!p) return SHIFTND_ERR_INVALID_ARGUMENT;
    shiftnd_problem q;
    int wkind;
    if (split_dtype(p, q, wkind) != SHIFTND_OK) return SHIFTND_ERR_UNSUPPORTED_DTYPE;
    p = &q;
    Geometry g;
    const int rc = pooled_geometry(p, pool, g);
    if (rc != SHIFTND_OK) return rc;
    if (empty_problem(g)) {
        g_last_path = SHIFTND_PATH_EMPTY;
        return SHIFTND_OK;
    }
    if (!x || !weights || !out) return SHIFTND_ERR_INVALID_ARGUMENT;
    // 3-D interpolating: the walk through the planes with the pool as its epilogue
    if (g_policy == 0 && walk_forward_pooled_eligible(g, p->dtype, x, out)) {
        g_last_path = SHIFTND_PATH_PLANE;
        return finish(walk_forward(g, p->dtype, x, weights, wkind, out, static_cast<hipStream_t>(stream)));
    }
    // 2-D sparse shift, 2 x 2 windows, fp32 / fp64: the linear sweep of one-step workgroups with the pool as its epilogue
    if (g_policy == 0 && step_forward_pooled_eligible(g, p->dtype, x, out)) {
        g_last_path = SHIFTND_PATH_SWEEP;
        return finish(step_forward_pooled(g, p->dtype, x, weights, wkind, out, static_cast<hipStream_t>(stream)));
    }
    // 3-D volumes, 2 x 2 x 2 windows, cropped or not (what the walk above does not take): pooled rows through LDS (round 6)
    if (g_policy == 0 && span_forward_pooled3_eligible(g, p->dtype, x, out)) {
        g_last_path = SHIFTND_PATH_PLANE;
        return finish(span_forward_pooled3(g, p->dtype, x, weights, wkind, out, static_cast<hipStream_t>(stream)));
    }
    // 1-D rows of at least 128 chunks, windows of 2: row_forward with the pool as its epilogue (round 6)
    if (g_policy == 0 && span_forward_pooled_eligible(g, p->dtype, x, out)) {
        g_last_path = SHIFTND_PATH_PLANE;
        return finish(span_forward_pooled(g, p->dtype, x, weights, wkind, out, static_cast<hipStream_t>(stream)));
    }
    if (!plane_pool_forward_eligible(g, p->dtype)) return SHIFTND_ERR_NOT_FUSED;
    g_last_path = SHIFTND_PATH_PLANE;
    return finish(plane_pool_forward(g, p->dtype, x, weights, wkind, out, static_cast<hipStream_t>(stream)));
}

int shiftnd_forward_quantized_pooled(const shiftnd_problem *p, const int32_t *pool, const void *x, const void *wq, int32_t wq_dtype,
                                     int64_t w_zero_point, int64_t x_zero_point, int32_t requant, void *out, void *stream) {
    if (!p || !pool) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (requant != SHIFTND_REQUANT_ZP_INSIDE && requant != SHIFTND_REQUANT_ZP_OUTSIDE) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (!is_quant_dtype(p->dtype) || !is_quant_dtype(wq_dtype)) return SHIFTND_ERR_UNSUPPORTED_DTYPE;
    shiftnd_problem q = *p;
    q.active = 0;
    Geometry g;
    const int rc = pooled_geometry(&q, pool, g, true);
    if (rc != SHIFTND_OK) return rc;
    if (empty_problem(g)) {
        g_last_path = SHIFTND_PATH_EMPTY;
        return SHIFTND_OK;
    }
    if (!x || !wq || !out) return SHIFTND_ERR_INVALID_ARGUMENT;
    if (!qpool_forward_eligible(g, p->dtype)) return SHIFTND_ERR_NOT_FUSED;
    g_last_path = SHIFTND_PATH_PLANE;
    return finish(qpool_forward(g, p->dtype, x, wq, wq_dtype, w_zero_point, x_zero_point, requant, out, static_cast<hipStream_t>(stream)));
}

static int backward_pooled_planned(const shiftnd_problem *p, const int32_t *pool, const void *grad_pooled, const void *x,
                                   const void *weights, void *grad_x, void *grad_w, void *workspace, size_t workspace_bytes,
                                   void *stream);

int shiftnd_backward_pooled(const shiftnd_problem *p, const int32_t *pool, const void *grad_pooled, const void *x,
                            const void *weights, void *grad_x, void *grad_w, void *workspace, size_t workspace_bytes,
                            void *stream) {
    int rc = backward_pooled_planned(p, pool, grad_pooled, x, weights, grad_x, grad_w, workspace, workspace_bytes, stream);
    if (rc == SHIFTND_ERR_WORKSPACE_TOO_SMALL && knobs_touched()) {   // (as shiftnd_backward)
        DefaultKnobs scope;
        rc = backward_pooled_planned(p, pool, grad_pooled, x, weights, grad_x, grad_w, workspace, workspace_bytes, stream);
    }
    return rc;
}

static int backward_pooled_planned(const shiftnd_problem *p, const int32_t *pool, const void *grad_pooled, const void *x,
                                   const void *weights, void *grad_x, void *grad_w, void *workspace, size_t workspace_bytes,
                                   void *stream) {
    if (!p) return SHIFTND_ERR_INVALID_ARGUMENT;
    shiftnd_problem q;
    int wkind;   // element type of `weights` and `grad_w`
    if (split_dtype(p, q, wkind) != SHIFTND_OK) return SHIFTND_ERR_UNSUPPORTED_DTYPE;
    p = &q;
    Geometry g;
    const int rc = pooled_geometry(p, pool, g);
    if (rc != SHIFTND_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool input_only = !x && !grad_w;
    if (input_only && (p->active || wkind != p->dtype)) return SHIFTND_ERR_INVALID_ARGUMENT;   // (also for an empty problem: the form does not exist)
    if (empty_geometry(g)) {
        g_last_path = SHIFTND_PATH_EMPTY;
        if (g.C > 0 && grad_w)
            if (hipMemsetAsync(grad_w, 0, static_cast<size_t>(g.C) * g.nd * dtype_size(wkind), st) != hipSuccess)
                return SHIFTND_ERR_LAUNCH_FAILED;
        return SHIFTND_OK;
    }
    if (input_only) {
        // the input gradient only (fixed shifts with a stride): a gather of grad_pooled with one division, no workspace.  The
        // kernels of shiftnd_backward's NULL form with the pool in the geometry (shiftnd_gradx.hip); never SHIFTND_ERR_NOT_FUSED
        if (!grad_pooled || !weights || !grad_x) return SHIFTND_ERR_INVALID_ARGUMENT;
        if (g_policy == 0 && gradx_embed_eligible(g, p->dtype, grad_pooled, grad_x)) {
            g_last_path = SHIFTND_PATH_PLANE;
            return finish(gradx_embed(g, p->dtype, grad_pooled, weights, grad_x, st));
        }
        g_last_path = SHIFTND_PATH_STRIDED;
        return finish(gradx_gather(g, p->dtype, grad_pooled, weights, grad_x, st));
    }
    if (!grad_pooled || !x || !weights || !grad_x || !grad_w || !workspace) return SHIFTND_ERR_INVALID_ARGUMENT;
    // 3-D interpolating: the walk through the planes with the pooled gradient expanded on the way into LDS
    if (g_policy == 0 && walk_backward_pooled_eligible(g, p->dtype, grad_pooled, x, grad_x)) {
        if (plane_backward_workspace(g, p->dtype) > workspace_bytes) return SHIFTND_ERR_WORKSPACE_TOO_SMALL;
        g_last_path = SHIFTND_PATH_PLANE;
        return finish(step_backward(g, p->dtype, grad_pooled, x, weights, wkind, grad_x, grad_w, workspace, st));
    }
    // cropped 3-D volumes, 2 x 2 x 2 windows: crop_backward3 with the pooled gradient expanded on its way into LDS (round 6)
    if (g_policy == 0 && g.nd == 3 && span_backward_pooled_eligible(g, p->dtype, grad_pooled, x, grad_x)) {
        if (span_backward_pooled_workspace(g, p->dtype) > workspace_bytes) return SHIFTND_ERR_WORKSPACE_TOO_SMALL;
        g_last_path = SHIFTND_PATH_PLANE;
        return finish(span_backward(g, p->dtype, grad_pooled, x, weights, wkind, grad_x, grad_w, workspace, st));
    }
    if (!plane_pool_backward_eligible(g, p->dtype, grad_x)) return SHIFTND_ERR_NOT_FUSED;
    // what the walk does not take of the 3-D interpolating backward: through the band-walk kernels 16 gradient corner rows per
    // step would be expanded from pooled rows -- measured slower than avg_pool backward + shiftnd_backward (N8 C128 16x112x112:
    // 1.42 vs 1.33 ms fp32, 1.32 vs 0.96 ms bf16), so it is not fused unless the plane-kernel policy is forced (tests)
    if (g.nd == 3 && g.active && g_policy != 2) return SHIFTND_ERR_NOT_FUSED;
    // (round 6) a cropped 3-D volume that crop_backward3 serves: the band-walk kernels with the pool fused are SLOWER than the average
    // pool's backward followed by crop_backward3 (N8 C128 16x56x56 cut 1/1/1 pool 2, sparse: bf16 0.32 vs 0.10 + the pool, fp32 0.33 vs
    // 0.17 + the pool; tools/module_matrix.py) -- not fused, the op composes the two
    if (g.nd == 3 && g_policy == 0) {
        Geometry u = g;   // the unpooled problem: gradient of the window, dense
        for (int d = 0; d < 3; ++d) u.K[d] = 0, u.P[d] = 0;
        u.os[4] = 1;
        u.os[3] = u.O[2];
        u.os[2] = u.O[2] * u.O[1];
        u.os[1] = u.O[2] * u.O[1] * u.O[0];
        u.os[0] = u.os[1] * u.C;
        if (span_backward_eligible(u, p->dtype, x, x, grad_x)) return SHIFTND_ERR_NOT_FUSED;   // (the gradient will be a fresh, aligned tensor)
    }
    if (plane_backward_workspace(g, p->dtype) > workspace_bytes) return SHIFTND_ERR_WORKSPACE_TOO_SMALL;
    g_last_path = SHIFTND_PATH_PLANE;
    return finish(plane_pool_backward(g, p->dtype, grad_pooled, x, weights, wkind, grad_x, grad_w, workspace, st));
}

}  // extern "C"
