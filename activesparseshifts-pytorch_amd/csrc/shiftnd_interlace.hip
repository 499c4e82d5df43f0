// shiftnd_interlace.hip -- temporal INTERLACING (TIN, arXiv 2001.06499): the per-clip temporal shift of shiftnd_tshift.hip fused with
// a per-clip, per-frame, per-channel weight (gfx950).  SHIFTND_SHIFT_DIM0 | SHIFTND_INTERLACE on p->dtype selects it.
//
//   out[n, t, c, :] = scale[n, t, c] * shift(x)[n, t, c, :]          shift: the per-clip op under offsets[n, c], out[t] = x[t - w]
//
// on segment-major tensors (memory order N, S0, C, S1, S2).  `weights` is ONE packed array: the N * C offsets [N, C] followed by the
// N * T * C scales [N, T, C]; `grad_w` has the same layout.  A plane (n, t, c) of M contiguous elements has one shift, one fraction
// and one scale, so the kernels are tshift_forward / tshift_backward with a per-plane scalar:
//
//   tinterlace_forward   forward_body's flat unit stream.  The scale of a unit's plane is entry (n * T + t) * C + c, the plane index
//                        the kernel has already.  The unit is blended (or copied), then multiplied in the compute type -- a multiply
//                        of its own, after the lerp -- and rounded once.  A filled plane is 0 * scale (the composition's sign of zero).
//   tinterlace_backward  backward_body's walk along t.  Every gradient frame that is loaded is multiplied by the scale of ITS OWN
//                        frame before use (a filled frame by 1: its zeros stay +0), so grad_x is the per-clip backward of
//                        scale * grad_out.  The scales are workgroup-uniform loads, three per step.  Three sums:
//                          offsets   per thread, fp64: (scale[t] * g[t]) * (x[B] - x[A]) over the walk; one block_sum per workgroup,
//                                    record ((chunk * N + n) * C + c) * 3 as under a per-clip table.
//                          scales    per STEP t, fp64: g[t] * y[t] with y[t] the blend of the x units the walk holds (xa, xb), in the
//                                    compute type, unrounded.  No barrier in the step loop: one cross-lane sum per wave and step, lane
//                                    0 of the wave writes record (((chunk * 4 + wave) * N * T * C) + (n * T + t) * C + c) * 3 -- an
//                                    idle wave (its first unit past the plane: a scalar test) walks nothing and writes zeros.  The
//                                    ragged form walks its chunk in rounds; a later round adds to the record the same lane wrote a
//                                    round before.
//                        Both sets are finished by launch_reduce_weight_grads (`chunks` groups of N * C entries; 4 * chunks groups of
//                        N * T * C entries): fixed order, deterministic, narrowed once to the table's type.
//
// Units, the ragged names and the 32-bit limits are those of shiftnd_tshift.hip; T is unbounded (nothing is sized by it).  No LDS
// beyond block_sum's, no scratch.  Two kernels in all: the element type is a launch-uniform switch inside each.
//
// Not built: the in-place / online forms, group expansion inside the kernel.  (Channels-last tensors: since built,
// shiftnd_interlace_frames.hip; the quantized forward: shiftnd_interlace_quant.hip.)
#include "shiftnd_temporal.hpp"

namespace shiftnd {
namespace {

// units per thread of the forward, every load issued before the first store.  Two for 16-bit elements: their bodies hold eight
// widened values a unit, four units in flight took 104 VGPRs (4 waves per SIMD) and -- the two kernels serve every element type, so
// the widest body sets the allocation -- slowed the fp32 stream too (0.139 -> 0.176 ms on [128, 256, 56, 56]); occupancy pays here
template <typename T> constexpr int fwd_in_flight() { return sizeof(typename T::S) == 2 ? 2 : 4; }
inline int fwd_in_flight_of(int dtype) { return dtype_size(dtype) == 2 ? 2 : 4; }
constexpr int kBwdInFlight = 2;     // units per thread and step of the walk
constexpr int64_t kChunkBytes = static_cast<int64_t>(kThreads) * kBwdInFlight * 16;   // of a plane, per workgroup of the walk
constexpr int kWaves = kThreads / 64;

struct InterlaceParams {
    int pad, wkind, active;
    uint32_t T, C, upp, chunks, clips;   // segments, channels, units per plane, workgroups per (n, c) line (backward), N
    FastDiv d_upp, d_C, d_T, d_per, d_chunks;   // d_per: by map_period(T, pad)
    int64_t plane_bytes, units;          // units: of the whole tensor (forward)
    int64_t scales, planes;              // first entry of the scales in the packed table (N * C); their count (N * T * C)
    int64_t step_records;                // first double of the per-step records in the workspace (chunks * N * C * 3)
};

constexpr int64_t kFill = -1, kPast = -2;

template <typename T, int E>
__device__ __forceinline__ void forward_body(const InterlaceParams &q, const char *__restrict__ x, const void *__restrict__ w,
                                             char *__restrict__ out) {
    using CT = typename T::C;
    constexpr int kFwdInFlight = fwd_in_flight<T>();
    constexpr int V = sizeof(typename T::S) * E;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * (kThreads * kFwdInFlight) + threadIdx.x;
    const int Tn = static_cast<int>(q.T);
    int64_t sa[kFwdInFlight], sb[kFwdInFlight];   // byte offset in x of the unit's two sources, or a mark
    CT dw[kFwdInFlight], sc[kFwdInFlight];
#pragma unroll
    for (int k = 0; k < kFwdInFlight; ++k) {
        const int64_t i = first + k * kThreads;
        sa[k] = sb[k] = kPast;
        dw[k] = sc[k] = CT(0);
        if (i >= q.units) continue;
        const uint32_t u = static_cast<uint32_t>(i);
        const uint32_t plane = fdiv(u, q.d_upp);
        const int64_t at = static_cast<int64_t>(u - plane * q.upp) * V;   // byte in the plane
        const uint32_t nt = fdiv(plane, q.d_C), c = plane - nt * q.C;
        const uint32_t n = fdiv(nt, q.d_T), t = nt - n * q.T;
        int64_t iw;
        prep_shift_forward<CT>(load_weight<CT>(w, q.wkind, static_cast<int64_t>(n) * q.C + c), q.active != 0, iw, dw[k]);
        sc[k] = load_weight<CT>(w, q.wkind, q.scales + plane);
        const int cs = canon_shift(iw, Tn, q.pad, q.d_per);
        const int s0 = source_frame(static_cast<int>(t), cs, Tn, q.pad), s1 = source_frame(static_cast<int>(t) + 1, cs, Tn, q.pad);
        const int64_t clip = static_cast<int64_t>(n) * q.T;
        sa[k] = s0 < 0 ? kFill : ((clip + s0) * q.C + c) * q.plane_bytes + at;
        sb[k] = (s1 < 0 || !q.active) ? kFill : ((clip + s1) * q.C + c) * q.plane_bytes + at;
    }
    Unit<T, E> a[kFwdInFlight], b[kFwdInFlight];
#pragma unroll
    for (int k = 0; k < kFwdInFlight; ++k) {
        a[k] = b[k] = zero_unit<T, E>();
        if (sa[k] >= 0) a[k] = load_unit<T, E, true>(x + sa[k]);   // (a filled plane issues no load)
        if (sb[k] >= 0) b[k] = load_unit<T, E, true>(x + sb[k]);
    }
#pragma unroll
    for (int k = 0; k < kFwdInFlight; ++k) {
        if (sa[k] == kPast) continue;
        Unit<T, E> r;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const CT v[2] = {widen<T>(a[k].e[e]), widen<T>(b[k].e[e])};
            const CT y = q.active ? interp_t<T, 1>(v, &dw[k]) : v[0];
            r.e[e] = narrow<T>(y * sc[k]);   // the scale AFTER the lerp, a multiply of its own
        }
        store_unit<T, E>(out + (first + k * kThreads) * V, r);
    }
}

template <typename T, int E>
__device__ __forceinline__ double backward_body(const InterlaceParams &q, const char *__restrict__ go, const char *__restrict__ x,
                                                const void *__restrict__ w, char *__restrict__ gx, double *__restrict__ ws, uint32_t n,
                                                uint32_t c, uint32_t chunk) {
    using CT = typename T::C;
    constexpr int V = sizeof(typename T::S) * E;
    const int Tn = static_cast<int>(q.T);
    int64_t sh;
    CT dw;
    prep_shift_backward<CT>(load_weight<CT>(w, q.wkind, static_cast<int64_t>(n) * q.C + c), q.active != 0, sh, dw);
    const int cs = canon_shift(sh, Tn, q.pad, q.d_per);     // x (and, interpolating, grad_out) at pad(t - sh), pad(t + 1 - sh)
    const int csn = canon_shift(-sh, Tn, q.pad, q.d_per);   // the sparse shift's grad_x: grad_out at pad(t + sh)
    const int64_t clip = static_cast<int64_t>(n) * q.T;
    auto plane = [&](int t) { return ((clip + t) * q.C + c) * q.plane_bytes; };
    // the scale of frame t of this (n, c) line; 1 for a filled frame, whose zeros stay +0 (workgroup-uniform)
    auto scale = [&](int t) { return t < 0 ? CT(1) : load_weight<CT>(w, q.wkind, q.scales + (clip + t) * q.C + c); };
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (the wave index as a scalar)
    // this wave's record of step 0; step t is t * C records on
    double *rec = ws + q.step_records + ((static_cast<int64_t>(chunk) * kWaves + wave) * q.planes + clip * q.C + c) * 3;
    double acc = 0.0;
    // the workgroup's kChunkBytes of the plane in rounds of kThreads * kBwdInFlight units (one round for 16-byte units)
#pragma unroll 1
    for (int round = 0; round < 16 / V; ++round) {
        // a wave whose first unit of the round lies past the plane is idle for the whole round (its second unit lies further on): it
        // walks nothing and reduces nothing -- in round 0 its records are written as zeros, later rounds leave them as they are
        const int64_t first = (static_cast<int64_t>(chunk) * (16 / V) + round) * (kThreads * kBwdInFlight);
        if (first + wave * 64 >= q.upp) {
            if (round == 0 && lane == 0)
                for (int t = 0; t < Tn; ++t) rec[static_cast<int64_t>(t) * q.C * 3] = 0.0;
            continue;
        }
        int64_t at[kBwdInFlight];
        bool in[kBwdInFlight];
#pragma unroll
        for (int k = 0; k < kBwdInFlight; ++k) {
            const int64_t u = first + k * kThreads + threadIdx.x;
            in[k] = u < q.upp;
            at[k] = u * V;
        }
        Unit<T, E> xa[kBwdInFlight], ga[kBwdInFlight];
        const int s0 = source_frame(0, cs, Tn, q.pad);
        CT sca = scale(s0);   // of the frame ga holds
#pragma unroll
        for (int k = 0; k < kBwdInFlight; ++k) {
            xa[k] = ga[k] = zero_unit<T, E>();
            if (s0 >= 0 && in[k]) xa[k] = load_unit<T, E, false>(x + plane(s0) + at[k]);
            if (s0 >= 0 && in[k] && q.active) ga[k] = load_unit<T, E, false>(go + plane(s0) + at[k]);
        }
#pragma unroll 1
        for (int t = 0; t < Tn; ++t) {
            const int s1 = source_frame(t + 1, cs, Tn, q.pad);
            const int sg = q.active ? s1 : source_frame(t, csn, Tn, q.pad);
            const CT scv = scale(t), scb = scale(sg);   // of the frames gv and gb hold
            Unit<T, E> xb[kBwdInFlight], gb[kBwdInFlight], gv[kBwdInFlight];
#pragma unroll
            for (int k = 0; k < kBwdInFlight; ++k) {
                xb[k] = gb[k] = gv[k] = zero_unit<T, E>();
                if (!in[k]) continue;
                if (s1 >= 0) xb[k] = load_unit<T, E, false>(x + plane(s1) + at[k]);
                if (sg >= 0) gb[k] = load_unit<T, E, false>(go + plane(sg) + at[k]);
                gv[k] = load_unit<T, E, false>(go + plane(t) + at[k]);
            }
            double step = 0.0;   // this thread's share of sum g[t] * y[t]
#pragma unroll
            for (int k = 0; k < kBwdInFlight; ++k) {
                if (in[k]) {   // (an idle thread adds nothing: 0 * scale is no zero under a scale that is not finite)
                    Unit<T, E> r;
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        const CT vx[2] = {widen<T>(xa[k].e[e]), widen<T>(xb[k].e[e])};
                        const CT g = widen<T>(gv[k].e[e]);
                        // weight_grads_nd<1> on the scaled gradient, the difference taken in fp64 (as tshift_backward)
                        const double diff = static_cast<double>(vx[1]) - static_cast<double>(vx[0]);
                        acc = fma_ct(static_cast<double>(g * scv), diff, acc);
                        const CT y = q.active ? interp_t<T, 1>(vx, &dw) : vx[0];
                        step = fma_ct(static_cast<double>(g), static_cast<double>(y), step);
                        const CT vg[2] = {widen<T>(ga[k].e[e]) * sca, widen<T>(gb[k].e[e]) * scb};   // the scale BEFORE the lerp
                        r.e[e] = narrow<T>(q.active ? interp_t<T, 1>(vg, &dw) : vg[1]);
                    }
                    store_unit<T, E>(gx + plane(t) + at[k], r);
                }
                xa[k] = xb[k];
                ga[k] = gb[k];
            }
            sca = scb;
            step = wave_sum(step);
            if (lane == 0) {
                double *p = rec + static_cast<int64_t>(t) * q.C * 3;
                *p = (round ? *p : 0.0) + step;
            }
        }
    }
    return acc;
}

// ONE kernel per pass: the element type (`dtype`), the unit (`elems` elements, with_unit) and `active` are launch-uniform, scalar
// branches.  (One kernel for the four element types, as strided_gather_forward is one for its element sizes: the library's kernel
// count is capped by a test, and the bodies share nothing at run time -- a launch runs exactly one of them.)
template <typename T>
__device__ __forceinline__ void forward_of(const InterlaceParams &q, const char *__restrict__ x, const void *__restrict__ w,
                                           char *__restrict__ out, int elems) {
    with_unit<16 / static_cast<int>(sizeof(typename T::S))>(elems, [&](auto e) { forward_body<T, decltype(e)::value>(q, x, w, out); });
}

__global__ __launch_bounds__(kThreads) void tinterlace_forward(InterlaceParams q, const char *__restrict__ x, const void *__restrict__ w,
                                                              char *__restrict__ out, int elems, int dtype) {
    switch (dtype) {
    case SHIFTND_F32: forward_of<f32_t>(q, x, w, out, elems); break;
    case SHIFTND_F64: forward_of<f64_t>(q, x, w, out, elems); break;
    case SHIFTND_F16: forward_of<f16_t>(q, x, w, out, elems); break;
    default: forward_of<bf16_t>(q, x, w, out, elems); break;
    }
}

template <typename T>
__device__ __forceinline__ double backward_of(const InterlaceParams &q, const char *__restrict__ go, const char *__restrict__ x,
                                              const void *__restrict__ w, char *__restrict__ gx, double *__restrict__ ws, uint32_t n,
                                              uint32_t c, uint32_t chunk, int elems) {
    double acc = 0.0;
    with_unit<16 / static_cast<int>(sizeof(typename T::S))>(
        elems, [&](auto e) { acc = backward_body<T, decltype(e)::value>(q, go, x, w, gx, ws, n, c, chunk); });
    return acc;
}

__global__ __launch_bounds__(kThreads) void tinterlace_backward(InterlaceParams q, const char *__restrict__ go,
                                                               const char *__restrict__ x, const void *__restrict__ w,
                                                               char *__restrict__ gx, double *__restrict__ ws, int elems, int dtype) {
    __shared__ double scratch[kThreads / 64];
    const uint32_t line = fdiv(blockIdx.x, q.d_chunks), chunk = blockIdx.x - line * q.chunks;
    const uint32_t n = fdiv(line, q.d_C), c = line - n * q.C;
    double acc;
    switch (dtype) {
    case SHIFTND_F32: acc = backward_of<f32_t>(q, go, x, w, gx, ws, n, c, chunk, elems); break;
    case SHIFTND_F64: acc = backward_of<f64_t>(q, go, x, w, gx, ws, n, c, chunk, elems); break;
    case SHIFTND_F16: acc = backward_of<f16_t>(q, go, x, w, gx, ws, n, c, chunk, elems); break;
    default: acc = backward_of<bf16_t>(q, go, x, w, gx, ws, n, c, chunk, elems); break;
    }
    const double total = block_sum(acc, scratch);
    // group `chunk` of the N * C entries n * C + c (tshift_backward's record under a per-clip table)
    if (threadIdx.x == 0) ws[((static_cast<size_t>(chunk) * q.clips + n) * q.C + c) * 3] = total;
}

int64_t chunks_of(const Geometry &g, int dtype) { return (frame_pixels(g) * dtype_size(dtype) + kChunkBytes - 1) / kChunkBytes; }

InterlaceParams make_params(const Geometry &g, int dtype, int wkind, int unit) {
    InterlaceParams q;
    q.pad = g.pad;
    q.wkind = wkind;
    q.active = g.active;
    q.T = static_cast<uint32_t>(g.S[3 - g.nd]);
    q.C = static_cast<uint32_t>(g.C);
    q.clips = static_cast<uint32_t>(g.N);
    q.plane_bytes = frame_pixels(g) * dtype_size(dtype);
    q.upp = static_cast<uint32_t>(q.plane_bytes / unit);
    q.chunks = static_cast<uint32_t>(chunks_of(g, dtype));
    q.scales = g.N * g.C;
    q.planes = g.N * q.T * g.C;
    q.units = q.planes * static_cast<int64_t>(q.upp);
    q.step_records = static_cast<int64_t>(q.chunks) * g.N * g.C * 3;
    q.d_upp = make_fastdiv(q.upp);
    q.d_C = make_fastdiv(q.C);
    q.d_T = make_fastdiv(q.T);
    q.d_per = make_fastdiv(static_cast<uint32_t>(map_period(static_cast<int>(q.T), g.pad)));
    q.d_chunks = make_fastdiv(q.chunks);
    return q;
}

void launch_forward(const InterlaceParams &q, int dtype, const void *x, const void *w, void *out, int unit, hipStream_t st) {
    const int64_t per = kThreads * fwd_in_flight_of(dtype);
    hipLaunchKernelGGL(tinterlace_forward, dim3(static_cast<unsigned>((q.units + per - 1) / per)), dim3(kThreads), 0, st, q,
                       static_cast<const char *>(x), w, static_cast<char *>(out), unit / dtype_size(dtype), dtype);
}

void launch_backward(const InterlaceParams &q, int dtype, int64_t lines, const void *go, const void *x, const void *w, void *gx,
                     double *ws, int unit, hipStream_t st) {
    hipLaunchKernelGGL(tinterlace_backward, dim3(static_cast<unsigned>(lines * q.chunks)), dim3(kThreads), 0, st, q,
                       static_cast<const char *>(go), static_cast<const char *>(x), w, static_cast<char *>(gx), ws,
                       unit / dtype_size(dtype), dtype);
}

}  // namespace

int tinterlace_forward(const Geometry &g, int dtype, const void *x, const void *w, int wkind, void *out, hipStream_t st) {
    const int unit = piece_bytes(frame_pixels(g) * dtype_size(dtype), {x, out});
    const InterlaceParams q = make_params(g, dtype, wkind, unit);
    note_kernel(unit == 16 ? "tinterlace_forward" : "tinterlace_forward_ragged");
    launch_forward(q, dtype, x, w, out, unit, st);
    return SHIFTND_OK;
}

// both partial sets, 3 doubles a record (launch_reduce_weight_grads' shape): chunks * N * C for the offsets, 4 * chunks * N * T * C for
// the scales -- a function of the geometry alone
size_t tinterlace_backward_workspace(const Geometry &g, int dtype) {
    const int64_t chunks = chunks_of(g, dtype), T = g.S[3 - g.nd];
    return static_cast<size_t>(chunks * g.N * g.C * (1 + kWaves * T)) * 3 * sizeof(double);
}

int tinterlace_backward(const Geometry &g, int dtype, const void *go, const void *x, const void *w, int wkind, void *gx, void *gw,
                        void *workspace, hipStream_t st) {
    const int unit = piece_bytes(frame_pixels(g) * dtype_size(dtype), {go, x, gx});
    const InterlaceParams q = make_params(g, dtype, wkind, unit);
    double *ws = static_cast<double *>(workspace);
    note_kernel(unit == 16 ? "tinterlace_backward" : "tinterlace_backward_ragged");
    const int64_t lines = g.N * g.C;
    launch_backward(q, dtype, lines, go, x, w, gx, ws, unit, st);
    // the packed gradient: [N, C] offsets (chunks groups), then [N, T, C] scales (4 * chunks groups), in the table's type
    launch_reduce_weight_grads(wkind, ws, static_cast<int>(q.chunks), static_cast<int>(q.scales), 1, gw, st);
    launch_reduce_weight_grads(wkind, ws + q.step_records, static_cast<int>(q.chunks) * kWaves, static_cast<int>(q.planes), 1,
                               static_cast<char *>(gw) + q.scales * dtype_size(wkind), st);
    return SHIFTND_OK;
}

}  // namespace shiftnd
