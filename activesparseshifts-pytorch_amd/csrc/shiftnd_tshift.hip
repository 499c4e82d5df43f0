// shiftnd_tshift.hip -- the LEARNABLE temporal shift: a 1-D sparse / interpolating shift along dim S0 of "segment-major" tensors
// (memory order N, S0, C, S1, S2), one weight per channel (gfx950).  SHIFTND_SHIFT_DIM0 on p->dtype selects it.
//
// A video tensor [N*T, C, H, W] whose clips of T frames are shifted along T by a TRAINED per-channel offset is, seen as a shift
// problem, [N, C, T, H*W] with strides {T*C*M, M, C*M, 1} and weights (w_c, 0).  The arithmetic is the library's 1-D one applied
// along the segment dim: prep_shift_forward / prep_shift_backward, interp_t<T, 1>, weight_grads_nd<1>.  Shift, fraction and the
// source segments are the same for a whole plane (n, t, c) of M contiguous elements, so the kernels work on planes:
//
//   tshift_forward   flat over the output in aligned units, four in flight per thread.  Per unit: its plane by three multiply-shift
//                    divisions, the channel's weight, the two source segments pad(t - iw), pad(t - iw + 1) (fold_index o
//                    canon_shift); nontemporal loads of the two source units (none for a filled plane; the second one not at all
//                    for the sparse shift, whose result is the source's bit pattern), widened, interpolated, rounded once,
//                    nontemporal store.
//   tshift_backward  a walk: a workgroup owns 8 KiB of the M elements of one (n, c) line and steps through t.  With
//                    A(t) = pad(t - sh), B(t) = pad(t + 1 - sh) = A(t + 1) the "+1" corners of step t are the "+0" corners of
//                    step t + 1 and stay in registers: per step one unit of x (and, interpolating, one of grad_out) at B(t) and
//                    the gradient's own unit at t are loaded, grad_x is stored once.  The sparse shift's grad_x is the unit of
//                    grad_out at pad(t + sh), bit for bit.  Every index is workgroup-uniform (scalar).  grad_out is read twice by
//                    the SAME workgroup, |sh| steps apart -- the second read is an L2 hit, so the loads are plain ones.
//                    grad_w: per thread an fp64 sum of grad_out * (x[B] - x[A]) (difference and product in fp64), one block_sum per workgroup, partial
//                    (group * C + c) * 3 + 0 with group = n * chunks + chunk, finished by launch_reduce_weight_grads: fixed order,
//                    deterministic.
//
// Units.  A unit is U = 16, 8, 4 or 2 bytes (at least one element): the largest power of two that divides the plane's bytes and
// every base address, so planes are made of whole, naturally aligned units and no unit holds two planes (two weights).  U = 16 is
// the whole-piece form (tshift_forward / tshift_backward); anything smaller -- 14 x 14 (8 bytes) and 7 x 7 (2 bytes) planes of
// 16-bit elements, bases one element off the 16-byte grid -- is the ragged form (*_ragged): the same code on narrower units,
// correct everywhere, never outside the tensors, slower.  U is launch-uniform: one kernel per element type and pass (8 kernels),
// `active` a run-time argument too.  No LDS beyond block_sum's, no scratch.
//
// Per-clip tables (SHIFTND_PER_CLIP).  `weights` / `grad_w` of shape [N, C], one row per clip: the same kernels under a
// launch-uniform row stride (TShiftParams::wrow: 0 for the [C] table, C for [N, C]) -- the weight of (n, c) is entry n * wrow + c, one
// integer multiply-add on values both kernels hold already.  The walk's partial record moves from ((n * chunks + chunk) * C + c) to
// ((chunk * N + n) * C + c): `chunks` groups of N * C entries, so that launch_reduce_weight_grads sums per (n, c) -- the same
// records, the same workspace bytes, a fixed order.  No new kernel, no template parameter.
//
// Not built: a cut window, channels-last tensors.  (The quantized interpolating forward: shiftnd_tshift_quant.hip.)
#include "shiftnd_temporal.hpp"

namespace shiftnd {
namespace {

constexpr int kFwdInFlight = 4;     // units per thread of the forward, every load issued before the first store
constexpr int kBwdInFlight = 2;     // units per thread and step of the walk
constexpr int64_t kChunkBytes = static_cast<int64_t>(kThreads) * kBwdInFlight * 16;   // of a plane, per workgroup of the walk

struct TShiftParams {
    int pad, wkind, active;
    uint32_t T, C, upp, chunks;        // segments, channels, units per plane, workgroups per (n, c) line (backward)
    FastDiv d_upp, d_C, d_T, d_per, d_chunks;   // d_per: by map_period(T, pad)
    int64_t plane_bytes, units;        // units: of the whole tensor (forward)
    uint32_t wrow, clips;              // weight of (n, c): entry n * wrow + c -- 0 for a [C] table, C for a per-clip [N, C] one; N
                                       // (behind the fields the per-channel call reads, whose offsets stay what they were)
};

template <typename T, int E>
__device__ __forceinline__ Unit<T, E> blend_units(const Unit<T, E> &a, const Unit<T, E> &b, typename T::C d) {
    Unit<T, E> r;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const typename T::C v[2] = {widen<T>(a.e[e]), widen<T>(b.e[e])};
        r.e[e] = narrow<T>(interp_t<T, 1>(v, &d));
    }
    return r;
}

constexpr int64_t kFill = -1, kPast = -2;

template <typename T, int E>
__device__ __forceinline__ void forward_body(const TShiftParams &q, const char *__restrict__ x, const void *__restrict__ w,
                                             char *__restrict__ out) {
    using CT = typename T::C;
    constexpr int V = sizeof(typename T::S) * E;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * (kThreads * kFwdInFlight) + threadIdx.x;
    const int Tn = static_cast<int>(q.T);
    int64_t sa[kFwdInFlight], sb[kFwdInFlight];   // byte offset in x of the unit's two sources, or a mark
    CT dw[kFwdInFlight];
#pragma unroll
    for (int k = 0; k < kFwdInFlight; ++k) {
        const int64_t i = first + k * kThreads;
        sa[k] = sb[k] = kPast;
        dw[k] = CT(0);
        if (i >= q.units) continue;
        const uint32_t u = static_cast<uint32_t>(i);
        const uint32_t plane = fdiv(u, q.d_upp);
        const int64_t at = static_cast<int64_t>(u - plane * q.upp) * V;   // byte in the plane
        const uint32_t nt = fdiv(plane, q.d_C), c = plane - nt * q.C;
        const uint32_t n = fdiv(nt, q.d_T), t = nt - n * q.T;
        int64_t iw;
        prep_shift_forward<CT>(load_weight<CT>(w, q.wkind, n * q.wrow + c), q.active != 0, iw, dw[k]);
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
        // the sparse shift copies: the source's bit pattern (NaN payloads, -0)
        store_unit<T, E>(out + (first + k * kThreads) * V, q.active ? blend_units<T, E>(a[k], b[k], dw[k]) : a[k]);
    }
}

template <typename T, int E>
__device__ __forceinline__ double backward_body(const TShiftParams &q, const char *__restrict__ go, const char *__restrict__ x,
                                                const void *__restrict__ w, char *__restrict__ gx, uint32_t n, uint32_t c,
                                                uint32_t chunk) {
    using CT = typename T::C;
    constexpr int V = sizeof(typename T::S) * E;
    const int Tn = static_cast<int>(q.T);
    int64_t sh;
    CT dw;
    prep_shift_backward<CT>(load_weight<CT>(w, q.wkind, n * q.wrow + c), q.active != 0, sh, dw);
    const int cs = canon_shift(sh, Tn, q.pad, q.d_per);     // x (and, interpolating, grad_out) at pad(t - sh), pad(t + 1 - sh)
    const int csn = canon_shift(-sh, Tn, q.pad, q.d_per);   // the sparse shift's grad_x: grad_out at pad(t + sh)
    const int64_t clip = static_cast<int64_t>(n) * q.T;
    auto plane = [&](int t) { return ((clip + t) * q.C + c) * q.plane_bytes; };
    double acc = 0.0;
    // the workgroup's kChunkBytes of the plane in rounds of kThreads * kBwdInFlight units (one round for 16-byte units)
#pragma unroll 1
    for (int round = 0; round < 16 / V; ++round) {
        int64_t at[kBwdInFlight];
        bool in[kBwdInFlight];
#pragma unroll
        for (int k = 0; k < kBwdInFlight; ++k) {
            const int64_t u = (static_cast<int64_t>(chunk) * (16 / V) + round) * (kThreads * kBwdInFlight) + k * kThreads + threadIdx.x;
            in[k] = u < q.upp;
            at[k] = u * V;
        }
        Unit<T, E> xa[kBwdInFlight], ga[kBwdInFlight];
        const int s0 = source_frame(0, cs, Tn, q.pad);
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
            Unit<T, E> xb[kBwdInFlight], gb[kBwdInFlight], gv[kBwdInFlight];
#pragma unroll
            for (int k = 0; k < kBwdInFlight; ++k) {
                xb[k] = gb[k] = gv[k] = zero_unit<T, E>();
                if (!in[k]) continue;
                if (s1 >= 0) xb[k] = load_unit<T, E, false>(x + plane(s1) + at[k]);
                if (sg >= 0) gb[k] = load_unit<T, E, false>(go + plane(sg) + at[k]);
                gv[k] = load_unit<T, E, false>(go + plane(t) + at[k]);
            }
#pragma unroll
            for (int k = 0; k < kBwdInFlight; ++k) {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    // weight_grads_nd<1>, the difference taken in fp64: exact for every type but fp64 itself, so that a sum
                    // that cancels to almost nothing keeps its digits
                    const double diff = static_cast<double>(widen<T>(xb[k].e[e])) - static_cast<double>(widen<T>(xa[k].e[e]));
                    acc = fma_ct(static_cast<double>(widen<T>(gv[k].e[e])), diff, acc);
                }
                if (in[k]) store_unit<T, E>(gx + plane(t) + at[k], q.active ? blend_units<T, E>(ga[k], gb[k], dw) : gb[k]);
                xa[k] = xb[k];
                ga[k] = gb[k];
            }
        }
    }
    return acc;
}

// ONE kernel per element type and pass: the unit (`elems` elements, with_unit) and `active` are launch-uniform, scalar branches
template <typename T>
__global__ __launch_bounds__(kThreads) void tshift_forward(TShiftParams q, const char *__restrict__ x, const void *__restrict__ w,
                                                          char *__restrict__ out, int elems) {
    with_unit<16 / static_cast<int>(sizeof(typename T::S))>(elems, [&](auto e) { forward_body<T, decltype(e)::value>(q, x, w, out); });
}

template <typename T>
__global__ __launch_bounds__(kThreads) void tshift_backward(TShiftParams q, const char *__restrict__ go, const char *__restrict__ x,
                                                           const void *__restrict__ w, char *__restrict__ gx,
                                                           double *__restrict__ partials, int elems) {
    __shared__ double scratch[kThreads / 64];
    const uint32_t line = fdiv(blockIdx.x, q.d_chunks), chunk = blockIdx.x - line * q.chunks;
    const uint32_t n = fdiv(line, q.d_C), c = line - n * q.C;
    double acc = 0.0;
    with_unit<16 / static_cast<int>(sizeof(typename T::S))>(
        elems, [&](auto e) { acc = backward_body<T, decltype(e)::value>(q, go, x, w, gx, n, c, chunk); });
    const double total = block_sum(acc, scratch);
    // group n * chunks + chunk of C channels, or -- a per-clip table -- group chunk of the N * C entries n * C + c
    const uint32_t group = q.wrow ? chunk * q.clips + n : n * q.chunks + chunk;   // (below 2^31: the reduction counts groups in an int)
    if (threadIdx.x == 0) partials[(static_cast<size_t>(group) * q.C + c) * 3] = total;
}

TShiftParams make_params(const Geometry &g, int dtype, int wkind, int unit, bool per_clip) {
    TShiftParams q;
    q.pad = g.pad;
    q.wkind = wkind;
    q.active = g.active;
    q.T = static_cast<uint32_t>(g.S[3 - g.nd]);
    q.C = static_cast<uint32_t>(g.C);
    q.wrow = per_clip ? q.C : 0;
    q.clips = static_cast<uint32_t>(g.N);
    q.plane_bytes = frame_pixels(g) * dtype_size(dtype);
    q.upp = static_cast<uint32_t>(q.plane_bytes / unit);
    q.chunks = static_cast<uint32_t>((q.plane_bytes + kChunkBytes - 1) / kChunkBytes);
    q.units = g.N * q.T * q.C * static_cast<int64_t>(q.upp);
    q.d_upp = make_fastdiv(q.upp);
    q.d_C = make_fastdiv(q.C);
    q.d_T = make_fastdiv(q.T);
    q.d_per = make_fastdiv(static_cast<uint32_t>(map_period(static_cast<int>(q.T), g.pad)));
    q.d_chunks = make_fastdiv(q.chunks);
    return q;
}

template <typename T>
void launch_forward(const TShiftParams &q, const void *x, const void *w, void *out, int unit, hipStream_t st) {
    const int64_t per = kThreads * kFwdInFlight;
    hipLaunchKernelGGL((tshift_forward<T>), dim3(static_cast<unsigned>((q.units + per - 1) / per)), dim3(kThreads), 0, st, q,
                       static_cast<const char *>(x), w, static_cast<char *>(out), unit / static_cast<int>(sizeof(typename T::S)));
}

template <typename T>
void launch_backward(const TShiftParams &q, int64_t lines, const void *go, const void *x, const void *w, void *gx, double *partials,
                     int unit, hipStream_t st) {
    hipLaunchKernelGGL((tshift_backward<T>), dim3(static_cast<unsigned>(lines * q.chunks)), dim3(kThreads), 0, st, q,
                       static_cast<const char *>(go), static_cast<const char *>(x), w, static_cast<char *>(gx), partials,
                       unit / static_cast<int>(sizeof(typename T::S)));
}

}  // namespace

// the geometry SHIFTND_SHIFT_DIM0 accepts: 2 or 3 spatial dims, the whole window, segment_forward_eligible's 32-bit limits
bool tshift_geometry_ok(const Geometry &g, int dtype) {
    return dtype <= SHIFTND_BF16 && g.nd >= 2 && !cropped(g) && segment_counts_fit(g, dtype_size(dtype));
}

bool tshift_tensor_ok(const Geometry &g, int dtype, const void *p, const int64_t *strides) {
    return aligned_to(p, dtype_size(dtype)) && dense_segment_major(g, strides);
}

int tshift_forward(const Geometry &g, int dtype, const void *x, const void *w, int wkind, bool per_clip, void *out, hipStream_t st) {
    const int unit = piece_bytes(frame_pixels(g) * dtype_size(dtype), {x, out});
    const TShiftParams q = make_params(g, dtype, wkind, unit, per_clip);
    note_kernel(unit == 16 ? "tshift_forward" : "tshift_forward_ragged");
    switch (dtype) {
    case SHIFTND_F32: launch_forward<f32_t>(q, x, w, out, unit, st); break;
    case SHIFTND_F64: launch_forward<f64_t>(q, x, w, out, unit, st); break;
    case SHIFTND_F16: launch_forward<f16_t>(q, x, w, out, unit, st); break;
    default: launch_forward<bf16_t>(q, x, w, out, unit, st); break;
    }
    return SHIFTND_OK;
}

size_t tshift_backward_workspace(const Geometry &g, int dtype) {
    const int64_t plane_bytes = frame_pixels(g) * dtype_size(dtype);
    return static_cast<size_t>(g.N * ((plane_bytes + kChunkBytes - 1) / kChunkBytes) * g.C) * 3 * sizeof(double);
}

int tshift_backward(const Geometry &g, int dtype, const void *go, const void *x, const void *w, int wkind, bool per_clip, void *gx,
                    void *gw, void *workspace, hipStream_t st) {
    const int unit = piece_bytes(frame_pixels(g) * dtype_size(dtype), {go, x, gx});
    const TShiftParams q = make_params(g, dtype, wkind, unit, per_clip);
    double *partials = static_cast<double *>(workspace);
    note_kernel(unit == 16 ? "tshift_backward" : "tshift_backward_ragged");
    const int64_t lines = g.N * g.C;
    switch (dtype) {
    case SHIFTND_F32: launch_backward<f32_t>(q, lines, go, x, w, gx, partials, unit, st); break;
    case SHIFTND_F64: launch_backward<f64_t>(q, lines, go, x, w, gx, partials, unit, st); break;
    case SHIFTND_F16: launch_backward<f16_t>(q, lines, go, x, w, gx, partials, unit, st); break;
    default: launch_backward<bf16_t>(q, lines, go, x, w, gx, partials, unit, st); break;
    }
    // [C] table: N * chunks groups of C entries; [N, C] table: chunks groups of N * C entries (the same records, the same bytes)
    const int64_t groups = per_clip ? q.chunks : g.N * q.chunks, entries = per_clip ? g.N * g.C : g.C;
    launch_reduce_weight_grads(wkind, partials, static_cast<int>(groups), static_cast<int>(entries), 1, gw, st);
    return SHIFTND_OK;
}

}  // namespace shiftnd
