// shiftnd_frames_learn.hip -- the LEARNABLE temporal shift of channels-last tensors: memory order N, S0, S1, S2, C (gfx950).
// SHIFTND_SHIFT_DIM0 | SHIFTND_FRAMES on p->dtype selects it.
//
// The problem is the one of shiftnd_tshift.hip -- a 1-D sparse / interpolating shift along S0 (the T frames of a clip), one weight
// per channel, the arithmetic of prep_shift_forward / prep_shift_backward, interp_t<T, 1>, weight_grads_nd<1> -- on the layout of
// shiftnd_frames.hip: a pixel's channel row is contiguous, so a 16-byte piece of it holds 2 to 8 channels with DIFFERENT weights.
// Source frames and fractions are per element, not per plane.  A thread keeps its piece column k of the rows for its whole life
// and reads the piece's weights once; a piece whose elements share their source frames ("uniform": the TSM-like tables) is moved
// with one 16-byte load per source, any other piece ("mixed": a trained table) element by element with element-sized loads from
// each element's own frames.  Both are exact; the fraction is per element in both.
//
//   frames_active_forward  the shape of frames_forward: a workgroup inside ONE frame (n, t), max(1, 256 / P) rows per step.  Per
//                          output piece the two sources fold_index(t - cs), fold_index(t + 1 - cs) of each element, kFwdInFlight
//                          pieces per thread with every load issued before the first store; widened, interpolated, rounded once.
//                          (The sparse forward under the flag is frames_forward itself.)
//   frames_backward        a walk, as tshift_backward: a workgroup owns rows_per_wg pixel rows of ONE clip n and a thread walks
//                          its piece through t = 0 .. T-1.  With A(t) = pad(t - sh), B(t) = pad(t + 1 - sh) = A(t + 1) the "+1"
//                          sources of step t are the "+0" sources of step t + 1 and stay in registers: per step the piece of x
//                          (and, interpolating, of grad_out) at B(t) and the gradient's own piece at t are loaded, grad_x is
//                          stored once.  The sparse shift's grad_x is grad_out at pad(t + sh), bit for bit.  grad_out is read
//                          twice by the same thread, |sh| steps apart: plain loads, the second one a cache hit.
//                          grad_w: ONE fp64 sum per element of the thread's piece of grad_out * (x[B] - x[A]) (difference and
//                          product in fp64), summed over the workgroup's rows in LDS in a fixed order, one partial record
//                          (group * C + c) * 3 with group = n * chunks + chunk, finished by launch_reduce_weight_grads.
//                          A per-clip table (SHIFTND_CLIP_FRAMES: [N, C], FramesLearnParams::wrow = C) re-indexes the same
//                          records as ((chunk * N + n) * C + c) * 3: `chunks` groups of N * C entries, one sum per (n, c).
//                          Deviation from the clip tile in LDS: no LDS staging, hence no limit on T and no refusal for it.
//
// ONE kernel per pass: the element type and the piece (`elems` elements, 16 bytes down to one element) are launch-uniform
// run-time switches over instantiations of one body; shiftnd_last_kernel() names the form, *_ragged for pieces under 16 bytes.
// Every access is naturally aligned and inside the tensors' bytes; the weights are read at entries [0, C) only.  No scratch.
#include "shiftnd_frames_learn.hpp"   // FramesLearnParams, gather_unit, blend_units, with_type_and_unit, make_params

namespace shiftnd {
namespace {

constexpr int kFwdInFlight = 4;        // pieces per thread of the forward, every load issued before the first store
constexpr int64_t kWantWorkgroups = 6144;   // the forward cuts frames into more workgroups while its grid is short of this many (as frames_forward)
constexpr int kMaxRowSteps = 8;        // the backward's workgroup walks at most this many steps of rows ...
constexpr int64_t kWantGroups = 2048;  // ... fewer while the grid is short of this many workgroups (8 per CU)

template <typename T, int E>
__device__ __forceinline__ void forward_body(const FramesLearnParams &q, const char *__restrict__ x, const void *__restrict__ table,
                                             char *__restrict__ out) {
    using CT = typename T::C;
    constexpr int V = sizeof(typename T::S) * E;
    const uint32_t frame = fdiv(blockIdx.x, q.d_chunks);   // n * T + t
    const uint32_t chunk = blockIdx.x - frame * q.chunks;
    const uint32_t n = fdiv(frame, q.d_T);
    const int t = static_cast<int>(frame - n * q.T), Tn = static_cast<int>(q.T);
    const void *const w = table_row(table, q.wkind, n, q.wrow);   // the clip's row of the table: once per workgroup, scalar
    const uint32_t rl = fdiv(threadIdx.x, q.d_span);       // the thread's row of a step, its piece of the row
    const uint32_t k0 = threadIdx.x - rl * q.span;
    if (rl >= q.rps) return;                               // (idle tail lanes where P does not divide 256)
    const int64_t first_row = static_cast<int64_t>(chunk) * q.rows_per_wg;
    const int rows = static_cast<int>(first_row + q.rows_per_wg < q.M ? q.rows_per_wg : q.M - first_row);
    const int rps = static_cast<int>(q.rps);
    const int64_t here = static_cast<int64_t>(frame) * q.frame_bytes + first_row * q.R;     // the workgroup's rows of the output
    const int64_t clip = static_cast<int64_t>(n) * q.T * q.frame_bytes + first_row * q.R;   // the same rows of the clip's frame 0
    const int64_t step = static_cast<int64_t>(q.rps) * q.R;
#pragma unroll 1
    for (uint32_t k = k0; k < q.P; k += kThreads) {        // (once unless a row has more than 256 pieces)
        int sa[E], sb[E];
        CT dw[E];
        bool uniform = true;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            int64_t iw;
            prep_shift_forward<CT>(load_weight<CT>(w, q.wkind, static_cast<int64_t>(k) * E + e), true, iw, dw[e]);
            const int cs = canon_shift(iw, Tn, q.pad, q.d_per);
            sa[e] = source_frame(t, cs, Tn, q.pad);
            sb[e] = source_frame(t + 1, cs, Tn, q.pad);
            uniform = uniform && sa[e] == sa[0] && sb[e] == sb[0];
        }
        const int64_t column = static_cast<int64_t>(k) * V;
        int64_t off = static_cast<int64_t>(rl) * q.R + column;
        if (uniform) {
            const char *srca = x + clip + (sa[0] < 0 ? 0 : sa[0]) * q.frame_bytes, *srcb = x + clip + (sb[0] < 0 ? 0 : sb[0]) * q.frame_bytes;
#pragma unroll 1
            for (int r = static_cast<int>(rl); r < rows; r += rps * kFwdInFlight) {
                Unit<T, E> a[kFwdInFlight], b[kFwdInFlight];
#pragma unroll
                for (int j = 0; j < kFwdInFlight; ++j) {
                    a[j] = b[j] = zero_unit<T, E>();
                    if (r + j * rps < rows) {   // (a fill issues no load)
                        if (sa[0] >= 0) a[j] = load_unit<T, E, true>(srca + off + j * step);
                        if (sb[0] >= 0) b[j] = load_unit<T, E, true>(srcb + off + j * step);
                    }
                }
#pragma unroll
                for (int j = 0; j < kFwdInFlight; ++j)
                    if (r + j * rps < rows) store_unit<T, E>(out + here + off + j * step, blend_units<T, E>(a[j], b[j], dw));
                off += kFwdInFlight * step;
            }
        } else {
            // mixed: each element from its own two frames, one row at a time (2 E element loads in flight)
#pragma unroll 1
            for (int r = static_cast<int>(rl); r < rows; r += rps) {
                const Unit<T, E> a = gather_unit<T, E, false>(x + clip + off, sa, false, q.frame_bytes);
                const Unit<T, E> b = gather_unit<T, E, false>(x + clip + off, sb, false, q.frame_bytes);
                store_unit<T, E>(out + here + off, blend_units<T, E>(a, b, dw));
                off += step;
            }
        }
    }
}

// `red`: kThreads * kMaxElems doubles of LDS
template <typename T, int E>
__device__ __forceinline__ void backward_body(const FramesLearnParams &q, const char *__restrict__ go, const char *__restrict__ x,
                                              const void *__restrict__ table, char *__restrict__ gx, double *__restrict__ partials,
                                              double *red) {
    using CT = typename T::C;
    constexpr int V = sizeof(typename T::S) * E;
    const int Tn = static_cast<int>(q.T);
    const uint32_t n = fdiv(blockIdx.x, q.d_chunks), chunk = blockIdx.x - n * q.chunks;
    const void *const w = table_row(table, q.wkind, n, q.wrow);   // the clip's row of the table: once per workgroup, scalar
    const uint32_t rl = fdiv(threadIdx.x, q.d_span), k0 = threadIdx.x - rl * q.span;
    const int64_t first_row = static_cast<int64_t>(chunk) * q.rows_per_wg;
    const int rows = static_cast<int>(first_row + q.rows_per_wg < q.M ? q.rows_per_wg : q.M - first_row);
    const int rps = static_cast<int>(q.rps);
    const int64_t clip = static_cast<int64_t>(n) * q.T * q.frame_bytes + first_row * q.R;   // the workgroup's rows of the clip's frame 0
    // a per-clip table: `chunks` groups of N * C entries, so that the reduction sums per (n, c) -- as tshift_backward
    const size_t group = q.wrow ? static_cast<size_t>(chunk) * q.clips + n : static_cast<size_t>(n) * q.chunks + chunk;
#pragma unroll 1
    for (uint32_t kb = 0; kb < q.P; kb += kThreads) {      // (once unless a row has more than 256 pieces; uniform: barriers inside)
        const uint32_t k = kb + k0;
        const bool mine = rl < q.rps && k < q.P;
        double acc[E];
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] = 0.0;
        if (mine) {
            int cs[E], csn[E];   // x (and, interpolating, grad_out) at pad(t - sh), pad(t + 1 - sh); the sparse grad_x: grad_out at pad(t + sh)
            CT dw[E];
            bool uniform = true;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                int64_t sh;
                prep_shift_backward<CT>(load_weight<CT>(w, q.wkind, static_cast<int64_t>(k) * E + e), q.active != 0, sh, dw[e]);
                cs[e] = canon_shift(sh, Tn, q.pad, q.d_per);
                csn[e] = canon_shift(-sh, Tn, q.pad, q.d_per);
                uniform = uniform && cs[e] == cs[0] && csn[e] == csn[0];
            }
            const int64_t column = static_cast<int64_t>(k) * V;
#pragma unroll 1
            for (int r = static_cast<int>(rl); r < rows; r += rps) {
                const int64_t at = clip + r * q.R + column;
                int s1[E], sg[E];
#pragma unroll
                for (int e = 0; e < E; ++e) s1[e] = source_frame(0, cs[e], Tn, q.pad);
                Unit<T, E> xa = gather_unit<T, E, false>(x + at, s1, uniform, q.frame_bytes), ga = zero_unit<T, E>();
                if (q.active) ga = gather_unit<T, E, false>(go + at, s1, uniform, q.frame_bytes);
#pragma unroll 1
                for (int t = 0; t < Tn; ++t) {
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        s1[e] = source_frame(t + 1, cs[e], Tn, q.pad);
                        sg[e] = q.active ? s1[e] : source_frame(t, csn[e], Tn, q.pad);
                    }
                    const Unit<T, E> xb = gather_unit<T, E, false>(x + at, s1, uniform, q.frame_bytes);
                    const Unit<T, E> gb = gather_unit<T, E, false>(go + at, sg, uniform, q.frame_bytes);
                    const Unit<T, E> gv = load_unit<T, E, false>(go + at + t * q.frame_bytes);
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        // weight_grads_nd<1>, the difference taken in fp64 (as tshift_backward)
                        const double diff = static_cast<double>(widen<T>(xb.e[e])) - static_cast<double>(widen<T>(xa.e[e]));
                        acc[e] = fma_ct(static_cast<double>(widen<T>(gv.e[e])), diff, acc[e]);
                    }
                    store_unit<T, E>(gx + at + t * q.frame_bytes, q.active ? blend_units<T, E>(ga, gb, dw) : gb);
                    xa = xb;
                    ga = gb;
                }
            }
        }
        // the rows of the workgroup: threads rl = 0 .. rps-1 hold the same piece column, summed in that order
        __syncthreads();
#pragma unroll
        for (int e = 0; e < E; ++e) red[e * kThreads + threadIdx.x] = acc[e];
        __syncthreads();
        if (mine && rl == 0) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                double total = 0.0;
#pragma unroll 1
                for (uint32_t j = 0; j < q.rps; ++j) total += red[e * kThreads + j * q.span + k0];
                partials[(group * q.C + static_cast<size_t>(k) * E + e) * 3] = total;
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void frames_active_forward(FramesLearnParams q, const char *__restrict__ x,
                                                                 const void *__restrict__ w, char *__restrict__ out) {
    with_type_and_unit(q.dtype, q.elems, [&](auto ty, auto e) { forward_body<decltype(ty), decltype(e)::value>(q, x, w, out); });
}

__global__ __launch_bounds__(kThreads) void frames_backward(FramesLearnParams q, const char *__restrict__ go,
                                                           const char *__restrict__ x, const void *__restrict__ w,
                                                           char *__restrict__ gx, double *__restrict__ partials) {
    __shared__ double red[kThreads * kMaxElems];
    with_type_and_unit(q.dtype, q.elems,
                       [&](auto ty, auto e) { backward_body<decltype(ty), decltype(e)::value>(q, go, x, w, gx, partials, red); });
}

// rows of a backward workgroup: from the geometry alone (the workspace query has no pointers), as if the pieces were 16 bytes
int64_t backward_rows_per_wg(const Geometry &g, int dtype) {
    const int64_t M = frame_pixels(g), pieces = (g.C * dtype_size(dtype) + 15) / 16;
    const int64_t rps = pieces < kThreads ? kThreads / pieces : 1;
    int64_t steps = kMaxRowSteps;
    while (steps > 1 && g.N * ((M + rps * steps - 1) / (rps * steps)) < kWantGroups) steps /= 2;
    return rps * steps;
}
int64_t backward_chunks(const Geometry &g, int dtype) {
    const int64_t rows = backward_rows_per_wg(g, dtype);
    return (frame_pixels(g) + rows - 1) / rows;
}

}  // namespace

// The sizes the kernels' index arithmetic needs (include/shiftnd_hip.h states them): those of frames_geometry_ok, and for the
// backward N * chunks workgroups / partial groups below 2^31 with the records below 2^46 bytes.
bool frames_learn_geometry_ok(const Geometry &g, int dtype) {
    if (dtype < SHIFTND_F32 || dtype > SHIFTND_BF16) return false;
    Geometry s = g;
    s.active = 0;
    if (!frames_geometry_ok(s, dtype)) return false;
    if (g.N == 0 || g.C == 0 || g.S[0] * g.S[1] * g.S[2] == 0) return true;
    const int64_t groups = g.N * backward_chunks(g, dtype);   // (N and chunks <= M are below 2^31: no overflow)
    return groups < (1LL << 31) && groups <= (1LL << 46) / (g.C * 24);
}

int frames_active_forward(const Geometry &g, int dtype, const void *x, const void *w, int wkind, bool per_clip, void *out,
                          hipStream_t st) {
    const int unit = piece_bytes(g.C * dtype_size(dtype), {x, out});
    FramesLearnParams q = make_params(g, dtype, wkind, unit, per_clip);
    // workgroups per frame: at least one batch of kFwdInFlight steps each, more steps while the grid is large
    const int64_t frames = g.N * q.T, batch_rows = static_cast<int64_t>(q.rps) * kFwdInFlight;
    const int64_t most = (q.M + batch_rows - 1) / batch_rows;
    const int64_t wanted = (kWantWorkgroups + frames - 1) / frames;
    const int64_t chunks = most < wanted ? most : wanted;
    q.rows_per_wg = static_cast<uint32_t>(((q.M + chunks - 1) / chunks + batch_rows - 1) / batch_rows * batch_rows);
    q.chunks = static_cast<uint32_t>((q.M + q.rows_per_wg - 1) / q.rows_per_wg);
    q.d_chunks = make_fastdiv(q.chunks);
    note_kernel(unit == 16 ? "frames_active_forward" : "frames_active_forward_ragged");
    void (*const kernel)(FramesLearnParams, const char *, const void *, char *) = frames_active_forward;   // (the kernel, not this function)
    const int64_t blocks = frames * q.chunks;   // (below 2^31: frames is, and a frame is cut only while the grid is short of 6144)
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, st, q, static_cast<const char *>(x), w,
                       static_cast<char *>(out));
    return SHIFTND_OK;
}

size_t frames_backward_workspace(const Geometry &g, int dtype) {
    return static_cast<size_t>(g.N * backward_chunks(g, dtype) * g.C) * 3 * sizeof(double);
}

int frames_backward(const Geometry &g, int dtype, const void *go, const void *x, const void *w, int wkind, bool per_clip, void *gx,
                    void *gw, void *workspace, hipStream_t st) {
    const int unit = piece_bytes(g.C * dtype_size(dtype), {go, x, gx});
    FramesLearnParams q = make_params(g, dtype, wkind, unit, per_clip);
    q.rows_per_wg = static_cast<uint32_t>(backward_rows_per_wg(g, dtype));
    q.chunks = static_cast<uint32_t>(backward_chunks(g, dtype));
    q.d_chunks = make_fastdiv(q.chunks);
    double *partials = static_cast<double *>(workspace);
    note_kernel(unit == 16 ? "frames_backward" : "frames_backward_ragged");
    void (*const kernel)(FramesLearnParams, const char *, const char *, const void *, char *, double *) = frames_backward;
    const int64_t groups = g.N * q.chunks;   // (below 2^31: frames_learn_geometry_ok)
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(groups)), dim3(kThreads), 0, st, q, static_cast<const char *>(go),
                       static_cast<const char *>(x), w, static_cast<char *>(gx), partials);
    // (per clip: N * C entries below 2^31 -- the caller has checked)
    const int64_t sums = per_clip ? q.chunks : groups, entries = per_clip ? g.N * g.C : g.C;
    launch_reduce_weight_grads(wkind, partials, static_cast<int>(sums), static_cast<int>(entries), 1, gw, st);
    return SHIFTND_OK;
}

}  // namespace shiftnd
