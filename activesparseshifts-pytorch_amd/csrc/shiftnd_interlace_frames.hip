// shiftnd_interlace_frames.hip -- temporal INTERLACING (TIN, arXiv 2001.06499) of channels-last tensors: memory order N, S0, S1, S2,
// C (gfx950).  SHIFTND_SHIFT_DIM0 | SHIFTND_INTERLACE_FRAMES on p->dtype selects it.
//
//   out[n, t, :, c] = scale[n, t, c] * shift(x)[n, t, :, c]          shift: the per-clip op under offsets[n, c], out[t] = x[t - w]
//
// The problem of shiftnd_interlace.hip on the layout of shiftnd_frames_learn.hip.  `weights` is the packed array of
// SHIFTND_INTERLACE: the N * C offsets [N, C] followed by the N * T * C scales [N, T, C]; `grad_w` has the same layout.  A pixel's
// channel row is contiguous, so a piece of it holds E channels with E offsets and, per frame, E scales: the scales of a thread's
// piece in frame (n, t) are the E CONTIGUOUS entries (n * T + t) * C + k * E of the scales, in the table's type.
//
//   frames_interlace_forward   forward_body of frames_active_forward under the clip's row of the offsets, in both modes (the sparse
//                              shift needs the multiply too).  A thread lies inside one frame, reads its piece's E scales once and
//                              applies them per element AFTER the lerp, a multiply of its own; 16-bit elements are widened, blended,
//                              scaled and rounded once; a filled element is 0 * scale.  Uniform pieces: 16-byte loads, in-flight
//                              pieces per thread as tinterlace_forward has them (2 for 16-bit elements, 4 otherwise).
//   frames_interlace_backward  frames_backward's walk along t with the carry in registers, the loops turned inside out: a
//                              workgroup owns rows_per_wg pixel rows of ONE clip and takes them in rounds of kSteps row steps
//                              (rps rows a step).  Within a round t is the OUTER loop and the round's row steps the inner one; the
//                              carried pieces of every row step (x and, interpolating, grad_out at A(t)) stay in registers.  Every
//                              gradient piece is multiplied per element by the scales of ITS OWN frame before use (a filled
//                              frame by 1: its zeros stay +0), so grad_x is the per-clip backward of scales * grad_out.  Sums:
//                                offsets   per thread and element, fp64, over the whole walk: (s[t] g[t]) * (x[B] - x[A]); once per
//                                          piece column through `red`, record (chunk * N + n) * C + c (frames_backward's
//                                          under a per-clip table, but dense: one double a record).
//                                scales    per step t: g[t] * y[t], y[t] the compute-type blend of the x pieces the walk holds,
//                                          unrounded -- fp64 from the first product on, over the thread's row steps of the round in
//                                          registers, then over the workgroup's rows through `red` in a fixed order: one barrier
//                                          pair per t and round.  Record chunk * N * T * C + (n * T + t) * C + c behind the
//                                          offsets' records; a later round adds to the record the same thread wrote a round
//                                          before.
//                              Both sets are finished by launch_reduce_weight_grads (`chunks` groups of N * C and of N * T * C
//                              entries): fixed order, no atomics, narrowed once to the table's type.  The workgroup's rows are
//                              frames_backward's plan (up to 8 row steps of 16-byte pieces), so the records are one double per
//                              (workgroup, t, c): 26 MB on [256, 256, 56, 56] fp16, T = 8, against 1.2 GB of tensor traffic.
//                              Pieces of the 16-bit types are EIGHT bytes here (kBwdElems): the per-element state of a piece is
//                              what sets the kernel's registers.
//
// Nothing is sized by T (no LDS tile, no per-t registers): T is unbounded.  No scratch.  Two kernels in all: the element type and
// the piece are launch-uniform switches inside each (with_type_and_unit).  Every access is naturally aligned and inside the
// tensors' bytes; the packed table is read at entries [0, N * C + N * T * C) only.
//
// Not built: the quantized / in-place / online forms, group expansion inside the kernel, an LDS clip tile for mixed pieces.
#include "shiftnd_frames_learn.hpp"

namespace shiftnd {
namespace {

constexpr int64_t kWantForward = 6144;   // the forward cuts frames into more workgroups while its grid is short of this many
constexpr int kSteps = 2;                // row steps of a round of the backward: their carried pieces live in registers
constexpr int kMaxRowSteps = 8;          // the backward's workgroup owns at most this many row steps of 16-byte pieces (frames_backward's plan) ...
constexpr int64_t kWantBackward = 768;   // ... fewer while its grid is short of this many workgroups: one resident set (256 CUs x 3).  Not
                                         // frames_backward's 2048: a workgroup writes T + 1 records a channel here, and on
                                         // [256, 1024, 14, 14] bf16 the 98 chunks of that plan made 231 MB of records for a 98-MiB tensor
// elements of a piece of the backward, at most: 16 bytes of fp32 / fp64, EIGHT bytes of the 16-bit types.  The walk keeps a dozen
// registers per element of its piece (shifts, fractions, three scales, two fp64 sums); with eight elements the one kernel took 260
// VGPRs for every type (1 wave per SIMD)
constexpr int kBwdElems = 4;
inline int backward_unit(int natural, int dtype) { const int cap = kBwdElems * dtype_size(dtype); return natural < cap ? natural : cap; }

// pieces per thread of the forward, every load issued before the first store: tinterlace_forward's figures, for its reason (the one
// kernel takes the widest body's registers, and the forward pays for occupancy)
template <typename T> constexpr int fwd_in_flight() { return sizeof(typename T::S) == 2 ? 2 : 4; }
inline int fwd_in_flight_of(int dtype) { return dtype_size(dtype) == 2 ? 2 : 4; }

// narrow(y * scale): the product is formed in the compute type, THEN rounded to the storage type, in every piece-width body of
// this kernel.  Left to itself the compiler turns fptrunc(fmul) of fp16 bodies into v_fma_mixlo_f16 with a +0 addend in some
// bodies (the exact product rounded once; 0 * -s = +0) and into v_mul_f32 + v_cvt in the others (rounded twice; -0): the same
// values under two piece widths then differ by one 16-bit ulp in about one element in 10^5 and in the sign of filled elements.
// The empty asm is an identity that pattern does not see through; it emits nothing.  The rule chosen is the one the source
// states and the composition, the fp32 / fp64 bodies and all but one body of tinterlace_forward follow.
template <typename T> __device__ __forceinline__ typename T::S narrow_scaled(typename T::C y, typename T::C scale) {
    typename T::C p = y * scale;
    if constexpr (sizeof(typename T::S) == 2) asm("" : "+v"(p));
    return narrow<T>(p);
}

// the blend (or, sparse, the A source alone), then the scale: a multiply of its own after the lerp, rounded once
template <typename T, int E>
__device__ __forceinline__ Unit<T, E> scaled_units(const Unit<T, E> &a, const Unit<T, E> &b, const typename T::C (&d)[E],
                                                   const typename T::C (&sc)[E], bool active) {
    using CT = typename T::C;
    Unit<T, E> r;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const CT v[2] = {widen<T>(a.e[e]), widen<T>(b.e[e])};
        const CT y = active ? interp_t<T, 1>(v, &d[e]) : v[0];
        r.e[e] = narrow_scaled<T>(y, sc[e]);
    }
    return r;
}

template <typename T, int E>
__device__ __forceinline__ void forward_body(const FramesLearnParams &q, const char *__restrict__ x, const void *__restrict__ table,
                                             char *__restrict__ out) {
    using CT = typename T::C;
    constexpr int kInFlight = fwd_in_flight<T>();
    constexpr int V = sizeof(typename T::S) * E;
    const bool active = q.active != 0;
    const uint32_t frame = fdiv(blockIdx.x, q.d_chunks);   // n * T + t
    const uint32_t chunk = blockIdx.x - frame * q.chunks;
    const uint32_t n = fdiv(frame, q.d_T);
    const int t = static_cast<int>(frame - n * q.T), Tn = static_cast<int>(q.T);
    const void *const w = table_row(table, q.wkind, n, q.C);   // the clip's row of the offsets: once per workgroup, scalar
    const int64_t scales = static_cast<int64_t>(q.clips) * q.C + static_cast<int64_t>(frame) * q.C;   // entry of scale (n, t, 0)
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
        CT dw[E], sc[E];
        bool uniform = true;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int64_t c = static_cast<int64_t>(k) * E + e;
            int64_t iw;
            prep_shift_forward<CT>(load_weight<CT>(w, q.wkind, c), active, iw, dw[e]);
            sc[e] = load_weight<CT>(table, q.wkind, scales + c);
            const int cs = canon_shift(iw, Tn, q.pad, q.d_per);
            sa[e] = source_frame(t, cs, Tn, q.pad);
            sb[e] = active ? source_frame(t + 1, cs, Tn, q.pad) : -1;   // (the sparse shift reads one source)
            uniform = uniform && sa[e] == sa[0] && sb[e] == sb[0];
        }
        const int64_t column = static_cast<int64_t>(k) * V;
        int64_t off = static_cast<int64_t>(rl) * q.R + column;
        if (uniform) {
            const char *srca = x + clip + (sa[0] < 0 ? 0 : sa[0]) * q.frame_bytes, *srcb = x + clip + (sb[0] < 0 ? 0 : sb[0]) * q.frame_bytes;
#pragma unroll 1
            for (int r = static_cast<int>(rl); r < rows; r += rps * kInFlight) {
                Unit<T, E> a[kInFlight], b[kInFlight];
#pragma unroll
                for (int j = 0; j < kInFlight; ++j) {
                    a[j] = b[j] = zero_unit<T, E>();
                    if (r + j * rps < rows) {   // (a fill issues no load)
                        if (sa[0] >= 0) a[j] = load_unit<T, E, true>(srca + off + j * step);
                        if (sb[0] >= 0) b[j] = load_unit<T, E, true>(srcb + off + j * step);
                    }
                }
#pragma unroll
                for (int j = 0; j < kInFlight; ++j)
                    if (r + j * rps < rows) store_unit<T, E>(out + here + off + j * step, scaled_units<T, E>(a[j], b[j], dw, sc, active));
                off += kInFlight * step;
            }
        } else {
            // mixed: each element from its own frames, one row at a time
#pragma unroll 1
            for (int r = static_cast<int>(rl); r < rows; r += rps) {
                const Unit<T, E> a = gather_unit<T, E, false>(x + clip + off, sa, false, q.frame_bytes);
                const Unit<T, E> b = gather_unit<T, E, false>(x + clip + off, sb, false, q.frame_bytes);
                store_unit<T, E>(out + here + off, scaled_units<T, E>(a, b, dw, sc, active));
                off += step;
            }
        }
    }
}

// `ws`: the offsets' records, then the scales' (see the head of the file); `red`: kThreads * kBwdElems doubles of LDS
template <typename T, int E>
__device__ __forceinline__ void backward_body(const FramesLearnParams &q, const char *__restrict__ go, const char *__restrict__ x,
                                              const void *__restrict__ table, char *__restrict__ gx, double *__restrict__ ws,
                                              double *red) {
    using CT = typename T::C;
    constexpr int V = sizeof(typename T::S) * E;
    const int Tn = static_cast<int>(q.T);
    const bool active = q.active != 0;
    const uint32_t n = fdiv(blockIdx.x, q.d_chunks), chunk = blockIdx.x - n * q.chunks;
    const void *const w = table_row(table, q.wkind, n, q.C);   // the clip's row of the offsets: once per workgroup, scalar
    const int64_t lines = static_cast<int64_t>(q.clips) * q.C, planes = lines * q.T;   // N * C offsets, N * T * C scales
    const int64_t scales = lines + static_cast<int64_t>(n) * q.T * q.C;                 // entry of scale (n, 0, 0)
    const uint32_t rl = fdiv(threadIdx.x, q.d_span), k0 = threadIdx.x - rl * q.span;
    const int64_t first_row = static_cast<int64_t>(chunk) * q.rows_per_wg;
    const int rows = static_cast<int>(first_row + q.rows_per_wg < q.M ? q.rows_per_wg : q.M - first_row);
    const int rps = static_cast<int>(q.rps);
    const int64_t clip = static_cast<int64_t>(n) * q.T * q.frame_bytes + first_row * q.R;   // the workgroup's rows of the clip's frame 0
    double *const rec_offsets = ws + static_cast<int64_t>(chunk) * lines + static_cast<int64_t>(n) * q.C;
    double *const rec_scales = ws + static_cast<int64_t>(q.chunks) * lines + static_cast<int64_t>(chunk) * planes +
                               static_cast<int64_t>(n) * q.T * q.C;
#pragma unroll 1
    for (uint32_t kb = 0; kb < q.P; kb += kThreads) {      // (once unless a row has more than 256 pieces; uniform: barriers inside)
        const uint32_t k = kb + k0;
        const bool mine = rl < q.rps && k < q.P;
        const int64_t c0 = static_cast<int64_t>(k) * E;   // the piece's first channel
        double acc[E];
        int cs[E], csn[E];   // x (and, interpolating, grad_out) at pad(t - sh), pad(t + 1 - sh); the sparse grad_x: grad_out at pad(t + sh)
        CT dw[E];
        bool uniform = true;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            acc[e] = 0.0;
            cs[e] = csn[e] = 0;
            dw[e] = CT(0);
            if (mine) {
                int64_t sh;
                prep_shift_backward<CT>(load_weight<CT>(w, q.wkind, c0 + e), active, sh, dw[e]);
                cs[e] = canon_shift(sh, Tn, q.pad, q.d_per);
                csn[e] = canon_shift(-sh, Tn, q.pad, q.d_per);
                uniform = uniform && cs[e] == cs[0] && csn[e] == csn[0];
            }
        }
        // the scale of frame f of the piece's element e; 1 for a filled frame, whose zeros stay +0
        auto scale = [&](int f, int e) { return f < 0 ? CT(1) : load_weight<CT>(table, q.wkind, scales + static_cast<int64_t>(f) * q.C + c0 + e); };
        const int64_t column = static_cast<int64_t>(k) * V, step = static_cast<int64_t>(q.rps) * q.R;
        // the workgroup's rows in rounds of kSteps row steps (uniform trip count: barriers inside)
#pragma unroll 1
        for (int r0 = 0; r0 < rows; r0 += rps * kSteps) {
            const int64_t at = clip + (r0 + static_cast<int>(rl)) * q.R + column;   // the piece in row step 0 of the round, frame 0
            bool in[kSteps];
#pragma unroll
            for (int j = 0; j < kSteps; ++j) in[j] = mine && r0 + static_cast<int>(rl) + j * rps < rows;
            int s1[E], sg[E];
#pragma unroll
            for (int e = 0; e < E; ++e) s1[e] = source_frame(0, cs[e], Tn, q.pad);
            Unit<T, E> xa[kSteps], ga[kSteps];
#pragma unroll
            for (int j = 0; j < kSteps; ++j) {
                xa[j] = ga[j] = zero_unit<T, E>();
                if (in[j]) {
                    xa[j] = gather_unit<T, E, false>(x + at + j * step, s1, uniform, q.frame_bytes);
                    if (active) ga[j] = gather_unit<T, E, false>(go + at + j * step, s1, uniform, q.frame_bytes);
                }
            }
#pragma unroll 1
            for (int t = 0; t < Tn; ++t) {
                // the scales of the frames ga, gv and gb hold.  (sca is read again, not carried from the step before: a cache hit
                // against E registers across the walk)
                CT sca[E], scv[E], scb[E];
                double sum[E];       // this thread's share of sum g[t] * y[t]
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    sca[e] = (mine && active) ? scale(source_frame(t, cs[e], Tn, q.pad), e) : CT(1);
                    s1[e] = source_frame(t + 1, cs[e], Tn, q.pad);
                    sg[e] = active ? s1[e] : source_frame(t, csn[e], Tn, q.pad);
                    scv[e] = mine ? scale(t, e) : CT(1);
                    scb[e] = mine ? scale(sg[e], e) : CT(1);
                    sum[e] = 0.0;
                }
#pragma unroll
                for (int j = 0; j < kSteps; ++j) {
                    if (!in[j]) continue;   // (an idle slot adds nothing: 0 * scale is no zero under a scale that is not finite)
                    const int64_t here = at + j * step;
                    const Unit<T, E> xb = gather_unit<T, E, false>(x + here, s1, uniform, q.frame_bytes);
                    const Unit<T, E> gb = gather_unit<T, E, false>(go + here, sg, uniform, q.frame_bytes);
                    const Unit<T, E> gv = load_unit<T, E, false>(go + here + t * q.frame_bytes);
                    Unit<T, E> r;
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        const CT vx[2] = {widen<T>(xa[j].e[e]), widen<T>(xb.e[e])};
                        const CT g = widen<T>(gv.e[e]);
                        // weight_grads_nd<1> on the scaled gradient, the difference taken in fp64 (as tinterlace_backward)
                        const double diff = static_cast<double>(vx[1]) - static_cast<double>(vx[0]);
                        acc[e] = fma_ct(static_cast<double>(g * scv[e]), diff, acc[e]);
                        const CT y = active ? interp_t<T, 1>(vx, &dw[e]) : vx[0];
                        sum[e] = fma_ct(static_cast<double>(g), static_cast<double>(y), sum[e]);
                        const CT vg[2] = {widen<T>(ga[j].e[e]) * sca[e], widen<T>(gb.e[e]) * scb[e]};   // the scale BEFORE the lerp
                        r.e[e] = narrow<T>(active ? interp_t<T, 1>(vg, &dw[e]) : vg[1]);
                    }
                    store_unit<T, E>(gx + here + t * q.frame_bytes, r);
                    xa[j] = xb;
                    ga[j] = gb;
                }
                // frame t over the rows of the workgroup: threads rl = 0 .. rps-1 hold the same piece column, summed in that order
                __syncthreads();
#pragma unroll
                for (int e = 0; e < E; ++e) red[e * kThreads + threadIdx.x] = sum[e];
                __syncthreads();
                if (mine && rl == 0) {
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        double total = 0.0;
#pragma unroll 1
                        for (uint32_t j = 0; j < q.rps; ++j) total += red[e * kThreads + j * q.span + k0];
                        double *p = rec_scales + static_cast<int64_t>(t) * q.C + c0 + e;
                        *p = (r0 ? *p : 0.0) + total;   // (a later round: the record this thread wrote a round before)
                    }
                }
            }
        }
        // the offsets: the rows of the workgroup, as above
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
                rec_offsets[c0 + e] = total;
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void frames_interlace_forward(FramesLearnParams q, const char *__restrict__ x,
                                                                    const void *__restrict__ w, char *__restrict__ out) {
    with_type_and_unit(q.dtype, q.elems, [&](auto ty, auto e) { forward_body<decltype(ty), decltype(e)::value>(q, x, w, out); });
}

__global__ __launch_bounds__(kThreads) void frames_interlace_backward(FramesLearnParams q, const char *__restrict__ go,
                                                                     const char *__restrict__ x, const void *__restrict__ w,
                                                                     char *__restrict__ gx, double *__restrict__ ws) {
    __shared__ double red[kThreads * kBwdElems];
    const auto body = [&](auto ty, auto e) { backward_body<decltype(ty), decltype(e)::value>(q, go, x, w, gx, ws, red); };
    switch (q.dtype) {   // with_type_and_unit under the backward's piece
    case SHIFTND_F32: with_unit<4>(q.elems, [&](auto e) { body(f32_t(), e); }); break;
    case SHIFTND_F64: with_unit<2>(q.elems, [&](auto e) { body(f64_t(), e); }); break;
    case SHIFTND_F16: with_unit<kBwdElems>(q.elems, [&](auto e) { body(f16_t(), e); }); break;
    default: with_unit<kBwdElems>(q.elems, [&](auto e) { body(bf16_t(), e); }); break;
    }
}

// rows of a backward workgroup: from the geometry alone (the workspace query has no pointers), as if the pieces were 16 bytes.
// (A narrower piece gives the kernel fewer rows a step; it then takes the same rows in more rounds.)
int64_t backward_rows_per_wg(const Geometry &g, int dtype) {
    const int64_t M = frame_pixels(g), pieces = (g.C * dtype_size(dtype) + 15) / 16;
    const int64_t rps = pieces < kThreads ? kThreads / pieces : 1;
    int64_t steps = kMaxRowSteps;
    while (steps > 1 && g.N * ((M + rps * steps - 1) / (rps * steps)) < kWantBackward) steps /= 2;
    return rps * steps;
}
int64_t backward_chunks(const Geometry &g, int dtype) {
    const int64_t rows = backward_rows_per_wg(g, dtype);
    return (frame_pixels(g) + rows - 1) / rows;
}

}  // namespace

// The sizes the kernels' index arithmetic needs (include/shiftnd_hip.h states them): those of frames_learn_geometry_ok, the packed
// table indexed and its two reductions counted in 32 bits (N * S0 * C < 2^31, which holds N * C below it too), and for the backward
// N * chunks workgroups below 2^31 with the records below 2^46 bytes.
bool frames_interlace_geometry_ok(const Geometry &g, int dtype) {
    if (!frames_learn_geometry_ok(g, dtype)) return false;
    const int64_t T = g.S[3 - g.nd];
    // (N, C and N * S0 are below 2^31 here: no overflow)
    if (g.N * g.C >= (1LL << 31) || g.N * T * g.C >= (1LL << 31)) return false;
    if (g.N == 0 || g.C == 0 || g.S[0] * g.S[1] * g.S[2] == 0) return true;
    const int64_t groups = g.N * backward_chunks(g, dtype);   // (N and chunks <= M are below 2^31: no overflow)
    return groups < (1LL << 31) && groups <= (1LL << 46) / (g.C * (1 + T) * 8);
}

int frames_interlace_forward(const Geometry &g, int dtype, const void *x, const void *w, int wkind, void *out, hipStream_t st) {
    const int unit = piece_bytes(g.C * dtype_size(dtype), {x, out});
    FramesLearnParams q = make_params(g, dtype, wkind, unit, true);
    // workgroups per frame: at least one batch of in-flight steps each, more steps while the grid is large (as frames_active_forward)
    const int64_t frames = g.N * q.T, batch_rows = static_cast<int64_t>(q.rps) * fwd_in_flight_of(dtype);
    const int64_t most = (q.M + batch_rows - 1) / batch_rows;
    const int64_t wanted = (kWantForward + frames - 1) / frames;
    const int64_t chunks = most < wanted ? most : wanted;
    q.rows_per_wg = static_cast<uint32_t>(((q.M + chunks - 1) / chunks + batch_rows - 1) / batch_rows * batch_rows);
    q.chunks = static_cast<uint32_t>((q.M + q.rows_per_wg - 1) / q.rows_per_wg);
    q.d_chunks = make_fastdiv(q.chunks);
    note_kernel(unit == 16 ? "frames_interlace_forward" : "frames_interlace_forward_ragged");
    void (*const kernel)(FramesLearnParams, const char *, const void *, char *) = frames_interlace_forward;   // (the kernel, not this function)
    const int64_t blocks = frames * q.chunks;   // (below 2^31: frames is, and a frame is cut only while the grid is short of 6144)
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, st, q, static_cast<const char *>(x), w,
                       static_cast<char *>(out));
    return SHIFTND_OK;
}

// both partial sets, ONE double a record (dense: launch_reduce_weight_grads under a record of 1): chunks * N * C for the offsets,
// chunks * N * T * C for the scales -- a function of the geometry alone
size_t frames_interlace_backward_workspace(const Geometry &g, int dtype) {
    const int64_t T = g.S[3 - g.nd];
    return static_cast<size_t>(backward_chunks(g, dtype) * g.N * g.C * (1 + T)) * sizeof(double);
}

int frames_interlace_backward(const Geometry &g, int dtype, const void *go, const void *x, const void *w, int wkind, void *gx, void *gw,
                              void *workspace, hipStream_t st) {
    const int natural = piece_bytes(g.C * dtype_size(dtype), {go, x, gx}), unit = backward_unit(natural, dtype);
    FramesLearnParams q = make_params(g, dtype, wkind, unit, true);
    q.rows_per_wg = static_cast<uint32_t>(backward_rows_per_wg(g, dtype));
    q.chunks = static_cast<uint32_t>(backward_chunks(g, dtype));
    q.d_chunks = make_fastdiv(q.chunks);
    double *ws = static_cast<double *>(workspace);
    note_kernel(natural == 16 ? "frames_interlace_backward" : "frames_interlace_backward_ragged");
    void (*const kernel)(FramesLearnParams, const char *, const char *, const void *, char *, double *) = frames_interlace_backward;
    const int64_t groups = g.N * q.chunks;   // (below 2^31: frames_interlace_geometry_ok)
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(groups)), dim3(kThreads), 0, st, q, static_cast<const char *>(go),
                       static_cast<const char *>(x), w, static_cast<char *>(gx), ws);
    // the packed gradient: [N, C] offsets, then [N, T, C] scales, `chunks` groups each, in the table's type
    const int64_t lines = g.N * g.C, planes = lines * q.T;
    launch_reduce_weight_grads(wkind, ws, static_cast<int>(q.chunks), static_cast<int>(lines), 1, gw, st, 1);
    launch_reduce_weight_grads(wkind, ws + q.chunks * lines, static_cast<int>(q.chunks), static_cast<int>(planes), 1,
                               static_cast<char *>(gw) + lines * dtype_size(wkind), st, 1);
    return SHIFTND_OK;
}

}  // namespace shiftnd
