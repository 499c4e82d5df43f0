// shiftnd_frames_learn.hpp -- what the two files of the channels-last LEARNABLE temporal kernels share (shiftnd_frames_learn.hip,
// shiftnd_interlace_frames.hip): the launch parameters, the piece gather, the per-element blend and the type / piece switch.  Internal.
//
// Everything here sits in an UNNAMED namespace on purpose: a kernel's symbol carries the namespace of its parameter types, and the
// kernels of shiftnd_frames_learn.hip keep the symbols (and the code) they had when these definitions lived in that file.
// The price: every includer gets its OWN FramesLearnParams and helpers, distinct types per translation unit -- nothing declared
// here can cross a file boundary.  Fine for the two includers; a third should weigh a named internal namespace (and new symbols).
#pragma once

#include "shiftnd_temporal.hpp"

namespace shiftnd {
namespace {

constexpr int kMaxElems = 8;           // elements of a 16-byte piece (2-byte types)

struct FramesLearnParams {
    int pad, wkind, active, dtype, elems;   // elems: elements per piece
    uint32_t T, P, span, rps;               // frames per clip, pieces per row, min(P, 256), rows per step = max(1, 256 / P)
    uint32_t chunks, rows_per_wg;           // workgroups per frame (forward) / per clip (backward), rows of each
    uint32_t C;
    uint32_t wrow, clips;                   // weight of (n, c): entry n * wrow + c -- 0 for a [C] table, C for a per-clip [N, C] one; N
    FastDiv d_chunks, d_T, d_span, d_per;   // d_per: by map_period(T, pad)
    int64_t M, R, frame_bytes;              // pixels per frame, bytes per row, bytes per frame
};

// the piece at `at` (its byte offset in frame 0 of the clip) whose element e comes from frame f[e], or is the fill (f[e] < 0):
// one piece load where the elements agree, element-sized loads otherwise
template <typename T, int E, bool NT>
__device__ __forceinline__ Unit<T, E> gather_unit(const char *at, const int (&f)[E], bool uniform, int64_t frame_bytes) {
    typedef typename raw_t<sizeof(typename T::S)>::type raw;
    Unit<T, E> u = zero_unit<T, E>();
    if (uniform) {
        if (f[0] >= 0) u = load_unit<T, E, NT>(at + f[0] * frame_bytes);
    } else {
        raw r[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            r[e] = 0;
            if (f[e] >= 0) r[e] = *reinterpret_cast<const raw *>(at + f[e] * frame_bytes + e * sizeof(raw));
        }
        __builtin_memcpy(u.e, r, sizeof(u.e));
    }
    return u;
}

// the interpolation of the tshift kernels, each element under its own fraction
template <typename T, int E>
__device__ __forceinline__ Unit<T, E> blend_units(const Unit<T, E> &a, const Unit<T, E> &b, const typename T::C (&d)[E]) {
    Unit<T, E> r;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const typename T::C v[2] = {widen<T>(a.e[e]), widen<T>(b.e[e])};
        r.e[e] = narrow<T>(interp_t<T, 1>(v, &d[e]));
    }
    return r;
}

// the element type and the piece: launch-uniform, scalar branches
template <typename F> __device__ __forceinline__ void with_type_and_unit(int dtype, int elems, F &&f) {
    switch (dtype) {
    case SHIFTND_F32: with_unit<4>(elems, [&](auto e) { f(f32_t(), e); }); break;
    case SHIFTND_F64: with_unit<2>(elems, [&](auto e) { f(f64_t(), e); }); break;
    case SHIFTND_F16: with_unit<8>(elems, [&](auto e) { f(f16_t(), e); }); break;
    default: with_unit<8>(elems, [&](auto e) { f(bf16_t(), e); }); break;
    }
}

// everything of the parameters but the plan (chunks, rows_per_wg, d_chunks), which each launcher makes
inline FramesLearnParams make_params(const Geometry &g, int dtype, int wkind, int unit, bool per_clip) {
    FramesLearnParams q;
    const int es = dtype_size(dtype);
    q.pad = g.pad;
    q.wkind = wkind;
    q.active = g.active;
    q.dtype = dtype;
    q.elems = unit / es;
    q.T = static_cast<uint32_t>(g.S[3 - g.nd]);
    q.C = static_cast<uint32_t>(g.C);
    q.wrow = per_clip ? q.C : 0;
    q.clips = static_cast<uint32_t>(g.N);
    q.M = frame_pixels(g);
    q.R = g.C * es;
    q.frame_bytes = q.M * q.R;
    q.P = static_cast<uint32_t>(q.R / unit);
    q.span = q.P < static_cast<uint32_t>(kThreads) ? q.P : static_cast<uint32_t>(kThreads);
    q.rps = static_cast<uint32_t>(kThreads) / q.span;
    q.d_T = make_fastdiv(q.T);
    q.d_span = make_fastdiv(q.span);
    q.d_per = make_fastdiv(static_cast<uint32_t>(map_period(static_cast<int>(q.T), g.pad)));
    return q;
}

}  // namespace
}  // namespace shiftnd
