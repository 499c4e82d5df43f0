// shiftnd_temporal.hpp -- what the six files of the temporal-shift family share (shiftnd_segment.hip, shiftnd_tshift.hip,
// shiftnd_frames.hip, shiftnd_frames_learn.hip, shiftnd_inplace.hip, shiftnd_stream.hip): one definition each.  Internal.
#pragma once

#include <initializer_list>

#include "shiftnd_common.hpp"
#include "shiftnd_launch.hpp"

namespace shiftnd {

// ---- device: a unit (a piece) of E elements of type T, moved as one vector of at most 16 bytes ----------------------------------
template <typename T, int E> struct Unit { typename T::S e[E]; };

template <typename T, int E, bool NT> __device__ __forceinline__ Unit<T, E> load_unit(const char *p) {
    constexpr int V = sizeof(typename T::S) * E;
    typedef typename vec_of<V>::type vec_t;
    const vec_t v = NT ? __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(p)) : *reinterpret_cast<const vec_t *>(p);
    Unit<T, E> u;
    __builtin_memcpy(u.e, &v, V);
    return u;
}
template <typename T, int E> __device__ __forceinline__ Unit<T, E> zero_unit() {
    Unit<T, E> u;
    __builtin_memset(u.e, 0, sizeof(u.e));
    return u;
}
template <typename T, int E> __device__ __forceinline__ void store_unit(char *p, const Unit<T, E> &u) {
    constexpr int V = sizeof(typename T::S) * E;
    typedef typename vec_of<V>::type vec_t;
    vec_t v;
    __builtin_memcpy(&v, u.e, V);
    __builtin_nontemporal_store(v, reinterpret_cast<vec_t *>(p));
}

// ONE kernel per element type and pass: the unit (`elems` elements, a power of two up to E) is launch-uniform, scalar branches
template <int E> struct UnitElems { static constexpr int value = E; };
template <int E, typename F> __device__ __forceinline__ void with_unit(int elems, F &&f) {
    if constexpr (E == 1) {
        f(UnitElems<1>());
    } else {
        if (elems == E) f(UnitElems<E>());
        else with_unit<E / 2>(elems, f);
    }
}

// source frame (segment) of coordinate p in [0, T] under the canonical shift cs (a size-1 dim ignores its shift), or -1 (fill)
__device__ __forceinline__ int source_frame(int p, int cs, int T, int pad) { return T == 1 ? 0 : fold_index(p - cs, T, pad); }

// row n of a table whose rows are `wrow` entries apart (0: a [C] table, every clip reads row 0; C: a per-clip [N, C] one).  The
// kernels call it with a workgroup-uniform n, once per workgroup: scalar arithmetic, none of it inside their loops
__device__ __forceinline__ const void *table_row(const void *w, int wkind, uint32_t n, uint32_t wrow) {
    const int64_t first = static_cast<int64_t>(n) * wrow;
    switch (wkind) {
    case SHIFTND_F64: return static_cast<const uint64_t *>(w) + first;
    case SHIFTND_F32: case SHIFTND_I32: return static_cast<const uint32_t *>(w) + first;
    case SHIFTND_F16: case SHIFTND_BF16: return static_cast<const uint16_t *>(w) + first;
    default: return static_cast<const uint8_t *>(w) + first;
    }
}

// the type a piece of 1 << UL bytes is moved as
template <int UL> struct piece_of;
template <> struct piece_of<4> { typedef shiftnd_u4 type; };
template <> struct piece_of<3> { typedef uint32_t type __attribute__((ext_vector_type(2))); };
template <> struct piece_of<2> { typedef uint32_t type; };
template <> struct piece_of<1> { typedef uint16_t type; };
template <> struct piece_of<0> { typedef uint8_t type; };

// do table entries [e0, e0 + N) hold the same bits?  N is a compile-time count: exactly N loads inside the table, issued together
// (shiftnd_frames.hip has its own raw_equal on purpose: a run-time count under 15 clamped loads, against exactly N loads here)
template <typename R, int N> __device__ __forceinline__ bool raw_equal_fixed(const void *w, int64_t e0) {
    const R *p = static_cast<const R *>(w) + e0;
    const R first = p[0];
    bool same = true;
#pragma unroll
    for (int e = 1; e < N; ++e) same = same && p[e] == first;
    return same;
}
// ... the 1 << n_log2 entries of a piece of 1 << UL bytes (n_log2 <= UL, launch-uniform: scalar branches)
template <typename R, int UL> __device__ __forceinline__ bool raw_equal_pow2(const void *w, int64_t e0, int n_log2) {
    if constexpr (UL >= 4) if (n_log2 == 4) return raw_equal_fixed<R, 16>(w, e0);
    if constexpr (UL >= 3) if (n_log2 == 3) return raw_equal_fixed<R, 8>(w, e0);
    if constexpr (UL >= 2) if (n_log2 == 2) return raw_equal_fixed<R, 4>(w, e0);
    if constexpr (UL >= 1) if (n_log2 == 1) return raw_equal_fixed<R, 2>(w, e0);
    return true;
}
template <int UL> __device__ __forceinline__ bool piece_entries_equal(const void *w, int wkind, int64_t e0, int n_log2) {
    switch (wkind) {
    case SHIFTND_F64: return raw_equal_pow2<uint64_t, UL>(w, e0, n_log2);
    case SHIFTND_F32: case SHIFTND_I32: return raw_equal_pow2<uint32_t, UL>(w, e0, n_log2);
    case SHIFTND_F16: case SHIFTND_BF16: return raw_equal_pow2<uint16_t, UL>(w, e0, n_log2);
    default: return raw_equal_pow2<uint8_t, UL>(w, e0, n_log2);
    }
}

// bytes [0, n) of a dword (n clamped to 0..4)
__device__ __forceinline__ uint32_t low_bytes(int n) { return n <= 0 ? 0u : (n >= 4 ? ~0u : (1u << (8 * n)) - 1u); }

// ---- host -----------------------------------------------------------------------------------------------------------------------
// pixels of a frame (elements of a plane): the spatial dims inside the shifted one, which is S[3 - nd]
inline int64_t frame_pixels(const Geometry &g) { return (g.nd == 3 ? g.S[1] : 1) * g.S[2]; }

inline int es_log2(int es) { return es == 8 ? 3 : (es == 4 ? 2 : (es == 2 ? 1 : 0)); }

// the fill as a dword pattern: a byte four times, the dword itself (floats: fill_bits == 0)
inline uint32_t fill_dword(int es, uint64_t fill_bits) {
    return es == 1 ? static_cast<uint32_t>(fill_bits & 0xff) * 0x01010101u : static_cast<uint32_t>(fill_bits);
}

// bytes of the piece (the unit): the widest power of two, at most 16, that divides the run's bytes -- a plane's or a pixel row's --
// and every base, so runs are made of whole, naturally aligned pieces.  Never below the element size: runs are whole elements and
// bases are element-aligned.  (Its log2: __builtin_ctz.)
inline int piece_bytes(int64_t run_bytes, std::initializer_list<const void *> bases) {
    uintptr_t bits = static_cast<uintptr_t>(run_bytes) | 16;
    for (const void *p : bases) bits |= reinterpret_cast<uintptr_t>(p);
    return static_cast<int>(bits & (~bits + 1));
}

// dense strides of memory order N, S0, C, S1, S2 (a dim of size 1 has no stride to check)
inline bool dense_segment_major(const Geometry &g, const int64_t *st) {
    const int lead = 3 - g.nd;
    const int64_t A = g.nd == 3 ? g.S[1] : 1, B = g.S[2], inner = A * B, T = g.S[lead];
    if (B > 1 && st[4] != 1) return false;
    if (A > 1 && st[3] != B) return false;
    if (g.C > 1 && st[1] != inner) return false;
    if (T > 1 && st[2 + lead] != g.C * inner) return false;
    return g.N == 1 || st[0] == T * g.C * inner;
}

// the 32-bit limits of the segment-major kernels: plane and unit counts go through FastDiv (below 2^31; the unit is the element where
// it is one byte, two bytes elsewhere, so a 1-byte tensor of 2^31 - 16 bytes or more is not served); T also enters the 32-bit padding
// map (periods of 2 T)
inline bool segment_counts_fit(const Geometry &g, int64_t es) {
    const int64_t T = g.S[3 - g.nd], inner = frame_pixels(g), limit = 1LL << 31;
    if (T >= (1LL << 30) || inner >= limit || g.N >= limit || g.C >= limit || g.N * T >= limit) return false;
    const int64_t planes = g.N * T * g.C;   // (every factor is below 2^31 here: no overflow)
    return planes < limit && planes * (es == 1 ? inner : inner * es / 2) + 16 < limit;
}

}  // namespace shiftnd
