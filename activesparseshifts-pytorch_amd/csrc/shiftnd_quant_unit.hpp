// shiftnd_quant_unit.hpp -- what the two quantized segment-major temporal kernels share (shiftnd_tshift_quant.hip,
// shiftnd_interlace_quant.hip): a unit of bytes as dwords, its nontemporal load and store, and the integer-domain blends
// (DESIGN 3.40 / 3.42).  Internal; device code only.
#pragma once

#include "shiftnd_temporal.hpp"

namespace shiftnd {

// a unit of V bytes as dwords (V < 4: the low bytes of one)
template <int V> struct QUnit { uint32_t d[V >= 4 ? V / 4 : 1]; };

template <int V> __device__ __forceinline__ QUnit<V> load_qunit(const char *p) {
    typedef typename vec_of<V>::type vec_t;
    const vec_t v = __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(p));
    QUnit<V> u;
    if constexpr (V >= 4) __builtin_memcpy(u.d, &v, V);
    else u.d[0] = v;
    return u;
}
template <int V> __device__ __forceinline__ void store_qunit(char *p, const QUnit<V> &u) {
    typedef typename vec_of<V>::type vec_t;
    vec_t v;
    if constexpr (V >= 4) __builtin_memcpy(&v, u.d, V);
    else v = static_cast<vec_t>(u.d[0]);
    __builtin_nontemporal_store(v, reinterpret_cast<vec_t *>(p));
}

// one-byte elements, as unsigned bytes (I8 flipped by the caller); zp in 0..255.  SCALED: the blend times `sc`, a multiply of its
// own after the lerp (temporal interlacing); without it `sc` is not looked at
template <int V, bool SCALED = false>
__device__ __forceinline__ QUnit<V> blend_bytes(const QUnit<V> &a, const QUnit<V> &b, float d, float zp, float sc = 1.0f) {
    QUnit<V> r;
    const float keep = 1.0f - d;   // lerp1's (1 - x), once per unit
#pragma unroll
    for (int i = 0; i < (V >= 4 ? V / 4 : 1); ++i) {
        uint32_t packed = 0;
#pragma unroll
        for (int e = 0; e < (V >= 4 ? 4 : V); ++e) {
            const float va = static_cast<float>((a.d[i] >> (8 * e)) & 0xffu) - zp;
            const float vb = static_cast<float>((b.d[i] >> (8 * e)) & 0xffu) - zp;
            float v = va * keep + vb * d;
            if constexpr (SCALED) v = v * sc;
            packed = __builtin_amdgcn_cvt_pk_u8_f32(rintf(v) + zp, e, packed);   // saturates to 0..255
        }
        r.d[i] = packed;
    }
    return r;
}

// I32 elements in fp64
template <int V, bool SCALED = false>
__device__ __forceinline__ QUnit<V> blend_words(const QUnit<V> &a, const QUnit<V> &b, double d, double zp, double sc = 1.0) {
    QUnit<V> r;
    const double keep = 1.0 - d;
#pragma unroll
    for (int i = 0; i < V / 4; ++i) {
        const double va = static_cast<double>(static_cast<int32_t>(a.d[i])) - zp;
        const double vb = static_cast<double>(static_cast<int32_t>(b.d[i])) - zp;
        double v = va * keep + vb * d;
        if constexpr (SCALED) v = v * sc;
        v = rint(v) + zp;
        v = v < -2147483648.0 ? -2147483648.0 : (v > 2147483647.0 ? 2147483647.0 : v);
        r.d[i] = static_cast<uint32_t>(static_cast<int32_t>(v));
    }
    return r;
}

// one source times `sc` (a fraction of exactly 0 under a scale other than 1: lerp1(a, b, 0) == a for finite b)
template <int V> __device__ __forceinline__ QUnit<V> scale_bytes(const QUnit<V> &a, float zp, float sc) {
    QUnit<V> r;
#pragma unroll
    for (int i = 0; i < (V >= 4 ? V / 4 : 1); ++i) {
        uint32_t packed = 0;
#pragma unroll
        for (int e = 0; e < (V >= 4 ? 4 : V); ++e) {
            const float va = static_cast<float>((a.d[i] >> (8 * e)) & 0xffu) - zp;
            packed = __builtin_amdgcn_cvt_pk_u8_f32(rintf(va * sc) + zp, e, packed);
        }
        r.d[i] = packed;
    }
    return r;
}
template <int V> __device__ __forceinline__ QUnit<V> scale_words(const QUnit<V> &a, double zp, double sc) {
    QUnit<V> r;
#pragma unroll
    for (int i = 0; i < V / 4; ++i) {
        const double va = static_cast<double>(static_cast<int32_t>(a.d[i])) - zp;
        double v = rint(va * sc) + zp;
        v = v < -2147483648.0 ? -2147483648.0 : (v > 2147483647.0 ? 2147483647.0 : v);
        r.d[i] = static_cast<uint32_t>(static_cast<int32_t>(v));
    }
    return r;
}

}  // namespace shiftnd
