// shiftnd_interlace_quant.hip -- QUANTIZED temporal interlacing and the quantized per-clip temporal shift: tinterlace_forward's
// problem (shiftnd_interlace.hip) on the int_repr of a per-tensor quantized segment-major tensor (memory order N, S0, C,
// S1, S2) under an fp32 table (gfx950).  shiftnd_forward_quantized under SHIFTND_SHIFT_DIM0 | SHIFTND_PER_CLIP (an [N, C] table) or
// SHIFTND_SHIFT_DIM0 | SHIFTND_INTERLACE (the packed table: N * C offsets, then N * S0 * C scales) with wq_dtype == SHIFTND_F32
// selects it.
//
// The result is defined in the integer domain -- the tensor's scale does not enter and nothing is dequantized:
//     r   = lerp1(q[pad(t - iw)] - zp, q[pad(t - iw + 1)] - zp, dw) * s      iw, dw: prep_shift_forward<F>(F(offsets[n, c]), active)
//     out = clamp(zp + rint(r), the element type's range)                     s: F(scales[n, t, c]), or 1; rint: half to even
// in F = fp32 for I8 / U8 and F = fp64 for I32; a filled frame contributes 0 to r, which is the zero point in out under any finite
// scale.  lerp1 is the library's (two multiplies and one add, -ffp-contract=off); the scale is ONE multiply after it.  A scale above 1
// can saturate: the clamp is part of the definition.
//
//   tinterlace_forward_quantized   tshift_forward_quantized's walk (shiftnd_tshift_quant.hip): flat over the output in naturally
//                    aligned units of 16 / 8 / 4 / 2 / 1 bytes, four in flight per thread, every load before the first store,
//                    nontemporal loads and stores, the element type and the unit as launch-uniform switches, I8 on the unsigned path
//                    through ^ 0x80.  What differs: the offset is entry n * C + c (clip n's row), the scale entry
//                    (n * T + t) * C + c behind the offsets in the same array (without scales the constant 1), and `active` is a
//                    run-time field (the sparse shift: the offset rounded half to even, fraction 0, the scale still applied).
//                    Per unit, by its fraction and scale:
//                      fraction 0, scale exactly 1   the first source's bytes, none of the arithmetic (TIN's pass-through channels)
//                      fraction 0, another scale     one source load, rint((q - zp) * s)
//                      otherwise                     two source loads, the blend, the multiply
//                    and a filled frame issues no load.  No LDS, no scratch, no workspace; nothing outside x, the table and out is
//                    touched: a source unit lies at the output unit's offset inside another plane of x.
//
// Limits: tshift_forward_quantized's (fewer than 2^31 - 16 elements; N * S0 * C < 2^31, which also bounds both table indices).
//
// Not built: channels-last tensors, a cut window, an in-place or online form, requantization to another scale, group expansion
// inside the kernel.
#include <type_traits>

#include "shiftnd_quant_unit.hpp"

namespace shiftnd {
namespace {

constexpr int kQInFlight = 4;   // units per thread, every load issued before the first store

struct QInterlaceParams {
    int pad, wide, active;           // wide: I32 elements (fp64 arithmetic); else one-byte elements (fp32)
    int scaled;                      // the table carries scales behind the offsets; else every scale is 1
    uint32_t T, C, upp;              // frames per clip, channels, units per plane
    FastDiv d_upp, d_C, d_T, d_per;  // d_per: by map_period(T, pad)
    int64_t plane_bytes, units;      // units: of the whole tensor
    int64_t scales;                  // first entry of the scales in the packed table (N * C)
    uint32_t flip;                   // I8: 0x80808080 (the bytes are handled as q + 128), else 0
    int32_t zp;                      // the zero point (I8: + 128, so 0..255 for both one-byte types)
};

constexpr int64_t kFill = -1, kPast = -2;

template <bool WIDE, int V>
__device__ __forceinline__ void qinterlace_body(const QInterlaceParams &q, const char *__restrict__ x, const float *__restrict__ w,
                                                char *__restrict__ out) {
    using CT = typename std::conditional<WIDE, double, float>::type;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * (kThreads * kQInFlight) + threadIdx.x;
    const int Tn = static_cast<int>(q.T);
    int64_t sa[kQInFlight], sb[kQInFlight];   // byte offset in x of the unit's two sources, or a mark
    CT dw[kQInFlight], sc[kQInFlight];
#pragma unroll
    for (int k = 0; k < kQInFlight; ++k) {
        const int64_t i = first + k * kThreads;
        sa[k] = sb[k] = kPast;
        dw[k] = CT(0);
        sc[k] = CT(1);
        if (i >= q.units) continue;
        const uint32_t u = static_cast<uint32_t>(i);
        const uint32_t plane = fdiv(u, q.d_upp);
        const int64_t at = static_cast<int64_t>(u - plane * q.upp) * V;   // byte in the plane
        const uint32_t nt = fdiv(plane, q.d_C), c = plane - nt * q.C;
        const uint32_t n = fdiv(nt, q.d_T), t = nt - n * q.T;
        int64_t iw;
        prep_shift_forward<CT>(static_cast<CT>(w[static_cast<int64_t>(n) * q.C + c]), q.active != 0, iw, dw[k]);
        if (q.scaled) sc[k] = static_cast<CT>(w[q.scales + plane]);
        const int cs = canon_shift(iw, Tn, q.pad, q.d_per);
        const int s0 = source_frame(static_cast<int>(t), cs, Tn, q.pad), s1 = source_frame(static_cast<int>(t) + 1, cs, Tn, q.pad);
        const int64_t clip = static_cast<int64_t>(n) * q.T;
        sa[k] = s0 < 0 ? kFill : ((clip + s0) * q.C + c) * q.plane_bytes + at;
        sb[k] = (s1 < 0 || dw[k] == CT(0)) ? kFill : ((clip + s1) * q.C + c) * q.plane_bytes + at;   // (fraction 0: the first source alone)
    }
    // a filled frame: the zero point in every element, so that q - zp is 0 (the bytes already flipped: `flip` is applied to loads only)
    const uint32_t zfill = WIDE ? static_cast<uint32_t>(q.zp) : static_cast<uint32_t>(q.zp) * 0x01010101u;
    QUnit<V> a[kQInFlight], b[kQInFlight];
#pragma unroll
    for (int k = 0; k < kQInFlight; ++k) {
#pragma unroll
        for (int i = 0; i < (V >= 4 ? V / 4 : 1); ++i) a[k].d[i] = b[k].d[i] = zfill;
        if (sa[k] >= 0) {   // (a filled frame issues no load)
            a[k] = load_qunit<V>(x + sa[k]);
#pragma unroll
            for (int i = 0; i < (V >= 4 ? V / 4 : 1); ++i) a[k].d[i] ^= q.flip;
        }
        if (sb[k] >= 0) {
            b[k] = load_qunit<V>(x + sb[k]);
#pragma unroll
            for (int i = 0; i < (V >= 4 ? V / 4 : 1); ++i) b[k].d[i] ^= q.flip;
        }
    }
#pragma unroll
    for (int k = 0; k < kQInFlight; ++k) {
        if (sa[k] == kPast) continue;
        QUnit<V> r = a[k];   // fraction 0 and scale exactly 1: the first source's bytes
        if (dw[k] != CT(0)) {
            if constexpr (WIDE) r = blend_words<V, true>(a[k], b[k], dw[k], static_cast<double>(q.zp), sc[k]);
            else r = blend_bytes<V, true>(a[k], b[k], dw[k], static_cast<float>(q.zp), sc[k]);
        } else if (sc[k] != CT(1)) {
            if constexpr (WIDE) r = scale_words<V>(a[k], static_cast<double>(q.zp), sc[k]);
            else r = scale_bytes<V>(a[k], static_cast<float>(q.zp), sc[k]);
        }
#pragma unroll
        for (int i = 0; i < (V >= 4 ? V / 4 : 1); ++i) r.d[i] ^= q.flip;
        store_qunit<V>(out + (first + k * kThreads) * V, r);
    }
}

// ONE kernel: the element type (q.wide, q.flip) and the unit (1 << unit_log2 bytes) are launch-uniform, scalar branches
__global__ __launch_bounds__(kThreads) void tinterlace_forward_quantized(QInterlaceParams q, const char *__restrict__ x,
                                                                        const float *__restrict__ w, char *__restrict__ out,
                                                                        int unit_log2) {
    if (q.wide) {
        if (unit_log2 == 4) qinterlace_body<true, 16>(q, x, w, out);
        else if (unit_log2 == 3) qinterlace_body<true, 8>(q, x, w, out);
        else qinterlace_body<true, 4>(q, x, w, out);
    } else {
        if (unit_log2 == 4) qinterlace_body<false, 16>(q, x, w, out);
        else if (unit_log2 == 3) qinterlace_body<false, 8>(q, x, w, out);
        else if (unit_log2 == 2) qinterlace_body<false, 4>(q, x, w, out);
        else if (unit_log2 == 1) qinterlace_body<false, 2>(q, x, w, out);
        else qinterlace_body<false, 1>(q, x, w, out);
    }
}

}  // namespace

// `scaled`: `w` is the packed table (SHIFTND_INTERLACE); else the [N, C] offsets alone (SHIFTND_PER_CLIP).  The geometry passes
// tshift_quantized_geometry_ok, whose N * S0 * C < 2^31 bounds both table indices
int tinterlace_quantized_forward(const Geometry &g, int dtype, const void *x, const void *w, bool scaled, int64_t zp, void *out,
                                 hipStream_t st) {
    const int es = dtype_size(dtype);
    const int unit = piece_bytes(frame_pixels(g) * es, {x, out});
    QInterlaceParams q;
    q.pad = g.pad;
    q.wide = dtype == SHIFTND_I32;
    q.active = g.active;
    q.scaled = scaled;
    q.T = static_cast<uint32_t>(g.S[3 - g.nd]);
    q.C = static_cast<uint32_t>(g.C);
    q.plane_bytes = frame_pixels(g) * es;
    q.upp = static_cast<uint32_t>(q.plane_bytes / unit);
    q.units = g.N * q.T * q.C * static_cast<int64_t>(q.upp);
    q.scales = g.N * g.C;
    q.d_upp = make_fastdiv(q.upp);
    q.d_C = make_fastdiv(q.C);
    q.d_T = make_fastdiv(q.T);
    q.d_per = make_fastdiv(static_cast<uint32_t>(map_period(static_cast<int>(q.T), g.pad)));
    q.flip = dtype == SHIFTND_I8 ? 0x80808080u : 0u;
    q.zp = static_cast<int32_t>(dtype == SHIFTND_I8 ? zp + 128 : zp);
    note_kernel("tinterlace_forward_quantized");
    const int64_t per = kThreads * kQInFlight;
    hipLaunchKernelGGL(tinterlace_forward_quantized, dim3(static_cast<unsigned>((q.units + per - 1) / per)), dim3(kThreads), 0, st, q,
                       static_cast<const char *>(x), static_cast<const float *>(w), static_cast<char *>(out), __builtin_ctz(unit));
    return SHIFTND_OK;
}

}  // namespace shiftnd
