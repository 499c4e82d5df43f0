// shiftnd_tshift_quant.hip -- the QUANTIZED interpolating temporal shift: tshift_forward's problem (shiftnd_tshift.hip)
// on the int_repr of a per-tensor quantized segment-major tensor (memory order N, S0, C, S1, S2), an fp32 [C] table (gfx950).
// shiftnd_forward_quantized under SHIFTND_SHIFT_DIM0 with wq_dtype == SHIFTND_F32 selects it.
//
// The result is defined in the integer domain -- the scale does not enter and nothing is dequantized:
//     r   = lerp1(q[pad(t - iw)] - zp, q[pad(t - iw + 1)] - zp, dw)      iw, dw: prep_shift_forward<F>(F(w_c), active = true)
//     out = clamp(zp + rint(r), the element type's range)                 rint: half to even
// in F = fp32 for I8 / U8 (q - zp is exact there) and F = fp64 for I32 (exact only there); a filled frame contributes 0 to r, which
// is the zero point in out.  lerp1 is the library's: two multiplies and one add, -ffp-contract=off.
//
//   tshift_forward_quantized   tshift_forward's structure: flat over the output in naturally aligned units, four in flight per
//                    thread.  Per unit: its plane by three multiply-shift divisions, the channel's fp32 weight (one load), the two
//                    source frames (fold_index o canon_shift), nontemporal loads of the two source units (none for a filled frame:
//                    its unit is the zero point in every element), then per element unpack, - zp, lerp1, rint, + zp, clamp, pack,
//                    and one nontemporal store.  A fraction of exactly 0 stores the first source unit's bytes (lerp1(a, b, 0) == a
//                    for finite b: the same values, none of the arithmetic).
//
// One-byte elements.  I8 shares U8's path: q ^ 0x80 is q + 128 as an unsigned byte, so with the zero point moved by 128 the
// differences q - zp are the same numbers; the result is flipped back.  `flip` (0x80808080 or 0) and the moved zero point are
// launch-uniform.  Unpack is a byte-to-float convert (v_cvt_f32_ubyteN), pack is v_cvt_pk_u8_f32, which converts, saturates to
// 0..255 (the clamp) and inserts the byte in one instruction; its argument is already a whole number, so its rounding does not matter.
//
// Units.  16, 8, 4, 2 or 1 bytes (at least one element): the largest power of two that divides the plane's bytes and every base
// (piece_bytes), so no unit holds two planes (two weights).  The element type and the unit are launch-uniform switches inside ONE
// kernel (scalar branches), as the unit is in tshift_forward.  No LDS, no scratch; nothing outside x, the table and out is touched:
// a source unit lies at the output unit's offset inside another plane of x.
//
// Not built: channels-last tensors, a cut window, an in-place or online form, requantization to another scale.  (Per-clip tables and
// temporal interlacing: shiftnd_interlace_quant.hip.)
#include <type_traits>

#include "shiftnd_quant_unit.hpp"   // QUnit, load_qunit / store_qunit, blend_bytes / blend_words

namespace shiftnd {
namespace {

constexpr int kQInFlight = 4;   // units per thread, every load issued before the first store

struct QTShiftParams {
    int pad, wide;                   // wide: I32 elements (fp64 arithmetic); else one-byte elements (fp32)
    uint32_t T, C, upp;              // frames per clip, channels, units per plane
    FastDiv d_upp, d_C, d_T, d_per;  // d_per: by map_period(T, pad)
    int64_t plane_bytes, units;      // units: of the whole tensor
    uint32_t flip;                   // I8: 0x80808080 (the bytes are handled as q + 128), else 0
    int32_t zp;                      // the zero point (I8: + 128, so 0..255 for both one-byte types)
};

constexpr int64_t kFill = -1, kPast = -2;

template <bool WIDE, int V>
__device__ __forceinline__ void qforward_body(const QTShiftParams &q, const char *__restrict__ x, const float *__restrict__ w,
                                              char *__restrict__ out) {
    using CT = typename std::conditional<WIDE, double, float>::type;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * (kThreads * kQInFlight) + threadIdx.x;
    const int Tn = static_cast<int>(q.T);
    int64_t sa[kQInFlight], sb[kQInFlight];   // byte offset in x of the unit's two sources, or a mark
    CT dw[kQInFlight];
#pragma unroll
    for (int k = 0; k < kQInFlight; ++k) {
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
        prep_shift_forward<CT>(static_cast<CT>(w[c]), true, iw, dw[k]);
        const int cs = canon_shift(iw, Tn, q.pad, q.d_per);
        const int s0 = source_frame(static_cast<int>(t), cs, Tn, q.pad), s1 = source_frame(static_cast<int>(t) + 1, cs, Tn, q.pad);
        const int64_t clip = static_cast<int64_t>(n) * q.T;
        sa[k] = s0 < 0 ? kFill : ((clip + s0) * q.C + c) * q.plane_bytes + at;
        sb[k] = (s1 < 0 || dw[k] == CT(0)) ? kFill : ((clip + s1) * q.C + c) * q.plane_bytes + at;   // (fraction 0: a copy of the first source)
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
        QUnit<V> r = a[k];
        if (dw[k] != CT(0)) {
            if constexpr (WIDE) r = blend_words<V>(a[k], b[k], dw[k], static_cast<double>(q.zp));
            else r = blend_bytes<V>(a[k], b[k], dw[k], static_cast<float>(q.zp));
        }
#pragma unroll
        for (int i = 0; i < (V >= 4 ? V / 4 : 1); ++i) r.d[i] ^= q.flip;
        store_qunit<V>(out + (first + k * kThreads) * V, r);
    }
}

// ONE kernel: the element type (q.wide, q.flip) and the unit (1 << unit_log2 bytes) are launch-uniform, scalar branches
__global__ __launch_bounds__(kThreads) void tshift_forward_quantized(QTShiftParams q, const char *__restrict__ x,
                                                                    const float *__restrict__ w, char *__restrict__ out,
                                                                    int unit_log2) {
    if (q.wide) {
        if (unit_log2 == 4) qforward_body<true, 16>(q, x, w, out);
        else if (unit_log2 == 3) qforward_body<true, 8>(q, x, w, out);
        else qforward_body<true, 4>(q, x, w, out);
    } else {
        if (unit_log2 == 4) qforward_body<false, 16>(q, x, w, out);
        else if (unit_log2 == 3) qforward_body<false, 8>(q, x, w, out);
        else if (unit_log2 == 2) qforward_body<false, 4>(q, x, w, out);
        else if (unit_log2 == 1) qforward_body<false, 2>(q, x, w, out);
        else qforward_body<false, 1>(q, x, w, out);
    }
}

}  // namespace

// the sizes: 2 or 3 spatial dims, the whole window, segment_counts_fit's 32-bit limits with the element as the unit (fewer than
// 2^31 - 16 elements in the tensor); the zero point inside the element type's range
bool tshift_quantized_geometry_ok(const Geometry &g, int dtype, int64_t zp) {
    const int64_t lo = dtype == SHIFTND_U8 ? 0 : (dtype == SHIFTND_I8 ? -128 : INT32_MIN);
    const int64_t hi = dtype == SHIFTND_U8 ? 255 : (dtype == SHIFTND_I8 ? 127 : INT32_MAX);
    return dtype >= SHIFTND_I8 && dtype <= SHIFTND_I32 && zp >= lo && zp <= hi && g.nd >= 2 && !cropped(g) && segment_counts_fit(g, 1);
}

int tshift_quantized_forward(const Geometry &g, int dtype, const void *x, const void *w, int64_t zp, void *out, hipStream_t st) {
    const int es = dtype_size(dtype);
    const int unit = piece_bytes(frame_pixels(g) * es, {x, out});
    QTShiftParams q;
    q.pad = g.pad;
    q.wide = dtype == SHIFTND_I32;
    q.T = static_cast<uint32_t>(g.S[3 - g.nd]);
    q.C = static_cast<uint32_t>(g.C);
    q.plane_bytes = frame_pixels(g) * es;
    q.upp = static_cast<uint32_t>(q.plane_bytes / unit);
    q.units = g.N * q.T * q.C * static_cast<int64_t>(q.upp);
    q.d_upp = make_fastdiv(q.upp);
    q.d_C = make_fastdiv(q.C);
    q.d_T = make_fastdiv(q.T);
    q.d_per = make_fastdiv(static_cast<uint32_t>(map_period(static_cast<int>(q.T), g.pad)));
    q.flip = dtype == SHIFTND_I8 ? 0x80808080u : 0u;
    q.zp = static_cast<int32_t>(dtype == SHIFTND_I8 ? zp + 128 : zp);
    note_kernel("tshift_forward_quantized");
    const int64_t per = kThreads * kQInFlight;
    hipLaunchKernelGGL(tshift_forward_quantized, dim3(static_cast<unsigned>((q.units + per - 1) / per)), dim3(kThreads), 0, st, q,
                       static_cast<const char *>(x), static_cast<const float *>(w), static_cast<char *>(out), __builtin_ctz(unit));
    return SHIFTND_OK;
}

}  // namespace shiftnd
