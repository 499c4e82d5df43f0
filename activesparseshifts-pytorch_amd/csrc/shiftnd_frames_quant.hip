// shiftnd_frames_quant.hip -- the QUANTIZED interpolating temporal shift of CHANNELS-LAST tensors: the problem of
// shiftnd_tshift_quant.hip on the layout of shiftnd_frames_learn.hip -- the int_repr of a per-tensor
// quantized tensor in memory order N, S0, S1, S2, C, an fp32 [C] table (gfx950).  shiftnd_forward_quantized under
// SHIFTND_SHIFT_DIM0 | SHIFTND_FRAMES with wq_dtype == SHIFTND_F32 selects it.
//
// The result is tshift_forward_quantized's, bit for bit, defined in the integer domain:
//     r   = lerp1(q[pad(t - iw)] - zp, q[pad(t - iw + 1)] - zp, dw)      iw, dw: prep_shift_forward<F>(F(w_c), active = true)
//     out = clamp(zp + rint(r), the element type's range)                 rint: half to even
// in F = fp32 for I8 / U8 and F = fp64 for I32; a filled frame contributes 0 to r, which is the zero point in out.  lerp1 is the
// library's: two multiplies and one add, -ffp-contract=off.  I8 shares U8's path through q ^ 0x80 with the zero point moved by 128;
// unpack is v_cvt_f32_ubyteN, pack is v_cvt_pk_u8_f32 (which saturates: the clamp).
//
//   frames_forward_quantized   the shape of frames_active_forward: a workgroup inside ONE frame (n, t), max(1, 256 / P) pixel rows
//                    per step, a thread keeps its piece column k of the rows for its whole life and reads the piece's weights ONCE.
//                    A pixel's channel row is contiguous, so a 16-byte piece holds 16 one-byte channels with 16 DIFFERENT weights:
//                    source frames and fractions are per ELEMENT in every path.  Per piece one of three paths, chosen once per
//                    thread and piece (constant over the thread's rows):
//       uniform      every element has the same two source frames (TSM-like and group tables): two piece loads per output piece,
//                    none for a filled frame (the zero point), no second load where every fraction is 0; kRowsUniform rows in
//                    flight, every load issued before the first store.
//       few frames   the elements draw on at most kSlots DISTINCT source frames (a fill is a slot that holds the zero point; an
//                    element whose fraction is exactly 0 asks for its first frame alone): those pieces are loaded WHOLE, with loads
//                    of the piece's width, and each element's two values are picked from its two slots -- one-byte elements with
//                    one v_perm_b32 per slot pair, dword and source, OR-ed (selectors built once per piece), I32 with selects;
//                    one row at a time, its up to kSlots loads issued together.  A trained table leaves almost no piece uniform: this is the path it runs on.
//       many frames  element by element from each element's own two frames, element-sized loads, one row at a time: right for any
//                    table, any S0, any padding.
//                    A fraction of exactly 0 gives the first source's element unchanged in all three: lerp1(a, b, 0) == a for a
//                    finite b, and rint(a - zp) + zp == a.
//
// Pieces.  16, 8, 4, 2 or 1 bytes (at least one element): piece_bytes(C * element size, {x, out}).  The element type and the piece
// are launch-uniform switches inside ONE kernel (scalar branches).  No LDS, no scratch.  Every access is naturally aligned and
// inside x, the table's C floats and out: a source piece lies at the output piece's offset inside another frame of the same clip.
// Frame bases are 64-bit, offsets inside a frame are below 2^31 elements (frames_geometry_ok).
//
// The blend helpers are NOT shared with shiftnd_tshift_quant.hip: that kernel blends a unit under ONE fraction (its (1 - d) is
// formed once per unit), this one under a fraction per element; a common header would have had to change the other kernel's code.
//
// Not built: a cut window, per-clip tables, an in-place or online form, requantization to another scale, an LDS clip tile.
#include <type_traits>

#include "shiftnd_temporal.hpp"

namespace shiftnd {
namespace {

constexpr int kRowsUniform = 4;            // rows in flight per thread, uniform pieces (frames_active_forward's kFwdInFlight: the plan's batch)
constexpr int kRowsFew = 1;                // ... pieces on the few-frames path: up to kSlots piece loads each
constexpr int kSlots = 6;                  // K: distinct source frames (a fill included) a piece may draw on to be loaded whole; even.
                                           // 6 takes every table within [-2, 2) (floors -2 .. 1: the frames t - 1 .. t + 3) and is what
                                           // the registers hold at frames_active_forward's 3 waves per SIMD without scratch
constexpr int64_t kWantWorkgroups = 6144;  // frames are cut into more workgroups while the grid is short of this many (as frames_active_forward)

static_assert(kSlots % 2 == 0 && kSlots <= 8, "slot pairs; three bits per slot");

struct QFramesParams {
    int pad, wide, unit_log2;               // wide: I32 elements (fp64 arithmetic); else one-byte elements (fp32)
    uint32_t T, P, span, rps;               // frames per clip, pieces per row, min(P, 256), rows per step = max(1, 256 / P)
    uint32_t chunks, rows_per_wg;           // workgroups per frame, rows of each
    FastDiv d_chunks, d_T, d_span, d_per;   // d_per: by map_period(T, pad)
    int64_t M, R, frame_bytes;              // pixels per frame, bytes per row, bytes per frame
    uint32_t flip;                          // I8: 0x80808080 (the bytes are handled as q + 128), else 0
    int32_t zp;                             // the zero point (I8: + 128, so 0..255 for both one-byte types)
};

// a piece of V bytes as dwords (V < 4: the low bytes of one)
template <int V> struct QPiece { uint32_t d[V >= 4 ? V / 4 : 1]; };

template <int V> __device__ __forceinline__ QPiece<V> fill_qpiece(uint32_t dword) {
    QPiece<V> u;
#pragma unroll
    for (int i = 0; i < (V >= 4 ? V / 4 : 1); ++i) u.d[i] = dword;
    return u;
}
// the piece at p, its bytes flipped (I8)
template <int V, bool NT> __device__ __forceinline__ QPiece<V> load_qpiece(const char *p, uint32_t flip) {
    typedef typename vec_of<V>::type vec_t;
    const vec_t v = NT ? __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(p)) : *reinterpret_cast<const vec_t *>(p);
    QPiece<V> u;
    if constexpr (V >= 4) __builtin_memcpy(u.d, &v, V);
    else u.d[0] = v;
#pragma unroll
    for (int i = 0; i < (V >= 4 ? V / 4 : 1); ++i) u.d[i] ^= flip;
    return u;
}
template <int V> __device__ __forceinline__ void store_qpiece(char *p, QPiece<V> u, uint32_t flip) {
    typedef typename vec_of<V>::type vec_t;
#pragma unroll
    for (int i = 0; i < (V >= 4 ? V / 4 : 1); ++i) u.d[i] ^= flip;
    vec_t v;
    if constexpr (V >= 4) __builtin_memcpy(&v, u.d, V);
    else v = static_cast<vec_t>(u.d[0]);
    __builtin_nontemporal_store(v, reinterpret_cast<vec_t *>(p));
}

// one dword of a piece, its elements each under its own fraction d[0 ..]:
//   one-byte elements (N of them, the low bytes) as unsigned bytes (I8 flipped by the loads), fp32, zp in 0..255;
//   an I32 element in fp64
template <bool WIDE, int N, typename CT> __device__ __forceinline__ uint32_t blend_dword(uint32_t a, uint32_t b, const CT *d, CT zp) {
    if constexpr (WIDE) {
        const double va = static_cast<double>(static_cast<int32_t>(a)) - zp;
        const double vb = static_cast<double>(static_cast<int32_t>(b)) - zp;
        double v = rint(va * (1.0 - d[0]) + vb * d[0]) + zp;   // lerp1
        v = v < -2147483648.0 ? -2147483648.0 : (v > 2147483647.0 ? 2147483647.0 : v);
        return static_cast<uint32_t>(static_cast<int32_t>(v));
    } else {
        uint32_t packed = 0;
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const float va = static_cast<float>((a >> (8 * e)) & 0xffu) - zp;
            const float vb = static_cast<float>((b >> (8 * e)) & 0xffu) - zp;
            const float v = va * (1.0f - d[e]) + vb * d[e];   // lerp1
            packed = __builtin_amdgcn_cvt_pk_u8_f32(rintf(v) + zp, e, packed);   // saturates to 0..255
        }
        return packed;
    }
}

template <bool WIDE, int V, typename CT, int E>
__device__ __forceinline__ QPiece<V> blend_each(const QPiece<V> &a, const QPiece<V> &b, const CT (&d)[E], CT zp) {
    constexpr int D = V >= 4 ? V / 4 : 1, N = E / D;   // dwords, elements of each
    QPiece<V> r;
#pragma unroll
    for (int i = 0; i < D; ++i) r.d[i] = blend_dword<WIDE, N, CT>(a.d[i], b.d[i], &d[i * N], zp);
    return r;
}

template <bool WIDE, int V>
__device__ __forceinline__ void qframes_body(const QFramesParams &q, const char *__restrict__ x, const float *__restrict__ w,
                                             char *__restrict__ out) {
    using CT = typename std::conditional<WIDE, double, float>::type;
    constexpr int E = WIDE ? V / 4 : V;       // elements of a piece
    constexpr int D = V >= 4 ? V / 4 : 1;     // its dwords
    constexpr int ES = WIDE ? 4 : 1;
    const uint32_t frame = fdiv(blockIdx.x, q.d_chunks);   // n * T + t
    const uint32_t chunk = blockIdx.x - frame * q.chunks;
    const uint32_t n = fdiv(frame, q.d_T);
    const int t = static_cast<int>(frame - n * q.T), Tn = static_cast<int>(q.T);
    const uint32_t rl = fdiv(threadIdx.x, q.d_span);       // the thread's row of a step, its piece of the row
    const uint32_t k0 = threadIdx.x - rl * q.span;
    if (rl >= q.rps) return;                               // (idle tail lanes where P does not divide 256)
    const int64_t first_row = static_cast<int64_t>(chunk) * q.rows_per_wg;
    const int rows = static_cast<int>(first_row + q.rows_per_wg < q.M ? q.rows_per_wg : q.M - first_row);
    const int rps = static_cast<int>(q.rps);
    const int64_t here = static_cast<int64_t>(frame) * q.frame_bytes + first_row * q.R;     // the workgroup's rows of the output
    const int64_t clip = static_cast<int64_t>(n) * q.T * q.frame_bytes + first_row * q.R;   // the same rows of the clip's frame 0
    const int64_t step = static_cast<int64_t>(q.rps) * q.R;
    // a filled frame: the zero point in every element, so that q - zp is 0 (in the flipped domain, as the loads deliver)
    const uint32_t zfill = WIDE ? static_cast<uint32_t>(q.zp) : static_cast<uint32_t>(q.zp) * 0x01010101u;
    const CT zp = static_cast<CT>(q.zp);
#pragma unroll 1
    for (uint32_t k = k0; k < q.P; k += kThreads) {        // (once unless a row has more than 256 pieces)
        int sa[E], sb[E];
        CT dw[E];
        bool uniform = true, blend = false;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            int64_t iw;
            prep_shift_forward<CT>(static_cast<CT>(w[static_cast<int64_t>(k) * E + e]), true, iw, dw[e]);
            const int cs = canon_shift(iw, Tn, q.pad, q.d_per);
            sa[e] = source_frame(t, cs, Tn, q.pad);
            sb[e] = source_frame(t + 1, cs, Tn, q.pad);
            uniform = uniform && sa[e] == sa[0] && sb[e] == sb[0];
            blend = blend || dw[e] != CT(0);
        }
        int64_t off = static_cast<int64_t>(rl) * q.R + static_cast<int64_t>(k) * V;
        if (uniform) {
            const bool la = sa[0] >= 0, lb = blend && sb[0] >= 0;   // (a fill issues no load; nor does a second source nobody blends)
            const char *srca = x + clip + (la ? sa[0] : 0) * q.frame_bytes, *srcb = x + clip + (lb ? sb[0] : 0) * q.frame_bytes;
#pragma unroll 1
            for (int r = static_cast<int>(rl); r < rows; r += rps * kRowsUniform) {
                QPiece<V> a[kRowsUniform], b[kRowsUniform];
#pragma unroll
                for (int j = 0; j < kRowsUniform; ++j) {
                    a[j] = b[j] = fill_qpiece<V>(zfill);
                    if (r + j * rps < rows) {
                        if (la) a[j] = load_qpiece<V, true>(srca + off + j * step, q.flip);
                        if (lb) b[j] = load_qpiece<V, true>(srcb + off + j * step, q.flip);
                    }
                }
#pragma unroll
                for (int j = 0; j < kRowsUniform; ++j)
                    if (r + j * rps < rows)
                        store_qpiece<V>(out + here + off + j * step, blend ? blend_each<WIDE, V>(a[j], b[j], dw, zp) : a[j], q.flip);
                off += kRowsUniform * step;
            }
            continue;
        }
        // the distinct frames the piece draws on (-1: the fill), in order of first use, and each element's two slots:
        //   one-byte elements: v_perm_b32 selectors per dword, slot pair and source -- byte j of the dword from slot 2 p (selector
        //   4 + j: the first operand) or 2 p + 1 (selector j), 0x0c (a zero byte) in the other pair's selector;
        //   I32: three bits per element and source
        int fr[kSlots];
#pragma unroll
        for (int s = 0; s < kSlots; ++s) fr[s] = -2;
        int used = 0;
        bool fits = true;
        constexpr uint32_t kIdle = V >= 4 ? 0u : (V == 2 ? 0x0c0c0000u : 0x0c0c0c00u);   // (the bytes past a piece under 4 bytes)
        uint32_t sel[2][kSlots / 2][D];   // [source][slot pair][dword]
        uint32_t idx = 0;                 // I32: slot of element e's source h at bits 3 * (h * E + e)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int p = 0; p < kSlots / 2; ++p)
#pragma unroll
                for (int i = 0; i < D; ++i) sel[h][p][i] = kIdle;
#pragma unroll
        for (int e = 0; e < E; ++e) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int f = (h == 0 || dw[e] == CT(0)) ? sa[e] : sb[e];   // (fraction 0: the first source alone)
                int s = -1;
#pragma unroll
                for (int j = 0; j < kSlots; ++j)
                    if (s < 0 && j < used && fr[j] == f) s = j;
                if (s < 0) {
                    if (used < kSlots) {
                        s = used;
#pragma unroll
                        for (int j = 0; j < kSlots; ++j) fr[j] = j == used ? f : fr[j];
                        ++used;
                    } else {
                        fits = false;
                        s = 0;
                    }
                }
                if constexpr (WIDE) {
                    idx |= static_cast<uint32_t>(s) << (3 * (h * E + e));
                } else {
                    const uint32_t code = static_cast<uint32_t>((s & 1) ? (e & 3) : 4 + (e & 3));
#pragma unroll
                    for (int p = 0; p < kSlots / 2; ++p) sel[h][p][e / 4] |= ((s >> 1) == p ? code : 0x0cu) << (8 * (e & 3));
                }
            }
        }
        if (fits) {
#pragma unroll 1
            for (int r = static_cast<int>(rl); r < rows; r += rps * kRowsFew) {
                QPiece<V> slot[kRowsFew][kSlots];
#pragma unroll
                for (int j = 0; j < kRowsFew; ++j)
#pragma unroll
                    for (int s = 0; s < kSlots; ++s) {
                        slot[j][s] = fill_qpiece<V>(zfill);
                        if (r + j * rps < rows && s < used && fr[s] >= 0)
                            slot[j][s] = load_qpiece<V, false>(x + clip + fr[s] * q.frame_bytes + off + j * step, q.flip);
                    }
#pragma unroll
                for (int j = 0; j < kRowsFew; ++j) {
                    if (r + j * rps >= rows) continue;
                    QPiece<V> ab[2];
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int i = 0; i < D; ++i) {
                            if constexpr (WIDE) {
                                const uint32_t s = (idx >> (3 * (h * E + i))) & 7u;
                                uint32_t v = slot[j][0].d[i];
#pragma unroll
                                for (int c = 1; c < kSlots; ++c) v = s == static_cast<uint32_t>(c) ? slot[j][c].d[i] : v;
                                ab[h].d[i] = v;
                            } else {
                                uint32_t v = 0;
#pragma unroll
                                for (int p = 0; p < kSlots / 2; ++p)
                                    v |= __builtin_amdgcn_perm(slot[j][2 * p].d[i], slot[j][2 * p + 1].d[i], sel[h][p][i]);
                                ab[h].d[i] = v;
                            }
                        }
                    store_qpiece<V>(out + here + off + j * step, blend_each<WIDE, V>(ab[0], ab[1], dw, zp), q.flip);
                }
                off += kRowsFew * step;
            }
            continue;
        }
        // many frames: each element from its own two frames, one row at a time, one dword of the piece after the other (up to 8
        // element loads in flight: the scheduling barrier keeps the 2 E loads of a piece, each under a 64-bit address, apart)
        typedef typename raw_t<ES>::type raw;
        constexpr int N = E / D;   // elements of a dword
        const uint32_t zelem = WIDE ? zfill : (zfill & 0xffu), felem = WIDE ? 0u : (q.flip & 0xffu);
#pragma unroll 1
        for (int r = static_cast<int>(rl); r < rows; r += rps) {
            const char *at = x + clip + off;
            QPiece<V> res;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                uint32_t a = 0, b = 0;
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    const int e = i * N + j;
                    uint32_t va = zelem, vb = zelem;
                    // (the frame numbers pass through an empty asm: their 2 E products with frame_bytes, 64-bit each, are formed
                    // here, per row, instead of being hoisted out of the row loop into 4 E registers)
                    int fa = sa[e], fb = sb[e];
                    asm volatile("" : "+v"(fa), "+v"(fb));
                    if (fa >= 0) va = static_cast<uint32_t>(*reinterpret_cast<const raw *>(at + fa * q.frame_bytes + e * ES)) ^ felem;
                    if (fb >= 0 && dw[e] != CT(0))
                        vb = static_cast<uint32_t>(*reinterpret_cast<const raw *>(at + fb * q.frame_bytes + e * ES)) ^ felem;
                    a |= va << (8 * j * (WIDE ? 0 : 1));
                    b |= vb << (8 * j * (WIDE ? 0 : 1));
                }
                res.d[i] = blend_dword<WIDE, N, CT>(a, b, &dw[i * N], zp);
                __builtin_amdgcn_sched_barrier(0);
            }
            store_qpiece<V>(out + here + off, res, q.flip);
            off += step;
        }
    }
}

// ONE kernel: the element type (q.wide, q.flip) and the piece (1 << q.unit_log2 bytes) are launch-uniform, scalar branches
__global__ __attribute__((amdgpu_waves_per_eu(3))) __launch_bounds__(kThreads) void frames_forward_quantized(QFramesParams q, const char *__restrict__ x,
                                                                    const float *__restrict__ w, char *__restrict__ out) {
    if (q.wide) {
        if (q.unit_log2 == 4) qframes_body<true, 16>(q, x, w, out);
        else if (q.unit_log2 == 3) qframes_body<true, 8>(q, x, w, out);
        else qframes_body<true, 4>(q, x, w, out);
    } else {
        if (q.unit_log2 == 4) qframes_body<false, 16>(q, x, w, out);
        else if (q.unit_log2 == 3) qframes_body<false, 8>(q, x, w, out);
        else if (q.unit_log2 == 2) qframes_body<false, 4>(q, x, w, out);
        else if (q.unit_log2 == 1) qframes_body<false, 2>(q, x, w, out);
        else qframes_body<false, 1>(q, x, w, out);
    }
}

}  // namespace

// the sizes: frames_geometry_ok's (2 or 3 spatial dims, the whole window, 64-bit frame bases, 32-bit counts inside a frame) on a
// quantized element type, the zero point inside the type's range
bool frames_quantized_geometry_ok(const Geometry &g, int dtype, int64_t zp) {
    const int64_t lo = dtype == SHIFTND_U8 ? 0 : (dtype == SHIFTND_I8 ? -128 : INT32_MIN);
    const int64_t hi = dtype == SHIFTND_U8 ? 255 : (dtype == SHIFTND_I8 ? 127 : INT32_MAX);
    if (dtype < SHIFTND_I8 || dtype > SHIFTND_I32 || zp < lo || zp > hi) return false;
    Geometry s = g;
    s.active = 0;   // (frames_geometry_ok speaks for the sparse kernels; the sizes are the same)
    return frames_geometry_ok(s, dtype);
}

int frames_quantized_forward(const Geometry &g, int dtype, const void *x, const void *w, int64_t zp, void *out, hipStream_t st) {
    const int es = dtype_size(dtype);
    const int unit = piece_bytes(g.C * es, {x, out});
    QFramesParams q;
    q.pad = g.pad;
    q.wide = dtype == SHIFTND_I32;
    q.unit_log2 = __builtin_ctz(unit);
    q.T = static_cast<uint32_t>(g.S[3 - g.nd]);
    q.M = frame_pixels(g);
    q.R = g.C * es;
    q.frame_bytes = q.M * q.R;
    q.P = static_cast<uint32_t>(q.R / unit);
    q.span = q.P < static_cast<uint32_t>(kThreads) ? q.P : static_cast<uint32_t>(kThreads);
    q.rps = static_cast<uint32_t>(kThreads) / q.span;
    q.d_T = make_fastdiv(q.T);
    q.d_span = make_fastdiv(q.span);
    q.d_per = make_fastdiv(static_cast<uint32_t>(map_period(static_cast<int>(q.T), g.pad)));
    q.flip = dtype == SHIFTND_I8 ? 0x80808080u : 0u;
    q.zp = static_cast<int32_t>(dtype == SHIFTND_I8 ? zp + 128 : zp);
    // workgroups per frame, as frames_active_forward: at least one batch of kRowsUniform steps each, more steps while the grid is large
    const int64_t frames = g.N * q.T, batch_rows = static_cast<int64_t>(q.rps) * kRowsUniform;
    const int64_t most = (q.M + batch_rows - 1) / batch_rows;
    const int64_t wanted = (kWantWorkgroups + frames - 1) / frames;
    const int64_t chunks = most < wanted ? most : wanted;
    q.rows_per_wg = static_cast<uint32_t>(((q.M + chunks - 1) / chunks + batch_rows - 1) / batch_rows * batch_rows);
    q.chunks = static_cast<uint32_t>((q.M + q.rows_per_wg - 1) / q.rows_per_wg);
    q.d_chunks = make_fastdiv(q.chunks);
    note_kernel(unit == 16 ? "frames_forward_quantized" : "frames_forward_quantized_ragged");
    void (*const kernel)(QFramesParams, const char *, const float *, char *) = frames_forward_quantized;   // (the kernel, not this function)
    const int64_t blocks = frames * q.chunks;   // (below 2^31: frames is, and a frame is cut only while the grid is short of 6144)
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, st, q, static_cast<const char *>(x),
                       static_cast<const float *>(w), static_cast<char *>(out));
    return SHIFTND_OK;
}

}  // namespace shiftnd
