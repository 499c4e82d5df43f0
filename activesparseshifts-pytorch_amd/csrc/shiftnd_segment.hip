// shiftnd_segment.hip -- the sparse shift of "segment-major" tensors: memory order N, S0, C, S1, S2 (gfx950).
//
// A video tensor [N*T, C, H, W] whose clips of T frames are shifted along T (the Temporal Shift Module, arXiv 1811.08383) is, seen as
// a shift problem, [N, C, T, H*W] with strides {T*C*M, M, C*M, 1}: the shifted dim lies OUTSIDE the channel dim.  For every
// (n, t, c) the op copies one contiguous plane of `inner` elements from segment pad(t - s_c) of the same sample, or fills it with
// the fill value: no arithmetic, and of the element type only its size and its fill pattern (all-zero bits in every float type;
// the zero point of a quantized tensor, one byte for int8 / uint8 and a dword for int32 -- a dword pattern in the params, the byte
// splatted four times).  The kernels stream the output flat in aligned 16-byte pieces and find each piece's plane with three
// multiply-shift divisions on a count of UNITS: the element where it is one byte, two bytes elsewhere (every other element size
// is a multiple, and a 32-bit unit count then covers 4 GiB of them).  Before these kernels this stride pattern ended in
// strided_gather_forward (one element per thread, 64-bit divisions).
//
// The host routes by strides alone and cannot read the device table, so the kernels are right for EVERY [C, ndim] table: a
// plane whose channel also shifts an inner dim is gathered through pad_index, one unit at a time (slow, exact), inside the same
// kernel; planes with zero inner shifts (every plane of a temporal shift) are the plane copy / fill.  The table is any kind
// gather_shift reads: floats rounded half to even, or I8 / U8 / I32 integers minus their zero point (quantized calls).
//
// One kernel, two forms (shiftnd_last_kernel() names the form):
//   segment_forward          planes of whole 16-byte pieces, 16-byte-aligned bases: one 16-byte nontemporal load and store per piece
//   segment_forward_ragged   everything else (7 x 7 and 14 x 14 planes of 8- and 16-bit elements, bases offset by an element, which
//                            for one-byte elements is any byte, with planes of an odd number of bytes): aligned
//                            16-byte stores; a piece lies in one plane or straddles two, and each part is funnelled out of the
//                            (at most two) ALIGNED 16-byte pieces of x that hold its source bytes.  Every load and store is
//                            naturally aligned, and a load is issued only when it holds a byte the result needs, so none leaves
//                            the 16-byte granules the tensor itself touches.  Partial pieces at the two ends of the tensor and
//                            pieces over more than two planes (planes under 16 bytes) move one unit at a time.  A filled
//                            part is the fill pattern: an int32 plane starts at a multiple of 4 bytes of the 4-byte-aligned
//                            tensor, so the dwords of an aligned output piece are whole elements.
// The backward of a fixed shift (shiftnd_backward's x == NULL form, whole window) is the forward under the negated table and
// arrives here through forward_common with the gradient's strides.
#include "shiftnd_temporal.hpp"

namespace shiftnd {
namespace {

constexpr int kWholeInFlight = 4;    // pieces per thread, every load issued before the first store
constexpr int kRaggedInFlight = 2;   // (up to four loads per piece)

struct SegmentParams {
    int nd, pad, wkind, es_log2;       // es: element bytes (the per-element gather only)
    uint32_t T, C, upp;                // segments, channels, units per plane
    FastDiv d_upp, d_C, d_T, d_per;    // d_per: by map_period(T, pad)
    int64_t A, B;                      // the plane as [A][B] elements (A = 1 for ndim 2)
    int64_t plane_bytes, total_bytes;
    int64_t wzp;                       // zero point of an integer table
    int unit_log2;                     // the stream unit: 0 (one byte) for 1-byte elements, 1 (two bytes) otherwise
    uint32_t fill;                     // what a filled plane holds, as a dword pattern (0 for floats)
};

struct Place {
    uint32_t n, t, c;          // sample, segment, channel of a plane
    int64_t s0, sA, sB;        // rint of the channel's table row
};

__device__ __forceinline__ Place place_plane(const SegmentParams &q, const void *w, uint32_t plane) {
    Place p;
    const uint32_t nt = fdiv(plane, q.d_C);
    p.c = plane - nt * q.C;
    p.n = fdiv(nt, q.d_T);
    p.t = nt - p.n * q.T;
    const int64_t row = static_cast<int64_t>(p.c) * q.nd;
    p.s0 = gather_shift(w, q.wkind, q.wzp, row);
    p.sA = q.nd == 3 ? gather_shift(w, q.wkind, q.wzp, row + 1) : 0;
    p.sB = gather_shift(w, q.wkind, q.wzp, row + q.nd - 1);
    return p;
}

// size-1 dims ignore their shift, like every kernel of the library
__device__ __forceinline__ bool inner_shift(const SegmentParams &q, const Place &p) {
    return (q.B > 1 && p.sB != 0) || (q.A > 1 && p.sA != 0);
}

// byte offset in x of the plane that plane `p` copies, or -1 (fill).  fold_index(t - canon_shift(s)) == pad_index(t - s) for t in
// [0, T] (shiftnd_common.hpp; checked by tests/test_host_logic.py)
__device__ __forceinline__ int64_t source_plane(const SegmentParams &q, const Place &p) {
    const int T = static_cast<int>(q.T);
    const int ts = fold_index(static_cast<int>(p.t) - canon_shift(p.s0, T, q.pad, q.d_per), T, q.pad);
    return ts < 0 ? -1 : ((static_cast<int64_t>(p.n) * q.T + ts) * q.C + p.c) * q.plane_bytes;
}

// The 16 output bytes from stream byte `sb` on, one unit at a time, the part inside the tensor: every padding map through
// pad_index, the inner dims included.
__device__ __forceinline__ void slow_units(const SegmentParams &q, const char *x, const void *w, char *out, int64_t sb) {
    const int ul = q.unit_log2, step = 1 << ul;
#pragma unroll 1
    for (int k = 0; k < 16; k += step) {
        const int64_t b = sb + k;
        if (b < 0 || b >= q.total_bytes) continue;
        const uint32_t u = static_cast<uint32_t>(b >> ul);
        const uint32_t plane = fdiv(u, q.d_upp);
        const int64_t at = static_cast<int64_t>(u - plane * q.upp) << ul;   // byte in the plane
        const Place p = place_plane(q, w, plane);
        const int64_t ts = pad_index(static_cast<int64_t>(p.t) - p.s0, q.T, q.pad);
        int64_t e = at >> q.es_log2;                                       // element in the plane
        const int64_t in_element = at - (e << q.es_log2);
        bool valid = ts >= 0;
        if (inner_shift(q, p)) {
            const int64_t a = e / q.B, bb = e - a * q.B;
            const int64_t as = q.A == 1 ? 0 : pad_index(a - p.sA, q.A, q.pad);
            const int64_t bs = q.B == 1 ? 0 : pad_index(bb - p.sB, q.B, q.pad);
            valid = valid && as >= 0 && bs >= 0;
            e = as * q.B + bs;
        }
        const char *from = x + ((static_cast<int64_t>(p.n) * q.T + ts) * q.C + p.c) * q.plane_bytes + (e << q.es_log2) + in_element;
        const uint32_t f = q.fill >> (8 * (static_cast<int>(in_element) & 3));   // (the unit's bytes of the element's fill)
        if (ul == 0) {
            uint8_t v = static_cast<uint8_t>(f);
            if (valid) v = *reinterpret_cast<const uint8_t *>(from);
            *reinterpret_cast<uint8_t *>(out + b) = v;
        } else {
            uint16_t v = static_cast<uint16_t>(f);
            if (valid) v = *reinterpret_cast<const uint16_t *>(from);
            *reinterpret_cast<uint16_t *>(out + b) = v;
        }
    }
}

constexpr int64_t kFill = -1, kSlow = -2, kPast = -3;

// planes of whole 16-byte pieces, 16-byte-aligned bases
__device__ __forceinline__ void whole_pieces_body(const SegmentParams &q, const char *__restrict__ x, const void *__restrict__ w,
                                                  char *__restrict__ out) {
    const int64_t first = static_cast<int64_t>(blockIdx.x) * (kThreads * kWholeInFlight) + threadIdx.x;
    const int64_t pieces = q.total_bytes >> 4;
    int64_t src[kWholeInFlight];   // byte offset of the piece's source in x, or one of the three marks
#pragma unroll
    for (int k = 0; k < kWholeInFlight; ++k) {
        const int64_t i = first + k * kThreads;
        if (i >= pieces) {
            src[k] = kPast;
            continue;
        }
        const uint32_t u = static_cast<uint32_t>(i) << (4 - q.unit_log2);
        const uint32_t plane = fdiv(u, q.d_upp);
        const Place p = place_plane(q, w, plane);
        const int64_t from = source_plane(q, p);
        src[k] = inner_shift(q, p) ? kSlow : (from < 0 ? kFill : from + (static_cast<int64_t>(u - plane * q.upp) << q.unit_log2));
    }
    shiftnd_u4 v[kWholeInFlight];
#pragma unroll
    for (int k = 0; k < kWholeInFlight; ++k) {
        v[k] = shiftnd_u4(q.fill);
        if (src[k] >= 0) v[k] = __builtin_nontemporal_load(reinterpret_cast<const shiftnd_u4 *>(x + src[k]));   // (a filled plane issues no load)
    }
    uint32_t slow = 0;   // (one copy of the slow path in the code, and no dynamically indexed array)
#pragma unroll
    for (int k = 0; k < kWholeInFlight; ++k) {
        if (src[k] == kSlow) slow |= 1u << k;
        else if (src[k] != kPast) __builtin_nontemporal_store(v[k], reinterpret_cast<shiftnd_u4 *>(out + (first + k * kThreads) * 16));
    }
#pragma unroll 1
    for (int k = 0; k < kWholeInFlight; ++k)
        if (slow >> k & 1) slow_units(q, x, w, out, (first + k * kThreads) * 16);
}

__device__ __forceinline__ uint32_t pick4(uint32_t i, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3) {
    return i == 0 ? a0 : (i == 1 ? a1 : (i == 2 ? a2 : a3));
}

// the 16 bytes from byte `at` (0..15) of the 32 bytes lo, hi
__device__ __forceinline__ shiftnd_u4 funnel(shiftnd_u4 lo, shiftnd_u4 hi, uint32_t at) {
    const uint32_t i = at >> 2, r = at & 3;
    const uint32_t e0 = pick4(i, lo.x, lo.y, lo.z, lo.w), e1 = pick4(i, lo.y, lo.z, lo.w, hi.x), e2 = pick4(i, lo.z, lo.w, hi.x, hi.y),
                   e3 = pick4(i, lo.w, hi.x, hi.y, hi.z), e4 = pick4(i, hi.x, hi.y, hi.z, hi.w);
    shiftnd_u4 v;
    v.x = __builtin_amdgcn_alignbyte(e1, e0, r);
    v.y = __builtin_amdgcn_alignbyte(e2, e1, r);
    v.z = __builtin_amdgcn_alignbyte(e3, e2, r);
    v.w = __builtin_amdgcn_alignbyte(e4, e3, r);
    return v;
}

// any plane size, element-aligned bases
__device__ __forceinline__ void ragged_pieces_body(const SegmentParams &q, const char *__restrict__ x, const void *__restrict__ w,
                                                   char *__restrict__ out) {
    const int64_t lead = static_cast<int64_t>(reinterpret_cast<uintptr_t>(out) & 15);   // bytes of the first aligned piece before the tensor
    const int64_t pieces = (lead + q.total_bytes + 15) >> 4;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * (kThreads * kRaggedInFlight) + threadIdx.x;
    // a piece = bytes [0, cut) of plane A + bytes [cut, 16) of the next plane B.  fromA / fromB: the ADDRESS output byte 0 of the piece
    // would be read from if the part's plane went on in both directions.  0: the part is filled, or absent -- no load is issued, and
    // the pieces, which start out as the fill pattern, funnel at offset 0 to the pattern itself
    uintptr_t fromA[kRaggedInFlight], fromB[kRaggedInFlight];
    int cut[kRaggedInFlight];
    int kind[kRaggedInFlight];   // 0, kSlow or kPast
#pragma unroll
    for (int k = 0; k < kRaggedInFlight; ++k) {
        const int64_t i = first + k * kThreads;
        const int64_t sb = i * 16 - lead;   // stream byte of the piece's byte 0
        fromA[k] = fromB[k] = 0;
        cut[k] = 16;
        kind[k] = static_cast<int>(i >= pieces ? kPast : ((sb < 0 || sb + 16 > q.total_bytes) ? kSlow : 0));
        if (kind[k] != 0) continue;
        const uint32_t u = static_cast<uint32_t>(sb >> q.unit_log2);
        const uint32_t plane = fdiv(u, q.d_upp);
        const int64_t at = static_cast<int64_t>(u - plane * q.upp) << q.unit_log2;   // byte in plane A (any byte, for 1-byte elements)
        const int64_t left = q.plane_bytes - at;
        const bool two = left < 16;
        cut[k] = two ? static_cast<int>(left) : 16;
        // (pb is used only where `two`, but looked up by every lane: with planes of 98 or 392 bytes every wave holds a piece that
        // straddles, and a branch around the look-up measured 2 - 3 % slower on those planes)
        const Place pa = place_plane(q, w, plane), pb = place_plane(q, w, plane + 1);
        if ((two && 16 - left > q.plane_bytes) || inner_shift(q, pa) || (two && inner_shift(q, pb))) {
            kind[k] = static_cast<int>(kSlow);
            continue;
        }
        const int64_t sa = source_plane(q, pa), sb2 = source_plane(q, pb);
        if (sa >= 0) fromA[k] = reinterpret_cast<uintptr_t>(x) + sa + at;
        if (two && sb2 >= 0) fromB[k] = reinterpret_cast<uintptr_t>(x) + sb2 - left;
    }
    // the aligned pieces of x that hold needed bytes: A needs [fromA, fromA + cut), B needs [fromB + cut, fromB + 16)
    shiftnd_u4 a0[kRaggedInFlight], a1[kRaggedInFlight], b0[kRaggedInFlight], b1[kRaggedInFlight];
#pragma unroll
    for (int k = 0; k < kRaggedInFlight; ++k) {
        a0[k] = a1[k] = b0[k] = b1[k] = shiftnd_u4(q.fill);
        const uintptr_t pa = fromA[k] & ~static_cast<uintptr_t>(15), pb = fromB[k] & ~static_cast<uintptr_t>(15);
        const int offa = static_cast<int>(fromA[k] & 15), offb = static_cast<int>(fromB[k] & 15);
        if (fromA[k]) a0[k] = __builtin_nontemporal_load(reinterpret_cast<const shiftnd_u4 *>(pa));
        if (fromA[k] && offa + cut[k] > 16) a1[k] = __builtin_nontemporal_load(reinterpret_cast<const shiftnd_u4 *>(pa + 16));
        if (fromB[k] && offb + cut[k] < 16) b0[k] = __builtin_nontemporal_load(reinterpret_cast<const shiftnd_u4 *>(pb));
        if (fromB[k] && offb != 0) b1[k] = __builtin_nontemporal_load(reinterpret_cast<const shiftnd_u4 *>(pb + 16));
    }
    uint32_t slow = 0;
#pragma unroll
    for (int k = 0; k < kRaggedInFlight; ++k) {
        const int64_t i = first + k * kThreads;
        if (kind[k] == kSlow) slow |= 1u << k;
        if (kind[k] != 0) continue;
        const shiftnd_u4 va = funnel(a0[k], a1[k], static_cast<uint32_t>(fromA[k] & 15));
        const shiftnd_u4 vb = funnel(b0[k], b1[k], static_cast<uint32_t>(fromB[k] & 15));
        const uint32_t m0 = low_bytes(cut[k]), m1 = low_bytes(cut[k] - 4), m2 = low_bytes(cut[k] - 8), m3 = low_bytes(cut[k] - 12);
        shiftnd_u4 v;
        v.x = (va.x & m0) | (vb.x & ~m0);
        v.y = (va.y & m1) | (vb.y & ~m1);
        v.z = (va.z & m2) | (vb.z & ~m2);
        v.w = (va.w & m3) | (vb.w & ~m3);
        __builtin_nontemporal_store(v, reinterpret_cast<shiftnd_u4 *>(out + (i * 16 - lead)));
    }
#pragma unroll 1
    for (int k = 0; k < kRaggedInFlight; ++k)
        if (slow >> k & 1) slow_units(q, x, w, out, (first + k * kThreads) * 16 - lead);
}

// ONE kernel for both forms (`ragged` is launch-uniform: a scalar branch), because the library's kernel budget has room for one
// (DESIGN 3.27); shiftnd_last_kernel() names the form that ran, segment_forward or segment_forward_ragged.
__global__ __launch_bounds__(kThreads) void segment_forward(SegmentParams q, const char *__restrict__ x, const void *__restrict__ w,
                                                           char *__restrict__ out, int ragged) {
    if (ragged) ragged_pieces_body(q, x, w, out);
    else whole_pieces_body(q, x, w, out);
}

bool whole_pieces(const Geometry &g, int dtype, const void *x, const void *out) {
    const int64_t plane_bytes = frame_pixels(g) * dtype_size(dtype);
    return plane_bytes % 16 == 0 && aligned_to(x, 16) && aligned_to(out, 16);
}

}  // namespace

// float tensors, and the int_repr of quantized ones (I8, U8, I32: the caller passes their fill pattern and an integer table)
bool segment_forward_eligible(const Geometry &g, int dtype, const void *x, const void *out) {
    if (g.active || dtype < SHIFTND_F32 || dtype > SHIFTND_I32 || cropped(g) || g.nd < 2) return false;
    const int64_t T = g.S[3 - g.nd], es = dtype_size(dtype);
    // (C > 1 and T > 1 from here on, so dense_segment_major checks the channel and the segment stride whatever they are)
    if (g.C <= 1 || T <= 1 || !dense_segment_major(g, g.xs) || !dense_segment_major(g, g.os)) return false;
    if (!aligned_to(x, es) || !aligned_to(out, es)) return false;
    return segment_counts_fit(g, es);   // (a tensor beyond them keeps the strided kernel)
}

int segment_forward(const Geometry &g, int dtype, const void *x, const void *w, int wkind, int64_t wzp, uint64_t fill_bits, void *out,
                    hipStream_t st) {
    const bool whole = whole_pieces(g, dtype, x, out);
    const int es = dtype_size(dtype);
    SegmentParams q;
    q.nd = g.nd;
    q.pad = g.pad;
    q.wkind = wkind;
    q.wzp = wzp;
    q.es_log2 = es_log2(es);
    q.unit_log2 = es == 1 ? 0 : 1;
    q.fill = fill_dword(es, fill_bits);
    q.T = static_cast<uint32_t>(g.S[3 - g.nd]);
    q.C = static_cast<uint32_t>(g.C);
    q.A = g.nd == 3 ? g.S[1] : 1;
    q.B = g.S[2];
    q.plane_bytes = q.A * q.B * es;
    q.upp = static_cast<uint32_t>(q.plane_bytes >> q.unit_log2);
    q.total_bytes = g.N * q.T * q.C * q.plane_bytes;
    q.d_upp = make_fastdiv(q.upp);
    q.d_C = make_fastdiv(q.C);
    q.d_T = make_fastdiv(q.T);
    q.d_per = make_fastdiv(static_cast<uint32_t>(map_period(static_cast<int>(q.T), g.pad)));
    const char *xb = static_cast<const char *>(x);
    char *ob = static_cast<char *>(out);
    const dim3 block(kThreads);
    note_kernel(whole ? "segment_forward" : "segment_forward_ragged");
    void (*const kernel)(SegmentParams, const char *, const void *, char *, int) = segment_forward;   // (the kernel, not this function)
    // pieces per workgroup and in all; a ragged tensor can start up to 15 bytes into its first aligned piece
    const int64_t per = kThreads * (whole ? kWholeInFlight : kRaggedInFlight), pieces = whole ? q.total_bytes / 16 : (q.total_bytes + 30) / 16;
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>((pieces + per - 1) / per)), block, 0, st, q, xb, w, ob, whole ? 0 : 1);
    return SHIFTND_OK;
}

}  // namespace shiftnd
