// shiftnd_gradx.hip -- the input gradient of the sparse shift WITHOUT the saved input (gfx950): shiftnd_backward's
// x == NULL && grad_w == NULL form, behind the fixed (grouped) shifts and frozen sparse-shift layers.
//
//   grad_x[n,c,i,j,k] = inside the window ? grad_out[n,c, pad(i-l_i+s_i), pad(j-l_j+s_j), pad(k-l_k+s_k)] : 0,   s = rint(w)
// (kernels/shifts_kernels.h, the `else` branch at the end of shift_backward_kernel_nchwd: a pure gather of grad_out).
//
// Five kernels, templated on the element width only (fp16 and bf16 are the same two bytes to a gather); padding mode, number of
// dims and every size are run-time arguments:
//   gradx_negate       out = -w, [C, nd] elements: a window that is the whole input is the sparse FORWARD of grad_out under -w
//                      (rint is odd-symmetric), so shiftnd_api.hip runs the forward routes on this table
//   gradx_embed<2|4|8> cut windows, contiguous tensors, grad_x rows of whole 16-byte pieces: one 16-byte piece of grad_x per thread
//                      and step, stored once, non-temporal.  A piece whose E source elements are consecutive inside one grad_out
//                      row (every piece but the few at the row ends) is read as the two ALIGNED 16-byte pieces around its source
//                      bytes and funnelled (v_alignbit); rows and columns outside the window are zeros from registers.
//   gradx_gather       everything else (strided tensors, channels-last with a cut, ragged grad_x rows): one element per thread.
//
// gradx_embed's row-end pieces: under zeros padding the same funnel under an element mask (a column outside the window and a
// source column outside the row are both zero); under the other paddings the row ends fold: E independent element loads.
//
// Reads of grad_out stay inside it by construction, not by masking: a funnelled piece needs source bytes [B, B + 16) of the tensor;
// its first aligned piece [B0, B0 + 16), B0 = B - B % 16, is issued only for 0 <= B0 and B0 + 16 <= bytes(grad_out) (the base is
// 16-byte aligned, an eligibility condition); the second, [B0 + 16, B0 + 32), only when B % 16 != 0 (else it is not needed) AND it
// ends at or before the tensor's last byte.  The handful of pieces at the two ends of grad_out that fail a test take the element
// path, which loads exactly elements of the row it stores.  Offsets are 64-bit byte offsets from the tensor base: no descriptor, no
// soffset, nothing a range check would have to see.
//
// With a run-time pool (shiftnd_backward_pooled's x == NULL && grad_w == NULL form; routed as gradx_embed_pool / gradx_gather_pool)
// the same two kernels gather from grad_pooled and divide by the window's count:
//   grad_x[n,c,i,j,k] = inside the window ? gp[n,c, t_i / K_i, t_j / K_j, t_k / K_k] / cnt : 0,   t_d = pad(o_d + s_d),
//   cnt = prod_d min(K_d, O_d - (t_d / K_d) * K_d)   (ceil_mode: the last window of a dim may be partial)
// in the compute type (div_count), rounded once to the tensor type.  `pooled` is a kernel argument: without a pool every wave takes
// the code above.  Pooled sources of neighbouring columns repeat and fold at row ends, so every pooled piece is E element loads at
// indices computed inside the pooled row (a fill reads the row's first element and is dropped by a select); a cut window and the
// whole-input window are the same code.
#include <algorithm>

#include "shiftnd_common.hpp"
#include "shiftnd_launch.hpp"

namespace shiftnd {
namespace {

// ---- -w ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gradx_negate(const void *__restrict__ w, void *__restrict__ out, int count, int es) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    // IEEE negation = the sign bit flipped, whatever the float format
    if (es == 2) static_cast<uint16_t *>(out)[i] = static_cast<const uint16_t *>(w)[i] ^ 0x8000u;
    else if (es == 4) static_cast<uint32_t *>(out)[i] = static_cast<const uint32_t *>(w)[i] ^ 0x80000000u;
    else static_cast<uint64_t *>(out)[i] = static_cast<const uint64_t *>(w)[i] ^ 0x8000000000000000ull;
}

// ---- cut windows, whole-piece rows --------------------------------------------------------------------------------
struct EmbedParams {
    const void *go;
    void *gx;
    const void *w;
    int wkind, nd, pad;
    int S0, S1, S2;   // grad_x volume (normalised dims)
    int O0, O1, O2;   // the window (grad_out's volume without a pool)
    int G0, G1, G2;   // the volume of the tensor that is read: the window, or its pooled sizes
    int pooled;       // 0: go is grad_out; 1: go is grad_pooled, window K = stride per dim
    int K0, K1, K2;
    FastDiv d_K0, d_K1, d_K2;
    int L0, L1, L2;   // first plane / row / column of the window
    int wc0, wc1, wc2;   // weight column of each normalised dim, or -1
    int C;
    int pc;              // 16-byte pieces per grad_x row
    int rows;            // S0 * S1 rows per (n, c) volume
    int rows_per_band, bands;   // a workgroup = one band of rows of one (n, c) volume
    FastDiv d_bands, d_C, d_pc, d_S1, dper0, dper1, dper2;
    int64_t go_bytes;    // bytes of grad_out
};

// the window coordinate o in [0, len) -> source coordinate in [0, len) or -1 (zero fill); cs = canon_shift(-s)
__device__ __forceinline__ int gradx_map(int o, int len, int cs, int pad) { return len == 1 ? 0 : fold_index(o - cs, len, pad); }

// bits of one element / cnt: divided in the compute type (fp32 for the 16-bit types), rounded once.  (A count above INT_MAX
// can only come from gradx_gather: gradx_embed's eligibility keeps counts below 2^31.)
template <typename T> __device__ __forceinline__ typename raw_t<sizeof(typename T::S)>::type pool_div_as(
    typename raw_t<sizeof(typename T::S)>::type bits, int64_t cnt) {
    typename T::S s;
    __builtin_memcpy(&s, &bits, sizeof(s));
    const typename T::C v = widen<T>(s);
    s = narrow<T>(cnt <= 0x7fffffffLL ? div_count(v, static_cast<int>(cnt)) : v / static_cast<typename T::C>(cnt));
    __builtin_memcpy(&bits, &s, sizeof(s));
    return bits;
}
template <int ES> __device__ __forceinline__ typename raw_t<ES>::type pool_div(typename raw_t<ES>::type bits, int64_t cnt, int dtype) {
    if constexpr (ES == 4) return pool_div_as<f32_t>(bits, cnt);
    else if constexpr (ES == 8) return pool_div_as<f64_t>(bits, cnt);
    else return dtype == SHIFTND_F16 ? pool_div_as<f16_t>(bits, cnt) : pool_div_as<bf16_t>(bits, cnt);
}

template <int ES>
__global__ __launch_bounds__(kThreads) void gradx_embed(const EmbedParams p) {
    constexpr int E = 16 / ES;
    using R = typename raw_t<ES>::type;
    // consecutive block ids go round the 8 XCDs: give each XCD one contiguous range of bands (neighbouring bands share grad_out rows)
    const uint32_t G = gridDim.x, bid = blockIdx.x;
    const uint32_t per = G >> 3, rem = G & 7u, xcd = bid & 7u;
    const uint32_t wid = xcd * per + (xcd < rem ? xcd : rem) + (bid >> 3);
    const uint32_t plane = fdiv(wid, p.d_bands);
    const uint32_t band = wid - plane * static_cast<uint32_t>(p.bands);
    const uint32_t c = plane - fdiv(plane, p.d_C) * static_cast<uint32_t>(p.C);

    const int wcol[3] = {p.wc0, p.wc1, p.wc2};
    int64_t sh[3];
    gather_shifts3(p.w, p.wkind, 0, static_cast<int64_t>(c) * p.nd, wcol, sh);
    const int cs0 = p.wc0 >= 0 ? canon_shift(-sh[0], p.O0, p.pad, p.dper0) : 0;
    const int cs1 = p.wc1 >= 0 ? canon_shift(-sh[1], p.O1, p.pad, p.dper1) : 0;
    const int cs2 = p.wc2 >= 0 ? canon_shift(-sh[2], p.O2, p.pad, p.dper2) : 0;

    const int row0 = static_cast<int>(band) * p.rows_per_band;
    const int nrows = min(p.rows_per_band, p.rows - row0);
    const uint32_t pieces = static_cast<uint32_t>(nrows) * static_cast<uint32_t>(p.pc);
    const int64_t plane_elems = static_cast<int64_t>(p.G0) * p.G1 * p.G2;
    const R *gop = static_cast<const R *>(p.go) + static_cast<int64_t>(plane) * plane_elems;
    const int64_t plane_byte0 = static_cast<int64_t>(plane) * plane_elems * ES;
    shiftnd_u4 *gxp = static_cast<shiftnd_u4 *>(p.gx) + (static_cast<int64_t>(plane) * p.rows + row0) * p.pc;

    if (p.pooled) {
        // a loop of its own (the whole workgroup takes it or none does), so that the loop below is the code it was without a pool
        for (uint32_t q = threadIdx.x; q < pieces; q += kThreads) {
            const uint32_t r = fdiv(q, p.d_pc);
            const int j0 = static_cast<int>(q - r * static_cast<uint32_t>(p.pc)) * E;
            const uint32_t row = static_cast<uint32_t>(row0) + r;
            const uint32_t i0 = fdiv(row, p.d_S1);
            const int o0 = static_cast<int>(i0) - p.L0;
            const int o1 = static_cast<int>(row - i0 * static_cast<uint32_t>(p.S1)) - p.L1;
            const int m0 = (o0 >= 0 && o0 < p.O0) ? gradx_map(o0, p.O0, cs0, p.pad) : -1;
            const int m1 = (o1 >= 0 && o1 < p.O1) ? gradx_map(o1, p.O1, cs1, p.pad) : -1;
            shiftnd_u4 out = {0u, 0u, 0u, 0u};
            if (m0 >= 0 && m1 >= 0) {
                // the pooled row and the count of its windows along the two outer dims, then E elements of that row
                const uint32_t q0 = fdiv(static_cast<uint32_t>(m0), p.d_K0), q1 = fdiv(static_cast<uint32_t>(m1), p.d_K1);
                const int cnt01 = min(p.K0, p.O0 - static_cast<int>(q0) * p.K0) * min(p.K1, p.O1 - static_cast<int>(q1) * p.K1);
                const int64_t rowbase = (static_cast<int64_t>(q0) * p.G1 + q1) * p.G2;
                const int oa = j0 - p.L2;
                int m[E];
                uint32_t q2[E];
                R v[E];
#pragma unroll
                for (int k = 0; k < E; ++k) {
                    const int o = oa + k;
                    m[k] = (o >= 0 && o < p.O2) ? gradx_map(o, p.O2, cs2, p.pad) : -1;
                    q2[k] = fdiv(static_cast<uint32_t>(m[k] >= 0 ? m[k] : 0), p.d_K2);   // in [0, G2)
                }
#pragma unroll
                for (int k = 0; k < E; ++k) v[k] = gop[rowbase + q2[k]];
#pragma unroll
                for (int k = 0; k < E; ++k) {
                    const int64_t cnt = static_cast<int64_t>(cnt01) * min(p.K2, p.O2 - static_cast<int>(q2[k]) * p.K2);
                    v[k] = m[k] >= 0 ? pool_div<ES>(v[k], cnt, p.wkind) : R(0);
                }
                __builtin_memcpy(&out, v, 16);
            }
            __builtin_nontemporal_store(out, gxp + q);
        }
        return;
    }

    for (uint32_t q = threadIdx.x; q < pieces; q += kThreads) {
        const uint32_t r = fdiv(q, p.d_pc);
        const int j0 = static_cast<int>(q - r * static_cast<uint32_t>(p.pc)) * E;   // first column of the piece
        const uint32_t row = static_cast<uint32_t>(row0) + r;
        const uint32_t i0 = fdiv(row, p.d_S1);
        const int o0 = static_cast<int>(i0) - p.L0;
        const int o1 = static_cast<int>(row - i0 * static_cast<uint32_t>(p.S1)) - p.L1;
        const int m0 = (o0 >= 0 && o0 < p.O0) ? gradx_map(o0, p.O0, cs0, p.pad) : -1;
        const int m1 = (o1 >= 0 && o1 < p.O1) ? gradx_map(o1, p.O1, cs1, p.pad) : -1;
        shiftnd_u4 out = {0u, 0u, 0u, 0u};
        if (m0 >= 0 && m1 >= 0) {
            const int64_t rowbase = (static_cast<int64_t>(m0) * p.O1 + m1) * p.O2;   // elements from the volume's first
            const int oa = j0 - p.L2;    // window column of the piece's first element
            const int a = oa - cs2;      // ... and its source column when nothing folds
            const int64_t B = plane_byte0 + (rowbase + a) * ES;   // byte offset of that column from the tensor's first
            const uint32_t mis = static_cast<uint32_t>(B) & 15u;
            const int64_t B0 = B - mis;
            const bool affine = oa >= 0 && oa + E <= p.O2 && a >= 0 && a + E <= p.O2;
            // zeros padding: a column outside the window and a source column outside the row are both zero, so EVERY piece is the
            // funnelled bytes under a mask (whatever in-tensor bytes lie beside the row are read and dropped); the other paddings fold
            // at the row ends, which the element path does
            const bool masked = p.pad == 0 && oa + E > 0 && oa < p.O2 && a + E > 0 && a < p.O2;
            if ((affine || masked) && B0 >= 0 && B0 + 16 <= p.go_bytes && (mis == 0 || B0 + 32 <= p.go_bytes)) {
                const shiftnd_u4 *src = reinterpret_cast<const shiftnd_u4 *>(static_cast<const char *>(p.go) + B0);
                const shiftnd_u4 lo = src[0];
                shiftnd_u4 hi = {0u, 0u, 0u, 0u};
                if (mis != 0) hi = src[1];
                const uint32_t ws = mis >> 2, bits = (mis & 3u) * 8u;   // whole words, then 0 or 16 bits
                const uint32_t W[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                uint32_t X[5];
#pragma unroll
                for (int k = 0; k < 5; ++k) X[k] = ws == 0 ? W[k] : (ws == 1 ? W[k + 1] : (ws == 2 ? W[k + 2] : W[k + 3]));
#pragma unroll
                for (int k = 0; k < 4; ++k) out[k] = ES == 2 ? __builtin_amdgcn_alignbit(X[k + 1], X[k], bits) : X[k];
                if (!affine) {
                    R v[E];
                    __builtin_memcpy(v, &out, 16);
#pragma unroll
                    for (int k = 0; k < E; ++k) v[k] = (oa + k >= 0 && oa + k < p.O2 && a + k >= 0 && a + k < p.O2) ? v[k] : R(0);
                    __builtin_memcpy(&out, v, 16);
                }
            } else {
                // the pieces at the ends of the window's rows (folds, fills, columns outside the window): element by element
                // (every lane loads, a fill from the row's first element and a select: E independent loads, one wait)
                int m[E];
                R v[E];
#pragma unroll
                for (int k = 0; k < E; ++k) {
                    const int o = oa + k;
                    m[k] = (o >= 0 && o < p.O2) ? gradx_map(o, p.O2, cs2, p.pad) : -1;
                }
#pragma unroll
                for (int k = 0; k < E; ++k) v[k] = gop[rowbase + (m[k] >= 0 ? m[k] : 0)];
#pragma unroll
                for (int k = 0; k < E; ++k) v[k] = m[k] >= 0 ? v[k] : R(0);
                __builtin_memcpy(&out, v, 16);
            }
        }
        __builtin_nontemporal_store(out, gxp + q);
    }
}

// ---- everything else: one element per thread, run-time strides and element width ---------------------------------------
__global__ __launch_bounds__(kThreads) void gradx_gather(Geometry g, const void *__restrict__ go, const void *__restrict__ w,
                                                          int wkind, void *__restrict__ gx, int es, int64_t total, int pooled) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    if (pooled) {
        // a loop of its own (the whole grid takes it or none does), so that the loop below is the code it was without a pool
        for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += stride) {
            int64_t r = e;
            const int64_t i2 = r % g.S[2]; r /= g.S[2];
            const int64_t i1 = r % g.S[1]; r /= g.S[1];
            const int64_t i0 = r % g.S[0]; r /= g.S[0];
            const int64_t c = r % g.C;
            const int64_t n = r / g.C;
            int64_t off = n * g.os[0] + c * g.os[1];   // (os are grad_pooled's strides)
            int64_t cnt = 1;                           // elements of the window that holds this one
            bool pass = true;
#pragma unroll 1
            for (int d = 0; d < 3; ++d) {
                const int64_t o = (d == 0 ? i0 : (d == 1 ? i1 : i2)) - g.L[d];
                if (!pass || o < 0 || o >= g.O[d]) {
                    pass = false;
                    continue;
                }
                const int64_t sh = g.wcol[d] >= 0 ? gather_shift(w, wkind, 0, c * g.nd + g.wcol[d]) : 0;
                const int64_t t = g.O[d] == 1 ? 0 : pad_index(o + sh, g.O[d], g.pad);
                if (t < 0) {
                    pass = false;
                    continue;
                }
                const int64_t q = t / g.K[d];   // the pooled coordinate, in [0, P[d])
                const int64_t left = g.O[d] - q * g.K[d];
                cnt *= g.K[d] < left ? g.K[d] : left;
                off += q * g.os[2 + d];
            }
            const int64_t dst = n * g.gs[0] + c * g.gs[1] + i0 * g.gs[2] + i1 * g.gs[3] + i2 * g.gs[4];
            // an index inside grad_pooled whatever `pass` says (a fill reads the tensor's first element), a select afterwards
            off = pass ? off : 0;
            if (es == 2) static_cast<uint16_t *>(gx)[dst] = pass ? pool_div<2>(static_cast<const uint16_t *>(go)[off], cnt, wkind) : uint16_t(0);
            else if (es == 4) static_cast<uint32_t *>(gx)[dst] = pass ? pool_div<4>(static_cast<const uint32_t *>(go)[off], cnt, wkind) : 0u;
            else static_cast<uint64_t *>(gx)[dst] = pass ? pool_div<8>(static_cast<const uint64_t *>(go)[off], cnt, wkind) : 0ull;
        }
        return;
    }
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += stride) {
        int64_t r = e;
        const int64_t i2 = r % g.S[2]; r /= g.S[2];
        const int64_t i1 = r % g.S[1]; r /= g.S[1];
        const int64_t i0 = r % g.S[0]; r /= g.S[0];
        const int64_t c = r % g.C;
        const int64_t n = r / g.C;
        int64_t off = n * g.os[0] + c * g.os[1];
        bool pass = true;
#pragma unroll 1
        for (int d = 0; d < 3; ++d) {   // (one copy of the padding map's 64-bit divisions in the code)
            const int64_t o = (d == 0 ? i0 : (d == 1 ? i1 : i2)) - g.L[d];
            if (!pass || o < 0 || o >= g.O[d]) {
                pass = false;
                continue;
            }
            const int64_t sh = g.wcol[d] >= 0 ? gather_shift(w, wkind, 0, c * g.nd + g.wcol[d]) : 0;
            const int64_t t = g.O[d] == 1 ? 0 : pad_index(o + sh, g.O[d], g.pad);
            if (t < 0) pass = false;
            else off += t * g.os[2 + d];
        }
        const int64_t dst = n * g.gs[0] + c * g.gs[1] + i0 * g.gs[2] + i1 * g.gs[3] + i2 * g.gs[4];
        // a pure copy: the bit pattern travels, zero is all bits clear in every float format
        if (es == 2) static_cast<uint16_t *>(gx)[dst] = pass ? static_cast<const uint16_t *>(go)[off] : uint16_t(0);
        else if (es == 4) static_cast<uint32_t *>(gx)[dst] = pass ? static_cast<const uint32_t *>(go)[off] : 0u;
        else static_cast<uint64_t *>(gx)[dst] = pass ? static_cast<const uint64_t *>(go)[off] : 0ull;
    }
}

// element strides of a dense N, C, d0, d1, inner tensor with these spatial sizes (size-1 dims may carry any stride)
bool dense_strides(const int64_t st[5], int64_t N, int64_t C, const int64_t sz[3]) {
    int64_t expect = 1;
    for (int d = 2; d >= 0; --d) {
        if (sz[d] != 1 && st[2 + d] != expect) return false;
        expect *= sz[d];
    }
    if (C != 1 && st[1] != expect) return false;
    expect *= C;
    return N == 1 || st[0] == expect;
}

}  // namespace

size_t gradx_negate_workspace(const Geometry &g, int dtype) { return static_cast<size_t>(g.C) * g.nd * dtype_size(dtype); }

int gradx_negate_weights(const Geometry &g, int dtype, const void *w, void *out, hipStream_t st) {
    const int64_t count = g.C * g.nd;
    if (count > 0x7fffffffLL) return SHIFTND_ERR_TOO_LARGE;
    const unsigned grid = static_cast<unsigned>((count + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(gradx_negate, dim3(grid), dim3(kThreads), 0, st, w, out, static_cast<int>(count), dtype_size(dtype));
    return SHIFTND_OK;
}

// pieces a workgroup handles: 8 per thread (32 KiB of grad_x), rounded to whole rows
constexpr int kEmbedPieces = 8 * kThreads;

// a pool in the geometry: K is 0 when the call has no pool (shiftnd_backward), at least 1 per dim from shiftnd_backward_pooled
static bool gradx_pooled(const Geometry &g) { return g.K[0] > 0; }

bool gradx_embed_eligible(const Geometry &g, int dtype, const void *go, const void *gx) {
    const int es = dtype_size(dtype);
    const bool pooled = gradx_pooled(g);
    if (pooled) {   // 32-bit windows and counts
        int64_t cnt = 1;
        for (int d = 0; d < 3; ++d) {
            if (g.K[d] >= (1LL << 30)) return false;
            cnt *= std::min(std::max<int64_t>(g.K[d], 1), g.O[d]);
            if (cnt >= (1LL << 31)) return false;
        }
    }
    if (es != 2 && es != 4 && es != 8) return false;
    if ((reinterpret_cast<uintptr_t>(go) | reinterpret_cast<uintptr_t>(gx)) & 15u) return false;
    if ((g.S[2] * es) % 16 != 0) return false;   // grad_x rows of whole 16-byte pieces
    if (!dense_strides(g.os, g.N, g.C, pooled ? g.P : g.O) || !dense_strides(g.gs, g.N, g.C, g.S)) return false;
    for (int d = 0; d < 3; ++d)
        if (g.S[d] >= (1LL << 30)) return false;
    const int64_t rows = g.S[0] * g.S[1], pc = g.S[2] * es / 16;
    if (rows >= (1LL << 30) || pc * kEmbedPieces >= (1LL << 31)) return false;
    const int64_t rpb = std::max<int64_t>(1, (kEmbedPieces + pc - 1) / pc);
    const int64_t bands = (rows + rpb - 1) / rpb;
    return g.N * g.C < (1LL << 31) && g.N * g.C * bands < (1LL << 31);
}

int gradx_embed(const Geometry &g, int dtype, const void *go, const void *w, void *gx, hipStream_t st) {
    const int es = dtype_size(dtype);
    EmbedParams p;
    p.go = go;
    p.gx = gx;
    p.w = w;
    p.wkind = dtype;
    p.nd = g.nd;
    p.pad = g.pad;
    p.S0 = static_cast<int>(g.S[0]); p.S1 = static_cast<int>(g.S[1]); p.S2 = static_cast<int>(g.S[2]);
    p.O0 = static_cast<int>(g.O[0]); p.O1 = static_cast<int>(g.O[1]); p.O2 = static_cast<int>(g.O[2]);
    const bool pooled = gradx_pooled(g);
    const int64_t *G = pooled ? g.P : g.O;
    p.G0 = static_cast<int>(G[0]); p.G1 = static_cast<int>(G[1]); p.G2 = static_cast<int>(G[2]);
    p.pooled = pooled ? 1 : 0;
    p.K0 = static_cast<int>(std::max<int64_t>(g.K[0], 1)); p.K1 = static_cast<int>(std::max<int64_t>(g.K[1], 1));
    p.K2 = static_cast<int>(std::max<int64_t>(g.K[2], 1));
    p.d_K0 = make_fastdiv(static_cast<uint32_t>(p.K0));
    p.d_K1 = make_fastdiv(static_cast<uint32_t>(p.K1));
    p.d_K2 = make_fastdiv(static_cast<uint32_t>(p.K2));
    p.L0 = static_cast<int>(g.L[0]); p.L1 = static_cast<int>(g.L[1]); p.L2 = static_cast<int>(g.L[2]);
    p.wc0 = g.wcol[0]; p.wc1 = g.wcol[1]; p.wc2 = g.wcol[2];
    p.C = static_cast<int>(g.C);
    p.pc = static_cast<int>(g.S[2] * es / 16);
    p.rows = static_cast<int>(g.S[0] * g.S[1]);
    const int want = std::max(1, (kEmbedPieces + p.pc - 1) / p.pc);
    p.bands = (p.rows + want - 1) / want;
    p.rows_per_band = (p.rows + p.bands - 1) / p.bands;   // (even bands)
    p.bands = (p.rows + p.rows_per_band - 1) / p.rows_per_band;
    p.d_bands = make_fastdiv(static_cast<uint32_t>(p.bands));
    p.d_C = make_fastdiv(static_cast<uint32_t>(p.C));
    p.d_pc = make_fastdiv(static_cast<uint32_t>(p.pc));
    p.d_S1 = make_fastdiv(static_cast<uint32_t>(p.S1));
    p.dper0 = make_fastdiv(static_cast<uint32_t>(map_period(p.O0, g.pad)));
    p.dper1 = make_fastdiv(static_cast<uint32_t>(map_period(p.O1, g.pad)));
    p.dper2 = make_fastdiv(static_cast<uint32_t>(map_period(p.O2, g.pad)));
    p.go_bytes = g.N * g.C * G[0] * G[1] * G[2] * es;
    const dim3 grid(static_cast<unsigned>(g.N * g.C * p.bands)), block(kThreads);
    note_kernel(pooled ? "gradx_embed_pool" : "gradx_embed");
    switch (es) {
    case 2: hipLaunchKernelGGL((gradx_embed<2>), grid, block, 0, st, p); break;
    case 4: hipLaunchKernelGGL((gradx_embed<4>), grid, block, 0, st, p); break;
    default: hipLaunchKernelGGL((gradx_embed<8>), grid, block, 0, st, p); break;
    }
    return SHIFTND_OK;
}

int gradx_gather(const Geometry &g, int dtype, const void *go, const void *w, void *gx, hipStream_t st) {
    const int64_t total = g.N * g.C * g.S[0] * g.S[1] * g.S[2];
    const int64_t blocks = (total + kThreads - 1) / kThreads;
    const int64_t cap = 256LL * 32;   // 32 workgroups per CU, grid-stride beyond
    const bool pooled = gradx_pooled(g);
    note_kernel(pooled ? "gradx_gather_pool" : "gradx_gather");
    hipLaunchKernelGGL(gradx_gather, dim3(static_cast<unsigned>(blocks < cap ? blocks : cap)), dim3(kThreads), 0, st, g, go, w, dtype,
                       gx, dtype_size(dtype), total, pooled ? 1 : 0);
    return SHIFTND_OK;
}

}  // namespace shiftnd
