// shiftnd_frames.hip -- the temporal shift of channels-last tensors: memory order N, S0, S1, S2, C (gfx950).
//
// A channels-last video tensor [N*T, C, H, W] lies in the order n, t, pixel, channel.  Seen as the shift problem [N, C, T, H*W] its
// strides are {T*M*C, 1, M*C, C}: the shifted dim lies outside the pixels, the channels are the fastest dim.  A shift along T (the
// Temporal Shift Module, arXiv 1811.08383) then moves every piece of a pixel's channel row from the SAME piece of the SAME pixel of
// another frame of the clip, or fills it: no halo, no LDS, no transposition, and of the element type only its size and its fill
// pattern (all-zero bits for floats; the zero point of a quantized tensor, one byte splatted or an int32 -- a dword pattern).
//
// The call is explicit (SHIFTND_SHIFT_DIM0: `w` is a [C] table and acts on spatial dim 0 only), because strides alone cannot tell
// this problem from a genuine 2-D shift of an NHWC tensor, which belongs to cl_tiled_forward.
//
// One kernel.  A workgroup works inside ONE frame (n, t), so a thread keeps its channel piece k of the rows for its whole life: it
// reads the piece's table entries once, maps them to source frames with fold_index(t - canon_shift(s)) (the map of
// shiftnd_segment.hip, no division) and decides once whether they agree.  Then it walks the frame's pixels:
//   uniform piece  one nontemporal load from the source frame (none for a fill), one nontemporal store, the row offset advanced by
//                  an add; kInFlight pieces per thread with every load issued before the first store
//   mixed piece    (channels of one piece with different source frames: a random table, or a run boundary of the TSM table inside
//                  a piece) element by element: the same piece of each element's own source frame, the previous element's piece
//                  reused while the source frame repeats.  Exact, not fast.
// A workgroup covers max(1, 256 / P) whole rows per step (P pieces per row), so its lanes walk memory in order; rows of more than
// 256 pieces loop inside the row.
//
// The piece is the widest power-of-two unit, at most 16 bytes, that divides the row's bytes and both base addresses (never below the
// element size: rows are whole elements and bases are element-aligned).  shiftnd_last_kernel() names the form:
//   frames_forward          16-byte pieces (rows of whole 16-byte pieces, 16-byte-aligned bases)
//   frames_forward_ragged   8-, 4-, 2- or 1-byte pieces: the same structure
// Every access is naturally aligned and lies inside the bytes the tensors occupy; the table is read at entries [0, C) only.
// A per-clip table (SHIFTND_CLIP_FRAMES: [N, C], one row per clip) is a launch-uniform row stride, FramesParams::wrow: a workgroup lies
// inside one frame of one clip n, so it forms its row's base once and reads entries [n * C, (n + 1) * C) of the table.
// The input gradient of the op is this kernel on the gradient under the negated table.
#include <algorithm>

#include "shiftnd_temporal.hpp"

namespace shiftnd {
namespace {

// Measured on the five lines of tools/temporal_cl_bench.py (profiles/temporal_cl_variants.txt: one process per build, one box): 8
// pieces in flight beat 4 by 1 - 9 % and 2 by 3 - 20 %; at 4 in flight, workgroups of at most 16 steps with a grid of 6144 wanted beat
// at most 8 / 12288 wanted (14 x 14 and 7 x 7: 0.057 - 0.059 ms against 0.071 - 0.074) and at most 32 / 4096 (56 x 56 fp32: 0.146 -
// 0.148 against 0.154); 3072 wanted was 8 % faster on the two small lines and level elsewhere (not re-measured at 8 in flight).
constexpr int kInFlight = 8;               // pieces per thread, every load issued before the first store
constexpr int kMinRowGroups = kInFlight;   // a workgroup takes at least this many steps of rows (one batch) ...
constexpr int kMaxRowGroups = 16;          // ... and at most this many: the pieces one thread moves
constexpr int kWantWorkgroups = 6144;      // frames are cut into more workgroups until the grid has this many (24 per CU)

struct FramesParams {
    int pad, wkind, es_log2, unit_log2;   // element bytes and piece bytes as powers of two
    uint32_t T, P, span, rps;             // frames per clip, pieces per row, min(P, 256), rows per step = max(1, 256 / P)
    uint32_t chunks, rows_per_wg;         // workgroups per frame, rows (a multiple of rps * kInFlight) of each
    uint32_t wrow;                        // shift of (n, c): entry n * wrow + c -- 0 for a [C] table, C for a per-clip [N, C] one
    FastDiv d_chunks, d_T, d_span, d_per; // d_per: by map_period(T, pad)
    int64_t M, R, frame_bytes;            // pixels per frame, bytes per row, bytes per frame
    int64_t wzp;                          // zero point of an integer table
    uint32_t fill;                        // what a filled element holds, as a dword pattern (0 for floats)
};

// a piece of 1 << UL bytes in the low bytes of four dwords
template <int UL> __device__ __forceinline__ shiftnd_u4 load_piece(const char *p) {
    typedef typename piece_of<UL>::type piece_t;
    const piece_t v = __builtin_nontemporal_load(reinterpret_cast<const piece_t *>(p));
    shiftnd_u4 r = shiftnd_u4(0u);
    if constexpr (UL == 4) r = v;
    else if constexpr (UL == 3) { r.x = v.x; r.y = v.y; }
    else r.x = static_cast<uint32_t>(v);
    return r;
}
template <int UL> __device__ __forceinline__ void store_piece(char *p, shiftnd_u4 v) {
    typedef typename piece_of<UL>::type piece_t;
    piece_t s;
    if constexpr (UL == 4) s = v;
    else if constexpr (UL == 3) { s.x = v.x; s.y = v.y; }
    else s = static_cast<piece_t>(v.x);
    __builtin_nontemporal_store(s, reinterpret_cast<piece_t *>(p));
}

// do table entries [e0, e0 + n) (1 <= n <= 16) hold the same bits?  Unconditional loads inside the table, issued together
// (shiftnd_temporal.hpp has raw_equal_fixed for the in-place and online kernels on purpose: a compile-time count and exactly that many loads, against 15 clamped ones here)
template <typename R> __device__ __forceinline__ bool raw_equal(const void *w, int64_t e0, int n) {
    const R *p = static_cast<const R *>(w) + e0;
    const R first = p[0];
    bool same = true;
#pragma unroll
    for (int e = 1; e < 16; ++e) same = same && p[e < n ? e : 0] == first;
    return same;
}
__device__ __forceinline__ bool raw_entries_equal(const void *w, int wkind, int64_t e0, int n) {
    switch (wkind) {
    case SHIFTND_F64: return raw_equal<uint64_t>(w, e0, n);
    case SHIFTND_F32: case SHIFTND_I32: return raw_equal<uint32_t>(w, e0, n);
    case SHIFTND_F16: case SHIFTND_BF16: return raw_equal<uint16_t>(w, e0, n);
    default: return raw_equal<uint8_t>(w, e0, n);
    }
}

// source frame of channel c in frame t, or -1 (fill)
__device__ __forceinline__ int source_frame(const FramesParams &q, const void *w, int64_t c, int t) {
    const int T = static_cast<int>(q.T);
    return fold_index(t - canon_shift(gather_shift(w, q.wkind, q.wzp, c), T, q.pad, q.d_per), T, q.pad);
}

template <int UL>
__device__ __forceinline__ void frames_body(const FramesParams &q, const char *__restrict__ x, const void *__restrict__ table,
                                            char *__restrict__ out) {
    constexpr int kUnit = 1 << UL;
    const uint32_t frame = fdiv(blockIdx.x, q.d_chunks);   // n * T + t
    const uint32_t chunk = blockIdx.x - frame * q.chunks;
    const uint32_t n = fdiv(frame, q.d_T);
    const int t = static_cast<int>(frame - n * q.T);
    const void *const w = table_row(table, q.wkind, n, q.wrow);   // the clip's row of the table: once per workgroup, scalar
    const uint32_t rl = fdiv(threadIdx.x, q.d_span);       // the thread's row of a step, its piece of the row
    const uint32_t k0 = threadIdx.x - rl * q.span;
    if (rl >= q.rps) return;                               // (idle tail lanes where P does not divide 256)
    const int64_t first_row = static_cast<int64_t>(chunk) * q.rows_per_wg;
    const int rows = static_cast<int>(first_row + q.rows_per_wg < q.M ? q.rows_per_wg : q.M - first_row);   // of this workgroup
    const int rps = static_cast<int>(q.rps);
    const int64_t here = static_cast<int64_t>(frame) * q.frame_bytes + first_row * q.R;   // the workgroup's rows in both tensors
    const int64_t clip = static_cast<int64_t>(n) * q.T * q.frame_bytes + first_row * q.R;   // the same rows of the clip's frame 0
    const int64_t step = static_cast<int64_t>(q.rps) * q.R;
    const int epp = 1 << (UL - q.es_log2);                 // elements per piece
    const shiftnd_u4 fillv = shiftnd_u4(q.fill);
#pragma unroll 1
    for (uint32_t k = k0; k < q.P; k += kThreads) {        // (once unless a row has more than 256 pieces)
        const int64_t e0 = static_cast<int64_t>(k) * epp;
        // the piece's table entries, once: do its elements share one source frame?  The everyday case -- the TSM table is constant
        // over runs of channels -- shows on the raw entries (equal bits: one frame map for the piece); entries that differ are
        // mapped one by one, because different shifts can still meet in one source frame
        bool uniform = raw_entries_equal(w, q.wkind, e0, epp);
        const int ts0 = source_frame(q, w, e0, t);
        if (!uniform) {
            uniform = true;
#pragma unroll 1
            for (int e = 1; e < epp; ++e) uniform = uniform && source_frame(q, w, e0 + e, t) == ts0;
        }
        const int64_t column = static_cast<int64_t>(k) * kUnit;
        if (uniform) {
            const char *src = x + clip + (ts0 < 0 ? 0 : ts0) * q.frame_bytes + column;
            char *dst = out + here + column;
            int64_t off = static_cast<int64_t>(rl) * q.R;
#pragma unroll 1
            for (int r = static_cast<int>(rl); r < rows; r += rps * kInFlight) {
                shiftnd_u4 v[kInFlight];
#pragma unroll
                for (int j = 0; j < kInFlight; ++j) {
                    v[j] = fillv;
                    if (ts0 >= 0 && r + j * rps < rows) v[j] = load_piece<UL>(src + off + j * step);   // (a fill issues no load)
                }
#pragma unroll
                for (int j = 0; j < kInFlight; ++j)
                    if (r + j * rps < rows) store_piece<UL>(dst + off + j * step, v[j]);
                off += kInFlight * step;
            }
        } else {
#pragma unroll 1
            for (int r = static_cast<int>(rl); r < rows; r += rps) {
                const int64_t off = r * q.R + column;
                shiftnd_u4 acc = fillv, from = fillv;
                int held = -1;   // the source frame `from` was loaded from (-1: the fill)
#pragma unroll 1
                for (int e = 0; e < epp; ++e) {
                    const int ts = source_frame(q, w, e0 + e, t);
                    if (ts != held) {
                        from = fillv;
                        if (ts >= 0) from = load_piece<UL>(x + clip + ts * q.frame_bytes + off);
                        held = ts;
                    }
                    // the element's bytes [b, b + es) of the piece
                    const int b = e << q.es_log2, es = 1 << q.es_log2;
                    const uint32_t k0m = low_bytes(b + es) & ~low_bytes(b), k1m = low_bytes(b + es - 4) & ~low_bytes(b - 4),
                                   k2m = low_bytes(b + es - 8) & ~low_bytes(b - 8), k3m = low_bytes(b + es - 12) & ~low_bytes(b - 12);
                    acc.x = (acc.x & ~k0m) | (from.x & k0m);
                    acc.y = (acc.y & ~k1m) | (from.y & k1m);
                    acc.z = (acc.z & ~k2m) | (from.z & k2m);
                    acc.w = (acc.w & ~k3m) | (from.w & k3m);
                }
                store_piece<UL>(out + here + off, acc);
            }
        }
    }
}

// ONE kernel for every piece size (q.unit_log2 is launch-uniform: a scalar branch), because the library's kernel budget has room
// for one; shiftnd_last_kernel() names the form that ran, frames_forward or frames_forward_ragged.
__global__ __launch_bounds__(kThreads) void frames_forward(FramesParams q, const char *__restrict__ x, const void *__restrict__ w,
                                                          char *__restrict__ out) {
    switch (q.unit_log2) {
    case 4: frames_body<4>(q, x, w, out); break;
    case 3: frames_body<3>(q, x, w, out); break;
    case 2: frames_body<2>(q, x, w, out); break;
    case 1: frames_body<1>(q, x, w, out); break;
    default: frames_body<0>(q, x, w, out); break;
    }
}

}  // namespace

// The sizes the kernel's index arithmetic needs (include/shiftnd_hip.h states them): 32-bit frame and workgroup indices through
// FastDiv (below 2^31), the 32-bit padding map (periods of 2 T), 64-bit byte offsets below 2^46.
bool frames_geometry_ok(const Geometry &g, int dtype) {
    if (dtype < SHIFTND_F32 || dtype > SHIFTND_I32 || g.nd < 2 || cropped(g) || g.active) return false;
    const int64_t T = g.S[3 - g.nd], M = frame_pixels(g), es = dtype_size(dtype);
    const int64_t limit = 1LL << 31, bytes = 1LL << 46;
    if (T >= (1LL << 30) || M >= limit || g.N >= limit || g.C >= limit || g.N * T >= limit) return false;
    if (g.N == 0 || g.C == 0 || T == 0 || M == 0) return true;
    if (g.N * T * ((M + kMinRowGroups - 1) / kMinRowGroups) >= limit) return false;   // workgroups: a workgroup takes at least kMinRowGroups rows
    const int64_t row_bytes = g.C * es;                                        // (below 2^34)
    return M <= bytes / row_bytes && g.N * T <= bytes / (M * row_bytes);
}

// dense strides of memory order N, S0, S1, S2, C (a dim of size 1 has no stride to check) at an element-aligned base
bool frames_tensor_ok(const Geometry &g, int dtype, const void *p, const int64_t *st) {
    const int lead = 3 - g.nd;
    const int64_t A = g.nd == 3 ? g.S[1] : 1, B = g.S[2], T = g.S[lead];
    if (!aligned_to(p, dtype_size(dtype))) return false;
    if (g.C > 1 && st[1] != 1) return false;
    if (B > 1 && st[4] != g.C) return false;
    if (A > 1 && st[3] != B * g.C) return false;
    if (T > 1 && st[2 + lead] != A * B * g.C) return false;
    return g.N == 1 || st[0] == T * A * B * g.C;
}

int frames_forward(const Geometry &g, int dtype, const void *x, const void *w, int wkind, int64_t wzp, uint64_t fill_bits, bool per_clip,
                   void *out, hipStream_t st) {
    const int es = dtype_size(dtype);
    FramesParams q;
    q.pad = g.pad;
    q.wkind = wkind;
    q.wzp = wzp;
    q.wrow = per_clip ? static_cast<uint32_t>(g.C) : 0;
    q.es_log2 = es_log2(es);
    q.fill = fill_dword(es, fill_bits);
    q.T = static_cast<uint32_t>(g.S[3 - g.nd]);
    q.M = frame_pixels(g);
    q.R = g.C * es;
    q.frame_bytes = q.M * q.R;
    q.unit_log2 = __builtin_ctz(piece_bytes(q.R, {x, out}));
    q.P = static_cast<uint32_t>(q.R >> q.unit_log2);
    q.span = q.P < static_cast<uint32_t>(kThreads) ? q.P : static_cast<uint32_t>(kThreads);
    q.rps = static_cast<uint32_t>(kThreads) / q.span;
    // workgroups per frame: as few as kMaxRowGroups steps per workgroup allow, more while the grid is short of kWantWorkgroups (and a
    // workgroup keeps kMinRowGroups steps); the frame's rows are then split evenly
    const int64_t frames = g.N * q.T, step_rows = q.rps;
    const int64_t fewest = (q.M + step_rows * kMaxRowGroups - 1) / (step_rows * kMaxRowGroups);
    const int64_t most = (q.M + step_rows * kMinRowGroups - 1) / (step_rows * kMinRowGroups);
    const int64_t wanted = (kWantWorkgroups + frames - 1) / frames;
    const int64_t chunks = std::max(fewest, std::min(most, wanted));
    const int64_t batch_rows = step_rows * kInFlight;   // (whole batches: no workgroup ends in a batch of mostly idle loads but a frame's last)
    q.rows_per_wg = static_cast<uint32_t>(((q.M + chunks - 1) / chunks + batch_rows - 1) / batch_rows * batch_rows);
    q.chunks = static_cast<uint32_t>((q.M + q.rows_per_wg - 1) / q.rows_per_wg);
    q.d_chunks = make_fastdiv(q.chunks);
    q.d_T = make_fastdiv(q.T);
    q.d_span = make_fastdiv(q.span);
    q.d_per = make_fastdiv(static_cast<uint32_t>(map_period(static_cast<int>(q.T), g.pad)));
    note_kernel(q.unit_log2 == 4 ? "frames_forward" : "frames_forward_ragged");
    void (*const kernel)(FramesParams, const char *, const void *, char *) = frames_forward;   // (the kernel, not this function)
    const int64_t blocks = g.N * q.T * q.chunks;   // (below 2^31: frames_geometry_ok)
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, st, q, static_cast<const char *>(x), w,
                       static_cast<char *>(out));
    return SHIFTND_OK;
}

}  // namespace shiftnd
