// shiftnd_inplace.hip -- the temporal shift IN PLACE: out == x under SHIFTND_SHIFT_DIM0, both dense layouts (gfx950).
//
// A video tensor [N*T, C, ...] is, in either dense layout, clips of T frames of F = C * M * es bytes at frame stride F.  The fixed
// temporal shift (the Temporal Shift Module, arXiv 1811.08383) moves a channel's bytes of frame t from the SAME bytes of frame
// pad(t - s_c) of the same clip, or fills them.  The out-of-place kernels (shiftnd_segment.hip, shiftnd_frames.hip) own a fresh
// output and so copy the unshifted channels too -- three quarters of the tensor under the published table.  This kernel owns the
// tensor itself and touches only what changes.
//
// Ownership.  A thread owns one PIECE: a naturally aligned power-of-two byte range of at most 16 bytes at the same offset in every
// frame of ONE clip.  Pieces are disjoint and a thread reads and writes only bytes of its own piece in its own clip, never a wider
// granule around it.  So no other thread ever touches a byte this thread reads or writes: there is no cross-thread hazard and the
// kernel needs no barrier, LDS, atomic or workspace.  Inside the thread, every load of a line (the piece's bytes of all T frames
// under one shift) is issued before its first store; `x` is ONE pointer and not __restrict__, the accesses are plain C++
// (nontemporal builtins), so the thread's program order alone gives the right values.
//
// A frame is a sequence of RUNS: the C channel planes of M * es bytes (segment-major, memory order N, T, C, pixels; the run is the
// channel) or the M pixel rows of C * es bytes (channels-last, memory order N, T, pixels, C; the channel is the element's place in
// its row).  The piece is the widest power of two, at most 16 bytes, that divides the run's bytes and the base address (never below
// the element size), so no piece straddles two runs.  One thread per (clip, piece of a frame), consecutive lanes on consecutive
// pieces.
//   uniform piece   (every segment-major piece; a channels-last piece whose channels share one shift) one line under
//                   ts = fold_index(t - canon_shift(s)), the map of segment_forward and frames_forward: frames that fill issue no
//                   load, frames with ts == t are skipped, and a line whose shift maps every frame to itself (s == 0, T == 1, a
//                   whole period) touches no tensor byte at all -- the thread exits after reading its table entries.
//   mixed piece     (channels-last, channels of one piece with different shifts) the same line per ELEMENT of the piece, element-
//                   wide accesses.  Exact, not fast.
// The slots of a line are registers indexed by compile-time constants: kMaxFrames = 16 of them (64 data VGPRs for 16-byte pieces),
// slots >= T predicated off; the host route refuses T > 16.
// shiftnd_last_kernel() names the form: frames_inplace (16-byte pieces), frames_inplace_ragged (8-, 4-, 2- or 1-byte pieces).
// Every access is naturally aligned and lies inside the bytes the tensor occupies; the table is read at entries [0, C) only.
#include "shiftnd_temporal.hpp"

namespace shiftnd {
namespace {

constexpr int kMaxFrames = 16;   // register slots of a line: frames per clip served

struct InplaceParams {
    int pad, wkind, es_log2, unit_log2;   // element bytes and piece bytes as powers of two
    int cl;                               // 1: channels-last (runs are pixel rows), 0: segment-major (runs are channel planes)
    int small;                            // pieces per frame below 2^31: the run of a piece by FastDiv
    uint32_t T, chunks, ppr;              // frames per clip, workgroups per clip, pieces per run
    FastDiv d_chunks, d_ppr, d_per;       // d_per: by map_period(T, pad)
    int64_t ppf, frame_bytes;             // pieces per frame, bytes per frame
    int64_t wzp;                          // zero point of an integer table
    uint32_t fill;                        // what a filled element holds, as a dword pattern (0 for floats)
};

// the bytes [p, p + (1 << UL)) of every frame of the clip under the canonical shift `cs`: gather, then store
template <int UL> __device__ __forceinline__ void shift_line(const InplaceParams &q, char *p, int cs) {
    typedef typename piece_of<UL>::type piece_t;
    if (cs == 0) return;   // fold_index(t - 0) == t under every padding: nothing moves
    const int T = static_cast<int>(q.T);
    piece_t v[kMaxFrames];
    uint32_t moved = 0;    // frames whose content changes
#pragma unroll
    for (int t = 0; t < kMaxFrames; ++t) {
        v[t] = (piece_t)(q.fill);   // (a vector type: the dword splatted)
        if (t < T) {
            const int ts = fold_index(t - cs, T, q.pad);
            if (ts != t) {
                moved |= 1u << t;
                if (ts >= 0) v[t] = __builtin_nontemporal_load(reinterpret_cast<const piece_t *>(p + ts * q.frame_bytes));   // (a fill issues no load)
            }
        }
    }
#pragma unroll
    for (int t = 0; t < kMaxFrames; ++t)
        if (moved >> t & 1) __builtin_nontemporal_store(v[t], reinterpret_cast<piece_t *>(p + t * q.frame_bytes));
}

__device__ __forceinline__ int canon_of(const InplaceParams &q, int64_t s) {
    return canon_shift(s, static_cast<int>(q.T), q.pad, q.d_per);
}

template <int UL> __device__ __forceinline__ void inplace_body(const InplaceParams &q, char *x, const void *__restrict__ w) {
    const uint32_t n = fdiv(blockIdx.x, q.d_chunks);   // the clip
    const uint32_t chunk = blockIdx.x - n * q.chunks;
    const int64_t k = static_cast<int64_t>(chunk) * kThreads + threadIdx.x;   // the piece of a frame
    if (k >= q.ppf) return;
    int64_t run;   // the piece's run of the frame, its place in the run
    uint32_t kr;
    if (q.small) {
        const uint32_t r = fdiv(static_cast<uint32_t>(k), q.d_ppr);
        run = r;
        kr = static_cast<uint32_t>(k) - r * q.ppr;
    } else {
        run = k / q.ppr;
        kr = static_cast<uint32_t>(k - run * q.ppr);
    }
    char *p = x + static_cast<int64_t>(n) * q.T * q.frame_bytes + (k << UL);
    if (!q.cl) {   // the run is the channel
        shift_line<UL>(q, p, canon_of(q, gather_shift(w, q.wkind, q.wzp, run)));
        return;
    }
    // channels-last: the piece holds the channels [e0, e0 + epp) of its pixel.  Do they share one shift?  The everyday case -- the
    // TSM table is constant over runs of channels -- shows on the raw entries (equal bits); entries that differ are compared as
    // shifts, because different entries can round to one shift
    const int epp = 1 << (UL - q.es_log2);
    const int64_t e0 = static_cast<int64_t>(kr) * epp;
    const int64_t s0 = gather_shift(w, q.wkind, q.wzp, e0);
    bool uniform = piece_entries_equal<UL>(w, q.wkind, e0, UL - q.es_log2);
    if (!uniform) {
        uniform = true;
#pragma unroll 1
        for (int e = 1; e < epp; ++e) uniform = uniform && gather_shift(w, q.wkind, q.wzp, e0 + e) == s0;
    }
    if (uniform) {
        shift_line<UL>(q, p, canon_of(q, s0));
        return;
    }
    // mixed piece: a line per element (es_log2 < UL here: a piece of one element is uniform)
#pragma unroll 1
    for (int e = 0; e < epp; ++e) {
        const int cs = canon_of(q, gather_shift(w, q.wkind, q.wzp, e0 + e));
        char *pe = p + (e << q.es_log2);
        if constexpr (UL > 3) if (q.es_log2 == 3) shift_line<3>(q, pe, cs);
        if constexpr (UL > 2) if (q.es_log2 == 2) shift_line<2>(q, pe, cs);
        if constexpr (UL > 1) if (q.es_log2 == 1) shift_line<1>(q, pe, cs);
        if constexpr (UL > 0) if (q.es_log2 == 0) shift_line<0>(q, pe, cs);
    }
}

// ONE kernel for every piece size and both layouts (q.unit_log2 and q.cl are launch-uniform: scalar branches), because the library's
// kernel budget has room for one; shiftnd_last_kernel() names the form that ran, frames_inplace or frames_inplace_ragged.
__global__ __launch_bounds__(kThreads) void frames_inplace(InplaceParams q, char *x, const void *__restrict__ w) {
    switch (q.unit_log2) {
    case 4: inplace_body<4>(q, x, w); break;
    case 3: inplace_body<3>(q, x, w); break;
    case 2: inplace_body<2>(q, x, w); break;
    case 1: inplace_body<1>(q, x, w); break;
    default: inplace_body<0>(q, x, w); break;
    }
}

}  // namespace

// The sizes the kernel serves (include/shiftnd_hip.h states them): those of frames_geometry_ok, at most kMaxFrames frames per clip,
// and a grid of one thread per (clip, piece of a frame) below 2^31 workgroups whatever the piece (a piece is at least an element).
bool inplace_geometry_ok(const Geometry &g, int dtype) {
    if (!frames_geometry_ok(g, dtype)) return false;
    const int64_t T = g.S[3 - g.nd], M = frame_pixels(g);
    if (T > kMaxFrames) return false;
    if (g.N == 0 || g.C == 0 || T == 0 || M == 0) return true;
    return g.N * ((g.C * M + kThreads - 1) / kThreads) < (1LL << 31);   // (C * M * es is below 2^46: no overflow)
}

// 1: dense segment-major, 2: dense channels-last, 0: neither.  A tensor both describe (planes or channels of size 1) is segment-major
int inplace_layout(const Geometry &g, int dtype, const void *p, const int64_t *strides) {
    if (tshift_tensor_ok(g, dtype, p, strides)) return 1;
    return frames_tensor_ok(g, dtype, p, strides) ? 2 : 0;
}

int inplace_forward(const Geometry &g, int dtype, int layout, void *x, const void *w, int wkind, int64_t wzp, uint64_t fill_bits,
                    hipStream_t st) {
    const int es = dtype_size(dtype);
    const int64_t M = frame_pixels(g), run_bytes = (layout == 2 ? g.C : M) * es;
    InplaceParams q;
    q.pad = g.pad;
    q.wkind = wkind;
    q.wzp = wzp;
    q.cl = layout == 2 ? 1 : 0;
    q.es_log2 = es_log2(es);
    q.fill = fill_dword(es, fill_bits);
    q.T = static_cast<uint32_t>(g.S[3 - g.nd]);
    q.frame_bytes = g.C * M * es;
    q.unit_log2 = __builtin_ctz(piece_bytes(run_bytes, {x}));
    q.ppf = q.frame_bytes >> q.unit_log2;
    q.ppr = static_cast<uint32_t>(run_bytes >> q.unit_log2);   // (at most max(C, M): below 2^31)
    q.small = q.ppf < (1LL << 31) ? 1 : 0;
    q.chunks = static_cast<uint32_t>((q.ppf + kThreads - 1) / kThreads);
    q.d_chunks = make_fastdiv(q.chunks);
    q.d_ppr = make_fastdiv(q.ppr);
    q.d_per = make_fastdiv(static_cast<uint32_t>(map_period(static_cast<int>(q.T), g.pad)));
    note_kernel(q.unit_log2 == 4 ? "frames_inplace" : "frames_inplace_ragged");
    void (*const kernel)(InplaceParams, char *, const void *) = frames_inplace;
    const int64_t blocks = g.N * q.chunks;   // (below 2^31: inplace_geometry_ok)
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, st, q, static_cast<char *>(x), w);
    return SHIFTND_OK;
}

}  // namespace shiftnd
