// shiftnd_stream.hip -- the ONLINE temporal shift: one frame per call against a cached state, SHIFTND_SHIFT_DIM0 | SHIFTND_STREAM,
// both dense layouts (gfx950).
//
// Online video recognition (the uni-directional TSM, arXiv 1811.08383 section 4.2) sees one frame [B, C, ...] of B independent
// streams per call.  A channel with shift s > 0 shows what that channel held s frames ago; the last D frames of the shifted
// channels live in a state of D slots, each with the frame's shape and strides, slot k holding frame t-1-k.  One step, for every
// channel c with s = clamp(s_c, 0, D) > 0:
//     frame[:, c]   <- slot[s-1][:, c]
//     slot[k][:, c] <- slot[k-1][:, c]    for k = s-1 .. 1
//     slot[0][:, c] <- frame[:, c]        (the frame as it came in)
// A channel with s == 0 is neither read nor written, in the frame or in the state, and slots k >= s of a channel are never touched.
//
// Ownership, as in shiftnd_inplace.hip.  A thread owns one PIECE: a naturally aligned power-of-two byte range of at most 16 bytes at
// the same offset in the frame and in every slot of ONE stream.  Pieces are disjoint and a thread touches only bytes of its own
// piece, so there is no cross-thread hazard: no barrier, LDS, atomic or workspace.  The LINE of a piece under the shift s is s + 1
// pieces: the frame's and those of slots 0 .. s-1.  The thread gathers them into register slots -- every load is issued before the
// first store -- and stores them rotated by one place: register j goes to slot j for j < s, register s goes to the frame.  The
// pointers are not __restrict__ and the accesses are plain C++ (nontemporal builtins): program order alone gives the right values.
// The host refuses a frame that overlaps the state.
//
// A stream's frame is a sequence of RUNS: the C channel planes of M * es bytes (contiguous; the run is the channel) or the M pixel
// rows of C * es bytes (channels-last; the channel is the element's place in its row).  The piece is the widest power of two, at
// most 16 bytes, that divides the run's bytes and both bases, never below the element size, so no piece straddles two runs.  One
// thread per (stream, piece of a frame), consecutive lanes on consecutive pieces.
//   uniform piece   (every contiguous piece; a channels-last piece whose channels share one shift) one line.
//   mixed piece     (channels-last, channels of one piece with different shifts) a line per ELEMENT, element-wide accesses.
// The registers of a line are indexed by compile-time constants: kMaxLine = 16 of them (64 data VGPRs for 16-byte pieces), those
// above s predicated off; the host route refuses D > 15.  An entry outside [0, D] is clamped into it: the kernel cannot raise.
// shiftnd_last_kernel() names the form: frames_stream (16-byte pieces), frames_stream_ragged (8-, 4-, 2- or 1-byte pieces).
// Every access is naturally aligned and lies inside the frame or inside slots [0, D); the table is read at entries [0, C) only.
#include "shiftnd_temporal.hpp"

namespace shiftnd {
namespace {

constexpr int kMaxLine = 16;   // register slots of a line: the frame and at most 15 state slots

struct StreamParams {
    int wkind, es_log2, unit_log2;   // element bytes and piece bytes as powers of two
    int cl;                          // 1: channels-last (runs are pixel rows), 0: contiguous (runs are channel planes)
    int small;                       // pieces per frame below 2^31: the run of a piece by FastDiv
    int D;                           // state slots, 1 .. kMaxLine - 1
    uint32_t chunks, ppr;            // workgroups per stream, pieces per run
    FastDiv d_chunks, d_ppr;
    int64_t ppf, frame_bytes;        // pieces per stream's frame, bytes of a stream's frame
    int64_t slot_bytes;              // bytes from a slot to the next (the B streams' frames)
    int64_t wzp;                     // zero point of an integer table
};

__device__ __forceinline__ int clamp_shift(const StreamParams &q, int64_t s) {
    return static_cast<int>(s < 0 ? 0 : (s > q.D ? q.D : s));
}

// one piece of 1 << ul bytes at p (naturally aligned; ul is launch-uniform at every call site: scalar branches) in the low bytes of
// a 16-byte register group.  ONE copy of the line's code serves every piece size: five templated copies in one kernel took hipcc
// (ROCm 7.2) to 506 registers and one wave per SIMD, where each copy alone needs 77
__device__ __forceinline__ shiftnd_u4 load_piece(const char *p, int ul) {
    shiftnd_u4 r = (shiftnd_u4)(0u);
    switch (ul) {
    case 4: r = __builtin_nontemporal_load(reinterpret_cast<const shiftnd_u4 *>(p)); break;
    case 3: {
        const piece_of<3>::type t = __builtin_nontemporal_load(reinterpret_cast<const piece_of<3>::type *>(p));
        r.x = t.x;
        r.y = t.y;
        break;
    }
    case 2: r.x = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(p)); break;
    case 1: r.x = __builtin_nontemporal_load(reinterpret_cast<const uint16_t *>(p)); break;
    default: r.x = __builtin_nontemporal_load(reinterpret_cast<const uint8_t *>(p)); break;
    }
    return r;
}
__device__ __forceinline__ void store_piece(char *p, int ul, shiftnd_u4 r) {
    switch (ul) {
    case 4: __builtin_nontemporal_store(r, reinterpret_cast<shiftnd_u4 *>(p)); break;
    case 3: {
        piece_of<3>::type t;
        t.x = r.x;
        t.y = r.y;
        __builtin_nontemporal_store(t, reinterpret_cast<piece_of<3>::type *>(p));
        break;
    }
    case 2: __builtin_nontemporal_store(r.x, reinterpret_cast<uint32_t *>(p)); break;
    case 1: __builtin_nontemporal_store(static_cast<uint16_t>(r.x), reinterpret_cast<uint16_t *>(p)); break;
    default: __builtin_nontemporal_store(static_cast<uint8_t>(r.x), reinterpret_cast<uint8_t *>(p)); break;
    }
}

// the line of the bytes [f, f + (1 << ul)) of the frame and [st, st + (1 << ul)) of slot 0 under the shift s in [0, D]: gather, then
// store one place on
__device__ __forceinline__ void rotate_line(const StreamParams &q, char *f, char *st, int s, int ul) {
    if (s == 0) return;   // nothing moves
    shiftnd_u4 v[kMaxLine];   // v[0]: the frame, v[1 + k]: slot k
    v[0] = load_piece(f, ul);
#pragma unroll
    for (int j = 1; j < kMaxLine; ++j) {
        v[j] = (shiftnd_u4)(0u);
        if (j <= s) v[j] = load_piece(st + (j - 1) * q.slot_bytes, ul);
    }
#pragma unroll
    for (int j = 0; j < kMaxLine; ++j) {
        if (j < s) store_piece(st + j * q.slot_bytes, ul, v[j]);
        else if (j == s) store_piece(f, ul, v[j]);
    }
}

// ONE kernel for every piece size and both layouts (q.unit_log2, q.es_log2 and q.cl are launch-uniform: scalar branches): the library's
// kernel budget has room for one; shiftnd_last_kernel() names the form that ran, frames_stream or frames_stream_ragged.
__global__ __launch_bounds__(kThreads) void frames_stream(StreamParams q, char *frame, char *state, const void *__restrict__ w) {
    const uint32_t b = fdiv(blockIdx.x, q.d_chunks);   // the stream
    const uint32_t chunk = blockIdx.x - b * q.chunks;
    const int64_t k = static_cast<int64_t>(chunk) * kThreads + threadIdx.x;   // the piece of the stream's frame
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
    const int64_t at = static_cast<int64_t>(b) * q.frame_bytes + (k << q.unit_log2);
    char *f = frame + at, *st = state + at;
    // contiguous: the run is the channel.  Channels-last: the piece holds the channels [e0, e0 + epp) of its pixel; equal raw entries
    // (the everyday table is constant over runs of channels) are one shift, entries that differ are compared as clamped shifts
    const int epp_log2 = q.cl ? q.unit_log2 - q.es_log2 : 0, epp = 1 << epp_log2;
    const int64_t e0 = q.cl ? static_cast<int64_t>(kr) << epp_log2 : run;
    const int s0 = clamp_shift(q, gather_shift(w, q.wkind, q.wzp, e0));
    bool uniform = true;
    if (epp_log2 > 0) {
        uniform = piece_entries_equal<4>(w, q.wkind, e0, epp_log2);
        if (!uniform) {
            uniform = true;
#pragma unroll 1
            for (int e = 1; e < epp; ++e) uniform = uniform && clamp_shift(q, gather_shift(w, q.wkind, q.wzp, e0 + e)) == s0;
        }
    }
    if (uniform) {   // every contiguous piece; a channels-last piece whose channels share one shift
        rotate_line(q, f, st, s0, q.unit_log2);
        return;
    }
    // mixed piece: a line per element
#pragma unroll 1
    for (int e = 0; e < epp; ++e) {
        const int s = clamp_shift(q, gather_shift(w, q.wkind, q.wzp, e0 + e));
        rotate_line(q, f + (e << q.es_log2), st + (e << q.es_log2), s, q.es_log2);
    }
}

// dense strides of a frame [N, C, S1, S2] (normalised order; the S0 place is not looked at), contiguous or channels-last
bool dense_frame(const Geometry &g, const int64_t *st, bool cl) {
    const int64_t A = g.nd == 3 ? g.S[1] : 1, B = g.S[2], M = A * B;
    if (cl) {
        if (g.C > 1 && st[1] != 1) return false;
        if (B > 1 && st[4] != g.C) return false;
        if (A > 1 && st[3] != B * g.C) return false;
    } else {
        if (B > 1 && st[4] != 1) return false;
        if (A > 1 && st[3] != B) return false;
        if (g.C > 1 && st[1] != M) return false;
    }
    return g.N == 1 || st[0] == g.C * M;
}

}  // namespace

// The sizes the kernel serves (include/shiftnd_hip.h states them): those of inplace_geometry_ok with the D slots in the place of the
// frames of a clip, and at most kMaxLine - 1 slots.
bool stream_geometry_ok(const Geometry &g, int dtype) { return inplace_geometry_ok(g, dtype) && g.S[3 - g.nd] <= kMaxLine - 1; }

// 1: frame and state both dense contiguous, 2: both dense channels-last, 0: neither, or the two overlap.  A pair both describe (planes
// or channels of size 1) is contiguous.  The state's slots have the frame's strides and lie one frame apart.
int stream_layout(const Geometry &g, int dtype, const void *state, const int64_t *state_strides, const void *frame,
                  const int64_t *frame_strides) {
    const int64_t es = dtype_size(dtype), D = g.S[3 - g.nd], block = g.N * g.C * frame_pixels(g);
    if (!aligned_to(state, es) || !aligned_to(frame, es)) return 0;
    if (D > 1 && state_strides[2 + 3 - g.nd] != block) return 0;
    const uintptr_t f = reinterpret_cast<uintptr_t>(frame), s = reinterpret_cast<uintptr_t>(state);
    if (f < s + static_cast<uintptr_t>(D * block * es) && s < f + static_cast<uintptr_t>(block * es)) return 0;
    if (dense_frame(g, state_strides, false) && dense_frame(g, frame_strides, false)) return 1;
    return dense_frame(g, state_strides, true) && dense_frame(g, frame_strides, true) ? 2 : 0;
}

int stream_forward(const Geometry &g, int dtype, int layout, void *state, void *frame, const void *w, int wkind, int64_t wzp,
                   hipStream_t st) {
    const int es = dtype_size(dtype);
    const int64_t M = frame_pixels(g), run_bytes = (layout == 2 ? g.C : M) * es;
    StreamParams q;
    q.wkind = wkind;
    q.wzp = wzp;
    q.cl = layout == 2 ? 1 : 0;
    q.es_log2 = es_log2(es);
    q.D = static_cast<int>(g.S[3 - g.nd]);
    q.frame_bytes = g.C * M * es;
    q.slot_bytes = g.N * q.frame_bytes;
    q.unit_log2 = __builtin_ctz(piece_bytes(run_bytes, {state, frame}));
    q.ppf = q.frame_bytes >> q.unit_log2;
    q.ppr = static_cast<uint32_t>(run_bytes >> q.unit_log2);   // (at most max(C, M): below 2^31)
    q.small = q.ppf < (1LL << 31) ? 1 : 0;
    q.chunks = static_cast<uint32_t>((q.ppf + kThreads - 1) / kThreads);
    q.d_chunks = make_fastdiv(q.chunks);
    q.d_ppr = make_fastdiv(q.ppr);
    note_kernel(q.unit_log2 == 4 ? "frames_stream" : "frames_stream_ragged");
    void (*const kernel)(StreamParams, char *, char *, const void *) = frames_stream;
    const int64_t blocks = g.N * q.chunks;   // (below 2^31: stream_geometry_ok)
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, st, q, static_cast<char *>(frame),
                       static_cast<char *>(state), w);
    return SHIFTND_OK;
}

}  // namespace shiftnd
