// shiftnd_transpose.hip -- batched matrix transpose, the layout change between channels-last and contiguous
// tensors: dst[n][c][r] = src[n][r][c] for dense src[N][rows][cols], dst[N][cols][rows].
//
// Why it exists: the reference's float ops return an NCHW-contiguous tensor even for a channels-last input
// (cpu/shifts_cpu.cpp:221) and its CUDA backend walks a channels-last input through strides (uncoalesced).  With
// mixed layouts one side of a gather kernel is uncoalesced whichever way it iterates; changing the
// layout first with a tile transpose at copy bandwidth and running the contiguous kernels is several times faster.
//
// One workgroup moves a 64 x 64 element tile through LDS: 16-byte global loads along `cols`, 16-byte global stores
// along `rows`; the LDS row pitch is odd in dwords so the column-wise reads are bank-conflict free.  Ragged tiles
// and shapes whose rows are not whole 16-byte pieces take the element-wise path.
#include "shiftnd_common.hpp"
#include "shiftnd_launch.hpp"

namespace shiftnd {
namespace {

constexpr int kTile = 64;

template <int ESIZE, bool VEC>
__global__ __launch_bounds__(kThreads) void transpose_tiles(const void *__restrict__ src_, void *__restrict__ dst_, int rows,
                                                            int cols, int tiles_r, int tiles_c) {
#include "shiftnd_transpose_tile.inc"
}

// 8-byte elements: the form is a run-time argument (launch-uniform, a scalar branch) and one kernel serves both -- the library's
// kernel budget.  1-, 2- and 4-byte elements keep one kernel per form.
__global__ __launch_bounds__(kThreads) void transpose_tiles8(const void *__restrict__ src_, void *__restrict__ dst_, int rows, int cols,
                                                             int tiles_r, int tiles_c, int vec) {
    constexpr int ESIZE = 8;
    const bool VEC = vec != 0;
#include "shiftnd_transpose_tile.inc"
}

template <int ESIZE>
int launch_transpose(const void *src, void *dst, int64_t N, int64_t rows, int64_t cols, hipStream_t st) {
    const int64_t tr = (rows + kTile - 1) / kTile, tc = (cols + kTile - 1) / kTile;
    const int64_t blocks = N * tr * tc;
    if (blocks <= 0) return SHIFTND_OK;
    if (blocks >= (1LL << 31) || rows >= (1LL << 31) || cols >= (1LL << 31)) return SHIFTND_ERR_TOO_LARGE;
    const bool vec = (rows * ESIZE) % 16 == 0 && (cols * ESIZE) % 16 == 0 && reinterpret_cast<uintptr_t>(src) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(dst) % 16 == 0;
    if constexpr (ESIZE == 8)
        hipLaunchKernelGGL(transpose_tiles8, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, st, src, dst, static_cast<int>(rows),
                           static_cast<int>(cols), static_cast<int>(tr), static_cast<int>(tc), vec ? 1 : 0);
    else if (vec)
        hipLaunchKernelGGL((transpose_tiles<ESIZE, true>), dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, st, src, dst,
                           static_cast<int>(rows), static_cast<int>(cols), static_cast<int>(tr), static_cast<int>(tc));
    else
        hipLaunchKernelGGL((transpose_tiles<ESIZE, false>), dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, st, src, dst,
                           static_cast<int>(rows), static_cast<int>(cols), static_cast<int>(tr), static_cast<int>(tc));
    return SHIFTND_OK;
}

}  // namespace

int transpose_planes(const void *src, void *dst, int64_t N, int64_t rows, int64_t cols, int esize, hipStream_t st) {
    note_kernel("transpose_tiles");
    switch (esize) {
    case 1: return launch_transpose<1>(src, dst, N, rows, cols, st);
    case 2: return launch_transpose<2>(src, dst, N, rows, cols, st);
    case 4: return launch_transpose<4>(src, dst, N, rows, cols, st);
    case 8: return launch_transpose<8>(src, dst, N, rows, cols, st);
    default: return SHIFTND_ERR_UNSUPPORTED_DTYPE;
    }
}

}  // namespace shiftnd
