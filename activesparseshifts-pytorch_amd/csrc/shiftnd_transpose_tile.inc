// shiftnd_transpose_tile.inc -- the body of one workgroup's 64 x 64 tile of shiftnd_transpose.hip, included inside each kernel (not a
// function: the kernels' __restrict__ parameters and the instruction streams of the per-form kernels stay exactly as they were).
// Expects in scope: ESIZE (constant), VEC (constant or launch-uniform: rows and cols of whole 16-byte pieces, 16-byte-aligned
// bases), src_, dst_, rows, cols, tiles_r, tiles_c.
    using R = typename raw_t<ESIZE>::type;
    constexpr int E = 16 / ESIZE;                       // elements per 16-byte piece
    // bytes; the extra dword (two for 8-byte elements, whose LDS accesses must stay 8-byte aligned) staggers the banks
    constexpr int PITCH = kTile * ESIZE + (ESIZE == 8 ? 8 : 4);
    __shared__ __attribute__((aligned(16))) char tile[kTile * PITCH + 16];
    // consecutive workgroups walk the SHORTER tile dimension first (the channel dimension of either direction), so
    // the long contiguous side -- whole channels-last pixel rows -- is read or written as one contiguous region by
    // neighbouring workgroups (NCHW -> channels-last N16 C256 224x224 fp32: 1.37 -> see DESIGN.md)
    int b = blockIdx.x, tr, tc;
    if (tiles_r < tiles_c) {
        tr = b % tiles_r;
        b /= tiles_r;
        tc = b % tiles_c;
        b /= tiles_c;
    } else {
        tc = b % tiles_c;
        b /= tiles_c;
        tr = b % tiles_r;
        b /= tiles_r;
    }
    const int n = b;
    const int r0 = tr * kTile, c0 = tc * kTile;
    const R *src = static_cast<const R *>(src_) + static_cast<int64_t>(n) * rows * cols;
    R *dst = static_cast<R *>(dst_) + static_cast<int64_t>(n) * rows * cols;
    const bool full = r0 + kTile <= rows && c0 + kTile <= cols;
    if (VEC && full) {
        constexpr int VPR = kTile / E;                  // 16-byte pieces per tile row
#pragma unroll
        for (int k = 0; k < kTile * VPR / kThreads; ++k) {
            const int v = k * kThreads + static_cast<int>(threadIdx.x);
            const int r = v / VPR, cv = v - r * VPR;
            const Chunk<R, E> ch = load_chunk<R, E, true>(src + static_cast<int64_t>(r0 + r) * cols + c0 + cv * E);
            // the pitch is not a multiple of 16: element-size stores
#pragma unroll
            for (int e = 0; e < E; ++e) *reinterpret_cast<R *>(tile + r * PITCH + (cv * E + e) * ESIZE) = ch.e[e];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kTile * VPR / kThreads; ++k) {
            const int v = k * kThreads + static_cast<int>(threadIdx.x);
            const int c = v / VPR, rv = v - c * VPR;   // output row c of the tile, piece rv along the source rows
            Chunk<R, E> ch;
#pragma unroll
            for (int e = 0; e < E; ++e) ch.e[e] = *reinterpret_cast<const R *>(tile + (rv * E + e) * PITCH + c * ESIZE);
            store_chunk<R, E>(dst + static_cast<int64_t>(c0 + c) * rows + r0 + rv * E, ch);
        }
    } else {
        for (int v = threadIdx.x; v < kTile * kTile; v += kThreads) {
            const int r = v / kTile, c = v - r * kTile;
            if (r0 + r < rows && c0 + c < cols)
                *reinterpret_cast<R *>(tile + r * PITCH + c * ESIZE) = src[static_cast<int64_t>(r0 + r) * cols + c0 + c];
        }
        __syncthreads();
        for (int v = threadIdx.x; v < kTile * kTile; v += kThreads) {
            const int c = v / kTile, r = v - c * kTile;
            if (r0 + r < rows && c0 + c < cols)
                dst[static_cast<int64_t>(c0 + c) * rows + r0 + r] = *reinterpret_cast<const R *>(tile + r * PITCH + c * ESIZE);
        }
    }
