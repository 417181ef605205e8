// compact.hip -- in-place stable compaction of the per-row arrays after sc_index_delete_rows (gfx950).
//
// Deleting rows removes their STORED POSITIONS from every per-row array (X, xnorm, the bf16 / int8 / centred shadows, perm)
// and closes the gaps: survivor at position p moves to p - (deleted positions below p).  The host (sc_api.cpp,
// sc_index_delete_rows) walks the positions from the first deleted one in chunks of at most C rows; for a chunk
// [c0, c0 + cn) holding `del[lo, hi)` of the sorted deleted positions:
//
//   delete_flags_kernel         flags[p - c0] = 1 for the deleted positions of the chunk
//   delete_scan_blocks_kernel   keep = !flag; per 1 024-position tile the number of kept rows
//   delete_scan_sums_kernel     exclusive prefix over the tile counts (one workgroup)
//   delete_scan_emit_kernel     exclusive prefix inside the tile + tile offset = destination slot j of every kept row;
//                               src[j] = p - c0   (the inverse map: slot -> source, what the move kernels read)
//   move_rows16_kernel / move_words_kernel   dst[d0 + j] = src[c0 + src[j]],  d0 = c0 - lo
//
// Hazard.  Destination <= source for every row, but inside one launch a destination may be another row's source.  The m kept
// rows of a chunk land in [d0, d0 + m) and are read from [c0, c0 + cn).  With s = c0 - d0 = lo rows deleted before the chunk:
//   s >= m   the two ranges are disjoint (d0 + m <= c0): one launch moves the rows directly;
//   s <  m   the rows are first gathered into a bounce buffer of C rows and copied to their places by a second launch.
// Chunks are launched in ascending order on one stream, so a chunk never overwrites rows a later chunk still has to read
// (its destinations end below its own first source) and earlier chunks are complete.  The scratch is C rows + 8 B per
// position of a chunk: bounded, independent of the corpus size.
//
// Row moves are 16 B per lane over a flat index of 16-byte units (consecutive lanes, consecutive units): coalesced for every
// row size, and rows of 128 B (bf16 shadow at dim 64) still fill the wave.  Row strides are multiples of 16 B by
// construction (ld: 64 floats, ld8: 128 bytes, xcs: 16 B); xnorm / xscale / perm are single words.
//
// perm's VALUES are row ids and need the renumbering by id as well: new id = id - (deleted ids below id), the exclusive
// prefix of the deleted-id flags evaluated at id -- as a rank query (binary search) in the sorted deleted ids, which the
// device holds anyway (renumber_ids_kernel).
//
// Replaces (reference): Collection.delete(expr) of pymilvus, which the reference never calls.
#include "sc_common.h"

static const int SCAN_TILE = 1024;  // positions per workgroup of the scan kernels (256 threads x 4)

__global__ __launch_bounds__(256) void delete_flags_kernel(const uint32_t* __restrict__ del, int64_t lo, int64_t hi, int64_t c0,
                                                            uint32_t* __restrict__ flags) {
    for (int64_t i = lo + (int64_t)blockIdx.x * 256 + threadIdx.x; i < hi; i += (int64_t)gridDim.x * 256)
        flags[(int64_t)del[i] - c0] = 1u;
}

// exclusive scan of v over the 256 threads of a workgroup; *total = sum.  lds: 4 words.
static __device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* lds, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t t = lds[w];
        if (w < wave) before += t;
        all += t;
    }
    __syncthreads();
    *total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(256) void delete_scan_blocks_kernel(const uint32_t* __restrict__ flags, uint32_t cn, uint32_t* __restrict__ tile_sum) {
    __shared__ uint32_t lds[4];
    const uint32_t i0 = blockIdx.x * SCAN_TILE + threadIdx.x * 4;
    uint32_t kept = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (i0 + c < cn && flags[i0 + c] == 0u) ++kept;
    uint32_t total;
    (void)block_exclusive_scan(kept, lds, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// in place: tile_sum[t] <- kept rows in the tiles before t  (one workgroup; carries across rounds of 256 tiles)
__global__ __launch_bounds__(256) void delete_scan_sums_kernel(uint32_t* __restrict__ tile_sum, uint32_t tiles) {
    __shared__ uint32_t lds[4];
    uint32_t carry = 0;
    for (uint32_t t0 = 0; t0 < tiles; t0 += 256) {
        const uint32_t t = t0 + threadIdx.x;
        const uint32_t v = t < tiles ? tile_sum[t] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan(v, lds, &total);
        if (t < tiles) tile_sum[t] = carry + ex;
        carry += total;
    }
}

__global__ __launch_bounds__(256) void delete_scan_emit_kernel(const uint32_t* __restrict__ flags, uint32_t cn, const uint32_t* __restrict__ tile_sum,
                                                                uint32_t* __restrict__ src) {
    __shared__ uint32_t lds[4];
    const uint32_t i0 = blockIdx.x * SCAN_TILE + threadIdx.x * 4;
    bool keep[4];
    uint32_t kept = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        keep[c] = i0 + c < cn && flags[i0 + c] == 0u;
        kept += keep[c] ? 1u : 0u;
    }
    uint32_t total;
    uint32_t j = tile_sum[blockIdx.x] + block_exclusive_scan(kept, lds, &total);
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (keep[c]) src[j++] = i0 + c;
}

void sc_launch_delete_map(const uint32_t* del_dev, int64_t lo, int64_t hi, int64_t c0, uint32_t cn, uint32_t* flags, uint32_t* tile_sum, uint32_t* src,
                          hipStream_t s) {
    if (cn == 0) return;
    (void)hipMemsetAsync(flags, 0, (size_t)cn * 4, s);
    if (hi > lo) {
        int64_t blocks = (hi - lo + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(delete_flags_kernel, dim3((unsigned)blocks), dim3(256), 0, s, del_dev, lo, hi, c0, flags);
    }
    const uint32_t tiles = (cn + SCAN_TILE - 1) / SCAN_TILE;
    hipLaunchKernelGGL(delete_scan_blocks_kernel, dim3(tiles), dim3(256), 0, s, flags, cn, tile_sum);
    hipLaunchKernelGGL(delete_scan_sums_kernel, dim3(1), dim3(256), 0, s, tile_sum, tiles);
    hipLaunchKernelGGL(delete_scan_emit_kernel, dim3(tiles), dim3(256), 0, s, flags, cn, tile_sum, src);
}

// dst[j] = in[row0 + (src ? src[j] : j)] for m rows of upr 16-byte units; `in` and `dst` are the units of row 0.
// m * upr < 2^31 (the host sizes a chunk by bytes), row0 + src[j] is a 64-bit row number.
__global__ __launch_bounds__(256) void move_rows16_kernel(const uint4* __restrict__ in, int64_t row0, const uint32_t* __restrict__ src, uint32_t m, uint32_t upr,
                                                           uint4* __restrict__ dst) {
    const uint32_t total = m * upr, stride = gridDim.x * 256u;
    uint32_t u = blockIdx.x * 256u + threadIdx.x;
    // four independent 16-byte loads in flight per lane
    for (; u + 3u * stride < total; u += 4u * stride) {
        uint4 v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t uu = u + (uint32_t)c * stride, j = uu / upr, o = uu - j * upr;
            v[c] = in[(row0 + (int64_t)(src ? src[j] : j)) * (int64_t)upr + o];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) dst[u + (uint32_t)c * stride] = v[c];
    }
    for (; u < total; u += stride) {
        const uint32_t j = u / upr, o = u - j * upr;
        dst[u] = in[(row0 + (int64_t)(src ? src[j] : j)) * (int64_t)upr + o];
    }
}

__global__ __launch_bounds__(256) void move_words_kernel(const uint32_t* __restrict__ in, int64_t row0, const uint32_t* __restrict__ src, uint32_t m,
                                                          uint32_t* __restrict__ dst) {
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < m; j += gridDim.x * 256u) dst[j] = in[row0 + (int64_t)(src ? src[j] : j)];
}

// Rows of `row_bytes` (4, or a multiple of 16): dst row j <- row (row0 + src[j]) of `in` (src == nullptr: row0 + j).
// `in` and `dst` may alias only when the caller has shown the ranges disjoint (see the head of this file).
void sc_launch_move_rows(const void* in, int64_t row0, const uint32_t* src, uint32_t m, size_t row_bytes, void* dst, hipStream_t s) {
    if (m == 0) return;
    if (row_bytes == 4) {
        uint32_t blocks = (m + 255u) / 256u;
        if (blocks > 2048u) blocks = 2048u;
        hipLaunchKernelGGL(move_words_kernel, dim3(blocks), dim3(256), 0, s, (const uint32_t*)in, row0, src, m, (uint32_t*)dst);
        return;
    }
    const uint32_t upr = (uint32_t)(row_bytes / 16);
    const uint64_t total = (uint64_t)m * upr;
    uint64_t blocks = (total + 1023) / 1024;  // four units per lane
    if (blocks > 256u * 16u) blocks = 256u * 16u;
    hipLaunchKernelGGL(move_rows16_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const uint4*)in, row0, src, m, upr, (uint4*)dst);
}

// ids[i] <- ids[i] - |{d in del : d < ids[i]}|  (del sorted ascending, ndel >= 1)
__global__ __launch_bounds__(256) void renumber_ids_kernel(uint32_t* __restrict__ ids, int64_t n, const uint32_t* __restrict__ del, int64_t ndel) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint32_t v = ids[i];
        int64_t a = 0, b = ndel;  // first index with del[idx] >= v
        while (a < b) {
            const int64_t mid = (a + b) >> 1;
            if (del[mid] < v) a = mid + 1;
            else b = mid;
        }
        ids[i] = v - (uint32_t)a;
    }
}

void sc_launch_renumber_ids(uint32_t* ids, int64_t n, const uint32_t* del_dev, int64_t ndel, hipStream_t s) {
    if (n <= 0 || ndel <= 0) return;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(renumber_ids_kernel, dim3((unsigned)blocks), dim3(256), 0, s, ids, n, del_dev, ndel);
}
