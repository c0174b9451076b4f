// BF_FLAG_EXACT_SUM (include/beifong_hip.h), the two kernels that are not render kernels:
//   bf_sum_resolve_kernel : one thread per cell of a launch's limb buffer: hist[i] = fl(hist[i] + the cell's exact sum), one rounding
//   bf_sum_probe_kernel   : bf_exact_sum — caller-given (cell, value) pairs through hist_add<true> and flush_limbs, the device functions
//                           the kSum render kernels add with (bf_film.h)
// The arithmetic is bf_sum.h's; this file only moves limbs.
#include "bf_film.h"
#include "bf_launch.h"
#include "bf_sum.h"

BF_NS_BEGIN

__global__ void bf_sum_resolve_kernel(const long long *limbs, float *hist, uint32_t n_cells) {
    const uint32_t i = blockIdx.x * (uint32_t) kBlock + threadIdx.x;
    if (i >= n_cells) return;
    int64_t cell[bfs::kLimbs];
#pragma unroll
    for (int l = 0; l < bfs::kLimbs; ++l) cell[l] = limbs[(size_t) i * bfs::kLimbs + l];
    int64_t any = 0;
#pragma unroll
    for (int l = 0; l < bfs::kLimbs; ++l) any |= cell[l];
    if (any == 0) return;      // no addend (bf_sum.h: Resolved::empty): the caller's value stays as it is
    // the caller's value is one more addend — of the digits, not of the limbs: a limb may be one piece short of its headroom
    bfs::normalize(cell);
    const uint32_t old = __float_as_uint(hist[i]);
    if (bfs::finite_bits(old)) {
        bfs::add(cell, old);
        hist[i] = __uint_as_float(bfs::resolve(cell).bits);
    } else {
        // a non-finite value takes every finite sum with it, as in fp32
        hist[i] = hist[i] + __uint_as_float(bfs::resolve(cell).bits);
    }
}

__global__ void bf_sum_probe_kernel(uint64_t n, const uint32_t *cell, const float *value, uint32_t n_cells, uint32_t in_lds, float *g_limbs) {
    extern __shared__ __align__(16) unsigned char s_raw[];
    float *s_limbs = reinterpret_cast<float *>(s_raw);
    const int tid = threadIdx.x;
    const bool lds = in_lds != 0u;
    if (lds) {
        for (uint32_t i = tid; i < n_cells * (uint32_t) bfs::kCellFloats; i += kBlock) s_limbs[i] = 0.f;
        __syncthreads();
    }
    for (uint64_t i = (uint64_t) blockIdx.x * kBlock + tid; i < n; i += (uint64_t) gridDim.x * kBlock) {
        const uint32_t c = cell[i];
        if (c < n_cells) hist_add<true>(s_limbs, g_limbs, lds, c, value[i]);      // (the host has checked the indices: never out of bounds)
    }
    if (lds) flush_limbs(s_limbs, g_limbs, n_cells, tid);
}

BF_NS_END  // namespace bfd

extern "C" hipError_t bfk_sum_resolve(const void *limbs, float *hist, uint32_t n_cells, hipStream_t stream) {
    if (!n_cells) return hipSuccess;
    hipLaunchKernelGGL(bfd::bf_sum_resolve_kernel, dim3((n_cells + bfd::kBlock - 1) / bfd::kBlock), dim3(bfd::kBlock), 0, stream,
                       (const long long *) limbs, hist, n_cells);
    return hipGetLastError();
}

extern "C" hipError_t bfk_sum_probe(uint64_t n, const uint32_t *cell, const float *value, uint32_t n_cells, int in_lds, void *limbs,
                                    unsigned grid, hipStream_t stream) {
    const size_t lds_bytes = in_lds ? sizeof(float) * bfs::kCellFloats * (size_t) n_cells : 0;
    hipLaunchKernelGGL(bfd::bf_sum_probe_kernel, dim3(grid), dim3(bfd::kBlock), lds_bytes, stream, n, cell, value, n_cells,
                       in_lds ? 1u : 0u, (float *) limbs);
    return hipGetLastError();
}
