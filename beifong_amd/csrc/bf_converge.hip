// The convergence statistic of a BF_FLAG_MOMENT histogram on the device (specification: capi.converge_statistic):
// stat = max over the significant watched pairs of sqrt(var_of_mean) / |mean|, in fp64 from the fp32 cells.
//
// Three small kernels per statistic, each a grid-stride loop, handing over through bfd::ConvWork at kernel boundaries (the one
// hand-off between workgroups that needs no fence on a chip of eight L2s):
//   bf_conv_accumulate_kernel   one thread per cell: [adds the round's histogram blocks in block order,] flags a non-finite cell
//                               and takes max |m1| over the watched first-moment channels
//   bf_conv_stat_kernel         one thread per watched pair: significance against floor * max |m1|, rel, their maximum and count
//   bf_conv_finish_kernel       one thread: the three +inf cases, then {stat, n_significant, round} into the pinned slot
// Every combination across threads is an integer max / or / add, so the result is the same whatever the grid or the order.
#include "bf_converge.h"

namespace {
using bfd::ConvLayout;
using bfd::ConvResult;
using bfd::ConvWork;

constexpr int kConvBlock = 256;
constexpr unsigned kConvMaxGrid = 1024;
constexpr unsigned long long kInfBits = 0x7ff0000000000000ull;

__global__ __launch_bounds__(kConvBlock) void bf_conv_accumulate_kernel(float *__restrict__ hist, const float *__restrict__ blocks, uint32_t n_blocks,
                                                                        ConvLayout L, ConvWork *__restrict__ ws) {
    __shared__ uint32_t s_max[kConvBlock];
    __shared__ uint32_t s_bad[kConvBlock];
    uint32_t m = 0u, bad = 0u;
    const uint64_t stride = (uint64_t) gridDim.x * kConvBlock;
    for (uint64_t i = (uint64_t) blockIdx.x * kConvBlock + threadIdx.x; i < L.total; i += stride) {
        float v = hist[i];
        if (n_blocks) {
            for (uint32_t j = 0; j < n_blocks; ++j) v += blocks[(uint64_t) j * L.total + i];      // fixed order: a function of the blocks alone
            hist[i] = v;
        }
        const uint32_t mag = __float_as_uint(v) & 0x7fffffffu;
        if (mag >= 0x7f800000u) bad = 1u;
        const uint32_t c = (uint32_t) (i % L.chan);
        if (c - L.first0 < L.pairs) m = max(m, mag);      // (unsigned: c < first0 wraps out of range)
    }
    s_max[threadIdx.x] = m;
    s_bad[threadIdx.x] = bad;
    __syncthreads();
    for (int s = kConvBlock / 2; s > 0; s >>= 1) {
        if ((int) threadIdx.x < s) {
            s_max[threadIdx.x] = max(s_max[threadIdx.x], s_max[threadIdx.x + s]);
            s_bad[threadIdx.x] |= s_bad[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (s_max[0]) atomicMax(&ws->max_bits, s_max[0]);
        if (s_bad[0]) atomicOr(&ws->bad, 1u);
    }
}

__global__ __launch_bounds__(kConvBlock) void bf_conv_stat_kernel(const float *__restrict__ hist, ConvLayout L, double floor, ConvWork *__restrict__ ws) {
    __shared__ unsigned long long s_stat[kConvBlock];
    __shared__ unsigned long long s_sig[kConvBlock];
    // (written by the kernel before this one)
    const double max_m1 = (double) __uint_as_float(ws->max_bits);
    const bool any = ws->bad == 0u && max_m1 > 0.0;
    const double threshold = floor * max_m1;
    unsigned long long stat = 0ull, sig = 0ull;
    const uint64_t stride = (uint64_t) gridDim.x * kConvBlock;
    for (uint64_t q = (uint64_t) blockIdx.x * kConvBlock + threadIdx.x; any && q < L.n_pairs; q += stride) {
        const uint64_t base = (q / L.pairs) * L.chan;
        const uint32_t j = (uint32_t) (q % L.pairs);
        const double m1 = (double) hist[base + L.first0 + j];
        if (!(fabs(m1) >= threshold)) continue;
        ++sig;
        const double m2 = (double) hist[base + L.second0 + j], n = (double) hist[base + L.w_off];
        unsigned long long bits = kInfBits;      // n < 2, or a significant pair whose mean is 0 (floor 0)
        if (n >= 2.0 && m1 != 0.0) {
            // capi.moment_estimate, operation for operation (contraction is off: Makefile)
            const double mean = m1 / n;
            const double var = fmax(m2 / n - mean * mean, 0.0) / (n - 1.0);
            bits = (unsigned long long) __double_as_longlong(sqrt(var) / fabs(mean));
        }
        stat = max(stat, bits);
    }
    s_stat[threadIdx.x] = stat;
    s_sig[threadIdx.x] = sig;
    __syncthreads();
    for (int s = kConvBlock / 2; s > 0; s >>= 1) {
        if ((int) threadIdx.x < s) {
            s_stat[threadIdx.x] = max(s_stat[threadIdx.x], s_stat[threadIdx.x + s]);
            s_sig[threadIdx.x] += s_sig[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && s_sig[0]) {
        atomicMax(&ws->stat_bits, s_stat[0]);
        atomicAdd(&ws->n_sig, s_sig[0]);
    }
}

__global__ void bf_conv_finish_kernel(const ConvWork *__restrict__ ws, ConvResult *slot, uint32_t round) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    // +inf, never NaN: a non-finite cell, no significant pair, or a significant pair with n < 2 (its bits are the maximum already)
    const bool none = ws->bad != 0u || ws->n_sig == 0ull;
    slot->stat = __longlong_as_double((long long) (none ? kInfBits : ws->stat_bits));
    slot->n_significant = ws->bad ? 0ull : ws->n_sig;
    slot->round = round;
    slot->pad = 0u;
}

unsigned conv_grid(uint64_t n) { return (unsigned) ((n + kConvBlock - 1) / kConvBlock < kConvMaxGrid ? (n + kConvBlock - 1) / kConvBlock : kConvMaxGrid); }
}  // namespace

extern "C" hipError_t bfk_converge_round(float *hist, const float *blocks, uint32_t n_blocks, const bfd::ConvLayout *L, double floor,
                                         bfd::ConvWork *ws, bfd::ConvResult *slot, uint32_t round, hipStream_t stream) {
    if (!L->total || !L->n_pairs) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(ws, 0, sizeof(bfd::ConvWork), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bf_conv_accumulate_kernel, dim3(conv_grid(L->total)), dim3(kConvBlock), 0, stream, hist, blocks, n_blocks, *L, ws);
    hipLaunchKernelGGL(bf_conv_stat_kernel, dim3(conv_grid(L->n_pairs)), dim3(kConvBlock), 0, stream, (const float *) hist, *L, floor, ws);
    hipLaunchKernelGGL(bf_conv_finish_kernel, dim3(1), dim3(1), 0, stream, (const bfd::ConvWork *) ws, slot, round);
    return hipGetLastError();
}
