// What bf_converge.hip and the converge driver of bf_render.cpp share (bf_render_converge_device, bf_converge_statistic_device:
// include/beifong_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bfd {
// Where the watched pairs of a BF_FLAG_MOMENT histogram sit: pair q = (cell q / pairs, j = q % pairs) reads
// m1 = hist[cell * chan + first0 + j], m2 = hist[cell * chan + second0 + j] and n = hist[cell * chan + w_off].
struct ConvLayout {
    uint64_t total;        // floats of the histogram: cells * chan
    uint64_t n_pairs;      // cells * pairs
    uint32_t chan, pairs, first0, second0, w_off;
    uint32_t pad;
};
// What the passes of one statistic hand to each other through device memory (zeroed before the first pass).  The orders of
// non-negative floats and doubles are those of their bit patterns, so every word is combined by an integer atomic and the
// result does not depend on the order of the workgroups.
struct ConvWork {
    uint32_t max_bits;                 // max |m1| over the watched pairs, as fp32 bits
    uint32_t bad;                      // some cell of the histogram is not finite
    unsigned long long stat_bits;      // max rel over the significant pairs, as fp64 bits (+inf: a significant pair with n < 2)
    unsigned long long n_sig;          // significant pairs
    unsigned long long pad;
};
// one slot of the pinned host ring
struct ConvResult {
    double stat;
    uint64_t n_significant;
    uint32_t round;
    uint32_t pad;
};
}  // namespace bfd

// One statistic, stream-ordered: [hist += blocks[0] + ... + blocks[n_blocks - 1], each `L->total` floats, in that order] ->
// max |m1| -> max rel -> *slot = {stat, n_significant, round}.  n_blocks == 0: the histogram is only read.
extern "C" hipError_t bfk_converge_round(float *hist, const float *blocks, uint32_t n_blocks, const bfd::ConvLayout *L, double floor,
                                         bfd::ConvWork *ws, bfd::ConvResult *slot, uint32_t round, hipStream_t stream);
