// Lane packing over the live masks of a wavefront pool: a scheduling device of wf_shade, wf_trace (bf_wavefront.hip) and the
// tail kernel (bf_kernels.hip).  It mirrors nothing of the reference, which renders one path per thread from start to end.
#pragma once
#include "bf_device_math.h"

BF_NS_BEGIN

// ---------------------------------------------------------------------------
// on-the-fly compaction: a cursor over a segment of 64-bit batch masks hands the
// next set bits (= slots that need work) to the lanes that ask for one
// ---------------------------------------------------------------------------
BF_DEV uint32_t nth_set_bit(unsigned long long m, uint32_t r) {
    // position of the r-th (0-based) set bit of m; caller guarantees r < popc(m)
    uint32_t pos = 0;
#pragma unroll
    for (int shift = 32; shift >= 1; shift >>= 1) {
        unsigned long long lowmask = (1ull << shift) - 1ull;
        uint32_t cnt = (uint32_t) __popcll(m & lowmask);
        if (r >= cnt) {
            r -= cnt;
            m >>= shift;
            pos += shift;
        } else {
            m &= lowmask;
        }
    }
    return pos;
}

// Walks the set bits of a wave's share of a batch-mask array.  The words are fetched 64 at a
// time, one per lane, so skipping the empty words of a sparse pool costs one load and a few
// scalar bit operations per 64 batches instead of one dependent memory round trip per word
// (which made every late, nearly empty bounce iteration cost 200-400 us whatever little work
// it held).
//
// A wave's share of the mask array is INTERLEAVED, not contiguous: wave w of W owns batches w, w + W, w + 2 W, ...
// Live slots are not spread evenly over a pool — a rolling sequence keeps one render in each half of the main slots and
// all its old paths in the survivor area behind them (bf_wavefront.h) — and with contiguous segments the few waves that
// own the busy region did all the work while the others idled; batch-granular interleaving balances any distribution to
// within one batch per wave.  The words are still fetched 64 at a time (lane l reads the wave's (64 k + l)-th batch: a
// strided gather, one 8-byte word per cache line — the masks are a few MB per launch, the state rows GBs).
struct MaskCursor {
    const unsigned long long *masks;
    const unsigned long long *masks2;   // optional: the walk covers masks & masks2 (sel = 1) or masks & ~masks2 (sel = 2)
    uint32_t sel;
    uint32_t b, b_end;          // current batch / number of batches (wave-uniform)
    unsigned long long m;       // unconsumed bits of batch b (wave-uniform)
    uint32_t base, stride;      // this wave's first batch / distance between its batches (the number of waves sharing the array)
    uint32_t k;                 // chunk: lane l holds the word of batch base + (64 k + l) stride
    unsigned long long sub;     // slots of a batch this wave serves (all ones, or a 32- / 16-slot share: the tail's spreading)
    unsigned long long w;       // this lane's word of the chunk, & sub
    unsigned long long nz;      // wave-uniform: chunk words that are non-zero and not consumed yet
    // rotated / complemented walks (every cursor of the kernels is plain at present): the walk covers `b_end` batches starting at
    // physical batch `rot` (wrapping at `mod`), of the complemented words (inv: slots WITHOUT a live path) or — masks == nullptr —
    // of every slot.  Plain cursors: rot = 0, inv = 0, pb == b.
    uint32_t rot, mod, inv, pb;
};
BF_DEV unsigned long long wave_read_u64(unsigned long long v, int src) {
    unsigned lo = (unsigned) __shfl((int) (unsigned) v, src), hi = (unsigned) __shfl((int) (unsigned) (v >> 32), src);
    return ((unsigned long long) hi << 32) | lo;
}
BF_DEV void cursor_fetch(MaskCursor &c, int lane) {
    const uint32_t idx = c.base + (c.k * 64u + (uint32_t) lane) * c.stride;
    uint32_t p = idx + c.rot;
    if (p >= c.mod) p -= c.mod;
    c.w = 0ull;
    if (idx < c.b_end) {
        c.w = c.masks ? c.masks[p] : ~0ull;
        if (c.inv) c.w = ~c.w;
        c.w &= c.sub;
        if (c.sel) c.w &= c.sel == 1u ? c.masks2[p] : ~c.masks2[p];
    }
    c.nz = __ballot(c.w != 0ull);
}
// position the cursor on the wave's next non-empty batch (or at the end)
BF_DEV void cursor_seek(MaskCursor &c, int lane) {
    while (true) {
        if (c.nz) {
            const int j = __ffsll((unsigned long long) c.nz) - 1;
            c.nz &= c.nz - 1ull;
            c.b = c.base + (c.k * 64u + (uint32_t) j) * c.stride;
            c.pb = c.b + c.rot;
            if (c.pb >= c.mod) c.pb -= c.mod;
            c.m = wave_read_u64(c.w, j);
            return;
        }
        ++c.k;
        if (c.base + c.k * 64u * c.stride >= c.b_end) {
            c.b = c.b_end;
            c.m = 0ull;
            return;
        }
        cursor_fetch(c, lane);
    }
}
// `share` (1, 2 or 4): that many consecutive waves serve the same batches, each one its own 64 / share slots of every batch
BF_DEV void cursor_init(MaskCursor &c, const unsigned long long *masks, uint32_t wave_id, uint32_t n_waves, uint32_t n_batches, int lane,
                        uint32_t share = 1u, const unsigned long long *masks2 = nullptr, uint32_t sel = 0u, uint32_t rot = 0u,
                        uint32_t mod = 0xffffffffu, uint32_t inv = 0u) {
    c.rot = rot;
    c.mod = mod;
    c.inv = inv;
    c.pb = 0u;
    c.masks2 = masks2;
    c.sel = masks2 ? sel : 0u;
    c.sub = ~0ull;
    if (share > 1u) {
        const uint32_t width = 64u / share, q = wave_id % share;
        c.sub = ((1ull << width) - 1ull) << (width * q);
        wave_id /= share;
        n_waves = max(1u, n_waves / share);
    }
    c.masks = masks;
    c.b_end = n_batches;
    c.base = wave_id;
    c.stride = n_waves;
    c.k = 0u;
    c.m = 0ull;
    c.w = 0ull;
    c.nz = 0ull;
    if (wave_id >= n_batches) {
        c.b = n_batches;
        return;
    }
    cursor_fetch(c, lane);
    cursor_seek(c, lane);
}
BF_DEV bool cursor_empty(const MaskCursor &c) { return c.b >= c.b_end; }
BF_DEV void cursor_skip_empty(MaskCursor &c, int lane) {
    if (c.b < c.b_end && c.m == 0ull) cursor_seek(c, lane);
}
// Hands out up to `want` slots: the requesting lane of rank r (0-based among the
// requesters) receives a slot iff r < return value.  All control flow is uniform.
BF_DEV uint32_t cursor_take(MaskCursor &c, uint32_t want, bool requesting, uint32_t rank, uint32_t &slot, int lane) {
    uint32_t taken = 0;
    while (taken < want && c.b < c.b_end) {
        if (c.m == 0ull) {
            cursor_seek(c, lane);
            continue;
        }
        uint32_t cnt = (uint32_t) __popcll(c.m);
        uint32_t take = min(want - taken, cnt);
        if (requesting && rank >= taken && rank < taken + take) slot = c.pb * 64u + nth_set_bit(c.m, rank - taken);
        if (take == cnt) {
            c.m = 0ull;
        } else {
            uint32_t p = nth_set_bit(c.m, take - 1u);        // drop the `take` lowest set bits
            c.m &= ~((2ull << p) - 1ull);
        }
        taken += take;
    }
    return taken;
}

BF_NS_END  // namespace bfd
