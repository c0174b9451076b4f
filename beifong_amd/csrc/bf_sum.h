// The exact accumulator behind BF_FLAG_EXACT_SUM (include/beifong_hip.h): all of its arithmetic, in plain C++ with no HIP
// in it, so that the device kernels (bf_film.h, bf_sum.hip), the host entry bf_exact_sum_host (bf_api.cpp) and a host-only test
// program (tests/native/sum_check.cpp) compile the same text.
//
// A cell is a signed fixed-point integer whose bit i weighs 2^(i - 149).  A finite fp32 x is (-1)^s M 2^(shift - 149) with M < 2^24
// and shift = max(biased exponent, 1) - 1 in [0, 253], so every fp32 addend is an integer in that scale and integer addition, which
// is associative, gives the exact sum in any order.  The cell is kept as nine signed 64-bit limbs 32 bits apart (limb k weighs
// 2^(32 k - 149)): v = M << (shift & 31) is below 2^55, its low 32 bits go to limb shift >> 5 and the rest to the next limb, both
// negated for a negative x.  One addend gives a limb at most one piece below 2^32, so a limb holds the pieces of any N < 2^31 addends
// without overflow; the limbs are independent integers, so each piece may be added by a relaxed atomic, in LDS or in global memory, and
// LDS limbs may be added to global limbs limb by limb.  resolve() carry-propagates to sign and magnitude and rounds ONCE, to
// nearest-even: the cell's value is fl(sum of its addends).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BF_SUM_HD __host__ __device__ __forceinline__
#else
#define BF_SUM_HD inline
#endif

namespace bfs {
constexpr int kLimbs = 9;            // int64 limbs of a cell: 72 bytes
constexpr int kCellFloats = 18;      // ... which is this many floats where a launch counts its LDS in floats (DLaunch::lds_floats)
constexpr uint64_t kMaxAddends = 1ull << 31;      // a cell is exact for fewer addends than this

// the (at most two) pieces of an fp32 addend: `lo` to limb `limb`, `hi` to limb `limb + 1`; a zero piece need not be added.
// Any bit pattern gives limb <= 7 (a non-finite one has no meaning as an addend, but stays inside the cell)
struct Pieces {
    uint32_t limb;
    int64_t lo, hi;
};
BF_SUM_HD Pieces split(uint32_t bits) {
    const uint32_t e = (bits >> 23) & 0xffu, f = bits & 0x7fffffu;
    const uint64_t M = e ? (uint64_t) (f | 0x800000u) : (uint64_t) f;
    const uint32_t shift = (e ? e : 1u) - 1u;
    const uint64_t v = M << (shift & 31u);
    Pieces p;
    p.limb = shift >> 5;
    p.lo = (int64_t) (v & 0xffffffffull);
    p.hi = (int64_t) (v >> 32);
    if (bits >> 31) {
        p.lo = -p.lo;
        p.hi = -p.hi;
    }
    return p;
}
BF_SUM_HD bool finite_bits(uint32_t bits) { return ((bits >> 23) & 0xffu) != 0xffu; }

// one addend into a cell nobody else writes (the host entry; the resolve kernel's own copy of a cell)
BF_SUM_HD void add(int64_t *cell, uint32_t bits) {
    const Pieces p = split(bits);
    if (p.lo) cell[p.limb] += p.lo;
    if (p.hi) cell[p.limb + 1u] += p.hi;
}

// limbs -> digits: limbs 0-7 in [0, 2^32), the sign and everything above in limb 8.  |limb| < 2^63 - 2^32 on entry (N < 2^31 pieces
// below 2^32), so limb + carry cannot overflow
BF_SUM_HD void normalize(int64_t *cell) {
    int64_t carry = 0;
    for (int i = 0; i < kLimbs - 1; ++i) {
        const int64_t t = cell[i] + carry;
        cell[i] = t & 0xffffffffll;
        carry = t >> 32;      // arithmetic: floor
    }
    cell[kLimbs - 1] += carry;
}

struct Resolved {
    uint32_t bits;      // fl(sum) as an fp32 bit pattern; an exact zero is +0.0
    bool empty;         // every limb is zero: the cell received no non-zero addend, or its addends cancelled limb by limb
};
// Round a cell to fp32, nearest-even; the cell is left normalised to the magnitude's digits.  Subnormal results are kept (no flush); a
// magnitude at or above 2^128 - 2^103 is +-inf.  (`empty` is as close as nine limbs come to "received no addend": zero pieces are
// never added, and a cell whose addends cancel in every limb is indistinguishable from an untouched one; both resolve to +0.0.)
BF_SUM_HD Resolved resolve(int64_t *cell) {
    Resolved r;
    r.bits = 0u;
    int64_t any = 0;
    for (int i = 0; i < kLimbs; ++i) any |= cell[i];
    r.empty = any == 0;
    if (r.empty) return r;
    normalize(cell);
    const bool neg = cell[kLimbs - 1] < 0;
    if (neg) {
        for (int i = 0; i < kLimbs; ++i) cell[i] = -cell[i];
        normalize(cell);
    }
    // ten 32-bit digits of the magnitude (limb 8 stays below 2^54: at most 2^31 high pieces below 2^23 each)
    uint32_t d[kLimbs + 2];
    for (int i = 0; i < kLimbs - 1; ++i) d[i] = (uint32_t) cell[i];
    d[kLimbs - 1] = (uint32_t) ((uint64_t) cell[kLimbs - 1] & 0xffffffffull);
    d[kLimbs] = (uint32_t) ((uint64_t) cell[kLimbs - 1] >> 32);
    d[kLimbs + 1] = 0u;      // (so that a 64-bit window may start at the top digit)
    int top = -1;             // index of the highest set bit
    for (int i = kLimbs; i >= 0; --i)
        if (d[i]) {
            top = 32 * i + 31 - __builtin_clz(d[i]);
            break;
        }
    if (top < 0) return r;      // the addends cancelled: +0.0
    uint32_t bits;
    if (top <= 23) {
        bits = d[0];            // below 2^24 units of 2^-149: subnormals and the first binade are their own bit patterns
    } else {
        const int sh = top - 23;      // the 24-bit mantissa is bits [sh, sh + 24)
        const uint64_t win = (uint64_t) d[sh >> 5] | ((uint64_t) d[(sh >> 5) + 1] << 32);
        uint32_t m = (uint32_t) (win >> (sh & 31)) & 0xffffffu;
        const int g = sh - 1;         // the guard bit; everything below it is sticky
        const bool guard = (d[g >> 5] >> (g & 31)) & 1u;
        uint32_t sticky = d[g >> 5] & ((1u << (g & 31)) - 1u);
        for (int i = 0; i < (g >> 5); ++i) sticky |= d[i];
        if (guard && (sticky || (m & 1u))) ++m;
        // biased exponent sh + 1 with the implicit bit inside m: a mantissa that rounds up to 2^24 carries into the exponent
        const uint64_t b = ((uint64_t) (uint32_t) sh << 23) + m;
        bits = b >= 0x7f800000ull ? 0x7f800000u : (uint32_t) b;
    }
    r.bits = bits | (neg ? 0x80000000u : 0u);
    return r;
}
}  // namespace bfs
