// One set of sources, two builds of the device code (Makefile):
//   exact (default)      : IEEE fp32 division and square root; every path bit-identical to the oracle.
//   BF_FAST = 1          : -fno-hip-fp32-correctly-rounded-divide-sqrt: a / b and sqrt become v_rcp_f32 * a and
//                          v_sqrt_f32 (1 ulp class instead of correctly rounded); launched for BF_FLAG_FAST renders.
// Both objects are linked into one library, so nothing the fast build defines may share a symbol with the exact one: an
// inline template or __host__ __device__ helper of the same mangled name in both would be merged by the linker, and one
// mode would silently run the other's code.  The fast build therefore puts everything into the inline namespace
// bfd::fast (the structs keep their layouts: same source text) and renames its launchers with a _fast suffix.
#pragma once

#ifndef BF_FAST
#define BF_FAST 0
#endif

#if BF_FAST
#define BF_NS_BEGIN namespace bfd { inline namespace fast {
#define BF_NS_END } }
#define BF_LAUNCHER(name) name##_fast
#else
#define BF_NS_BEGIN namespace bfd {
#define BF_NS_END }
#define BF_LAUNCHER(name) name
#endif
