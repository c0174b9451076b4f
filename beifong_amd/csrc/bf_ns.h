// One set of sources, two builds of the device code (Makefile):
//   exact (default)      : IEEE fp32 division and square root; every path bit-identical to the oracle.
//   BF_FAST = 1          : -fno-hip-fp32-correctly-rounded-divide-sqrt: a / b and sqrt become v_rcp_f32 * a and
//                          v_sqrt_f32 (1 ulp class instead of correctly rounded); launched for BF_FLAG_FAST renders.
// Both objects are linked into one library, so nothing the fast build defines may share a symbol with the exact one: an
// inline template or __host__ __device__ helper of the same mangled name in both would be merged by the linker, and one
// mode would silently run the other's code.  The fast build therefore puts everything into the inline namespace
// bfd::fast (the structs keep their layouts: same source text) and renames its launchers with a _fast suffix.
// What is built how (Makefile): bf_kernels.hip (the one-kernel render and the tail) and bf_wavefront.hip (wf_shade, wf_trace) in
// both modes; bf_geom.hip (the kernels that move geometry), bf_query.hip (ray and plugin queries, probes), bf_build.hip and
// bf_converge.hip once, exact: what they compute is shared by both modes.  bf_launch.h declares every launcher of the first four.
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
