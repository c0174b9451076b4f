// Device-side BVH builder (bf_build.hip): bf_scene_rebuild_bvh's rebuild of both trees over the triangle rows a handle
// renders now.  Same heuristic as the host builder (bf_bvh.cpp), level-synchronous, deterministic.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

struct bfk_build_in {
    const float4 *tris;        // posed rows, kTriStride float4 per slot (device)
    uint32_t n_tris;
    float origin_scale;        // the bound on ray origins the boxes are padded for (bf_bvh.h)
    int want_wide;             // also produce the sixteen-wide tree
    hipStream_t stream;
};

struct bfk_build_out {
    // fresh device allocations, the caller's to free: nodes [n_nodes] Node4 (nullptr if none), wnodes [n_wnodes + 1] Node16
    // (the padding node zeroed; nullptr unless want_wide), order [n_tris]: new slot p holds old slot order[p]
    float4 *nodes, *wnodes;
    uint32_t *order;
    uint32_t n_nodes, n_wnodes;
    int32_t root, wroot;
    uint32_t stack4, depth4, stack16, depth16, depth2;
    float lo[3], hi[3];        // unpadded bounds of all triangles
};

// status: 0 ok, 1 out of memory, 2 device error, 3 a depth / stack bound is not met; `err` gets the text
extern "C" int bfk_build_bvh(const bfk_build_in *in, bfk_build_out *out, char *err, size_t err_len);
// dst[rows * p + r] = src[rows * order[p] + r] for p < n (float4 rows; uint4 tables alike)
extern "C" hipError_t bfk_build_gather(const uint32_t *order, uint32_t n, const float4 *src, float4 *dst, uint32_t rows, hipStream_t stream);
// test hook: the n-th device allocation of the next builds fails (0: off)
extern "C" void bfk_build_fail_alloc(int nth);
