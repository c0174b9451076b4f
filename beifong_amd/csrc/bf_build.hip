// Device-side binned-SAH BVH builder for gfx950 (bf_scene_rebuild_bvh).
//
// The heuristic is the host builder's (bf_bvh.cpp): 16 centroid bins per axis, leaves of at most kMaxLeaf triangles, binary
// depth at most kMaxDepth, boxes padded by 2e-6 max(extent, |lo|, |hi|) + 2e-7 origin_scale + 1e-30.  Three things DIFFER from
// the host builder, none of them in what a traversal returns: (1) a node whose remaining depth budget only fits a balanced
// subtree is cut in the middle of its triangle ORDER (Morton order, kept by the stable partitions), where the host cuts at the
// centroid median of the widest axis (nth_element); the same cut serves a node whose centroids all coincide, as on the host;
// (2) within a leaf and between equal-cost splits the order is the Morton order's, not std::partition's; (3) the four-wide
// nodes are breadth-first throughout, the host's only in their first kTopNodes.  The SAH cost is evaluated as the host does,
// product by product: the file is compiled with -ffp-contract=off like the rest of the library.  The build is level-synchronous:
//
//   prepare   per-triangle boxes, scene bounds; the triangles sorted by (30-bit Morton code of the centroid, primitive word)
//             (hipCUB radix sort), so the start order — hence every "cut in the middle" — is a function of the triangle SET
//   per level bounds of the level's nodes, 3 x 16 bins per node, the SAH sweep, the children, and a STABLE partition of every
//             node's index range by one exclusive scan over the left flags (hipCUB) — no atomics on positions
//   collapse  four-wide (Node4, breadth-first, so the first kTopNodes nodes are the top levels) and sixteen-wide (Node16)
//             nodes from the binary tree, level by level, child slots assigned by scans
//
// Two paths per level: a node of more than kSmall triangles is binned by one thread per triangle (a workgroup whose 256
// triangles all lie in one node keeps the node's histogram in LDS and flushes it once; a mixed one adds to the global bins),
// then evaluated by one wave; a node of at most kSmall triangles is bounded, binned and evaluated by one wave on its own,
// triangle j in lane j (the deep levels: hundreds of thousands of tiny nodes).
// Minima, maxima and counts are order-independent, the positions come from scans: the tree is a pure function of the rows,
// and a rebuild of rebuilt rows reproduces the arrays byte for byte.
//
// The split rule, the adoption rule and the padding are restated in numpy by tests/sah_ref.py, which recovers the binary tree from
// the four-wide arrays and holds every node of it to them (tests/test_gpu_build_splits.py; the host builder: tests/test_sah_ref_host.py).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bf_build.h"
#include "bf_bvh.h"
#include "bf_device.h"

namespace bfb {

using bf::kEmptyChild;
using bf::kMaxDepth;
using bf::kMaxLeaf;
constexpr uint32_t kTriStride = bfd::kTriStride;
constexpr uint32_t kSmall = 64;           // a node of at most this many triangles is one wave's
constexpr uint32_t kNone = 0xffffffffu;
constexpr int kBins = 16;
constexpr uint32_t kBinWords = 8;         // lo.xyz, hi.xyz (ordered), count, unused
#define BFB_INF __builtin_inff()

// order-preserving map of a float onto an unsigned integer: atomicMin / atomicMax on it are the float's
__device__ inline uint32_t f2o(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float o2f(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }
#define BFB_OMIN 0xff800000u      // f2o(+inf): neutral of a minimum
#define BFB_OMAX 0x007fffffu      // f2o(-inf): neutral of a maximum

// internal node of the binary tree (more than kMaxLeaf triangles), in breadth-first order
struct BNode {
    uint32_t first, count, depth, bin;      // bin: the node's block of the level's bin scratch (more than kSmall triangles)
    uint32_t b[12];                         // ordered: triangle bounds lo.xyz, hi.xyz, centroid bounds lo.xyz, hi.xyz
    int32_t child[2];                       // bf_bvh.h: Node::child
    uint32_t mode, axis, best_bin, nleft;   // mode 0: bins <= best_bin of `axis` go left; 1: the first nleft of the order
    uint32_t pad[2];
};
static_assert(sizeof(BNode) == 96, "BNode");

__device__ inline float sel3(float x, float y, float z, int a) { return a == 0 ? x : (a == 1 ? y : z); }
__device__ inline int bin_of(float c, float lo, float scale) { return min(kBins - 1, max(0, (int) ((c - lo) * scale))); }
__device__ inline bool force_median(uint32_t depth, uint32_t count) {
    uint32_t need = 0;
    while (((uint32_t) kMaxLeaf << need) < count) ++need;
    return depth + need + 1 >= (uint32_t) kMaxDepth;
}
__device__ inline float half_area(const float *lo, const float *hi) {
    const float d0 = hi[0] - lo[0], d1 = hi[1] - lo[1], d2 = hi[2] - lo[2];
    if (d0 < 0 || d1 < 0 || d2 < 0) return 0.f;
    return d0 * d1 + d1 * d2 + d2 * d0;
}
// all-lanes reduction of twelve ordered words (minima at 0..2 and 6..8, maxima at 3..5 and 9..11)
__device__ inline void wave_reduce12(uint32_t *v) {
    for (int m = 32; m > 0; m >>= 1)
        for (int k = 0; k < 12; ++k) {
            const uint32_t o = (uint32_t) __shfl_xor((int) v[k], m);
            v[k] = ((k % 6) < 3) ? min(v[k], o) : max(v[k], o);
        }
}

// ---- prepare ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prep_kernel(const float4 *__restrict__ tris, uint32_t n, float4 *__restrict__ tlo, float4 *__restrict__ thi,
                                                   uint32_t *__restrict__ prim, uint32_t *__restrict__ all) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t v[12] = {BFB_OMIN, BFB_OMIN, BFB_OMIN, BFB_OMAX, BFB_OMAX, BFB_OMAX, BFB_OMIN, BFB_OMIN, BFB_OMIN, BFB_OMAX, BFB_OMAX, BFB_OMAX};
    if (i < n) {
        const float4 a = tris[kTriStride * i], b = tris[kTriStride * i + 1], c = tris[kTriStride * i + 2];
        const float lo[3] = {fminf(a.x, fminf(b.x, c.x)), fminf(a.y, fminf(b.y, c.y)), fminf(a.z, fminf(b.z, c.z))};
        const float hi[3] = {fmaxf(a.x, fmaxf(b.x, c.x)), fmaxf(a.y, fmaxf(b.y, c.y)), fmaxf(a.z, fmaxf(b.z, c.z))};
        tlo[i] = make_float4(lo[0], lo[1], lo[2], 0.f);
        thi[i] = make_float4(hi[0], hi[1], hi[2], 0.f);
        prim[i] = __float_as_uint(a.w);
        for (int k = 0; k < 3; ++k) {
            const float ce = 0.5f * (lo[k] + hi[k]);
            v[k] = f2o(lo[k]), v[3 + k] = f2o(hi[k]), v[6 + k] = f2o(ce), v[9 + k] = f2o(ce);
        }
    }
    wave_reduce12(v);
    if ((threadIdx.x & 63u) == 0u)
        for (int k = 0; k < 12; ++k) {
            if ((k % 6) < 3) atomicMin(&all[k], v[k]);
            else atomicMax(&all[k], v[k]);
        }
}

__device__ inline uint32_t spread10(uint32_t x) {
    x &= 0x3ffu;
    x = (x | (x << 16)) & 0x030000ffu;
    x = (x | (x << 8)) & 0x0300f00fu;
    x = (x | (x << 4)) & 0x030c30c3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}
__global__ __launch_bounds__(256) void key_kernel(const float4 *__restrict__ tlo, const float4 *__restrict__ thi, const uint32_t *__restrict__ prim,
                                                  uint32_t n, const uint32_t *__restrict__ all, unsigned long long *__restrict__ keys,
                                                  uint32_t *__restrict__ vals) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 a = tlo[i], b = thi[i];
    const float c[3] = {0.5f * (a.x + b.x), 0.5f * (a.y + b.y), 0.5f * (a.z + b.z)};
    uint32_t q[3];
    for (int k = 0; k < 3; ++k) {
        const float lo = o2f(all[6 + k]), ext = o2f(all[9 + k]) - lo;
        q[k] = ext > 0.f ? (uint32_t) min(1023, max(0, (int) ((c[k] - lo) * (1024.f / ext)))) : 0u;
    }
    const uint32_t code = (spread10(q[0]) << 2) | (spread10(q[1]) << 1) | spread10(q[2]);
    keys[i] = ((unsigned long long) code << 32) | prim[i];
    vals[i] = i;
}

__global__ void root_kernel(BNode *nodes, uint32_t n, uint32_t *pos_node) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) pos_node[i] = 0u;
    if (i == 0) {
        BNode r;
        r.first = 0, r.count = n, r.depth = 0, r.bin = n > kSmall ? 0u : kNone;
        for (int k = 0; k < 12; ++k) r.b[k] = (k % 6) < 3 ? BFB_OMIN : BFB_OMAX;
        r.child[0] = r.child[1] = kEmptyChild;
        r.mode = r.axis = r.best_bin = r.nleft = 0;
        r.pad[0] = r.pad[1] = 0;
        nodes[0] = r;
    }
}

// ---- one level ----------------------------------------------------------------------------------------------------------------
__global__ void bins_init_kernel(uint32_t *bins, uint32_t n_words) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_words) return;
    const uint32_t k = i % kBinWords;
    bins[i] = k < 3 ? BFB_OMIN : (k < 6 ? BFB_OMAX : 0u);
}

// bounds of the level's large nodes: one thread per triangle position; a wave inside one node reduces before it adds
__global__ __launch_bounds__(256) void bounds_large_kernel(BNode *nodes, const uint32_t *__restrict__ pos_node, const uint32_t *__restrict__ idx,
                                                           const float4 *__restrict__ tlo, const float4 *__restrict__ thi, uint32_t n) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    uint32_t nd = p < n ? pos_node[p] : kNone;
    if (nd != kNone && nodes[nd].count <= kSmall) nd = kNone;
    uint32_t v[12] = {BFB_OMIN, BFB_OMIN, BFB_OMIN, BFB_OMAX, BFB_OMAX, BFB_OMAX, BFB_OMIN, BFB_OMIN, BFB_OMIN, BFB_OMAX, BFB_OMAX, BFB_OMAX};
    if (nd != kNone) {
        const uint32_t t = idx[p];
        const float4 a = tlo[t], b = thi[t];
        const float lo[3] = {a.x, a.y, a.z}, hi[3] = {b.x, b.y, b.z};
        for (int k = 0; k < 3; ++k) {
            const float ce = 0.5f * (lo[k] + hi[k]);
            v[k] = f2o(lo[k]), v[3 + k] = f2o(hi[k]), v[6 + k] = f2o(ce), v[9 + k] = f2o(ce);
        }
    }
    const uint32_t first_nd = (uint32_t) __shfl((int) nd, 0);
    const bool uniform = __all(nd == first_nd);
    if (uniform) {
        if (first_nd == kNone) return;
        wave_reduce12(v);
        if ((threadIdx.x & 63u) != 0u) return;
    } else if (nd == kNone) {
        return;
    }
    uint32_t *dst = nodes[nd].b;
    for (int k = 0; k < 12; ++k) {
        if ((k % 6) < 3) atomicMin(&dst[k], v[k]);
        else atomicMax(&dst[k], v[k]);
    }
}

// bins of the level's large nodes: one thread per triangle position
__global__ __launch_bounds__(256) void bin_large_kernel(const BNode *__restrict__ nodes, const uint32_t *__restrict__ pos_node,
                                                        const uint32_t *__restrict__ idx, const float4 *__restrict__ tlo,
                                                        const float4 *__restrict__ thi, uint32_t n, uint32_t *bins) {
    __shared__ uint32_t hist[3 * kBins * kBinWords];
    __shared__ uint32_t s_first, s_last;
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    uint32_t nd = p < n ? pos_node[p] : kNone;
    if (threadIdx.x == 0) s_first = nd;
    if (threadIdx.x == 255) s_last = nd;
    for (uint32_t i = threadIdx.x; i < 3 * kBins * kBinWords; i += 256u) {
        const uint32_t k = i % kBinWords;
        hist[i] = k < 3 ? BFB_OMIN : (k < 6 ? BFB_OMAX : 0u);
    }
    __syncthreads();
    // positions of a node are contiguous: the workgroup lies in one node iff its first and last positions do
    const bool block_uniform = s_first != kNone && s_first == s_last;
    bool act = nd != kNone;
    uint32_t bin_block = 0;
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, clo[3] = {0, 0, 0}, ext[3] = {0, 0, 0};
    if (act) {
        const BNode &N = nodes[nd];
        act = N.count > kSmall && !force_median(N.depth, N.count);
        bin_block = N.bin;
        for (int k = 0; k < 3; ++k) clo[k] = o2f(N.b[6 + k]), ext[k] = o2f(N.b[9 + k]) - clo[k];
    }
    if (act) {
        const uint32_t t = idx[p];
        const float4 a = tlo[t], b = thi[t];
        lo[0] = a.x, lo[1] = a.y, lo[2] = a.z, hi[0] = b.x, hi[1] = b.y, hi[2] = b.z;
        for (int ax = 0; ax < 3; ++ax) {
            if (!(ext[ax] > 0.f)) continue;
            const int bi = bin_of(0.5f * (lo[ax] + hi[ax]), clo[ax], (float) kBins / ext[ax]);
            uint32_t *h = block_uniform ? &hist[(ax * kBins + bi) * kBinWords] : &bins[((size_t) bin_block * 3 * kBins + ax * kBins + bi) * kBinWords];
            for (int k = 0; k < 3; ++k) {
                atomicMin(&h[k], f2o(lo[k]));
                atomicMax(&h[3 + k], f2o(hi[k]));
            }
            atomicAdd(&h[6], 1u);
        }
    }
    if (!block_uniform) return;
    __syncthreads();
    const BNode &N = nodes[s_first];
    if (N.count <= kSmall || force_median(N.depth, N.count)) return;
    uint32_t *g = &bins[(size_t) N.bin * 3 * kBins * kBinWords];
    for (uint32_t i = threadIdx.x; i < 3 * kBins * kBinWords; i += 256u) {
        const uint32_t k = i % kBinWords;
        if (k > 6 || hist[(i / kBinWords) * kBinWords + 6] == 0u) continue;
        if (k < 3) atomicMin(&g[i], hist[i]);
        else if (k < 6) atomicMax(&g[i], hist[i]);
        else atomicAdd(&g[i], hist[i]);
    }
}

// one wave per node of the level: bounds and bins of a small node, the SAH sweep over 3 x 16 bins (lane = 16 axis + bin), the
// split and which children are internal
__global__ __launch_bounds__(256) void eval_kernel(BNode *nodes, uint32_t lb, uint32_t n_level, const uint32_t *__restrict__ idx,
                                                   const float4 *__restrict__ tlo, const float4 *__restrict__ thi, const uint32_t *__restrict__ bins,
                                                   uint32_t *__restrict__ flags) {
    const uint32_t w = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (w >= n_level) return;
    BNode &N = nodes[lb + w];
    const uint32_t first = N.first, count = N.count, depth = N.depth;
    const bool force = force_median(depth, count);
    const int ax = min((int) (lane >> 4), 2), bb = (int) (lane & 15u);
    const bool bin_lane = lane < 48u;
    float blo[3] = {BFB_INF, BFB_INF, BFB_INF}, bhi[3] = {-BFB_INF, -BFB_INF, -BFB_INF};
    uint32_t bcnt = 0;
    uint32_t nb[12];
    if (count <= kSmall) {
        float lo[3] = {BFB_INF, BFB_INF, BFB_INF}, hi[3] = {-BFB_INF, -BFB_INF, -BFB_INF}, ce[3] = {0, 0, 0};
        const bool act = lane < count;
        if (act) {
            const uint32_t t = idx[first + lane];
            const float4 a = tlo[t], b = thi[t];
            lo[0] = a.x, lo[1] = a.y, lo[2] = a.z, hi[0] = b.x, hi[1] = b.y, hi[2] = b.z;
            for (int k = 0; k < 3; ++k) ce[k] = 0.5f * (lo[k] + hi[k]);
        }
        for (int k = 0; k < 3; ++k) {
            nb[k] = f2o(lo[k]), nb[3 + k] = f2o(hi[k]);
            nb[6 + k] = act ? f2o(ce[k]) : BFB_OMIN, nb[9 + k] = act ? f2o(ce[k]) : BFB_OMAX;
        }
        wave_reduce12(nb);
        if (lane == 0)
            for (int k = 0; k < 12; ++k) N.b[k] = nb[k];
        const float mlo = o2f(nb[6 + ax]), mext = o2f(nb[9 + ax]) - mlo;
        const bool binning = bin_lane && !force && mext > 0.f;
        const float scale = (float) kBins / mext;
        for (uint32_t j = 0; j < count; ++j) {
            const float cx = __shfl(ce[0], (int) j), cy = __shfl(ce[1], (int) j), cz = __shfl(ce[2], (int) j);
            const float l0 = __shfl(lo[0], (int) j), l1 = __shfl(lo[1], (int) j), l2 = __shfl(lo[2], (int) j);
            const float h0 = __shfl(hi[0], (int) j), h1 = __shfl(hi[1], (int) j), h2 = __shfl(hi[2], (int) j);
            if (binning && bin_of(sel3(cx, cy, cz, ax), mlo, scale) == bb) {
                blo[0] = fminf(blo[0], l0), blo[1] = fminf(blo[1], l1), blo[2] = fminf(blo[2], l2);
                bhi[0] = fmaxf(bhi[0], h0), bhi[1] = fmaxf(bhi[1], h1), bhi[2] = fmaxf(bhi[2], h2);
                ++bcnt;
            }
        }
    } else {
        for (int k = 0; k < 12; ++k) nb[k] = N.b[k];
        if (bin_lane && !force) {
            const uint32_t *g = &bins[((size_t) N.bin * 3 * kBins + lane) * kBinWords];
            for (int k = 0; k < 3; ++k) blo[k] = o2f(g[k]), bhi[k] = o2f(g[3 + k]);
            bcnt = g[6];
        }
    }
    // the sweep: lane (axis, b) weighs the split "bins 0..b left"
    float Llo[3] = {BFB_INF, BFB_INF, BFB_INF}, Lhi[3] = {-BFB_INF, -BFB_INF, -BFB_INF};
    float Rlo[3] = {BFB_INF, BFB_INF, BFB_INF}, Rhi[3] = {-BFB_INF, -BFB_INF, -BFB_INF};
    uint32_t Lc = 0, Rc = 0;
    for (int k = 0; k < kBins; ++k) {
        const int src = (int) (lane & 48u) | k;
        float vlo[3], vhi[3];
        for (int a = 0; a < 3; ++a) vlo[a] = __shfl(blo[a], src), vhi[a] = __shfl(bhi[a], src);
        const uint32_t vc = (uint32_t) __shfl((int) bcnt, src);
        if (vc == 0u) continue;
        if (k <= bb) {
            for (int a = 0; a < 3; ++a) Llo[a] = fminf(Llo[a], vlo[a]), Lhi[a] = fmaxf(Lhi[a], vhi[a]);
            Lc += vc;
        } else {
            for (int a = 0; a < 3; ++a) Rlo[a] = fminf(Rlo[a], vlo[a]), Rhi[a] = fmaxf(Rhi[a], vhi[a]);
            Rc += vc;
        }
    }
    float cost = BFB_INF;
    if (bin_lane && bb < kBins - 1 && Lc > 0u && Rc > 0u) cost = half_area(Llo, Lhi) * (float) Lc + half_area(Rlo, Rhi) * (float) Rc;
    int best = (int) lane;
    for (int m = 32; m > 0; m >>= 1) {
        const float oc = __shfl_xor(cost, m);
        const int ol = __shfl_xor(best, m);
        if (oc < cost || (oc == cost && ol < best)) cost = oc, best = ol;
    }
    const bool sah = cost < BFB_INF;      // (the host's rule: the first strictly smaller cost, axes then bins in order)
    const uint32_t nleft = sah ? (uint32_t) __shfl((int) Lc, best) : count / 2u;
    if (lane == 0) {
        N.mode = sah ? 0u : 1u;
        N.axis = sah ? (uint32_t) (best >> 4) : 0u;
        N.best_bin = sah ? (uint32_t) (best & 15) : 0u;
        N.nleft = nleft;
        flags[2u * w] = nleft > (uint32_t) kMaxLeaf ? 1u : 0u;
        flags[2u * w + 1u] = count - nleft > (uint32_t) kMaxLeaf ? 1u : 0u;
    }
}

// the level's children: internal ones become the next level's nodes at le + (their rank among the level's internal children)
__global__ void children_kernel(BNode *nodes, uint32_t lb, uint32_t n_level, uint32_t le, uint32_t cap, const uint32_t *__restrict__ flags,
                                const uint32_t *__restrict__ scan, uint32_t *ctr) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_level) return;
    BNode &N = nodes[lb + i];
    for (uint32_t k = 0; k < 2u; ++k) {
        const uint32_t f = k ? N.first + N.nleft : N.first, c = k ? N.count - N.nleft : N.nleft;
        if (flags[2u * i + k]) {
            const uint32_t ci = le + scan[2u * i + k];
            if (ci >= cap) {
                ctr[2] = 1u;
                N.child[k] = kEmptyChild;
                continue;
            }
            BNode r;
            r.first = f, r.count = c, r.depth = N.depth + 1u;
            r.bin = c > kSmall ? atomicAdd(&ctr[0], 1u) : kNone;      // (which scratch block: no effect on the result)
            for (int q = 0; q < 12; ++q) r.b[q] = (q % 6) < 3 ? BFB_OMIN : BFB_OMAX;
            r.child[0] = r.child[1] = kEmptyChild;
            r.mode = r.axis = r.best_bin = r.nleft = 0;
            r.pad[0] = r.pad[1] = 0;
            nodes[ci] = r;
            N.child[k] = (int32_t) ci;
        } else {
            N.child[k] = ~(int32_t) ((f << 3) | (c - 1u));
        }
    }
    if (i == n_level - 1u) ctr[1] = scan[2u * i + 1u] + flags[2u * i + 1u];
}

__global__ __launch_bounds__(256) void flag_kernel(const BNode *__restrict__ nodes, const uint32_t *__restrict__ pos_node, const uint32_t *__restrict__ idx,
                                                   const float4 *__restrict__ tlo, const float4 *__restrict__ thi, uint32_t n, uint32_t lb,
                                                   uint32_t *__restrict__ flags) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const uint32_t nd = pos_node[p];
    uint32_t left = 0;
    if (nd != kNone && nd >= lb) {
        const BNode &N = nodes[nd];
        if (N.mode == 0u) {
            const uint32_t t = idx[p];
            const float4 a = tlo[t], b = thi[t];
            const int ax = (int) N.axis;
            const float lo = o2f(N.b[6 + ax]), ext = o2f(N.b[9 + ax]) - lo;
            left = bin_of(0.5f * (sel3(a.x, a.y, a.z, ax) + sel3(b.x, b.y, b.z, ax)), lo, (float) kBins / ext) <= (int) N.best_bin ? 1u : 0u;
        } else {
            left = p - N.first < N.nleft ? 1u : 0u;
        }
    }
    flags[p] = left;
}

// the stable partition: a triangle keeps its rank among those of its node that go the same way (scan = exclusive sum of flags)
__global__ __launch_bounds__(256) void scatter_kernel(const BNode *__restrict__ nodes, const uint32_t *__restrict__ pos_node,
                                                      const uint32_t *__restrict__ idx, const uint32_t *__restrict__ flags,
                                                      const uint32_t *__restrict__ scan, uint32_t n, uint32_t *__restrict__ idx_out,
                                                      uint32_t *__restrict__ pos_node_out) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const uint32_t nd = pos_node[p];
    if (nd == kNone) {
        idx_out[p] = idx[p];
        pos_node_out[p] = kNone;
        return;
    }
    const BNode &N = nodes[nd];
    const uint32_t lrank = scan[p] - scan[N.first], k = flags[p] ? 0u : 1u;
    uint32_t q = k ? N.first + N.nleft + ((p - N.first) - lrank) : N.first + lrank;
    if (q >= n) q = p;      // (cannot happen: the left count is the bins' own)
    idx_out[q] = idx[p];
    pos_node_out[q] = N.child[k] >= 0 ? (uint32_t) N.child[k] : kNone;
}

// ---- collapse -----------------------------------------------------------------------------------------------------------------
// the padded box of every child record of the binary tree (record 2 i + k = child k of node i): two float4,
// (lo.xyz, hi.x), (hi.y, hi.z, reference, surface measure as collapse_bvh4 / collapse_bvh16 compare it)
__global__ __launch_bounds__(256) void cbox_kernel(const BNode *__restrict__ nodes, uint32_t n_nodes, const uint32_t *__restrict__ idx,
                                                   const float4 *__restrict__ tlo, const float4 *__restrict__ thi, float abs_pad, float4 *__restrict__ cb,
                                                   uint32_t *ctr) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= 2u * n_nodes) return;
    const BNode &N = nodes[r >> 1];
    const int32_t ref = N.child[r & 1u];
    float lo[3] = {BFB_INF, BFB_INF, BFB_INF}, hi[3] = {-BFB_INF, -BFB_INF, -BFB_INF};
    if (ref >= 0) {
        for (int k = 0; k < 3; ++k) lo[k] = o2f(nodes[ref].b[k]), hi[k] = o2f(nodes[ref].b[3 + k]);
    } else {
        const uint32_t enc = ~(uint32_t) ref, f = enc >> 3, c = (enc & 7u) + 1u;
        for (uint32_t j = 0; j < c; ++j) {
            const uint32_t t = idx[f + j];
            const float4 a = tlo[t], b = thi[t];
            lo[0] = fminf(lo[0], a.x), lo[1] = fminf(lo[1], a.y), lo[2] = fminf(lo[2], a.z);
            hi[0] = fmaxf(hi[0], b.x), hi[1] = fmaxf(hi[1], b.y), hi[2] = fmaxf(hi[2], b.z);
        }
    }
    float m = 0.f;
    for (int k = 0; k < 3; ++k) m = fmaxf(m, fmaxf(hi[k] - lo[k], fmaxf(fabsf(lo[k]), fabsf(hi[k]))));
    const float e = 2e-6f * m + abs_pad + 1e-30f;
    for (int k = 0; k < 3; ++k) lo[k] -= e, hi[k] += e;
    const float d0 = hi[0] - lo[0], d1 = hi[1] - lo[1], d2 = hi[2] - lo[2];
    cb[2u * r] = make_float4(lo[0], lo[1], lo[2], hi[0]);
    cb[2u * r + 1u] = make_float4(hi[1], hi[2], __int_as_float(ref), d0 * d1 + d1 * d2 + d2 * d0);
    if ((r & 1u) == 0u && N.count > bf::kWideLeaf) atomicAdd(&ctr[4], 1u);      // how many sixteen-wide nodes there can be
    if (N.depth + 1u > (uint32_t) kMaxDepth) ctr[2] = 2u;
    if ((r & 1u) == 0u) atomicMax(&ctr[5], N.depth + 1u);                       // binary depth: the deepest leaf's
}

// one level of the W-wide collapse, step 1: the node at out index qb + j adopts grandchildren, largest surface first, and writes
// its boxes; a child that stays internal leaves its BINARY index in the reference word and a 1 in flags
template <int W> __device__ inline bool expandable(const BNode *nodes, int32_t ref) {
    return W == 4 ? ref >= 0 : (ref >= 0 && nodes[ref].count > bf::kWideLeaf);
}
template <int W>
__global__ __launch_bounds__(256) void collapse_a_kernel(const BNode *__restrict__ nodes, const float4 *__restrict__ cb, const uint32_t *__restrict__ fr,
                                                         uint32_t qb, uint32_t n_level, float *__restrict__ out, uint32_t *__restrict__ flags,
                                                         const uint32_t *__restrict__ need_in, uint32_t *__restrict__ acc, uint32_t *ctr) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_level) return;
    const uint32_t g = qb + j, b = fr[g];
    uint32_t rec[W];
    int n = 2;
    rec[0] = 2u * b, rec[1] = 2u * b + 1u;
    while (n < W) {
        int best = -1;
        float best_area = -1.f;
        for (int i = 0; i < n; ++i) {
            const float4 q = cb[2u * rec[i] + 1u];
            if (expandable<W>(nodes, __float_as_int(q.z)) && q.w > best_area) best_area = q.w, best = i;
        }
        if (best < 0) break;
        const uint32_t r = (uint32_t) __float_as_int(cb[2u * rec[best] + 1u].z);
        rec[best] = 2u * r;
        rec[n++] = 2u * r + 1u;
    }
    for (int i = 0; i < W; ++i) {
        const bool used = i < n;
        float4 a = make_float4(BFB_INF, BFB_INF, BFB_INF, -BFB_INF), q = make_float4(-BFB_INF, -BFB_INF, __int_as_float(kEmptyChild), 0.f);
        if (used) a = cb[2u * rec[i]], q = cb[2u * rec[i] + 1u];
        int32_t ref = __float_as_int(q.z);
        uint32_t internal = 0;
        if (used) {
            if (expandable<W>(nodes, ref)) {
                internal = 1u;
            } else if (W == 16) {
                uint32_t f, c;
                if (ref >= 0) f = nodes[ref].first, c = nodes[ref].count;
                else f = (~(uint32_t) ref) >> 3, c = ((~(uint32_t) ref) & 7u) + 1u;
                ref = ~(int32_t) ((f << 4) | (c - 1u));
            }
        }
        flags[(uint32_t) W * j + i] = internal;
        if (W == 4) {
            float *o = out + 32u * (size_t) g;
            o[i] = a.x, o[4 + i] = a.y, o[8 + i] = a.z, o[12 + i] = a.w, o[16 + i] = q.x, o[20 + i] = q.y;
            o[24 + i] = __int_as_float(ref);
            o[28 + i] = 0.f;
        } else {
            float4 *o = reinterpret_cast<float4 *>(out + 128u * (size_t) g) + 2 * i;
            o[0] = a;
            o[1] = make_float4(q.x, q.y, __int_as_float(ref), 0.f);
        }
    }
    // worst-case traversal stack below the root: children - 1 per level (four-wide), children per level (sixteen-wide)
    const uint32_t need = need_in[g] + (uint32_t) (W == 4 ? n - 1 : n);
    acc[g] = need;
    atomicMax(&ctr[3], need);
}
// step 2: internal children get the out indices qe + rank, in (node, slot) order
template <int W>
__global__ __launch_bounds__(256) void collapse_b_kernel(uint32_t *__restrict__ fr, uint32_t qb, uint32_t n_level, uint32_t qe, uint32_t cap,
                                                         float *__restrict__ out, const uint32_t *__restrict__ flags, const uint32_t *__restrict__ scan,
                                                         uint32_t *__restrict__ need, const uint32_t *__restrict__ acc, uint32_t *ctr) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= (uint32_t) W * n_level) return;
    const uint32_t g = qb + s / W, i = s % W;
    if (flags[s]) {
        float *word = W == 4 ? out + 32u * (size_t) g + 24 + i : out + 128u * (size_t) g + 8 * i + 6;
        const uint32_t ci = qe + scan[s];
        if (ci < cap) {
            fr[ci] = (uint32_t) __float_as_int(*word);
            need[ci] = acc[g];
            *word = __int_as_float((int32_t) ci);
        } else {
            ctr[2] = 3u;
        }
    }
    if (s == (uint32_t) W * n_level - 1u) ctr[1] = scan[s] + flags[s];
}

__global__ void gather_kernel(const uint32_t *__restrict__ order, uint32_t n, const float4 *__restrict__ src, float4 *__restrict__ dst, uint32_t rows) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n * rows) return;
    const uint32_t p = i / rows, r = i % rows;
    dst[i] = src[(size_t) rows * order[p] + r];
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static int g_fail_alloc = 0;

struct Scratch {
    std::vector<void *> dev;
    void *pinned = nullptr;
    int n_alloc = 0;
    hipError_t alloc(void **p, size_t bytes) {
        *p = nullptr;
        ++n_alloc;
        if (g_fail_alloc && n_alloc == g_fail_alloc) return hipErrorOutOfMemory;
        hipError_t e = hipMalloc(p, bytes ? bytes : 16);
        if (e == hipSuccess) dev.push_back(*p);
        return e;
    }
    void keep(void *p) {      // hand an allocation to the caller
        for (auto &q : dev)
            if (q == p) q = nullptr;
    }
    ~Scratch() {
        for (void *p : dev)
            if (p) (void) hipFree(p);
        if (pinned) (void) hipHostFree(pinned);
    }
};

static int fail(char *err, size_t n, int st, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    if (err && n) vsnprintf(err, n, fmt, ap);
    va_end(ap);
    return st;
}
#define BFB_TRY(expr)                                                                                          \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ == hipErrorOutOfMemory) return fail(err, err_len, 1, "%s: %s", #expr, hipGetErrorString(e_));   \
        if (e_ != hipSuccess) return fail(err, err_len, 2, "%s: %s", #expr, hipGetErrorString(e_));            \
    } while (0)
static inline dim3 grid_for(size_t n) { return dim3((unsigned) ((n + 255) / 256)); }

template <int W>
static int collapse(Scratch &S, hipStream_t stream, const BNode *nodes, const float4 *cb, uint32_t cap, uint32_t *fr, uint32_t *need, uint32_t *acc,
                    uint32_t *flags, uint32_t *scan, void *tmp, size_t tmp_bytes, uint32_t *ctr, uint32_t *hb, float *out, uint32_t *n_out,
                    uint32_t *depth_out, uint32_t *stack_out, char *err, size_t err_len) {
    BFB_TRY(hipMemsetAsync(fr, 0, sizeof(uint32_t), stream));        // the root: binary node 0
    BFB_TRY(hipMemsetAsync(need, 0, sizeof(uint32_t), stream));
    BFB_TRY(hipMemsetAsync(ctr, 0, 4 * sizeof(uint32_t), stream));
    uint32_t qb = 0, n_level = 1, depth = 0;
    while (n_level) {
        const uint32_t qe = qb + n_level;
        ++depth;
        if (depth > 64u) return fail(err, err_len, 3, "device BVH build: the %d-wide collapse did not end", W);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(collapse_a_kernel<W>), grid_for(n_level), dim3(256), 0, stream, nodes, cb, fr, qb, n_level, out, flags, need, acc, ctr);
        size_t tb = tmp_bytes;
        BFB_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, tb, flags, scan, (int) (W * n_level), stream));
        hipLaunchKernelGGL(HIP_KERNEL_NAME(collapse_b_kernel<W>), grid_for((size_t) W * n_level), dim3(256), 0, stream, fr, qb, n_level, qe, cap, out, flags, scan,
                           need, acc, ctr);
        BFB_TRY(hipGetLastError());
        BFB_TRY(hipMemcpyAsync(hb, ctr, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        BFB_TRY(hipStreamSynchronize(stream));
        if (hb[2]) return fail(err, err_len, 3, "device BVH build: the %d-wide collapse outgrew its node array", W);
        qb = qe;
        n_level = hb[1];
    }
    *n_out = qb;
    *depth_out = depth;
    *stack_out = hb[3];
    return 0;
}

}  // namespace bfb

extern "C" void bfk_build_fail_alloc(int nth) { bfb::g_fail_alloc = nth; }

extern "C" hipError_t bfk_build_gather(const uint32_t *order, uint32_t n, const float4 *src, float4 *dst, uint32_t rows, hipStream_t stream) {
    if (!n || !rows) return hipSuccess;
    hipLaunchKernelGGL(bfb::gather_kernel, bfb::grid_for((size_t) n * rows), dim3(256), 0, stream, order, n, src, dst, rows);
    return hipGetLastError();
}

extern "C" int bfk_build_bvh(const bfk_build_in *in, bfk_build_out *out, char *err, size_t err_len) {
    using namespace bfb;
    *out = bfk_build_out();
    const uint32_t n = in->n_tris;
    hipStream_t stream = in->stream;
    if (n == 0) return fail(err, err_len, 2, "device BVH build: no triangles");
    if (n >= (1u << 27)) return fail(err, err_len, 3, "device BVH build: %u triangles (at most 2^27 - 1)", n);
    Scratch S;
    float4 *tlo = nullptr, *thi = nullptr, *cb = nullptr;
    uint32_t *prim = nullptr, *idx_a = nullptr, *idx_b = nullptr, *pn_a = nullptr, *pn_b = nullptr, *flags = nullptr, *scan = nullptr, *ctr = nullptr, *all = nullptr;
    unsigned long long *keys_a = nullptr, *keys_b = nullptr;
    BNode *nodes = nullptr;
    uint32_t *bins = nullptr;
    const uint32_t cap = n + 1u, bin_cap = n / kSmall + 2u;
    const size_t fs = 2 * (size_t) n + 8;
    BFB_TRY(S.alloc((void **) &tlo, (size_t) n * sizeof(float4)));
    BFB_TRY(S.alloc((void **) &thi, (size_t) n * sizeof(float4)));
    BFB_TRY(S.alloc((void **) &prim, (size_t) n * 4));
    BFB_TRY(S.alloc((void **) &idx_a, (size_t) n * 4));
    BFB_TRY(S.alloc((void **) &idx_b, (size_t) n * 4));
    BFB_TRY(S.alloc((void **) &pn_a, (size_t) n * 4));
    BFB_TRY(S.alloc((void **) &pn_b, (size_t) n * 4));
    BFB_TRY(S.alloc((void **) &keys_a, (size_t) n * 8));
    BFB_TRY(S.alloc((void **) &keys_b, (size_t) n * 8));
    BFB_TRY(S.alloc((void **) &flags, fs * 4));
    BFB_TRY(S.alloc((void **) &scan, fs * 4));
    BFB_TRY(S.alloc((void **) &ctr, 8 * 4));
    BFB_TRY(S.alloc((void **) &all, 12 * 4));
    BFB_TRY(S.alloc((void **) &nodes, (size_t) cap * sizeof(BNode)));
    BFB_TRY(S.alloc((void **) &bins, (size_t) bin_cap * 3 * kBins * kBinWords * 4));
    BFB_TRY(hipHostMalloc(&S.pinned, 256));
    uint32_t *hb = (uint32_t *) S.pinned;
    size_t tmp_bytes = 0, sort_bytes = 0;
    BFB_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, flags, scan, (int) fs, stream));
    BFB_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, keys_a, keys_b, idx_b, idx_a, (int) n, 0, 62, stream));
    tmp_bytes = tmp_bytes > sort_bytes ? tmp_bytes : sort_bytes;
    void *tmp = nullptr;
    BFB_TRY(S.alloc(&tmp, tmp_bytes));

    // prepare: boxes, scene bounds, the start order
    {
        uint32_t h_all[12];
        for (int k = 0; k < 12; ++k) h_all[k] = (k % 6) < 3 ? BFB_OMIN : BFB_OMAX;
        std::memcpy(hb + 16, h_all, sizeof(h_all));
        BFB_TRY(hipMemcpyAsync(all, hb + 16, sizeof(h_all), hipMemcpyHostToDevice, stream));
    }
    hipLaunchKernelGGL(prep_kernel, grid_for(n), dim3(256), 0, stream, in->tris, n, tlo, thi, prim, all);
    hipLaunchKernelGGL(key_kernel, grid_for(n), dim3(256), 0, stream, tlo, thi, prim, n, all, keys_a, idx_b);
    BFB_TRY(hipGetLastError());
    {
        size_t tb = tmp_bytes;
        BFB_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, tb, keys_a, keys_b, idx_b, idx_a, (int) n, 0, 62, stream));
    }
    BFB_TRY(hipMemcpyAsync(hb + 32, all, 12 * 4, hipMemcpyDeviceToHost, stream));
    BFB_TRY(hipStreamSynchronize(stream));
    auto o2f_h = [](uint32_t o) {
        const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
        float f;
        std::memcpy(&f, &u, 4);
        return f;
    };
    float scale = in->origin_scale;
    for (int k = 0; k < 3; ++k) {
        out->lo[k] = o2f_h(hb[32 + k]);
        out->hi[k] = o2f_h(hb[35 + k]);
        scale = std::fmax(scale, std::fmax(std::fabs(out->lo[k]), std::fabs(out->hi[k])));
    }
    const float abs_pad = 2e-7f * scale;

    uint32_t n_bnodes = 0;
    if (n > (uint32_t) kMaxLeaf) {
        hipLaunchKernelGGL(root_kernel, grid_for(n), dim3(256), 0, stream, nodes, n, pn_a);
        BFB_TRY(hipMemsetAsync(flags + n, 0, 4, stream));
        uint32_t lb = 0, n_level = 1, n_large = n > kSmall ? 1u : 0u, levels = 0;
        while (n_level) {
            if (++levels > (uint32_t) kMaxDepth + 2u) return fail(err, err_len, 3, "device BVH build: the tree is deeper than %d levels", kMaxDepth);
            const uint32_t le = lb + n_level;
            if (n_large) {
                if (n_large > bin_cap) return fail(err, err_len, 2, "device BVH build: bin scratch outgrown");
                const uint32_t words = n_large * 3 * kBins * kBinWords;
                hipLaunchKernelGGL(bins_init_kernel, grid_for(words), dim3(256), 0, stream, bins, words);
                hipLaunchKernelGGL(bounds_large_kernel, grid_for(n), dim3(256), 0, stream, nodes, pn_a, idx_a, tlo, thi, n);
                hipLaunchKernelGGL(bin_large_kernel, grid_for(n), dim3(256), 0, stream, nodes, pn_a, idx_a, tlo, thi, n, bins);
            }
            hipLaunchKernelGGL(eval_kernel, grid_for((size_t) n_level * 64), dim3(256), 0, stream, nodes, lb, n_level, idx_a, tlo, thi, bins, flags);
            BFB_TRY(hipGetLastError());
            size_t tb = tmp_bytes;
            BFB_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, tb, flags, scan, (int) (2 * n_level), stream));
            BFB_TRY(hipMemsetAsync(ctr, 0, 3 * 4, stream));
            hipLaunchKernelGGL(children_kernel, grid_for(n_level), dim3(256), 0, stream, nodes, lb, n_level, le, cap, flags, scan, ctr);
            // (flags[n] must be zero for the scan over n + 1 words below: the children's flags end before it, 2 n_level <= n)
            hipLaunchKernelGGL(flag_kernel, grid_for(n), dim3(256), 0, stream, nodes, pn_a, idx_a, tlo, thi, n, lb, flags);
            BFB_TRY(hipMemsetAsync(flags + n, 0, 4, stream));
            tb = tmp_bytes;
            BFB_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, tb, flags, scan, (int) (n + 1), stream));
            hipLaunchKernelGGL(scatter_kernel, grid_for(n), dim3(256), 0, stream, nodes, pn_a, idx_a, flags, scan, n, idx_b, pn_b);
            BFB_TRY(hipGetLastError());
            BFB_TRY(hipMemcpyAsync(hb, ctr, 3 * 4, hipMemcpyDeviceToHost, stream));
            BFB_TRY(hipStreamSynchronize(stream));
            if (hb[2]) return fail(err, err_len, 2, "device BVH build: node array outgrown");
            std::swap(idx_a, idx_b);
            std::swap(pn_a, pn_b);
            n_large = hb[0];
            lb = le;
            n_level = hb[1];
        }
        n_bnodes = lb;
    }
    out->order = idx_a;
    if (n_bnodes == 0) {
        // one leaf of at most kMaxLeaf triangles: no nodes at all
        out->root = ~(int32_t) (n - 1u);
        out->wroot = ~(int32_t) (n - 1u);
        out->depth2 = 0;
        if (in->want_wide) {
            BFB_TRY(S.alloc((void **) &out->wnodes, sizeof(bf::Node16)));
            BFB_TRY(hipMemsetAsync(out->wnodes, 0, sizeof(bf::Node16), stream));
            BFB_TRY(hipStreamSynchronize(stream));
            S.keep(out->wnodes);
        }
        S.keep(out->order);
        return 0;
    }

    // the binary tree's padded child boxes, then the two collapses
    BFB_TRY(S.alloc((void **) &cb, (size_t) n_bnodes * 4 * sizeof(float4)));
    BFB_TRY(hipMemsetAsync(ctr, 0, 8 * 4, stream));
    hipLaunchKernelGGL(cbox_kernel, grid_for(2 * (size_t) n_bnodes), dim3(256), 0, stream, nodes, n_bnodes, idx_a, tlo, thi, abs_pad, cb, ctr);
    BFB_TRY(hipGetLastError());
    BFB_TRY(hipMemcpyAsync(hb, ctr, 8 * 4, hipMemcpyDeviceToHost, stream));
    BFB_TRY(hipStreamSynchronize(stream));
    if (hb[2]) return fail(err, err_len, 3, "device BVH build: binary depth exceeds %d", kMaxDepth);
    const uint32_t cap16 = hb[4];
    out->depth2 = hb[5];
    uint32_t *fr = nullptr, *need = nullptr, *acc = nullptr;
    float *tmp4 = nullptr;
    BFB_TRY(S.alloc((void **) &fr, (size_t) (n_bnodes + 1) * 4));
    BFB_TRY(S.alloc((void **) &need, (size_t) (n_bnodes + 1) * 4));
    BFB_TRY(S.alloc((void **) &acc, (size_t) (n_bnodes + 1) * 4));
    BFB_TRY(S.alloc((void **) &tmp4, (size_t) n_bnodes * sizeof(bf::Node4)));
    int st = collapse<4>(S, stream, nodes, cb, n_bnodes, fr, need, acc, flags, scan, tmp, tmp_bytes, ctr, hb, tmp4, &out->n_nodes, &out->depth4, &out->stack4,
                         err, err_len);
    if (st) return st;
    out->root = 0;
    if (out->stack4 > 3u * (uint32_t) kMaxDepth) return fail(err, err_len, 3, "device BVH build: four-wide stack need %u exceeds %d", out->stack4, 3 * kMaxDepth);
    BFB_TRY(S.alloc((void **) &out->nodes, (size_t) out->n_nodes * sizeof(bf::Node4)));
    BFB_TRY(hipMemcpyAsync(out->nodes, tmp4, (size_t) out->n_nodes * sizeof(bf::Node4), hipMemcpyDeviceToDevice, stream));
    if (in->want_wide) {
        if (n <= bf::kWideLeaf) {
            out->wroot = ~(int32_t) (n - 1u);
            out->n_wnodes = 0;
        } else {
            float *tmp16 = nullptr;
            BFB_TRY(S.alloc((void **) &tmp16, (size_t) (cap16 + 1) * sizeof(bf::Node16)));
            st = collapse<16>(S, stream, nodes, cb, cap16, fr, need, acc, flags, scan, tmp, tmp_bytes, ctr, hb, tmp16, &out->n_wnodes, &out->depth16,
                              &out->stack16, err, err_len);
            if (st) return st;
            out->wroot = 0;
            BFB_TRY(S.alloc((void **) &out->wnodes, (size_t) (out->n_wnodes + 1) * sizeof(bf::Node16)));
            BFB_TRY(hipMemcpyAsync(out->wnodes, tmp16, (size_t) out->n_wnodes * sizeof(bf::Node16), hipMemcpyDeviceToDevice, stream));
        }
        if (!out->wnodes) BFB_TRY(S.alloc((void **) &out->wnodes, sizeof(bf::Node16)));
        BFB_TRY(hipMemsetAsync((char *) out->wnodes + (size_t) out->n_wnodes * sizeof(bf::Node16), 0, sizeof(bf::Node16), stream));
    }
    BFB_TRY(hipStreamSynchronize(stream));
    S.keep(out->order);
    S.keep(out->nodes);
    if (out->wnodes) S.keep(out->wnodes);
    return 0;
}
