// Meshes posed by a few numbers per render: skins (a pose is n_bones 3x4 matrices) and morph targets (a pose is n_targets
// weights, and the bones of a skin behind them).  bf_skin_vertices_kernel (bf_skin_vertices_dq_kernel for a shape whose skin mode is
// BF_SKIN_DUAL_QUATERNION: the bones are then converted to dual quaternions here) or bf_morph_vertices_kernel computes the vertices into the
// handle's scratch, and from there on a pose is a device-form vertex update and a batch a device-form deform batch of bf_mesh.cpp, with the
// bound on the coordinates derived here.  State: MeshState::skins / morphs / pose_vtx (bf_scene.h); kernels: bf_geom.hip.
#include "bf_scene.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

namespace {

// One bone table ([n_bones][12]) of skin `sk`: every entry finite, and per axis r the bound B[r] >= |posed coordinate r| of every
// vertex raised to cover it.  X_c >= |coordinate c| of everything the bones are applied to: the skin's rest extent (skin_extent), or
// what morph_extent derives for a morph ahead of the skin.  Derivation (u = 2^-24, W = the largest float64 sum of a weight row):
//   q_k[r] = fl(fl(fl(fl(m_r0 x) + fl(m_r1 y)) + fl(m_r2 z)) + m_r3) of bone b = i_k: each product carries one rounding and the
//     three sums one each, so |q_k[r]| <= Q_b[r] (1 + u)^4 with Q_b[r] = |m_r0| X_0 + |m_r1| X_1 + |m_r2| X_2 + |m_r3|;
//   p'[r] = fl(fl(fl(fl(w0 q_0) + fl(w1 q_1)) + fl(w2 q_2)) + fl(w3 q_3)): again one rounding per product and three sums, so
//     |p'[r]| <= (sum_k w_k |q_k[r]|) (1 + u)^4 <= W max_b Q_b[r] (1 + u)^8, the maximum over the bones some vertex gives a non-zero
//     weight (a zero-weight slot adds fl(0 q) = +-0 exactly, whatever its bone's finite matrix holds).
//   (1 + u)^8 < 1 + 5e-7; results that round into the subnormal range err by at most 2^-150 per operation instead.  The factor
//   1 + 1e-5 below (origin_bound's margin) covers both, the evaluation of Q in float64 and the rounding of B to float.
// `who` ends in ':' or ','.
bf_status skin_bound(const MeshSkin &sk, const double X[3], uint32_t shape, const float *bones, const char *who, double B[3]) {
    for (uint32_t b = 0; b < sk.n_bones; ++b) {
        const float *m = bones + 12 * (size_t) b;
        for (int j = 0; j < 12; ++j)
            if (!std::isfinite(m[j])) return fail(BF_ERR_INVALID, "%s shape %u: bone %u has a non-finite entry", who, shape, b);
        if (!sk.bone_used[b]) continue;
        for (int r = 0; r < 3; ++r) {
            double q = std::fabs((double) m[4 * r + 3]);
            for (int c = 0; c < 3; ++c) q += std::fabs((double) m[4 * r + c]) * X[c];
            B[r] = std::max(B[r], sk.weight_sum * q * (1.0 + 1e-5) + 1e-37);
        }
    }
    return BF_OK;
}

// ---- dual-quaternion skinning (BF_SKIN_DUAL_QUATERNION): what the host does to a bone table ----------------------------------------
// A bone is rigid if, in float64, max |R^T R - I| <= 1e-4 and det R > 0 (entries finite: checked before).
bool bone_rigid(const float *m) {
    double R[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[r][c] = (double) m[4 * r + c];
    double dev = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            dev = std::max(dev, std::fabs(R[0][i] * R[0][j] + R[1][i] * R[1][j] + R[2][i] * R[2][j] - (i == j ? 1.0 : 0.0)));
    const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                       R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
    return dev <= 1e-4 && det > 0.0;
}
// The conversion of one rigid bone [R | t] to a unit dual quaternion, stated ONCE, here (this object is compiled with
// -ffp-contract=off, so motion.bone_dual_quaternions restates it in numpy bit for bit).  float64, rounded to float once at the end:
//   tr = (m00 + m11) + m22;  the branch is the largest of (tr, m00, m11, m22), the first among equals in that order
//   branch tr:   s = sqrt(((1 + m00) + m11) + m22), w = s / 2, f = 0.5 / s, x = (m21 - m12) f, y = (m02 - m20) f, z = (m10 - m01) f
//   branch m00:  s = sqrt(((1 + m00) - m11) - m22), x = s / 2, f = 0.5 / s, w = (m21 - m12) f, y = (m01 + m10) f, z = (m02 + m20) f
//   branch m11:  s = sqrt(((1 - m00) + m11) - m22), y = s / 2, f = 0.5 / s, w = (m02 - m20) f, x = (m01 + m10) f, z = (m12 + m21) f
//   branch m22:  s = sqrt(((1 - m00) - m11) + m22), z = s / 2, f = 0.5 / s, w = (m10 - m01) f, x = (m02 + m20) f, y = (m12 + m21) f
//   q = (w, x, y, z) / sqrt(((w w + x x) + y y) + z z), each component divided
//   dual = (0, t) q / 2:  dw = -0.5 ((tx x + ty y) + tz z),  dx = 0.5 ((tx w + ty z) - tz y),  dy = 0.5 ((ty w + tz x) - tx z),
//                         dz = 0.5 ((tz w + tx y) - ty x)
//   out = (w, x, y, z, dw, dx, dy, dz)
void bone_dq(const float *m, float out[8]) {
    const double m00 = m[0], m01 = m[1], m02 = m[2], tx = m[3], m10 = m[4], m11 = m[5], m12 = m[6], ty = m[7], m20 = m[8], m21 = m[9],
                 m22 = m[10], tz = m[11];
    const double tr = (m00 + m11) + m22;
    int branch = 0;
    double best = tr;
    if (m00 > best) branch = 1, best = m00;
    if (m11 > best) branch = 2, best = m11;
    if (m22 > best) branch = 3, best = m22;
    double w, x, y, z;
    if (branch == 0) {
        const double s = std::sqrt(((1.0 + m00) + m11) + m22), f = 0.5 / s;
        w = s / 2.0, x = (m21 - m12) * f, y = (m02 - m20) * f, z = (m10 - m01) * f;
    } else if (branch == 1) {
        const double s = std::sqrt(((1.0 + m00) - m11) - m22), f = 0.5 / s;
        x = s / 2.0, w = (m21 - m12) * f, y = (m01 + m10) * f, z = (m02 + m20) * f;
    } else if (branch == 2) {
        const double s = std::sqrt(((1.0 - m00) + m11) - m22), f = 0.5 / s;
        y = s / 2.0, w = (m02 - m20) * f, x = (m01 + m10) * f, z = (m12 + m21) * f;
    } else {
        const double s = std::sqrt(((1.0 - m00) - m11) + m22), f = 0.5 / s;
        z = s / 2.0, w = (m10 - m01) * f, x = (m02 + m20) * f, y = (m12 + m21) * f;
    }
    const double len = std::sqrt(((w * w + x * x) + y * y) + z * z);
    w = w / len, x = x / len, y = y / len, z = z / len;
    out[0] = (float) w, out[1] = (float) x, out[2] = (float) y, out[3] = (float) z;
    out[4] = (float) (-0.5 * ((tx * x + ty * y) + tz * z));
    out[5] = (float) (0.5 * ((tx * w + ty * z) - tz * y));
    out[6] = (float) (0.5 * ((ty * w + tz * x) - tx * z));
    out[7] = (float) (0.5 * ((tz * w + tx * y) - ty * x));
}
// skin_bound for a shape in BF_SKIN_DUAL_QUATERNION: every entry finite, every bone some vertex weighs rigid, and B raised (all
// three axes alike) over the posed coordinates.  Derivation (u = 2^-24, W = sk.weight_sum, kappa = sk.pivot_min, T = the largest
// |t|_2 over the bones some vertex weighs, |X| = the 2-norm of X, |.| of a quaternion its 4-norm):
//   the table: q_k = D_k.real has |q_k| = 1 and D_k.dual = (0, t_k) q_k / 2 has |D_k.dual| = |t_k| / 2 <= T / 2, each within a
//     factor 1 +- 2u (normalised in float64, rounded once); a bone no vertex weighs is the identity and adds fl(+-0 D) = +-0;
//   b.real . q_p = sum_k s_k w_k (q_k . q_p) = sum_k w_k |q_k . q_p| >= w_p |q_p|^2 >= kappa (1 - 4u): s_k is the sign of the
//     ROUNDED dot, which can differ from the true one only where |q_k . q_p| <= 4u, and then the term is off by at most 8u w_k; the
//     seven roundings of a component of b add at most 4u W more.  So |b.real| >= b.real . q_p / |q_p| >= kappa - 16u W, and with
//     kappa >= 0.2497 (the largest of four weights that sum to at least 1 - 1e-3), |b.real| >= kappa (1 - 1e-5);
//   |b.dual| <= sum_k w_k |D_k.dual| (1 + 4u) <= W T / 2 (1 + 6u), hence |e| = |b.dual| / |b.real| <= W T / (2 kappa) (1 + 2e-5) and
//     the translation 2 vec(e r*) has 2-norm 2 |e| |r| <= W T / kappa (1 + 3e-5), |r| = 1 +- 4u;
//   rotate(r, x) is the rotation by r / |r| of x up to (|r|^2 - 1) terms and nine roundings of magnitudes <= 4 |x|: at most
//     |X| (1 + 64u) per coordinate; the translation's evaluation and the final sum add five roundings more.
//   Together |x'_c| <= (|X| + W T / kappa) (1 + 5e-5): the factor 1 + 1e-4 below covers it, the evaluation in float64 and the
//   rounding of B to float; results in the subnormal range err by 2^-150 per operation instead, below the 1e-37 added.
// The normal has no bound of its own: the gather refuses one that is not finite, as ever.  `who` ends in ':' or ','.
bf_status skin_bound_dq(const MeshSkin &sk, const double X[3], uint32_t shape, const float *bones, const char *who, double B[3]) {
    double T = 0.0;
    for (uint32_t b = 0; b < sk.n_bones; ++b) {
        const float *m = bones + 12 * (size_t) b;
        for (int j = 0; j < 12; ++j)
            if (!std::isfinite(m[j])) return fail(BF_ERR_INVALID, "%s shape %u: bone %u has a non-finite entry", who, shape, b);
        if (!sk.bone_used[b]) continue;
        if (!bone_rigid(m))
            return fail(BF_ERR_INVALID, "%s shape %u: bone %u is not rigid (BF_SKIN_DUAL_QUATERNION takes rotations and translations only: "
                                        "max |R^T R - I| <= 1e-4, det R > 0)", who, shape, b);
        T = std::max(T, std::sqrt((double) m[3] * m[3] + (double) m[7] * m[7] + (double) m[11] * m[11]));
    }
    const double bound = (std::sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]) + sk.weight_sum * T / (double) sk.pivot_min) * (1.0 + 1e-4) + 1e-37;
    for (int r = 0; r < 3; ++r) B[r] = std::max(B[r], bound);
    return BF_OK;
}
// one render's bone table as the DQ kernels read it: [n_bones][8], a bone no vertex weighs as the identity
void skin_table_dq(const MeshSkin &sk, const float *bones, float *out) {
    static const float identity[8] = {1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (uint32_t b = 0; b < sk.n_bones; ++b) {
        if (sk.bone_used[b]) bone_dq(bones + 12 * (size_t) b, out + 8 * (size_t) b);
        else std::memcpy(out + 8 * (size_t) b, identity, sizeof(identity));
    }
}

// ... a bound as the float the gather checks against (and the shape's base box takes); a bound float cannot hold is refused
bf_status skin_bound_float(const double B[3], uint32_t shape, const char *who, float *bound, float box6[6], const char *why) {
    float mx = std::numeric_limits<float>::min();
    for (int r = 0; r < 3; ++r) {
        const bool fits = B[r] < 0.5 * (double) std::numeric_limits<float>::max();
        const float f = fits ? std::nextafter((float) B[r], std::numeric_limits<float>::infinity()) : 0.f;
        if (!fits)
            return fail(BF_ERR_INVALID, "%s shape %u: the bound on the posed coordinates is not finite (%s)", who, shape, why);
        if (box6) box6[r] = -f, box6[3 + r] = f;
        mx = std::max(mx, f);
    }
    *bound = mx;
    return BF_OK;
}

// One pose's weights ([n_targets]) of morph `mo`: every weight finite, and per axis c the extent X[c] >= |morphed coordinate c| of every
// vertex raised to cover it.  Derivation (u = 2^-24, K = n_targets, R_c = max |rest coordinate c|, D_k,c = max |delta coordinate c| of
// target k): t_k = fl(w_k d_k) has |t_k| <= |w_k| D_k,c (1 + u), and p_k = fl(p_{k-1} + t_k) has |p_k| <= (|p_{k-1}| + |t_k|)(1 + u), so
//   |p_K| <= (R_c + sum_k |w_k| D_k,c) (1 + u)^(K + 1),   and (1 + u)^(K + 1) < 1 + 2 (K + 1) u for K <= 256 (1.6e-5 at the most: more
// than origin_bound's 1e-5, hence a factor of its own).  A result that rounds into the subnormal range errs by at most 2^-150 per
// operation instead, 2 K of them: below the 1e-37 added.  A zero weight contributes |0| D = 0 however large its target's deltas are,
// as fl(0 d) = +-0 does on the device.  The sum is taken in float64, whose own rounding the factor 2 covers.  `who` ends in ':' or ','.
bf_status morph_extent(const MeshMorph &mo, uint32_t shape, const float *weights, const char *who, double X[3]) {
    double s[3] = {(double) mo.rest_abs[0], (double) mo.rest_abs[1], (double) mo.rest_abs[2]};
    for (uint32_t k = 0; k < mo.n_targets; ++k) {
        if (!std::isfinite(weights[k])) return fail(BF_ERR_INVALID, "%s shape %u: the weight of target %u is not finite", who, shape, k);
        for (int c = 0; c < 3; ++c) s[c] += std::fabs((double) weights[k]) * (double) mo.delta_abs[3 * (size_t) k + c];
    }
    for (int c = 0; c < 3; ++c) X[c] = std::max(X[c], s[c] * (1.0 + 2.0 * (mo.n_targets + 1.0) * 0x1p-24) + 1e-37);
    return BF_OK;
}
// floats of `n_versions` poses' weights in a staged table ([n_versions][n_targets]), padded to 16 bytes so that the bone tables behind stay aligned
size_t morph_weight_floats(const MeshMorph &mo, uint32_t n_versions) { return ((size_t) n_versions * mo.n_targets + 3) & ~size_t(3); }

// ---- a shape posed per render: what a single pose and a batch, of a skin or of a morph, do the same way -----------------------------
// mo: null for a pure skin; sk: null for a pure morph (a morph with both is skinned behind its targets).  weights ([n_renders]
// [n_targets]) and bones ([n_renders][n_bones][12]) are the caller's host tables, from render 0 on.
struct PosedShape {
    uint32_t shape;
    const bf_geometry::MeshTopo *tp;
    const MeshMorph *mo;
    const MeshSkin *sk;
    const float *weights, *bones;
    bool dq;                                                                         // sk in BF_SKIN_DUAL_QUATERNION on this handle
    uint32_t n_vertices() const { return mo ? mo->n_vertices : sk->n_vertices; }
    const float *rest_nrm() const { return mo ? mo->rest_nrm : sk->rest_nrm; }      // the morph's, blended by the skin behind it
    const float *bones_of(uint32_t k) const { return bones + (size_t) k * sk->n_bones * 12; }      // render k's, in the caller's table
    size_t n_bone_floats() const { return sk ? (size_t) sk->n_bones * (dq ? 8 : 12) : 0; }         // of one render, in the staged table
    const char *why() const { return mo ? "weights or bones too large for the targets" : "bones too large for the rest pose"; }
};

// The checks of a posed shape common to a pose and a batch: what a vertex update refuses of the shape, then (morph: bf_*_morph*) a shape
// without a morph and, if the call has bones for it, without the skin they need; else a shape without a skin.
bf_status check_posed_shape(const bf_scene *scene, uint32_t shape, bool morph, const float *weights, const float *bones, const char *who,
                            PosedShape *out) {
    const bf_geometry::MeshTopo *tp = nullptr;
    const bf_status st = check_deform_shape(scene, shape, false, who, &tp);
    if (st != BF_OK) return st;
    const MeshState &m = scene->mesh;
    const MeshMorph *mo = morph && shape < m.morphs.size() ? m.morphs[shape].get() : nullptr;
    const MeshSkin *sk = (!morph || bones) && shape < m.skins.size() ? m.skins[shape].get() : nullptr;
    if (morph && !mo) return fail(BF_ERR_INVALID, "%s shape %u has no morph (bf_scene_set_morph attaches one)", who, shape);
    if (!morph && !sk) return fail(BF_ERR_INVALID, "%s shape %u has no skin (bf_scene_set_skin attaches one)", who, shape);
    if (morph && bones && !sk)
        return fail(BF_ERR_INVALID, "%s bones for shape %u, which has no skin (bf_scene_set_skin attaches one)", who, shape);
    *out = {shape, tp, mo, sk, weights, bones, sk && m.skins_dq(shape)};
    return BF_OK;
}

// The bound of render `k`: B raised over the posed coordinates.  The morph's extent is the bound, or what the skin bound takes in place
// of the skin's rest extent.
bf_status pose_bound(const PosedShape &p, uint32_t k, const char *who, double B[3]) {
    double X[3] = {0.0, 0.0, 0.0};
    if (p.mo) {
        const bf_status st = morph_extent(*p.mo, p.shape, p.weights + (size_t) k * p.mo->n_targets, who, X);
        if (st != BF_OK) return st;
    } else {
        for (int c = 0; c < 3; ++c) X[c] = (double) p.sk->rest_abs[c];
    }
    if (p.sk) return (p.dq ? skin_bound_dq : skin_bound)(*p.sk, X, p.shape, p.bones_of(k), who, B);
    for (int c = 0; c < 3; ++c) B[c] = std::max(B[c], X[c]);
    return BF_OK;
}

// floats of one version of the shape in the scratch: positions, then normals if it has rest normals and they are wanted (not under
// BF_NORMALS_RECOMPUTE: the morphed or blended normals are then not computed)
size_t pose_floats(const PosedShape &p, bool with_normals) { return (size_t) p.n_vertices() * 3 * (p.rest_nrm() && with_normals ? 2 : 1); }

// The staged table of renders k0 .. k0 + kc: [kc][n_targets] weights, padded to 16 bytes (none without a morph), then [kc][n_bones][12]
// bones if the shape is skinned ([kc][n_bones][8] dual quaternions, converted here, if it is in BF_SKIN_DUAL_QUATERNION).
size_t pose_table_floats(const PosedShape &p, uint32_t kc) { return (p.mo ? morph_weight_floats(*p.mo, kc) : 0) + kc * p.n_bone_floats(); }
void pose_table_pack(const PosedShape &p, uint32_t k0, uint32_t kc, float *host) {
    if (p.mo) {
        const size_t wf = morph_weight_floats(*p.mo, kc), n = (size_t) kc * p.mo->n_targets;
        std::memcpy(host, p.weights + (size_t) k0 * p.mo->n_targets, n * sizeof(float));
        std::memset(host + n, 0, (wf - n) * sizeof(float));
        host += wf;
    }
    if (p.sk && p.dq) {
        for (uint32_t k = 0; k < kc; ++k) skin_table_dq(*p.sk, p.bones_of(k0 + k), host + k * p.n_bone_floats());
    } else if (p.sk) {
        std::memcpy(host, p.bones_of(k0), kc * p.n_bone_floats() * sizeof(float));
    }
}

// The launch: kc versions of the shape from its table on the device into the scratch at `out` ([kc][nv][3] positions, then the
// normals), where src->pos / nrm point afterwards: version v of the gather reads slice v.  A pure skin has its own kernel.
bf_status pose_vertices(const PosedShape &p, bool with_normals, const float *table, uint32_t kc, float *out, bfd::DDeformSrc *src,
                        hipStream_t stream) {
    const MeshSkin *sk = p.sk;
    const float *rest_nrm = with_normals ? p.rest_nrm() : nullptr;
    float *pos = out, *nrm = rest_nrm ? out + (size_t) kc * p.n_vertices() * 3 : nullptr;
    if (p.mo) {
        const MeshMorph &mo = *p.mo;
        HIP_TRY(bfk_launch_morph_vertices(mo.rest_pos, rest_nrm, mo.dpos, mo.dnrm, mo.n_vertices, mo.n_targets, table, sk ? sk->index : nullptr,
                                          sk ? sk->weight : nullptr, sk ? table + morph_weight_floats(mo, kc) : nullptr, sk ? sk->n_bones : 0u,
                                          p.dq ? 1 : 0, pos, nrm, kc, stream));
    } else {
        HIP_TRY((p.dq ? bfk_launch_skin_vertices_dq : bfk_launch_skin_vertices)(sk->rest_pos, rest_nrm, sk->index, sk->weight, sk->n_vertices, table, sk->n_bones, pos, nrm, kc, stream));
    }
    src->pos = pos;
    src->nrm = nrm;
    return BF_OK;
}

// the handle's scratch for posed vertices, at least `bytes`
bf_status pose_scratch(bf_scene *scene, size_t bytes, hipStream_t stream, const char *who) {
    return vertex_scratch(scene->mesh.pose_vtx, scene->mesh.pose_vtx_cap, bytes, stream, who, "posed vertices");
}

// bf_scene_pose_skin / bf_scene_pose_morph (`name`) behind their argument checks: the base of the shape becomes pose 0 of `p`
bf_status pose_shape(bf_scene *scene, const PosedShape &p, const char *name, hipStream_t stream) {
    const std::string fn_ = std::string(name) + ":";
    const char *fn = fn_.c_str();
    double B[3] = {0.0, 0.0, 0.0};
    float bound = 0.f, box[6];
    bf_status st = BF_OK;
    if ((st = pose_bound(p, 0u, fn, B)) != BF_OK || (st = skin_bound_float(B, p.shape, fn, &bound, box, p.why())) != BF_OK) return st;
    if (scene->d.n_tris == 0 || p.n_vertices() == 0) return BF_OK;
    BF_ENTER_AS(scene, name);
    MeshState &m = scene->mesh;
    if ((st = mesh_enter(scene, stream)) != BF_OK) return st;
    if ((st = velocity_before(scene, stream)) != BF_OK) return st;
    const bool with_normals = !m.recomputes(p.shape);      // BF_NORMALS_RECOMPUTE: update_vertices_locked computes them
    if ((st = pose_scratch(scene, pose_floats(p, with_normals) * sizeof(float), stream, fn)) != BF_OK) return st;
    const size_t bytes = pose_table_floats(p, 1u) * sizeof(float);
    bf_scene::Stage *stg = nullptr;
    if ((st = stage_acquire(scene, bytes, &stg)) != BF_OK) return st;
    pose_table_pack(p, 0u, 1u, (float *) stg->host);
    if ((st = stage_commit(stg, bytes, stream)) != BF_OK) return st;
    bfd::DDeformSrc at = {};
    if ((st = pose_vertices(p, with_normals, (const float *) stg->dev, 1u, m.pose_vtx, &at, stream)) != BF_OK) return st;
    HIP_TRY(hipEventRecord(stg->ev, stream));      // the table is read by the kernel
    if ((st = update_vertices_locked(scene, p.shape, *p.tp, at.pos, at.nrm, bound, box, true, stream)) != BF_OK) return st;
    if ((st = velocity_after(scene, p.shape, stream)) != BF_OK) return st;
    return mark_last(scene, stream);
}

// bf_render_skin_batch_device / bf_render_morph_batch_device (`name`; morph: the latter): render k sees shape shapes[j] posed by slice k
// of weights[j] (morph) and bones[j] (a skin batch: all of them; a morph batch: NULL, or NULL for the shapes that are not skinned).
bf_status render_posed_batch(const char *name, bool morph, bf_scene *scene, const bf_launch *launch, uint32_t n_renders, const uint64_t *seeds,
                             uint32_t n_posed, const uint32_t *shapes, const float *const *weights, const float *const *bones, uint32_t n_shapes,
                             const float *to_world, float *hist_dev, bf_path_record *records_dev, void *stream_, bf_stats *stats_out) {
    const std::string fn_ = std::string(name) + ":";
    const char *fn = fn_.c_str();
    if (n_posed && (!shapes || !(morph ? weights : bones))) return fail(BF_ERR_INVALID, "%s null argument", fn);
    bf_status st = check_batch_call(fn, morph ? "morph" : "skin", scene, launch, n_renders, to_world, n_shapes, hist_dev);
    if (st != BF_OK) return st;
    n_shapes = scene->info.n_shapes;
    // the gather's table: a posed shape's entry is marked here and pointed at the chunk's posed vertices below
    std::vector<bfd::DDeformSrc> src(n_shapes);
    std::memset(src.data(), 0, src.size() * sizeof(bfd::DDeformSrc));
    std::vector<PosedShape> posed(n_posed);
    size_t version_floats = 0;      // posed vertices of all listed shapes, per render
    double B[3] = {0.0, 0.0, 0.0};
    for (uint32_t j = 0; j < n_posed; ++j) {
        PosedShape &p = posed[j];
        if ((st = check_posed_shape(scene, shapes[j], morph, morph ? weights[j] : nullptr, bones ? bones[j] : nullptr, fn, &p)) != BF_OK) return st;
        if (morph ? !p.weights : !p.bones) return fail(BF_ERR_INVALID, "%s shape %u: null %s", fn, p.shape, morph ? "weights" : "bones");
        if (src[p.shape].pos) return fail(BF_ERR_INVALID, "%s shape %u is listed twice", fn, p.shape);
        src[p.shape].pos = (const float *) (uintptr_t) 16;      // (marks the shape; never read)
        src[p.shape].nv = p.tp->n_vertices;
        for (uint32_t k = 0; k < n_renders; ++k) {
            char who[96];
            std::snprintf(who, sizeof(who), "%s render %u,", fn, k);
            if ((st = pose_bound(p, k, who, B)) != BF_OK) return st;
        }
        version_floats += pose_floats(p, !scene->mesh.recomputes(p.shape));
    }
    float bound = std::numeric_limits<float>::min();
    if (n_posed && (st = skin_bound_float(B, shapes[0], fn, &bound, nullptr, posed[0].why())) != BF_OK) return st;
    std::vector<uint8_t> moves(to_world ? (size_t) n_renders * n_shapes : 0, 0);
    if (to_world && (st = check_rigid_tables(scene, fn, n_renders, n_shapes, to_world, moves.data())) != BF_OK) return st;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BF_ENTER_AS(scene, name);
    if (batch_ends_early(scene, launch, n_renders, seeds, hist_dev, records_dev, stream_, stats_out, &st)) return st;
    MeshState &m = scene->mesh;
    return deform_versions(scene, launch, n_renders, seeds, src, bound, to_world, moves, hist_dev, records_dev, stream_, stats_out, name,
                           [&](uint32_t k0, uint32_t kc, bfd::DDeformSrc *hs) -> bf_status {
        // the chunk's tables, one shape after the other, and, from them, its posed vertices in the scratch, likewise
        bf_status pst = pose_scratch(scene, (size_t) kc * version_floats * sizeof(float), stream, fn);
        if (pst != BF_OK || !n_posed) return pst;
        size_t floats = 0;
        for (const PosedShape &p : posed) floats += pose_table_floats(p, kc);
        const size_t bytes = floats * sizeof(float);
        bf_scene::Stage *stg = nullptr;
        if ((pst = stage_acquire(scene, bytes, &stg)) != BF_OK) return pst;
        float *hb = (float *) stg->host;
        for (const PosedShape &p : posed) {
            pose_table_pack(p, k0, kc, hb);
            hb += pose_table_floats(p, kc);
        }
        if ((pst = stage_commit(stg, bytes, stream)) != BF_OK) return pst;
        const float *db = (const float *) stg->dev;
        float *out = m.pose_vtx;
        for (const PosedShape &p : posed) {
            // (BF_NORMALS_RECOMPUTE: no morphed or blended normals; deform_versions computes the posed surface's behind this)
            const bool with_normals = !m.recomputes(p.shape);
            if ((pst = pose_vertices(p, with_normals, db, kc, out, &hs[p.shape], stream)) != BF_OK) return pst;
            db += pose_table_floats(p, kc);
            out += (size_t) kc * pose_floats(p, with_normals);
        }
        HIP_TRY(hipEventRecord(stg->ev, stream));      // the tables are read by the kernels
        return BF_OK;
    });
}

}  // namespace

extern "C" {

bf_status bf_scene_set_skin(bf_scene *scene, uint32_t shape, uint32_t n_bones, const float *rest_positions, const float *rest_normals,
                            const uint32_t *bone_index, const float *bone_weight) {
    const char *fn = "bf_scene_set_skin:";
    if (!scene) return fail(BF_ERR_INVALID, "%s null scene", fn);
    const bf_geometry::MeshTopo *tp = nullptr;
    bf_status st = check_deform_shape(scene, shape, n_bones && rest_normals, fn, &tp);
    if (st != BF_OK) return st;
    if (n_bones == 0) {
        BF_ENTER(scene);
        if (shape < scene->mesh.skins.size()) scene->mesh.skins[shape].reset();
        return BF_OK;
    }
    if (n_bones > 256u) return fail(BF_ERR_INVALID, "%s shape %u: %u bones (at most 256 per shape)", fn, shape, n_bones);
    if (!rest_positions || !bone_index || !bone_weight) return fail(BF_ERR_INVALID, "%s shape %u: null array", fn, shape);
    if (tp->has_normals && !rest_normals)
        return fail(BF_ERR_INVALID, "%s shape %u was created with vertex normals: its skin needs rest normals", fn, shape);
    const uint32_t nv = tp->n_vertices;
    auto skin = std::make_shared<MeshSkin>();
    skin->n_bones = n_bones;
    skin->n_vertices = nv;
    skin->bone_used.assign(n_bones, 0);
    for (uint32_t v = 0; v < nv; ++v) {
        for (int c = 0; c < 3; ++c) {
            const float x = rest_positions[3 * (size_t) v + c];
            if (!std::isfinite(x) || (rest_normals && !std::isfinite(rest_normals[3 * (size_t) v + c])))
                return fail(BF_ERR_INVALID, "%s shape %u: non-finite rest value at vertex %u", fn, shape, v);
            skin->rest_abs[c] = std::max(skin->rest_abs[c], std::fabs(x));
        }
        double sum = 0.0;
        for (int k = 0; k < 4; ++k) {
            const uint32_t b = bone_index[4 * (size_t) v + k];
            const float w = bone_weight[4 * (size_t) v + k];
            if (b >= n_bones) return fail(BF_ERR_INVALID, "%s shape %u: vertex %u names bone %u of %u", fn, shape, v, b, n_bones);
            if (!std::isfinite(w) || w < 0.f) return fail(BF_ERR_INVALID, "%s shape %u: vertex %u has weight %g for bone %u", fn, shape, v, (double) w, b);
            if (w > 0.f) skin->bone_used[b] = 1;
            sum += (double) w;
        }
        if (!(std::fabs(sum - 1.0) <= 1e-3)) return fail(BF_ERR_INVALID, "%s shape %u: the weights of vertex %u sum to %.9g, not 1", fn, shape, v, sum);
        skin->weight_sum = std::max(skin->weight_sum, sum);
        const float *wr = bone_weight + 4 * (size_t) v;
        skin->pivot_min = std::min(skin->pivot_min, std::max(std::max(wr[0], wr[1]), std::max(wr[2], wr[3])));
    }
    BF_ENTER(scene);
    if (nv) {
        // one block: weights, indices (16-byte rows first), rest positions, rest normals
        const size_t row = (size_t) nv * 16, vec = (size_t) nv * 12, bytes = 2 * row + vec * (rest_normals ? 2 : 1);
        std::vector<char> host(bytes);
        std::memcpy(host.data(), bone_weight, row);
        std::memcpy(host.data() + row, bone_index, row);
        std::memcpy(host.data() + 2 * row, rest_positions, vec);
        if (rest_normals) std::memcpy(host.data() + 2 * row + vec, rest_normals, vec);
        const hipError_t he = hipMalloc(&skin->block, bytes);
        if (he != hipSuccess) {
            (void) hipGetLastError();
            return fail(BF_ERR_NOMEM, "%s shape %u: hipMalloc(%zu bytes): %s", fn, shape, bytes, hipGetErrorString(he));
        }
        HIP_TRY(hipMemcpy(skin->block, host.data(), bytes, hipMemcpyHostToDevice));
        const char *blk = (const char *) skin->block;
        skin->weight = (const float4 *) blk;
        skin->index = (const uint4 *) (blk + row);
        skin->rest_pos = (const float *) (blk + 2 * row);
        skin->rest_nrm = rest_normals ? (const float *) (blk + 2 * row + vec) : nullptr;
    }
    MeshState &m = scene->mesh;
    if (m.skins.size() < scene->info.n_shapes) m.skins.resize(scene->info.n_shapes);
    m.skins[shape] = std::move(skin);      // (the skin it replaces goes with its last handle; hipFree waits for the kernels that read it)
    return BF_OK;
}

bf_status bf_scene_set_skin_mode(bf_scene *scene, uint32_t shape, uint32_t mode) {
    const char *fn = "bf_scene_set_skin_mode:";
    if (!scene) return fail(BF_ERR_INVALID, "%s null scene", fn);
    if (mode != BF_SKIN_LINEAR && mode != BF_SKIN_DUAL_QUATERNION)
        return fail(BF_ERR_INVALID, "%s shape %u: unknown mode %u (BF_SKIN_LINEAR or BF_SKIN_DUAL_QUATERNION)", fn, shape, mode);
    const bf_geometry::MeshTopo *tp = nullptr;
    const bf_status st = check_deform_shape(scene, shape, false, fn, &tp);
    if (st != BF_OK) return st;
    BF_ENTER(scene);
    MeshState &m = scene->mesh;
    if (m.skin_mode.size() < scene->info.n_shapes) m.skin_mode.resize(scene->info.n_shapes, (uint8_t) BF_SKIN_LINEAR);
    m.skin_mode[shape] = (uint8_t) mode;      // read by the next call that takes bones for the shape; nothing moves now
    return BF_OK;
}

bf_status bf_scene_get_skin_mode(const bf_scene *scene, uint32_t shape, uint32_t *mode_out) {
    const char *fn = "bf_scene_get_skin_mode:";
    if (!scene || !mode_out) return fail(BF_ERR_INVALID, "%s null argument", fn);
    if (shape >= scene->info.n_shapes) return fail(BF_ERR_INVALID, "%s shape %u: the scene has %u shapes", fn, shape, scene->info.n_shapes);
    if (scene->ends.shapes_host[shape].type != BF_SHAPE_MESH) return fail(BF_ERR_INVALID, "%s shape %u is not a mesh", fn, shape);
    BF_ENTER(scene);
    *mode_out = scene->mesh.skins_dq(shape) ? BF_SKIN_DUAL_QUATERNION : BF_SKIN_LINEAR;
    return BF_OK;
}

bf_status bf_bone_dual_quaternions(uint32_t n_bones, const float *bones, float *out) {
    const char *fn = "bf_bone_dual_quaternions:";
    if (n_bones && (!bones || !out)) return fail(BF_ERR_INVALID, "%s null array", fn);
    for (uint32_t b = 0; b < n_bones; ++b) {
        const float *m = bones + 12 * (size_t) b;
        for (int j = 0; j < 12; ++j)
            if (!std::isfinite(m[j])) return fail(BF_ERR_INVALID, "%s bone %u has a non-finite entry", fn, b);
        if (!bone_rigid(m)) return fail(BF_ERR_INVALID, "%s bone %u is not rigid (max |R^T R - I| <= 1e-4, det R > 0)", fn, b);
    }
    for (uint32_t b = 0; b < n_bones; ++b) bone_dq(bones + 12 * (size_t) b, out + 8 * (size_t) b);
    return BF_OK;
}

bf_status bf_scene_set_morph(bf_scene *scene, uint32_t shape, uint32_t n_targets, const float *rest_positions, const float *rest_normals,
                             const float *delta_positions, const float *delta_normals) {
    const char *fn = "bf_scene_set_morph:";
    if (!scene) return fail(BF_ERR_INVALID, "%s null scene", fn);
    const bf_geometry::MeshTopo *tp = nullptr;
    bf_status st = check_deform_shape(scene, shape, n_targets && rest_normals, fn, &tp);
    if (st != BF_OK) return st;
    if (n_targets == 0) {
        BF_ENTER(scene);
        if (shape < scene->mesh.morphs.size()) scene->mesh.morphs[shape].reset();
        return BF_OK;
    }
    if (n_targets > 256u) return fail(BF_ERR_INVALID, "%s shape %u: %u targets (at most 256 per shape)", fn, shape, n_targets);
    if (!rest_positions || !delta_positions) return fail(BF_ERR_INVALID, "%s shape %u: null array", fn, shape);
    if (tp->has_normals && !rest_normals)
        return fail(BF_ERR_INVALID, "%s shape %u was created with vertex normals: its morph needs rest normals", fn, shape);
    if (delta_normals && !rest_normals) return fail(BF_ERR_INVALID, "%s shape %u: normal deltas without rest normals", fn, shape);
    const uint32_t nv = tp->n_vertices;
    auto morph = std::make_shared<MeshMorph>();
    morph->n_targets = n_targets;
    morph->n_vertices = nv;
    morph->delta_abs.assign((size_t) 3 * n_targets, 0.f);
    for (uint32_t v = 0; v < nv; ++v)
        for (int c = 0; c < 3; ++c) {
            const float x = rest_positions[3 * (size_t) v + c];
            if (!std::isfinite(x) || (rest_normals && !std::isfinite(rest_normals[3 * (size_t) v + c])))
                return fail(BF_ERR_INVALID, "%s shape %u: non-finite rest value at vertex %u", fn, shape, v);
            morph->rest_abs[c] = std::max(morph->rest_abs[c], std::fabs(x));
        }
    for (uint32_t k = 0; k < n_targets; ++k)
        for (uint32_t v = 0; v < nv; ++v)
            for (int c = 0; c < 3; ++c) {
                const size_t i = 3 * ((size_t) k * nv + v) + c;
                if (!std::isfinite(delta_positions[i]) || (delta_normals && !std::isfinite(delta_normals[i])))
                    return fail(BF_ERR_INVALID, "%s shape %u: non-finite delta of target %u at vertex %u", fn, shape, k, v);
                morph->delta_abs[3 * (size_t) k + c] = std::max(morph->delta_abs[3 * (size_t) k + c], std::fabs(delta_positions[i]));
            }
    BF_ENTER(scene);
    if (nv) {
        // one block: rest positions, rest normals, position deltas, normal deltas
        const size_t vec = (size_t) nv * 12, del = vec * n_targets;
        const size_t bytes = vec * (rest_normals ? 2 : 1) + del * (delta_normals ? 2 : 1);
        const hipError_t he = hipMalloc(&morph->block, bytes);
        if (he != hipSuccess) {
            (void) hipGetLastError();
            return fail(BF_ERR_NOMEM, "%s shape %u: hipMalloc(%zu bytes): %s", fn, shape, bytes, hipGetErrorString(he));
        }
        char *blk = (char *) morph->block;
        size_t at = 0;
        auto put = [&](const float *src, size_t n) -> const float * {
            if (!src) return nullptr;
            char *dst = blk + at;
            at += n;
            return hipMemcpy(dst, src, n, hipMemcpyHostToDevice) == hipSuccess ? (const float *) dst : nullptr;
        };
        morph->rest_pos = put(rest_positions, vec);
        morph->rest_nrm = put(rest_normals, vec);
        morph->dpos = put(delta_positions, del);
        morph->dnrm = put(delta_normals, del);
        if (!morph->rest_pos || !morph->dpos || (rest_normals && !morph->rest_nrm) || (delta_normals && !morph->dnrm))
            return fail(BF_ERR_DEVICE, "%s shape %u: hipMemcpy of %zu bytes: %s", fn, shape, bytes, hipGetErrorString(hipGetLastError()));
    }
    MeshState &m = scene->mesh;
    if (m.morphs.size() < scene->info.n_shapes) m.morphs.resize(scene->info.n_shapes);
    m.morphs[shape] = std::move(morph);      // (the morph it replaces goes with its last handle; hipFree waits for the kernels that read it)
    return BF_OK;
}

bf_status bf_scene_pose_skin(bf_scene *scene, uint32_t shape, const float *bones, void *stream_) {
    if (!scene || !bones) return fail(BF_ERR_INVALID, "%s: null argument", __func__);
    PosedShape p;
    const bf_status st = check_posed_shape(scene, shape, false, nullptr, bones, "bf_scene_pose_skin:", &p);
    return st != BF_OK ? st : pose_shape(scene, p, __func__, reinterpret_cast<hipStream_t>(stream_));
}

bf_status bf_scene_pose_morph(bf_scene *scene, uint32_t shape, const float *weights, const float *bones, void *stream_) {
    if (!scene || !weights) return fail(BF_ERR_INVALID, "%s: null argument", __func__);
    PosedShape p;
    const bf_status st = check_posed_shape(scene, shape, true, weights, bones, "bf_scene_pose_morph:", &p);
    return st != BF_OK ? st : pose_shape(scene, p, __func__, reinterpret_cast<hipStream_t>(stream_));
}

bf_status bf_render_skin_batch_device(bf_scene *scene, const bf_launch *launch, uint32_t n_renders, const uint64_t *seeds, uint32_t n_skinned,
                                      const uint32_t *shapes, const float *const *bones, uint32_t n_shapes, const float *to_world, float *hist_dev,
                                      bf_path_record *records_dev, void *stream_, bf_stats *stats_out) {
    return render_posed_batch(__func__, false, scene, launch, n_renders, seeds, n_skinned, shapes, nullptr, bones, n_shapes, to_world, hist_dev,
                              records_dev, stream_, stats_out);
}

bf_status bf_render_morph_batch_device(bf_scene *scene, const bf_launch *launch, uint32_t n_renders, const uint64_t *seeds, uint32_t n_morphed,
                                       const uint32_t *shapes, const float *const *weights, const float *const *bones, uint32_t n_shapes,
                                       const float *to_world, float *hist_dev, bf_path_record *records_dev, void *stream_, bf_stats *stats_out) {
    return render_posed_batch(__func__, true, scene, launch, n_renders, seeds, n_morphed, shapes, weights, bones, n_shapes, to_world, hist_dev,
                              records_dev, stream_, stats_out);
}

}  // extern "C"
