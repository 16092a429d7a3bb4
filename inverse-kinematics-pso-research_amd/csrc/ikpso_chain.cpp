// ikpso_chain.cpp -- the chain parser (ikpso_chain.h): the reference-order origin
// transform, collider records and boxes, parse_chain, and the fp64 folding
// algebra of build_dh.  No HIP call: tests/host/chain_dump.cpp links this file alone.
#include "ikpso_chain.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <cmath>

#include "ikpso_swarm.h"

namespace ikpso {

bool chain_supported(const ChainHost& ch)
{
    return visit_topology(ch, [](auto) {});
}

namespace {

// ---- reference-order 4x4 host math for the origin transform M0 -----------
// M0 = I * T(position) * Rx * Ry * Rz (src/kernel.cu:36-38), computed with
// the reference's product order so the REFERENCE arithmetic mode reproduces
// it bit for bit.
struct M4 {
    float c[16];
};

M4 m4_create(float f)
{
    M4 m;
    for (float& x : m.c) x = 0.0f;
    for (int i = 0; i < 4; ++i) m.c[i + 4 * i] = f;
    return m;
}

M4 m4_mul(const M4& l, const M4& r)
{
#pragma clang fp contract(off)
    M4 o = m4_create(0.0f);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            float s = 0.0f;
            for (int x = 0; x < 4; ++x) s += l.c[x + j * 4] * r.c[x * 4 + i];
            o.c[i + j * 4] = s;
        }
    return o;
}

// Correctly rounded fp32 sin/cos: what the device REFERENCE mode computes.
float sin_cr(float x) { return (float)sin((double)x); }
float cos_cr(float x) { return (float)cos((double)x); }

M4 origin_matrix(const ikpso_node& n)
{
    M4 m = m4_create(1.0f);
    M4 t = m4_create(1.0f);
    t.c[3] = n.position[0];
    t.c[7] = n.position[1];
    t.c[11] = n.position[2];
    m = m4_mul(m, t);
    const float a = n.rotation[0], b = n.rotation[1], c = n.rotation[2];
    M4 rx = m4_create(1.0f);
    rx.c[5] = cos_cr(a);
    rx.c[6] = -sin_cr(a);
    rx.c[9] = sin_cr(a);
    rx.c[10] = cos_cr(a);
    m = m4_mul(m, rx);
    M4 ry = m4_create(1.0f);
    ry.c[0] = cos_cr(b);
    ry.c[2] = sin_cr(b);
    ry.c[8] = -sin_cr(b);
    ry.c[10] = cos_cr(b);
    m = m4_mul(m, ry);
    M4 rz = m4_create(1.0f);
    rz.c[0] = cos_cr(c);
    rz.c[1] = -sin_cr(c);
    rz.c[4] = sin_cr(c);
    rz.c[5] = cos_cr(c);
    return m4_mul(m, rz);
}

uint32_t as_bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// ---- the folded serial chain (TopoDH), fp64 host algebra ------------------
struct D3 {
    double m[3][3];
};

D3 d3_eye()
{
    D3 r{};
    for (int i = 0; i < 3; ++i) r.m[i][i] = 1.0;
    return r;
}

D3 d3_mul(const D3& a, const D3& b)
{
    D3 r{};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            for (int x = 0; x < 3; ++x) r.m[i][j] += a.m[i][x] * b.m[x][j];
    return r;
}

// Rx / Ry / Rz of the reference (src/matrix_operations.cuh:136-161)
D3 d3_rot(int axis, double t)
{
    D3 r = d3_eye();
    const double c = cos(t), s = sin(t);
    const int i = (axis + 1) % 3, j = (axis + 2) % 3;  // x: (y, z); y: (z, x); z: (x, y)
    r.m[i][i] = c;
    r.m[i][j] = -s;
    r.m[j][i] = s;
    r.m[j][j] = c;
    return r;
}

// Q_c with Q_c Rz(t) Q_c^T = R_c(t): the cyclic permutation taking z to axis c.
D3 d3_q(int c)
{
    D3 r{};
    for (int i = 0; i < 3; ++i) r.m[(i + c + 1) % 3][i] = 1.0;  // Q e_i = e_{(i + c + 1) % 3}
    return r;
}

D3 d3_t(const D3& a)
{
    D3 r{};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r.m[i][j] = a.m[j][i];
    return r;
}

// Device record of one obj_t collider (ikpso_collide.h): the inverse
// quaternion is quatInvert2's (same fp32 operations as the device would do)
// and the radius bounds every support point of the box.
CollRec collider_record(const ikpso_collider& c)
{
    CollRec r{};
    r.px = c.pos[0];
    r.py = c.pos[1];
    r.pz = c.pos[2];
    r.qx = c.quat[0];
    r.qy = c.quat[1];
    r.qz = c.quat[2];
    r.qw = c.quat[3];
    float qi[4];
    quat_inverse(c.quat, qi);
    r.ix = qi[0];
    r.iy = qi[1];
    r.iz = qi[2];
    r.iw = qi[3];
    r.sx = c.x;
    r.sy = c.y;
    r.sz = c.z;
    r.radius = sphere_radius(fabsf(c.x), fabsf(c.y), fabsf(c.z), quat_gain(c.quat[0], c.quat[1], c.quat[2], c.quat[3]));
    return r;
}

// The collider as an oriented box for the FAST separating-axis test (kFastSat): the
// columns of the linear map quatRotVec(., q) (src/kernel.cu:1012-1037) -- the box's
// axes -- computed in fp64, the half extents and the centre: box[0..8] = axes (axis
// c at box[3c..3c+2], normalised), box[9..11] = |x, y, z| / 2 times the columns'
// lengths, box[12..14] = centre.  A quaternion a little off unit length (the
// reference's initColliders box 1 has |q|^2 = 1.0001) makes the map a rotation scaled
// and skewed by ~|q|^2 - 1: below 1e-3 that moves the box's faces by less than GJK's
// own ~3.5e-4 tolerance band; beyond it (false) the FAST builds test it by GJK.
bool collider_box(const ikpso_collider& c, float* box)
{
    const double x = c.quat[0], y = c.quat[1], z = c.quat[2], w = c.quat[3];
    double m[3][3];  // m[row][col]: quatRotVec(e_col)
    for (int col = 0; col < 3; ++col) {
        const double v[3] = {col == 0 ? 1.0 : 0.0, col == 1 ? 1.0 : 0.0, col == 2 ? 1.0 : 0.0};
        const double c1x = y * v[2] - z * v[1] + w * v[0], c1y = z * v[0] - x * v[2] + w * v[1],
                     c1z = x * v[1] - y * v[0] + w * v[2];
        const double c2x = y * c1z - z * c1y, c2y = z * c1x - x * c1z, c2z = x * c1y - y * c1x;
        m[0][col] = v[0] + 2.0 * c2x;
        m[1][col] = v[1] + 2.0 * c2y;
        m[2][col] = v[2] + 2.0 * c2z;
    }
    bool ortho = true;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const double d = m[0][a] * m[0][b] + m[1][a] * m[1][b] + m[2][a] * m[2][b];
            ortho = ortho && fabs(d - (a == b ? 1.0 : 0.0)) <= 1e-3;
        }
    const double half[3] = {0.5 * fabs((double)c.x), 0.5 * fabs((double)c.y), 0.5 * fabs((double)c.z)};
    for (int col = 0; col < 3; ++col) {
        const double n = sqrt(m[0][col] * m[0][col] + m[1][col] * m[1][col] + m[2][col] * m[2][col]);
        ortho = ortho && n > 0.0;
        for (int row = 0; row < 3; ++row) box[3 * col + row] = (float)(n > 0.0 ? m[row][col] / n : 0.0);
        box[9 + col] = (float)(half[col] * n);
    }
    box[12] = c.pos[0];
    box[13] = c.pos[1];
    box[14] = c.pos[2];
    box[15] = 0.0f;
    return ortho;
}

// An empty chain of J joints, its per-node and per-angle tables sized and cleared.
ChainHost sized_chain(int J)
{
    ChainHost ch;
    ch.J = J;
    ch.parent.assign(J + 1, -1);
    ch.eff_slot.assign(J + 1, -1);
    ch.len.assign(J + 1, 0.0f);
    ch.eff_w.assign(J + 1, 0.0f);
    ch.lo.assign(3 * J, 0.0f);
    ch.hi.assign(3 * J, 0.0f);
    ch.rest.assign(3 * J, 0.0f);
    ch.tgt0.assign(3 * J, 0.0f);
    return ch;
}

// The first n angles all have the clamp bounds lo[0], hi[0], bit for bit.
bool uniform_bounds(const ChainHost& ch, int n)
{
    for (int d = 0; d < n; ++d)
        if (as_bits(ch.lo[d]) != as_bits(ch.lo[0]) || as_bits(ch.hi[d]) != as_bits(ch.hi[0])) return false;
    return true;
}

}  // namespace

ikpso_status parse_chain(const std::vector<ikpso_node>& nodes, const ikpso_pso_config& pso,
                         const ikpso_fitness_config& fit, const Extras& ex, ChainHost& ch)
{
    const int n = (int)nodes.size();
    if (n < 2 || n - 1 > kMaxJoints) return IKPSO_ERR_INVALID_ARG;
    const int J = n - 1;
    ch = sized_chain(J);
    int E = 0;
    bool ref7 = (J == 7), serial = true;
    uint64_t eff_mask = 0;
    static const int kRef7[8] = {-1, 0, 1, 2, 3, 4, 4, 4};
    for (int k = 1; k <= J; ++k) {
        const ikpso_node& nd = nodes[k];
        if (nd.parent_index < 0 || nd.parent_index >= k) return IKPSO_ERR_INVALID_ARG;
        ch.parent[k] = nd.parent_index;
        ch.len[k] = nd.length;
        serial = serial && nd.parent_index == k - 1;
        if (J == 7) ref7 = ref7 && nd.parent_index == kRef7[k];
        for (int c = 0; c < 3; ++c) {
            ch.lo[3 * (k - 1) + c] = nd.min_rotation[c];
            ch.hi[3 * (k - 1) + c] = nd.max_rotation[c];
            ch.rest[3 * (k - 1) + c] = nd.rotation[c];
        }
        if (nd.node_type == IKPSO_NODE_EFFECTOR) {
            eff_mask |= 1ull << k;
            ch.eff_slot[k] = E++;
            ch.eff_w[k] = nd.effector_weight;
            for (int c = 0; c < 3; ++c) ch.tgt0[3 * (k - 1) + c] = nd.target_position[c];
        }
    }
    ch.E = E;
    // joint-axis mask: bit d = 3(k-1)+c of free_mask when Euler angle c of node k is free
    ch.free_mask = 0;
    for (int k = 1; k <= J; ++k)
        for (int c = 0; c < 3; ++c) {
            const int d = 3 * (k - 1) + c;
            if (d >= 64) break;  // > 21 joints: no compiled kernel (rejected below)
            if (!ex.axis_mask || ((ex.axis_mask[k] >> c) & 1)) ch.free_mask |= 1ull << d;
        }
    for (int k = 1; k <= J && ex.axis_mask; ++k)
        if (ex.axis_mask[k] > 7) return IKPSO_ERR_INVALID_ARG;
    ch.dfree = __builtin_popcountll(ch.free_mask);
    ch.masked = 3 * J <= 64 && ch.dfree != 3 * J;
    if (ch.dfree == 0) return IKPSO_ERR_INVALID_ARG;  // nothing to optimise
    ch.uniform_bounds = uniform_bounds(ch, 3 * J);
    // [0, 2pi] limits are [0, 1] in revolutions (ChainConsts::rlo / rhi, the same fp32 products)
    volatile float inv = 0.159154943091895336f;  // (no contraction or constant folding differences)
    const float rlo = ch.lo[0] * inv, rhi = ch.hi[0] * inv;
    ch.unit_rev_bounds = ch.uniform_bounds && rlo == 0.0f && rhi == 1.0f;
    ch.ordered_bounds = ch.uniform_bounds && std::isfinite(ch.lo[0]) && std::isfinite(ch.hi[0]) &&
                        ch.lo[0] <= ch.hi[0];
    ref7 = ref7 && eff_mask == 0xE0ull;                // effectors = nodes 5, 6, 7
    serial = serial && eff_mask == (1ull << J);        // single tip effector
    ch.topo = ref7 ? TopoKind::Ref7 : (serial ? TopoKind::SerialTip : TopoKind::Generic);
    const M4 m0 = origin_matrix(nodes[0]);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) ch.m0[4 * r + c] = m0.c[4 * r + c];
    ch.w = pso.inertia;
    ch.c1 = pso.local;
    ch.c2 = pso.global;
    // fitConfig.{angle,distance}Weight / (DEGREES_OF_FREEDOM / 3) (src/kernel.cu:150)
    ch.aw_j = fit.angle_weight / (float)J;
    ch.dw_j = fit.distance_weight / (float)J;
    ch.use_posref = fit.distance_weight != 0.0f;
    ch.lim_w = ex.limit_weight;
    ch.use_penalty = ex.limit_weight != 0.0f && ex.soft_lo && ex.soft_hi;
    // aux = [posref 4J | soft_lo 3J | soft_hi 3J | pad to 16 floats | collider records | near limits |
    //        collider boxes], the colliders being those within the arm's reach (below)
    //
    // near_collider's limit for node k and collider c (ikpso_collide.h): one sphere around
    // the node's link box and node box, centred at the link's midpoint, that any box pair
    // node_collides would test lies within.  Every node position is within
    // |origin| + sum |len| of the frame's origin (a bound on the exact test's |centre|_1
    // margin term through |a|_1 <= sqrt(3) |a|).
    //
    // Host-side pruning: every node (and link midpoint) lies within the arm's length sum
    // sum_k |len_k| of the origin's position, so a collider farther from it than that plus
    // near_collider's limit for every node can never pass the inline sphere test, let
    // alone the exact one (the margin covers the fp32 FK's rounding, ~1e-6 of the reach):
    // it can never contribute to any fitness, and is left out.  With none left the chain
    // is solved without the term, by the plain kernels -- bit-identical answers in
    // REFERENCE arithmetic (the same reference operation order), and in FAST the plain
    // kernels' own arithmetic.  IKPSO_KEEP_FAR_COLLIDERS=1 keeps every collider (to time
    // the collider kernels with nothing near).
    double reach = sqrt((double)ch.m0[3] * ch.m0[3] + (double)ch.m0[7] * ch.m0[7] + (double)ch.m0[11] * ch.m0[11]);
    double arm = 0.0;
    for (int k = 1; k <= J; ++k) arm += fabs((double)ch.len[k]);
    reach = (reach + arm) * 1.001;
    const double gb = (double)kGainBound, lw = (double)kGizmo * 0.25;
    const double rn = 0.5 * sqrt(3.0) * (double)kGizmo * gb;
    const int nin = ex.collider_count;
    std::vector<CollRec> recs(nin);
    std::vector<float> lims((size_t)nin * J);
    std::vector<int> kept;
    const char* keep = getenv("IKPSO_KEEP_FAR_COLLIDERS");
    const bool keep_all = keep && keep[0] == '1';
    for (int i = 0; i < nin; ++i) {
        const CollRec r = recs[i] = collider_record(ex.colliders[i]);
        if (!std::isfinite(r.radius) || !std::isfinite(r.px) || !std::isfinite(r.py) || !std::isfinite(r.pz))
            return IKPSO_ERR_INVALID_ARG;
        const double c1 = fabs((double)r.px) + fabs((double)r.py) + fabs((double)r.pz);
        const double dx = (double)r.px - ch.m0[3], dy = (double)r.py - ch.m0[7], dz = (double)r.pz - ch.m0[11];
        const double dist = sqrt(dx * dx + dy * dy + dz * dz);
        const double margin = 1e-3 + 1e-4 * (arm + dist + c1);
        bool reachable = false;
        for (int k = 1; k <= J; ++k) {
            const double len = fabs((double)ch.len[k]);
            const double rl = 0.5 * sqrt(len * len + 2.0 * lw * lw) * gb;
            const double rk = std::max(rl, 0.5 * len * 1.00001 + rn);
            const double reach_kc = rk + (double)r.radius;
            const double lim = (reach_kc + 1e-3 + 1e-4 * (sqrt(3.0) * reach + c1 + reach_kc)) * 1.0001;
            if (!std::isfinite(lim)) return IKPSO_ERR_INVALID_ARG;
            lims[(size_t)i * J + (k - 1)] = (float)(lim * lim);
            reachable = reachable || dist - arm <= sqrt((double)lims[(size_t)i * J + (k - 1)]) + margin;
        }
        if (reachable || keep_all) kept.push_back(i);
    }
    ch.colliders_dropped = nin - (int)kept.size();
    ch.num_coll = (int)kept.size();
    ch.coll_index = kept;
    ch.coll_given = nin;
    ch.coll_off = ((size_t)10 * J + 15) & ~size_t(15);
    ch.coll_lim_off = ch.coll_off + (size_t)16 * ch.num_coll;
    ch.coll_box_off = (ch.coll_lim_off + (size_t)J * ch.num_coll + 15) & ~size_t(15);
    ch.aux.assign(ch.coll_box_off + (size_t)16 * ch.num_coll, 0.0f);
    for (int j = 0; j < ch.num_coll; ++j) {
        const int i = kept[j];
        memcpy(ch.aux.data() + ch.coll_off + 16 * (size_t)j, &recs[i], sizeof(CollRec));
        ch.coll_obb = ch.coll_obb && collider_box(ex.colliders[i], ch.aux.data() + ch.coll_box_off + 16 * (size_t)j);
        for (int k = 1; k <= J; ++k)
            ch.aux[ch.coll_lim_off + (size_t)(k - 1) * ch.num_coll + j] = lims[(size_t)i * J + (k - 1)];
    }
    if (ch.use_posref && ex.positions)
        for (int i = 0; i < 4 * J; ++i) ch.aux[i] = ex.positions[i + (ex.posref_node_slot ? 8 : 0)];
    if (ch.use_penalty)  // soft limits are given per free dimension; a locked angle adds max(-inf, 0)^2 = 0
        for (int d = 0, r = 0; d < 3 * J; ++d) {
            const bool fr = d < 64 && ((ch.free_mask >> d) & 1);
            ch.aux[4 * J + d] = fr ? ex.soft_lo[r] : -INFINITY;
            ch.aux[7 * J + d] = fr ? ex.soft_hi[r] : INFINITY;
            r += fr;
        }
    // the transcendental unit's range (kHwTrigMaxAbs): every evaluated angle is
    // clamped to [lo, hi] after the first update, the warm start is the rest pose
    for (int d = 0; d < 3 * J && d < 64; ++d)
        if ((ch.free_mask >> d) & 1)
            ch.poly_trig = ch.poly_trig || !(fabsf(ch.lo[d]) <= kHwTrigMaxAbs) || !(fabsf(ch.hi[d]) <= kHwTrigMaxAbs) ||
                           !(fabsf(ch.rest[d]) <= kHwTrigMaxAbs);
    // symmetric soft limits within one revolution of every clamp bound (kTermSymPenalty): checked in the
    // kernels' revolution units, where the overshoot |x| - h of a clamped angle is <= 1
    if (ch.use_penalty && ch.uniform_bounds) {
        const float rmax = fmaxf(fabsf(rlo), fabsf(rhi));
        ch.sym_penalty = true;
        for (int d = 0; d < 3 * J; ++d) {
            const float slo = ch.aux[4 * J + d], shi = ch.aux[7 * J + d];
            ch.sym_penalty = ch.sym_penalty && as_bits(slo) == (as_bits(shi) ^ 0x80000000u) && shi >= 0.0f &&
                             rmax - shi * inv <= 1.0f;
        }
    }
    if (!chain_supported(ch)) return IKPSO_ERR_UNSUPPORTED;
    return IKPSO_OK;
}

// Number of compiled TopoDH instantiations (ikpso_inst_dh_*.hip).
constexpr int kDHMin = 3, kDHMax = 12;

// The folded form of a masked serial chain with a tip effector (TopoDH, FAST
// kernels): every free Euler axis becomes one joint W_j = W_{j-1} C_j Rz(t_j),
// q_j = q_{j-1} + W_j s_j (see TopoDH).  The constants are products of the
// locked rotations (at their rest angles), the axis permutations Q_c, the
// origin transform and the link translations, multiplied out in fp64 and
// rounded once.  False when the chain does not fold (tree, several effectors,
// distance or collider term, no compiled width).
bool build_dh(const std::vector<ikpso_node>& nodes, const ChainHost& eu, const Extras& ex, ChainHost& dh)
{
    const int J = eu.J, N = eu.dfree;
    if (eu.topo != TopoKind::SerialTip || eu.use_posref || eu.num_coll > 0 || !eu.masked || eu.poly_trig) return false;
    if (N < kDHMin || N > kDHMax) return false;
    const ikpso_node& o = nodes[0];
    D3 g = d3_mul(d3_mul(d3_rot(0, o.rotation[0]), d3_rot(1, o.rotation[1])), d3_rot(2, o.rotation[2]));
    double sc[3] = {o.position[0], o.position[1], o.position[2]};  // offset in the current joint frame
    std::vector<D3> C;
    std::vector<std::array<double, 3>> S;
    std::array<double, 3> q0{};
    for (int k = 1; k <= J; ++k) {
        for (int c = 0; c < 3; ++c) {
            const int d = 3 * (k - 1) + c;
            if ((eu.free_mask >> d) & 1) {
                if (C.empty())
                    q0 = {sc[0], sc[1], sc[2]};
                else
                    S.back() = {sc[0], sc[1], sc[2]};
                C.push_back(d3_mul(g, d3_q(c)));
                S.push_back({0.0, 0.0, 0.0});
                g = d3_t(d3_q(c));
                sc[0] = sc[1] = sc[2] = 0.0;
            } else {
                g = d3_mul(g, d3_rot(c, nodes[k].rotation[c]));
            }
        }
        const double len = nodes[k].length;  // T(len, 0, 0) after the node's rotation
        for (int r = 0; r < 3; ++r) sc[r] += len * g.m[r][0];
    }
    S.back() = {sc[0], sc[1], sc[2]};
    dh = sized_chain(N);
    dh.E = 1;
    dh.topo = TopoKind::DH;
    for (int k = 1; k <= N; ++k) dh.parent[k] = k - 1;
    dh.eff_slot[N] = 0;
    dh.eff_w[N] = eu.eff_w[J];
    for (int c = 0; c < 3; ++c) dh.tgt0[3 * (N - 1) + c] = eu.tgt0[3 * (J - 1) + c];
    for (int d = 0, r = 0; d < 3 * J; ++d)
        if ((eu.free_mask >> d) & 1) {
            dh.lo[r] = eu.lo[d];
            dh.hi[r] = eu.hi[d];
            dh.rest[r] = eu.rest[d];
            ++r;
        }
    dh.uniform_bounds = uniform_bounds(dh, N);
    dh.w = eu.w;
    dh.c1 = eu.c1;
    dh.c2 = eu.c2;
    dh.aw_j = eu.aw_j;  // angleWeight / node count of the chain, as calculateDistance
    dh.dw_j = 0.0f;
    dh.use_posref = false;
    dh.lim_w = eu.lim_w;
    dh.use_penalty = eu.use_penalty;
    dh.coll_off = ((size_t)10 * N + 15) & ~size_t(15);
    dh.dh_off = dh.coll_off;
    dh.aux.assign(dh.dh_off + 12 * (size_t)N + 4, 0.0f);
    if (dh.use_penalty)
        for (int d = 0, r = 0; d < 3 * J; ++d)
            if ((eu.free_mask >> d) & 1) {
                dh.aux[4 * N + r] = ex.soft_lo[r];
                dh.aux[7 * N + r] = ex.soft_hi[r];
                ++r;
            }
    dh.free_mask = (1ull << N) - 1;
    dh.dfree = N;
    dh.masked = false;
    float* dc = dh.aux.data() + dh.dh_off;
    for (int j = 0; j < N; ++j) {
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) dc[12 * j + 3 * r + c] = (float)C[j].m[r][c];
        for (int r = 0; r < 3; ++r) dc[12 * j + 9 + r] = (float)S[j][r];
    }
    for (int r = 0; r < 3; ++r) dc[12 * N + r] = (float)q0[r];
    for (int r = 0; r < 3; ++r)  // what the loop left in g: G (ChainHost::tip_rot)
        for (int c = 0; c < 3; ++c) dh.tip_rot[3 * r + c] = (float)g.m[r][c];
    return chain_supported(dh);
}

bool aim_axis_folded(const ChainHost& ch, const float axis[3], float out[3])
{
    const double a[3] = {(double)axis[0], (double)axis[1], (double)axis[2]};
    const double n = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    if (!std::isfinite(n) || !(n >= 1e-6)) return false;  // (a NaN or infinite component makes n so)
    for (int r = 0; r < 3; ++r)
        out[r] = (float)(((double)ch.tip_rot[3 * r] * a[0] + (double)ch.tip_rot[3 * r + 1] * a[1] +
                          (double)ch.tip_rot[3 * r + 2] * a[2]) /
                         n);
    return true;
}

}  // namespace ikpso
