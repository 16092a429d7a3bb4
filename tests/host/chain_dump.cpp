// chain_dump.cpp -- the chain parser (csrc/ikpso_chain.cpp) on its own: parses a fixed list of
// scenes and prints, for each, parse_chain's status, whether build_dh folded, and every field
// of the resulting ChainHost (floats as their bit patterns).  tests/test_chain_host.py compares
// the output with tests/golden/chain_host.txt.  Links ikpso_chain.cpp and nothing else of the
// library, so it runs without a GPU.
//
// Host sanitizer run (a plain executable, nothing preloaded; CSRC = the package's csrc/):
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -I$CSRC -Iinclude tests/host/chain_dump.cpp $CSRC/ikpso_chain.cpp -o chain_dump_san
//   ./chain_dump_san > /dev/null
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ikpso_chain.h"

using namespace ikpso;

namespace {

struct Scene {
    std::vector<ikpso_node> nodes;
    ikpso_fitness_config fit{3.0f, 0.0f, 0.1f};
    std::vector<uint8_t> mask;
    std::vector<float> positions, soft_lo, soft_hi;
    float limit_weight = 0.0f;
    std::vector<ikpso_collider> colliders;
    bool node_slot = false;
    bool keep_far = false;  // IKPSO_KEEP_FAR_COLLIDERS=1 around the parse
};

const float kTwoPi = 2.0f * (float)M_PI;
const float kPi = (float)M_PI;

ikpso_node make_node(int type, int parent, float length, float rx, float ry, float rz, float lo, float hi)
{
    ikpso_node n{};
    n.node_type = type;
    n.parent_index = parent;
    n.length = length;
    n.rotation[0] = rx, n.rotation[1] = ry, n.rotation[2] = rz;
    for (int c = 0; c < 3; ++c) n.min_rotation[c] = lo, n.max_rotation[c] = hi;
    return n;
}

void make_effector(ikpso_node& n, float tx, float ty, float tz)
{
    n.node_type = IKPSO_NODE_EFFECTOR;
    n.effector_weight = 1.0f;
    n.target_position[0] = tx, n.target_position[1] = ty, n.target_position[2] = tz;
}

// ikpso.reference_scene(): four elbows, three effectors on the last one
Scene reference_tree()
{
    Scene s;
    s.nodes.push_back(make_node(IKPSO_NODE_ORIGIN, -1, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, kTwoPi));
    for (int k = 1; k <= 4; ++k) s.nodes.push_back(make_node(IKPSO_NODE, k - 1, 1.0f, 0.0f, 1.57f, 0.0f, 0.0f, kTwoPi));
    s.nodes.push_back(make_node(IKPSO_NODE, 4, 1.0f, 0.0f, 1.57f, 0.0f, 0.0f, kTwoPi));
    s.nodes.push_back(make_node(IKPSO_NODE, 4, 1.0f, 0.0f, 0.0f, 1.57f, 0.0f, kTwoPi));
    s.nodes.push_back(make_node(IKPSO_NODE, 4, 1.0f, 0.0f, 0.0f, 1.57f, 0.0f, kTwoPi));
    make_effector(s.nodes[5], 0.75f, 1.0f, -2.5f);
    make_effector(s.nodes[6], -0.75f, 1.0f, -2.5f);
    make_effector(s.nodes[7], 0.0f, 0.0f, -2.5f);
    return s;
}

// a serial chain with a tip effector, its origin moved and turned, every node a little different
Scene serial(int joints, float lo = -kPi, float hi = kPi)
{
    Scene s;
    ikpso_node o = make_node(IKPSO_NODE_ORIGIN, -1, 0.0f, 0.2f, -0.4f, 0.6f, lo, hi);
    o.position[0] = 0.1f, o.position[1] = -0.2f, o.position[2] = 0.3f;
    s.nodes.push_back(o);
    for (int k = 1; k <= joints; ++k)
        s.nodes.push_back(make_node(IKPSO_NODE, k - 1, 0.25f + 0.01f * k, 0.05f * k, 0.3f, -0.02f * k, lo, hi));
    make_effector(s.nodes[joints], 0.5f, -0.25f, 1.0f);
    return s;
}

// the 7-joint chain with `free_axes` Euler axes free: the first axes in the order node 1 x,
// node 2 y, node 3 z, node 4 x, ..., then round again from node 1 y
Scene masked7(int free_axes)
{
    Scene s = serial(7);
    s.mask.assign(8, 0);
    for (int i = 0; i < free_axes; ++i) s.mask[1 + i % 7] |= (uint8_t)(1u << ((i % 7 + i / 7) % 3));
    return s;
}

void soft_limits(Scene& s, int dims, bool symmetric)
{
    s.limit_weight = 0.5f;
    for (int d = 0; d < dims; ++d) {
        s.soft_hi.push_back(1.0f + 0.125f * d);
        s.soft_lo.push_back(symmetric ? -s.soft_hi[d] : -0.5f);
    }
}

void distance_term(Scene& s, bool node_slot)
{
    s.fit.distance_weight = 1.5f;
    s.node_slot = node_slot;
    for (size_t i = 0; i < 4 * (s.nodes.size() + 1); ++i) s.positions.push_back(0.25f * (float)i - 3.0f);
}

ikpso_collider make_box(float px, float py, float pz, float qx, float qy, float qz, float qw)
{
    ikpso_collider c{};
    c.x = 1.0f, c.y = 0.5f, c.z = 0.75f;
    c.pos[0] = px, c.pos[1] = py, c.pos[2] = pz;
    c.quat[0] = qx, c.quat[1] = qy, c.quat[2] = qz, c.quat[3] = qw;
    return c;
}

uint32_t bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

void put(const char* name, const std::vector<int>& v)
{
    printf("  %s[%zu]:", name, v.size());
    for (int x : v) printf(" %d", x);
    printf("\n");
}

void put(const char* name, const float* v, size_t n)
{
    printf("  %s[%zu]:", name, n);
    for (size_t i = 0; i < n; ++i) printf(" %08x", bits(v[i]));
    printf("\n");
}

void put(const char* name, const std::vector<float>& v) { put(name, v.data(), v.size()); }

void dump(const char* form, const ChainHost& ch)
{
    static const char* const kTopo[] = {"ref7", "serial_tip", "generic", "dh"};
    printf(" %s: J=%d E=%d topo=%s dof=%d kernel_dims=%d\n", form, ch.J, ch.E, kTopo[(int)ch.topo], ch.dof(),
           ch.kernel_dims());
    put("parent", ch.parent);
    put("eff_slot", ch.eff_slot);
    put("len", ch.len);
    put("eff_w", ch.eff_w);
    put("lo", ch.lo);
    put("hi", ch.hi);
    put("rest", ch.rest);
    put("tgt0", ch.tgt0);
    put("m0", ch.m0, 12);
    const float coef[6] = {ch.w, ch.c1, ch.c2, ch.aw_j, ch.dw_j, ch.lim_w};
    put("w_c1_c2_awj_dwj_limw", coef, 6);
    printf("  use_posref=%d use_penalty=%d uniform_bounds=%d unit_rev_bounds=%d ordered_bounds=%d sym_penalty=%d\n",
           ch.use_posref, ch.use_penalty, ch.uniform_bounds, ch.unit_rev_bounds, ch.ordered_bounds, ch.sym_penalty);
    printf("  num_coll=%d colliders_dropped=%d coll_off=%zu coll_lim_off=%zu coll_box_off=%zu coll_obb=%d\n",
           ch.num_coll, ch.colliders_dropped, ch.coll_off, ch.coll_lim_off, ch.coll_box_off, ch.coll_obb);
    printf("  free_mask=%016llx dfree=%d masked=%d poly_trig=%d dh_off=%zu aux_dev=%s\n",
           (unsigned long long)ch.free_mask, ch.dfree, ch.masked, ch.poly_trig, ch.dh_off, ch.aux_dev ? "set" : "null");
    put("aux", ch.aux);
}

void run(const char* name, const Scene& s)
{
    Extras ex;
    ex.axis_mask = s.mask.empty() ? nullptr : s.mask.data();
    ex.positions = s.positions.empty() ? nullptr : s.positions.data();
    ex.posref_node_slot = s.node_slot;
    ex.limit_weight = s.limit_weight;
    ex.soft_lo = s.soft_lo.empty() ? nullptr : s.soft_lo.data();
    ex.soft_hi = s.soft_hi.empty() ? nullptr : s.soft_hi.data();
    ex.colliders = s.colliders.empty() ? nullptr : s.colliders.data();
    ex.collider_count = (int)s.colliders.size();
    const ikpso_pso_config pso{0.5f, 0.5f, 1.25f, 15};
    if (s.keep_far) setenv("IKPSO_KEEP_FAR_COLLIDERS", "1", 1);
    ChainHost eu, dh;
    const ikpso_status st = parse_chain(s.nodes, pso, s.fit, ex, eu);
    if (s.keep_far) unsetenv("IKPSO_KEEP_FAR_COLLIDERS");
    const bool folded = st == IKPSO_OK && build_dh(s.nodes, eu, ex, dh);
    printf("%s: status=%d folded=%d\n", name, (int)st, folded ? 1 : 0);
    if (st == IKPSO_OK) dump("euler", eu);
    if (folded) dump("folded", dh);
}

}  // namespace

int main()
{
    unsetenv("IKPSO_KEEP_FAR_COLLIDERS");
    Scene s;

    // ---- topology and size
    run("reference_tree", reference_tree());
    for (int j : {5, 6, 14, 15, 20, 21, 32, 33}) {
        char name[32];
        snprintf(name, sizeof name, "serial%d", j);
        run(name, serial(j));
    }
    s = serial(4);  // a 4-joint tree: nodes 3 and 4 both hang off node 2, both effectors
    s.nodes[4].parent_index = 2;
    make_effector(s.nodes[3], -0.5f, 0.25f, 0.5f);
    run("tree4_two_effectors", s);
    s = serial(6);
    s.nodes[3].parent_index = 3;
    run("self_parent", s);

    // ---- axis masks
    run("mask7_one_axis_per_joint", masked7(7));
    run("mask7_two_axes", masked7(2));
    run("mask7_thirteen_axes", masked7(13));
    run("mask7_all_locked", masked7(0));
    s = masked7(7);
    s.mask[3] = 8;
    run("mask7_byte_8", s);
    s = masked7(7);
    distance_term(s, false);
    run("mask7_distance_weight", s);
    s = masked7(7);
    s.colliders.push_back(make_box(0.5f, 0.0f, 0.5f, 0.0f, 0.0f, 0.0f, 1.0f));
    run("mask7_collider_in_reach", s);
    s = masked7(7);
    s.nodes[2].max_rotation[1] = 101.0f;  // a free axis (node 2 y)
    run("mask7_bound_101", s);

    // ---- bounds
    s = serial(7);
    s.nodes[4].max_rotation[2] = 2.5f;
    run("bounds_non_uniform", s);
    run("bounds_uniform_reversed", serial(7, 1.0f, -1.0f));
    run("bounds_101_rad", serial(7, -101.0f, 101.0f));

    // ---- soft limits (given per free dimension)
    s = serial(7, -4.0f, 4.0f);
    soft_limits(s, 21, true);
    run("soft_symmetric", s);
    s = serial(7, -4.0f, 4.0f);
    soft_limits(s, 21, false);
    run("soft_asymmetric", s);
    s = masked7(7);
    soft_limits(s, 7, true);
    run("soft_symmetric_masked", s);
    s = masked7(7);
    soft_limits(s, 7, false);
    run("soft_asymmetric_masked", s);
    s = serial(7, -8.0f, 8.0f);  // symmetric, but more than a revolution inside the clamp bound
    soft_limits(s, 21, true);
    run("soft_symmetric_beyond_revolution", s);

    // ---- distance term
    s = reference_tree();
    distance_term(s, false);
    run("posref_plain_slots", s);
    s = reference_tree();
    distance_term(s, true);
    run("posref_node_slot", s);

    // ---- colliders
    const ikpso_collider near_box = make_box(1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f);
    const ikpso_collider far_box = make_box(100.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f);
    s = reference_tree();
    s.colliders = {near_box};
    run("collider_in_reach", s);
    s.colliders = {far_box};
    run("collider_far", s);
    s.keep_far = true;
    run("collider_far_kept", s);
    s = reference_tree();
    s.colliders = {far_box, near_box, make_box(0.0f, 0.0f, -1.0f, -0.403f, -0.819f, 0.273f, 0.304f)};
    run("collider_far_near_and_quat_1_0001", s);  // |q|^2 = 1.0001: still a box
    s.colliders = {make_box(0.0f, 0.0f, -1.0f, 0.50249378f, 0.50249378f, 0.50249378f, 0.50249378f)};
    run("collider_quat_1_01", s);  // |q|^2 = 1.01: not a box
    s.colliders = {near_box, make_box(NAN, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f)};
    run("collider_centre_not_finite", s);
    return 0;
}
