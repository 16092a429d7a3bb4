/* evalframes_c.c -- ikpso_solver_evaluate_frames from plain C: B copies of the reference tree (four
 * elbows, three wrist effectors) follow a few pose waypoints with ikpso_solve_track_frames, then the
 * answers go back to the device with each frame's start pose as `rest` and the same targets and
 * weights.  The entry returns the fitness the solve minimised (orientation term included), every
 * node's rotation and, per wrist, |R - R_target|_F^2 = 4 (1 - cos theta): the mean angle theta of each
 * wrist to its target is printed from it.  Exits 3 if the entry's fitness and the solve's differ by more
 * than 1e-3 of the fitness (the FAST tolerance on a fitness) plus four times what a float and a double
 * evaluation of the header's expression differ by on the host.
 * usage: evalframes_c [B] [iterations per frame] [weight of effectors 0, 1, 2] */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ikpso.h"

#define CHECK_HIP(x)                                                                   \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) {                                                        \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_));  \
            return 1;                                                                  \
        }                                                                              \
    } while (0)
#define CHECK_IK(x)                                                                          \
    do {                                                                                     \
        ikpso_status s_ = (x);                                                               \
        if (s_ != IKPSO_OK) {                                                                \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, ikpso_status_string(s_));      \
            return 1;                                                                        \
        }                                                                                    \
    } while (0)

#define NODES 8
#define EFF 3
#define DOF 21
#define FRAMES 3
#define REL 1e-3 /* the FAST tolerance on a fitness */

static const int kParent[NODES] = {-1, 0, 1, 2, 3, 4, 4, 4};

static void reference_arm(ikpso_node* n)
{
    static const float rest[NODES][3] = {{0, 0, 0},     {0, 1.57f, 0}, {0, 1.57f, 0}, {0, 1.57f, 0},
                                         {0, 1.57f, 0}, {0, 1.57f, 0}, {0, 0, 1.57f}, {0, 0, 1.57f}};
    const float two_pi = 2.0f * 3.14159265358979323846f;
    memset(n, 0, sizeof(ikpso_node) * NODES);
    for (int k = 0; k < NODES; ++k) {
        n[k].node_type = k == 0 ? IKPSO_NODE_ORIGIN : (k >= 5 ? IKPSO_NODE_EFFECTOR : IKPSO_NODE);
        n[k].parent_index = kParent[k];
        n[k].effector_weight = k >= 5 ? 1.0f : 0.0f;
        for (int c = 0; c < 3; ++c) {
            n[k].rotation[c] = rest[k][c];
            n[k].max_rotation[c] = two_pi;
        }
        n[k].length = k == 0 ? 0.0f : 1.0f;
    }
}

/* The header's definitions in one precision: world frames and positions of the three effectors (nodes
 * 5, 6, 7) for 21 Euler angles -- the origin's Rx Ry Rz, then Rx Ry Rz of every node down the path; a
 * link moves along the x column -- and the fitness of ikpso_solve_track_frames on them. */
#define DEFINE_TREE(real, SFX, SIN, COS)                                                                        \
    static void turn##SFX(real R[9], int axis, real t) /* R <- R * R_axis(t) */                                 \
    {                                                                                                           \
        const int i = (axis + 1) % 3, j = (axis + 2) % 3;                                                       \
        const real c = COS(t), s = SIN(t);                                                                      \
        for (int r = 0; r < 3; ++r) {                                                                           \
            const real a = R[3 * r + i], b = R[3 * r + j];                                                      \
            R[3 * r + i] = a * c + b * s;                                                                       \
            R[3 * r + j] = b * c - a * s;                                                                       \
        }                                                                                                       \
    }                                                                                                           \
    static void tree_pose##SFX(const ikpso_node* n, const float* q, real R[EFF][9], real p[EFF][3])             \
    {                                                                                                           \
        real Rn[NODES][9], pn[NODES][3];                                                                        \
        memset(Rn[0], 0, sizeof(Rn[0]));                                                                        \
        Rn[0][0] = Rn[0][4] = Rn[0][8] = 1;                                                                     \
        for (int c = 0; c < 3; ++c) {                                                                           \
            turn##SFX(Rn[0], c, (real)n[0].rotation[c]);                                                        \
            pn[0][c] = (real)n[0].position[c];                                                                  \
        }                                                                                                       \
        for (int k = 1; k < NODES; ++k) {                                                                       \
            memcpy(Rn[k], Rn[kParent[k]], sizeof(Rn[k]));                                                       \
            for (int c = 0; c < 3; ++c) turn##SFX(Rn[k], c, (real)q[3 * (k - 1) + c]);                          \
            for (int c = 0; c < 3; ++c) pn[k][c] = pn[kParent[k]][c] + (real)n[k].length * Rn[k][3 * c];        \
        }                                                                                                       \
        for (int e = 0; e < EFF; ++e) {                                                                         \
            memcpy(R[e], Rn[5 + e], sizeof(R[e]));                                                              \
            memcpy(p[e], pn[5 + e], sizeof(p[e]));                                                              \
        }                                                                                                       \
    }                                                                                                           \
    static real tree_fitness##SFX(const ikpso_node* n, float angle_weight, const float* q, const float* rest,   \
                                  const float* tg, const float* rot, const float* w)                            \
    {                                                                                                           \
        real R[EFF][9], p[EFF][3], position = 0, angle = 0, orient = 0;                                         \
        tree_pose##SFX(n, q, R, p);                                                                             \
        for (int e = 0; e < EFF; ++e) {                                                                         \
            real d2 = 0, r2 = 0;                                                                                \
            for (int c = 0; c < 3; ++c) d2 += (p[e][c] - (real)tg[3 * e + c]) * (p[e][c] - (real)tg[3 * e + c]); \
            for (int c = 0; c < 9; ++c) r2 += (R[e][c] - (real)rot[9 * e + c]) * (R[e][c] - (real)rot[9 * e + c]); \
            position += (real)n[5 + e].effector_weight * d2;                                                    \
            if (w[e] != 0.0f) orient += (real)n[5 + e].effector_weight * (real)w[e] * r2;                       \
        }                                                                                                       \
        for (int d = 0; d < DOF; ++d) angle += ((real)rest[d] - (real)q[d]) * ((real)rest[d] - (real)q[d]);     \
        return (position + (real)angle_weight / (real)(NODES - 1) * angle) + orient;                            \
    }
DEFINE_TREE(double, _d, sin, cos)
DEFINE_TREE(float, _f, sinf, cosf)

int main(int argc, char** argv)
{
    const int B = argc > 1 ? atoi(argv[1]) : 16;
    const int iters = argc > 2 ? atoi(argv[2]) : 100;
    float weights[EFF] = {1.0f, 1.0f, 1.0f}; /* host memory: one weight per effector */
    for (int e = 0; e < EFF; ++e)
        if (argc > 3 + e) weights[e] = (float)atof(argv[3 + e]);
    const int P = 1024, D = DOF, T = FRAMES;
    const float angle_weight = 0.05f;
    if (B <= 0 || iters < 0) return 1;
    ikpso_node chain[NODES];
    reference_arm(chain);

    /* waypoints: the effector frames of joint vectors a little way from the rest pose, inside [0, 2 pi] */
    const size_t nb = (size_t)T * B;
    float* h_tg = (float*)malloc(sizeof(float) * nb * EFF * 3);
    float* h_rot = (float*)malloc(sizeof(float) * nb * EFF * 9);
    for (int t = 0; t < T; ++t)
        for (int b = 0; b < B; ++b) {
            const size_t cell = (size_t)t * B + b;
            float q[DOF];
            double R[EFF][9], p[EFF][3];
            for (int d = 0; d < D; ++d)
                q[d] = chain[1 + d / 3].rotation[d % 3] + (float)(0.35 * (0.5 + 0.5 * sin(1.7 * d + 0.9 * b + 0.3 * t)));
            tree_pose_d(chain, q, R, p);
            for (int e = 0; e < EFF; ++e) {
                for (int c = 0; c < 3; ++c) h_tg[(cell * EFF + e) * 3 + c] = (float)p[e][c];
                for (int c = 0; c < 9; ++c) h_rot[(cell * EFF + e) * 9 + c] = (float)R[e][c];
            }
        }
    float *d_tg, *d_rot, *d_ang, *d_fit, *d_rest, *d_efit, *d_erot, *d_eerr;
    CHECK_HIP(hipMalloc((void**)&d_tg, sizeof(float) * nb * EFF * 3));
    CHECK_HIP(hipMalloc((void**)&d_rot, sizeof(float) * nb * EFF * 9));
    CHECK_HIP(hipMemcpy(d_tg, h_tg, sizeof(float) * nb * EFF * 3, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_rot, h_rot, sizeof(float) * nb * EFF * 9, hipMemcpyHostToDevice));
    CHECK_HIP(hipMalloc((void**)&d_ang, sizeof(float) * nb * D));
    CHECK_HIP(hipMalloc((void**)&d_fit, sizeof(float) * nb));
    CHECK_HIP(hipMalloc((void**)&d_rest, sizeof(float) * nb * D));
    CHECK_HIP(hipMalloc((void**)&d_efit, sizeof(float) * nb));
    CHECK_HIP(hipMalloc((void**)&d_erot, sizeof(float) * nb * (NODES - 1) * 9));
    CHECK_HIP(hipMalloc((void**)&d_eerr, sizeof(float) * nb * EFF));

    ikpso_solver_desc desc;
    memset(&desc, 0, sizeof(desc));
    desc.chain = chain;
    desc.node_count = NODES;
    desc.particles = P;
    desc.pso.inertia = 0.5f;
    desc.pso.local = 0.5f;
    desc.pso.global = 1.25f;
    desc.pso.iterations = iters;
    desc.fit.angle_weight = angle_weight;
    desc.fit.error_threshold = 0.1f;
    desc.kernel = IKPSO_KERNEL_RESIDENT;
    ikpso_solver* s;
    CHECK_IK(ikpso_solver_create(&desc, &s));
    CHECK_IK(ikpso_solver_seed(s, B, 0, 0, NULL));
    CHECK_IK(ikpso_solve_track_frames(s, d_tg, d_rot, weights, NULL, B, T, iters, -1.0f, d_ang, d_fit, NULL, NULL,
                                      NULL));

    /* frame t started from frame t - 1's answer, frame 0 from the chain's rotations: that is `rest` */
    float* h_ang = (float*)malloc(sizeof(float) * nb * D);
    float* h_rest = (float*)malloc(sizeof(float) * nb * D);
    float* h_fit = (float*)malloc(sizeof(float) * nb);
    CHECK_HIP(hipMemcpy(h_ang, d_ang, sizeof(float) * nb * D, hipMemcpyDeviceToHost)); /* waits for the solve */
    CHECK_HIP(hipMemcpy(h_fit, d_fit, sizeof(float) * nb, hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b)
        for (int d = 0; d < D; ++d) h_rest[(size_t)b * D + d] = chain[1 + d / 3].rotation[d % 3];
    memcpy(h_rest + (size_t)B * D, h_ang, sizeof(float) * (nb - B) * D);
    CHECK_HIP(hipMemcpy(d_rest, h_rest, sizeof(float) * nb * D, hipMemcpyHostToDevice));

    CHECK_IK(ikpso_solver_evaluate_frames(s, d_ang, d_tg, d_rest, d_rot, weights, (int64_t)nb, d_efit, NULL, d_erot,
                                          d_eerr, NULL));
    float* h_efit = (float*)malloc(sizeof(float) * nb);
    float* h_eerr = (float*)malloc(sizeof(float) * nb * EFF);
    float* h_erot = (float*)malloc(sizeof(float) * nb * (NODES - 1) * 9);
    CHECK_HIP(hipMemcpy(h_efit, d_efit, sizeof(float) * nb, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(h_eerr, d_eerr, sizeof(float) * nb * EFF, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(h_erot, d_erot, sizeof(float) * nb * (NODES - 1) * 9, hipMemcpyDeviceToHost));

    /* the tolerance's floor: four times the spread of a float evaluation of the same expression */
    double spread = 0.0;
    for (size_t cell = 0; cell < nb; ++cell) {
        const float *q = h_ang + cell * D, *r = h_rest + cell * D, *tg = h_tg + cell * EFF * 3, *rt = h_rot + cell * EFF * 9;
        const double f64 = tree_fitness_d(chain, angle_weight, q, r, tg, rt, weights);
        const double f32 = (double)tree_fitness_f(chain, angle_weight, q, r, tg, rt, weights);
        spread = fmax(spread, fabs(f32 - f64));
    }
    const double floor_ = 4.0 * spread;

    double angle[EFF] = {0.0, 0.0, 0.0}, worst = 0.0, worst_tol = 0.0;
    int finite = 1, agree = 1;
    for (size_t cell = 0; cell < nb; ++cell) {
        for (int e = 0; e < EFF; ++e) { /* |R - T|_F^2 = 4 (1 - cos theta) */
            const double c = 1.0 - (double)h_eerr[cell * EFF + e] / 4.0;
            angle[e] += acos(fmax(-1.0, fmin(1.0, c))) / (double)nb;
            finite &= isfinite(h_eerr[cell * EFF + e]);
        }
        const double want = (double)h_fit[cell], diff = fabs((double)h_efit[cell] - want);
        finite &= isfinite(h_efit[cell]) && isfinite(h_fit[cell]);
        if (diff > REL * want + floor_) agree = 0;
        if (diff >= worst) worst = diff, worst_tol = REL * want + floor_;
    }
    printf("kernel %s: %d trees x %d waypoints x %d iterations, weights %g %g %g\n", ikpso_solver_kernel_name(s), B, T,
           iters, weights[0], weights[1], weights[2]);
    for (int e = 0; e < EFF; ++e) printf("wrist %d: angle to target %.6f rad\n", e, angle[e]);
    printf("wrist 0 of tree 0, last waypoint, x axis: %.4f %.4f %.4f\n", h_erot[((nb - B) * (NODES - 1) + 4) * 9 + 0],
           h_erot[((nb - B) * (NODES - 1) + 4) * 9 + 3], h_erot[((nb - B) * (NODES - 1) + 4) * 9 + 6]);
    printf("fitness: evaluate_frames against the solve, max |difference| %.3e (tolerance there %.3e, floor %.3e)\n",
           worst, worst_tol, floor_);
    printf("finite %d agree %d\n", finite, agree);
    ikpso_solver_destroy(s);
    return !finite ? 2 : (agree ? 0 : 3);
}
