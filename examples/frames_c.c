/* frames_c.c -- ikpso_solve_track_frames from plain C: B copies of the reference tree (four elbows,
 * three wrist effectors) follow a few waypoints each in one call, every effector given a position AND
 * the orientation its node frame should have.  The targets are the effector frames of joint vectors
 * inside the limits, so each is reachable.  A second solver, seeded alike, runs the same call with
 * every weight 0 (position-only IK, ikpso_solve_track's kernel); per effector the mean angle between
 * the node frame and its target is printed for both, and the mean position error.
 * usage: frames_c [B] [iterations per frame] [weight of effectors 0, 1, 2] */
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
#define FRAMES 2

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

static void turn(double R[9], int axis, double t) /* R <- R * R_axis(t) */
{
    const int i = (axis + 1) % 3, j = (axis + 2) % 3;
    const double c = cos(t), s = sin(t);
    for (int r = 0; r < 3; ++r) {
        const double a = R[3 * r + i], b = R[3 * r + j];
        R[3 * r + i] = a * c + b * s;
        R[3 * r + j] = b * c - a * s;
    }
}

/* World frames and positions of the three effectors (nodes 5, 6, 7) for 21 Euler angles, in double:
 * the origin's Rx Ry Rz, then Rx Ry Rz of every node down the path; a link moves along the x column. */
static void tree_pose(const ikpso_node* n, const float* q, double R[EFF][9], double p[EFF][3])
{
    double Rn[NODES][9], pn[NODES][3];
    memset(Rn[0], 0, sizeof(Rn[0]));
    Rn[0][0] = Rn[0][4] = Rn[0][8] = 1.0;
    for (int c = 0; c < 3; ++c) {
        turn(Rn[0], c, n[0].rotation[c]);
        pn[0][c] = n[0].position[c];
    }
    for (int k = 1; k < NODES; ++k) {
        memcpy(Rn[k], Rn[kParent[k]], sizeof(Rn[k]));
        for (int c = 0; c < 3; ++c) turn(Rn[k], c, (double)q[3 * (k - 1) + c]);
        for (int c = 0; c < 3; ++c) pn[k][c] = pn[kParent[k]][c] + (double)n[k].length * Rn[k][3 * c];
    }
    for (int e = 0; e < EFF; ++e) {
        memcpy(R[e], Rn[5 + e], sizeof(R[e]));
        memcpy(p[e], pn[5 + e], sizeof(p[e]));
    }
}

int main(int argc, char** argv)
{
    const int B = argc > 1 ? atoi(argv[1]) : 32;
    const int iters = argc > 2 ? atoi(argv[2]) : 100;
    float weights[EFF] = {1.0f, 1.0f, 1.0f}; /* host memory: one weight per effector */
    const float none[EFF] = {0.0f, 0.0f, 0.0f};
    for (int e = 0; e < EFF; ++e)
        if (argc > 3 + e) weights[e] = (float)atof(argv[3 + e]);
    const int P = 1024, D = DOF, T = FRAMES;
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
            tree_pose(chain, q, R, p);
            for (int e = 0; e < EFF; ++e) {
                for (int c = 0; c < 3; ++c) h_tg[(cell * EFF + e) * 3 + c] = (float)p[e][c];
                for (int c = 0; c < 9; ++c) h_rot[(cell * EFF + e) * 9 + c] = (float)R[e][c];
            }
        }
    float *d_tg, *d_rot, *d_ang[2], *d_fit[2], *d_res[2];
    CHECK_HIP(hipMalloc((void**)&d_tg, sizeof(float) * nb * EFF * 3));
    CHECK_HIP(hipMalloc((void**)&d_rot, sizeof(float) * nb * EFF * 9));
    CHECK_HIP(hipMemcpy(d_tg, h_tg, sizeof(float) * nb * EFF * 3, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_rot, h_rot, sizeof(float) * nb * EFF * 9, hipMemcpyHostToDevice));
    for (int i = 0; i < 2; ++i) {
        CHECK_HIP(hipMalloc((void**)&d_ang[i], sizeof(float) * nb * D));
        CHECK_HIP(hipMalloc((void**)&d_fit[i], sizeof(float) * nb));
        CHECK_HIP(hipMalloc((void**)&d_res[i], sizeof(float) * nb));
    }

    ikpso_solver_desc desc;
    memset(&desc, 0, sizeof(desc));
    desc.chain = chain;
    desc.node_count = NODES;
    desc.particles = P;
    desc.pso.inertia = 0.5f;
    desc.pso.local = 0.5f;
    desc.pso.global = 1.25f;
    desc.pso.iterations = iters;
    desc.fit.angle_weight = 0.0f; /* pose IK: nothing pulls towards the start pose */
    desc.fit.error_threshold = 0.1f;
    desc.kernel = IKPSO_KERNEL_RESIDENT;
    ikpso_solver* s[2];
    for (int i = 0; i < 2; ++i) {
        CHECK_IK(ikpso_solver_create(&desc, &s[i]));
        CHECK_IK(ikpso_solver_seed(s[i], B, 0, 0, NULL));
    }
    /* orientation targets per effector, and the twin with the term switched off */
    CHECK_IK(ikpso_solve_track_frames(s[0], d_tg, d_rot, weights, NULL, B, T, iters, -1.0f, d_ang[0], d_fit[0],
                                      d_res[0], NULL, NULL));
    CHECK_IK(ikpso_solve_track_frames(s[1], d_tg, d_rot, none, NULL, B, T, iters, -1.0f, d_ang[1], d_fit[1], d_res[1],
                                      NULL, NULL));
    CHECK_HIP(hipDeviceSynchronize());

    float* h_ang = (float*)malloc(sizeof(float) * nb * D);
    float* h_res = (float*)malloc(sizeof(float) * nb);
    double pos_err[2], ang_err[2][EFF];
    int finite = 1;
    for (int i = 0; i < 2; ++i) {
        CHECK_HIP(hipMemcpy(h_ang, d_ang[i], sizeof(float) * nb * D, hipMemcpyDeviceToHost));
        CHECK_HIP(hipMemcpy(h_res, d_res[i], sizeof(float) * nb, hipMemcpyDeviceToHost));
        pos_err[i] = 0.0;
        for (int e = 0; e < EFF; ++e) ang_err[i][e] = 0.0;
        for (size_t cell = 0; cell < nb; ++cell) {
            double R[EFF][9], p[EFF][3];
            tree_pose(chain, h_ang + cell * D, R, p);
            for (int e = 0; e < EFF; ++e) {
                double chord = 0.0; /* |R - R_target|_F = 2 sqrt(2) sin(theta / 2) */
                for (int c = 0; c < 9; ++c) {
                    const double d = R[e][c] - (double)h_rot[(cell * EFF + e) * 9 + c];
                    chord += d * d;
                }
                chord = sqrt(chord);
                ang_err[i][e] += 2.0 * asin(fmin(1.0, chord / (2.0 * sqrt(2.0)))) / (double)nb;
                finite &= isfinite(chord);
            }
            pos_err[i] += (double)h_res[cell] / (double)nb;
            finite &= isfinite(h_res[cell]);
        }
    }
    printf("kernel %s (weights 0: %s): %d trees x %d waypoints x %d iterations, weights %g %g %g\n",
           ikpso_solver_kernel_name(s[0]), ikpso_solver_kernel_name(s[1]), B, T, iters, weights[0], weights[1],
           weights[2]);
    for (int e = 0; e < EFF; ++e)
        printf("effector %d: angle error %.6f rad (weights 0: %.6f rad)\n", e, ang_err[0][e], ang_err[1][e]);
    printf("position error, summed over the effectors: %.6f m (weights 0: %.6f m)\n", pos_err[0], pos_err[1]);
    printf("finite %d\n", finite);
    ikpso_solver_destroy(s[0]);
    ikpso_solver_destroy(s[1]);
    return finite ? 0 : 2;
}
