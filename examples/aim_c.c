/* aim_c.c -- ikpso_solve_track_aim from plain C: B KUKA LBR iiwa 14 arms (standard DH, mapped onto
 * the node table as ikpso/dh.py does, joint axes alone free) follow four waypoints each in one call
 * with the tool's z axis held pointing straight down -- drilling, pouring, a probe on a line -- and
 * the rotation about that axis left to the solver.  The DH tool frame's z axis is the effector
 * node's x axis (the last link's direction; ikpso.dh.DHArm.node_axis((0, 0, 1))), so aim_axis is
 * (1, 0, 0) and every aim_dir (0, 0, -1).  A second solver, seeded alike, runs the same call with
 * aim weight 0 (position-only IK, wherever the tool then points); per frame the mean position
 * error and the mean angle between the tool axis and the direction are printed for both.
 * usage: aim_c [B] [iterations per frame] [aim weight] */
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

#define NODES 12
#define JOINTS 7
#define FRAMES 4
#define HALF_PI 1.57079632679489661923

/* The iiwa's node table: a joint node (z free within +-limit of its offset) and, after a joint
 * with d != 0, a locked node Ry(-pi/2) carrying the offset as its link. */
static const struct {
    double x, y, z, length, limit;
} kArm[NODES] = {{0, 0, 0, 0, 0},
                 {0, 0, 0, 0, 2.96705972839036},
                 {0, -HALF_PI, 0, 0.36, 0},
                 {-HALF_PI, 0, HALF_PI, 0, 2.0943951023932},
                 {HALF_PI, 0, 0, 0, 2.96705972839036},
                 {0, -HALF_PI, 0, 0.42, 0},
                 {HALF_PI, 0, -HALF_PI, 0, 2.0943951023932},
                 {-HALF_PI, 0, 0, 0, 2.96705972839036},
                 {0, -HALF_PI, 0, 0.4, 0},
                 {-HALF_PI, 0, HALF_PI, 0, 2.0943951023932},
                 {HALF_PI, 0, 0, 0, 3.05432619099008},
                 {0, -HALF_PI, 0, 0.126, 0}};

static void arm_table(ikpso_node* n, uint8_t* mask)
{
    memset(n, 0, sizeof(ikpso_node) * NODES);
    for (int k = 0; k < NODES; ++k) {
        n[k].node_type = k == 0 ? IKPSO_NODE_ORIGIN : (k == NODES - 1 ? IKPSO_NODE_EFFECTOR : IKPSO_NODE);
        n[k].parent_index = k - 1;
        n[k].effector_weight = k == NODES - 1 ? 1.0f : 0.0f;
        n[k].length = (float)kArm[k].length;
        const double r[3] = {kArm[k].x, kArm[k].y, kArm[k].z};
        for (int c = 0; c < 3; ++c) n[k].rotation[c] = n[k].min_rotation[c] = n[k].max_rotation[c] = (float)r[c];
        n[k].min_rotation[2] = (float)(kArm[k].z - kArm[k].limit);
        n[k].max_rotation[2] = (float)(kArm[k].z + kArm[k].limit);
        mask[k] = kArm[k].limit > 0 ? 4 : 0; /* bit 2: the z angle */
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

/* The effector node's world frame and position for the seven free z angles, in double. */
static void arm_pose(const ikpso_node* n, const float* z, double R[9], double p[3])
{
    int j = 0;
    memset(R, 0, sizeof(double) * 9);
    R[0] = R[4] = R[8] = 1.0;
    p[0] = p[1] = p[2] = 0.0;
    for (int k = 1; k < NODES; ++k) {
        turn(R, 0, n[k].rotation[0]);
        turn(R, 1, n[k].rotation[1]);
        turn(R, 2, kArm[k].limit > 0 ? (double)z[j++] : (double)n[k].rotation[2]);
        for (int c = 0; c < 3; ++c) p[c] += (double)n[k].length * R[3 * c];
    }
}

int main(int argc, char** argv)
{
    const int B = argc > 1 ? atoi(argv[1]) : 32;
    const int iters = argc > 2 ? atoi(argv[2]) : 100;
    const float weight = argc > 3 ? (float)atof(argv[3]) : 1.0f;
    const int P = 1024, D = JOINTS, T = FRAMES;
    if (B <= 0 || iters < 0 || !(weight >= 0.0f)) return 1;
    ikpso_node chain[NODES];
    uint8_t mask[NODES];
    arm_table(chain, mask);

    /* waypoints: arm b's tip moves 15 mm per frame along x from a point of its own in front of the
     * base, inside the reach of an arm whose last link hangs straight down */
    const size_t nb = (size_t)T * B;
    const float axis[3] = {1.0f, 0.0f, 0.0f}; /* host memory: the tool z axis in the node frame */
    float* h_tg = (float*)malloc(sizeof(float) * nb * 3);
    float* h_dir = (float*)malloc(sizeof(float) * nb * 3);
    for (int t = 0; t < T; ++t)
        for (int b = 0; b < B; ++b) {
            float* p = h_tg + ((size_t)t * B + b) * 3;
            float* d = h_dir + ((size_t)t * B + b) * 3;
            p[0] = (float)(0.6 + 0.08 * sin(1.3 * b) + 0.015 * t);
            p[1] = (float)(0.2 * cos(0.7 * b));
            p[2] = (float)(0.3 + 0.1 * sin(2.1 * b));
            d[0] = d[1] = 0.0f;
            d[2] = -1.0f;
        }
    float *d_tg, *d_dir, *d_ang[2], *d_fit[2], *d_res[2];
    CHECK_HIP(hipMalloc((void**)&d_tg, sizeof(float) * nb * 3));
    CHECK_HIP(hipMalloc((void**)&d_dir, sizeof(float) * nb * 3));
    CHECK_HIP(hipMemcpy(d_tg, h_tg, sizeof(float) * nb * 3, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_dir, h_dir, sizeof(float) * nb * 3, hipMemcpyHostToDevice));
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
    desc.fit.angle_weight = 0.0f; /* aim IK: nothing pulls towards the start pose */
    desc.fit.error_threshold = 0.1f;
    desc.kernel = IKPSO_KERNEL_RESIDENT;
    desc.axis_mask = mask;
    ikpso_solver* s[2];
    for (int i = 0; i < 2; ++i) {
        CHECK_IK(ikpso_solver_create(&desc, &s[i]));
        CHECK_IK(ikpso_solver_seed(s[i], B, 0, 0, NULL));
    }
    /* aim targets, and the twin with the term switched off */
    CHECK_IK(ikpso_solve_track_aim(s[0], d_tg, d_dir, axis, weight, NULL, B, T, iters, -1.0f, d_ang[0], d_fit[0],
                                   d_res[0], NULL, NULL));
    CHECK_IK(ikpso_solve_track_aim(s[1], d_tg, d_dir, axis, 0.0f, NULL, B, T, iters, -1.0f, d_ang[1], d_fit[1],
                                   d_res[1], NULL, NULL));
    CHECK_HIP(hipDeviceSynchronize());

    float* h_ang = (float*)malloc(sizeof(float) * nb * D);
    float* h_res = (float*)malloc(sizeof(float) * nb);
    double pos_err[2][FRAMES], ang_err[2][FRAMES];
    int finite = 1;
    for (int i = 0; i < 2; ++i) {
        CHECK_HIP(hipMemcpy(h_ang, d_ang[i], sizeof(float) * nb * D, hipMemcpyDeviceToHost));
        CHECK_HIP(hipMemcpy(h_res, d_res[i], sizeof(float) * nb, hipMemcpyDeviceToHost));
        for (int t = 0; t < T; ++t) {
            pos_err[i][t] = ang_err[i][t] = 0.0;
            for (int b = 0; b < B; ++b) {
                const size_t cell = (size_t)t * B + b;
                double R[9], p[3], chord = 0.0;
                arm_pose(chain, h_ang + cell * D, R, p);
                for (int c = 0; c < 3; ++c) { /* |R a - d|, R a the frame's x column */
                    const double e = R[3 * c] - (double)h_dir[cell * 3 + c];
                    chord += e * e;
                }
                chord = sqrt(chord);
                ang_err[i][t] += 2.0 * asin(fmin(1.0, 0.5 * chord)) / B;
                pos_err[i][t] += (double)h_res[cell] / B;
                finite &= isfinite(h_res[cell]) && isfinite(chord);
            }
        }
    }
    printf("kernel %s: %d arms x %d aim waypoints x %d iterations, aim weight %g\n",
           ikpso_solver_kernel_name(s[0]), B, T, iters, weight);
    for (int t = 0; t < T; ++t)
        printf("frame %d: position error %.6f m, aim error %.6f rad (weight 0: %.6f m, %.6f rad)\n", t,
               pos_err[0][t], ang_err[0][t], pos_err[1][t], ang_err[1][t]);
    printf("finite %d\n", finite);
    ikpso_solver_destroy(s[0]);
    ikpso_solver_destroy(s[1]);
    return finite ? 0 : 2;
}
