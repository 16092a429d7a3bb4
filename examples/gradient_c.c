/* gradient_c.c -- ikpso_solver_evaluate_gradient from plain C: B copies of the reference tree (four
 * elbows, three wrist effectors) are solved for reachable wrist targets by a few PSO iterations, then every
 * answer is polished through the C ABI alone by projected gradient descent on the solver's own objective:
 *   q' = clamp(q - step * gradient, lo, hi)   (the chain's bounds),
 * accepted only if out_fitness decreases -- otherwise the tree keeps q and halves its step (backtracking);
 * an accepted step grows the tree's step by a quarter.  Every tree has a step of its own, and one call
 * evaluates the whole batch.  A demonstration, not a refine entry: no convergence rate is promised, only
 * that no tree ends above where it started, which the accept rule guarantees.  The fitness before and after
 * is printed per swarm.
 * usage: gradient_c [B] [PSO iterations] [descent steps] */
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

/* R <- R * R_axis(t) */
static void turn(double R[9], int axis, double t)
{
    const int i = (axis + 1) % 3, j = (axis + 2) % 3;
    const double c = cos(t), s = sin(t);
    for (int r = 0; r < 3; ++r) {
        const double a = R[3 * r + i], b = R[3 * r + j];
        R[3 * r + i] = a * c + b * s;
        R[3 * r + j] = b * c - a * s;
    }
}

/* positions of the three wrists (nodes 5, 6, 7) for 21 Euler angles, from the header's definition */
static void wrists(const ikpso_node* n, const float* q, double p[EFF][3])
{
    double Rn[NODES][9], pn[NODES][3];
    memset(Rn[0], 0, sizeof(Rn[0]));
    Rn[0][0] = Rn[0][4] = Rn[0][8] = 1;
    for (int c = 0; c < 3; ++c) {
        turn(Rn[0], c, n[0].rotation[c]);
        pn[0][c] = n[0].position[c];
    }
    for (int k = 1; k < NODES; ++k) {
        memcpy(Rn[k], Rn[kParent[k]], sizeof(Rn[k]));
        for (int c = 0; c < 3; ++c) turn(Rn[k], c, q[3 * (k - 1) + c]);
        for (int c = 0; c < 3; ++c) pn[k][c] = pn[kParent[k]][c] + n[k].length * Rn[k][3 * c];
    }
    for (int e = 0; e < EFF; ++e) memcpy(p[e], pn[5 + e], sizeof(p[e]));
}

int main(int argc, char** argv)
{
    const int B = argc > 1 ? atoi(argv[1]) : 8;
    const int iters = argc > 2 ? atoi(argv[2]) : 20;
    const int steps = argc > 3 ? atoi(argv[3]) : 40;
    const int P = 256, D = DOF;
    if (B <= 0 || iters < 0 || steps < 0) return 1;
    ikpso_node chain[NODES];
    reference_arm(chain);

    /* targets: the wrist positions of joint vectors a little way from the rest pose, inside [0, 2 pi] */
    float* h_tg = (float*)malloc(sizeof(float) * B * EFF * 3);
    for (int b = 0; b < B; ++b) {
        float q[DOF];
        double p[EFF][3];
        for (int d = 0; d < D; ++d) q[d] = chain[1 + d / 3].rotation[d % 3] + (float)(0.35 * (0.5 + 0.5 * sin(1.7 * d + 0.9 * b)));
        wrists(chain, q, p);
        for (int e = 0; e < EFF; ++e)
            for (int c = 0; c < 3; ++c) h_tg[((size_t)b * EFF + e) * 3 + c] = (float)p[e][c];
    }
    float *d_tg, *d_ang, *d_try, *d_fit, *d_grad;
    CHECK_HIP(hipMalloc((void**)&d_tg, sizeof(float) * B * EFF * 3));
    CHECK_HIP(hipMemcpy(d_tg, h_tg, sizeof(float) * B * EFF * 3, hipMemcpyHostToDevice));
    CHECK_HIP(hipMalloc((void**)&d_ang, sizeof(float) * B * D));
    CHECK_HIP(hipMalloc((void**)&d_try, sizeof(float) * B * D));
    CHECK_HIP(hipMalloc((void**)&d_fit, sizeof(float) * B));
    CHECK_HIP(hipMalloc((void**)&d_grad, sizeof(float) * B * D));

    ikpso_solver_desc desc;
    memset(&desc, 0, sizeof(desc));
    desc.chain = chain;
    desc.node_count = NODES;
    desc.particles = P;
    desc.pso.inertia = 0.5f;
    desc.pso.local = 0.5f;
    desc.pso.global = 1.25f;
    desc.pso.iterations = iters;
    desc.fit.angle_weight = 0.05f;
    desc.fit.error_threshold = 0.1f;
    desc.kernel = IKPSO_KERNEL_RESIDENT;
    ikpso_solver* s;
    CHECK_IK(ikpso_solver_create(&desc, &s));
    CHECK_IK(ikpso_solver_seed(s, B, 0, 0, NULL));
    CHECK_IK(ikpso_solve_batch(s, d_tg, NULL, B, iters, d_ang, NULL, NULL, NULL));

    float* q = (float*)malloc(sizeof(float) * B * D);     /* the accepted angles */
    float* g = (float*)malloc(sizeof(float) * B * D);     /* their gradient */
    float* f = (float*)malloc(sizeof(float) * B);         /* their fitness */
    float* qt = (float*)malloc(sizeof(float) * B * D);    /* the trial */
    float* gt = (float*)malloc(sizeof(float) * B * D);
    float* ft = (float*)malloc(sizeof(float) * B);
    float* f0 = (float*)malloc(sizeof(float) * B);
    double* step = (double*)malloc(sizeof(double) * B);
    CHECK_HIP(hipMemcpy(q, d_ang, sizeof(float) * B * D, hipMemcpyDeviceToHost)); /* waits for the solve */
    /* the objective's rest pose is the chain's own (rest = NULL), its targets the solve's */
    CHECK_IK(ikpso_solver_evaluate_gradient(s, d_ang, d_tg, NULL, NULL, NULL, (int64_t)B, d_fit, d_grad, NULL));
    CHECK_HIP(hipMemcpy(f, d_fit, sizeof(float) * B, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(g, d_grad, sizeof(float) * B * D, hipMemcpyDeviceToHost));
    memcpy(f0, f, sizeof(float) * B);
    for (int b = 0; b < B; ++b) step[b] = 0.05;
    printf("kernel %s: %d trees x %d iterations, then %d projected gradient steps\n", ikpso_solver_kernel_name(s), B,
           iters, steps);
    int accepted = 0;
    for (int it = 0; it < steps; ++it) {
        for (int b = 0; b < B; ++b)
            for (int d = 0; d < D; ++d) {
                const ikpso_node* n = &chain[1 + d / 3];
                double v = (double)q[(size_t)b * D + d] - step[b] * (double)g[(size_t)b * D + d];
                v = fmin(fmax(v, (double)n->min_rotation[d % 3]), (double)n->max_rotation[d % 3]);
                qt[(size_t)b * D + d] = (float)v;
            }
        CHECK_HIP(hipMemcpy(d_try, qt, sizeof(float) * B * D, hipMemcpyHostToDevice));
        CHECK_IK(ikpso_solver_evaluate_gradient(s, d_try, d_tg, NULL, NULL, NULL, (int64_t)B, d_fit, d_grad, NULL));
        CHECK_HIP(hipMemcpy(ft, d_fit, sizeof(float) * B, hipMemcpyDeviceToHost));
        CHECK_HIP(hipMemcpy(gt, d_grad, sizeof(float) * B * D, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b) {
            if (ft[b] < f[b]) { /* NaN and FLT_MAX (a collision) never pass */
                memcpy(q + (size_t)b * D, qt + (size_t)b * D, sizeof(float) * D);
                memcpy(g + (size_t)b * D, gt + (size_t)b * D, sizeof(float) * D);
                f[b] = ft[b];
                step[b] *= 1.25;
                ++accepted;
            } else {
                step[b] *= 0.5;
            }
        }
    }
    int ok = 1;
    for (int b = 0; b < B; ++b) {
        printf("swarm %d: fitness %.6e -> %.6e\n", b, (double)f0[b], (double)f[b]);
        ok &= isfinite(f[b]) && f[b] <= f0[b];
    }
    printf("accepted %d of %d trial steps; no swarm above its start: %d\n", accepted, B * steps, ok);
    ikpso_solver_destroy(s);
    return ok ? 0 : 2;
}
