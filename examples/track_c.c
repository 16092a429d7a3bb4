/* track_c.c -- ikpso_solve_track from plain C: B reference arms (src/Main.cpp:76-116) follow
 * T waypoints each in one call, every frame warm-started from the previous frame's answer and
 * stopped once its fitness meets a threshold.  A second solver, seeded alike, runs the loop the
 * call replaces (one ikpso_solve_batch_until per frame, fed the previous answers) and the two
 * are compared bit for bit.
 * usage: track_c [B] [T] [iterations per frame] [stop fitness] */
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

static void reference_arm(ikpso_node* n)
{
    static const int parent[8] = {-1, 0, 1, 2, 3, 4, 4, 4};
    static const float rest[8][3] = {{0, 0, 0},     {0, 1.57f, 0}, {0, 1.57f, 0}, {0, 1.57f, 0},
                                     {0, 1.57f, 0}, {0, 1.57f, 0}, {0, 0, 1.57f}, {0, 0, 1.57f}};
    static const float reset[3][3] = {{0.75f, 1, -2.5f}, {-0.75f, 1, -2.5f}, {0, 0, -2.5f}};
    const float two_pi = 2.0f * 3.14159265358979323846f;
    memset(n, 0, sizeof(ikpso_node) * 8);
    for (int k = 0; k < 8; ++k) {
        n[k].node_type = k == 0 ? IKPSO_NODE_ORIGIN : (k >= 5 ? IKPSO_NODE_EFFECTOR : IKPSO_NODE);
        n[k].parent_index = parent[k];
        n[k].effector_weight = k >= 5 ? 1.0f : 0.0f;
        for (int c = 0; c < 3; ++c) {
            n[k].rotation[c] = rest[k][c];
            n[k].max_rotation[c] = two_pi;
            if (k >= 5) n[k].target_position[c] = reset[k - 5][c];
        }
        n[k].length = k == 0 ? 0.0f : 1.0f;
    }
}

int main(int argc, char** argv)
{
    const int B = argc > 1 ? atoi(argv[1]) : 64;
    const int T = argc > 2 ? atoi(argv[2]) : 32;
    const int iters = argc > 3 ? atoi(argv[3]) : 15;
    const float stop = argc > 4 ? (float)atof(argv[4]) : 0.05f;
    const int P = 1024, D = 21, E = 3;
    if (B <= 0 || T <= 0 || iters < 0) return 1;
    ikpso_node chain[8];
    reference_arm(chain);

    /* targets [T][B][E][3]: the reset targets carried round a small circle, one phase per arm */
    const size_t frame = (size_t)B * E * 3, nb = (size_t)T * B;
    float* h_tg = (float*)malloc(sizeof(float) * T * frame);
    for (int t = 0; t < T; ++t)
        for (int b = 0; b < B; ++b)
            for (int e = 0; e < E; ++e) {
                const float ph = 0.05f * t + 0.7f * b;
                float* p = h_tg + t * frame + ((size_t)b * E + e) * 3;
                p[0] = chain[5 + e].target_position[0] + 0.25f * cosf(ph);
                p[1] = chain[5 + e].target_position[1] + 0.25f * sinf(ph);
                p[2] = chain[5 + e].target_position[2];
            }
    float *d_tg, *d_ang[2], *d_fit[2], *d_res[2];
    int32_t* d_it[2];
    CHECK_HIP(hipMalloc((void**)&d_tg, sizeof(float) * T * frame));
    CHECK_HIP(hipMemcpy(d_tg, h_tg, sizeof(float) * T * frame, hipMemcpyHostToDevice));
    for (int i = 0; i < 2; ++i) {
        CHECK_HIP(hipMalloc((void**)&d_ang[i], sizeof(float) * nb * D));
        CHECK_HIP(hipMalloc((void**)&d_fit[i], sizeof(float) * nb));
        CHECK_HIP(hipMalloc((void**)&d_res[i], sizeof(float) * nb));
        CHECK_HIP(hipMalloc((void**)&d_it[i], sizeof(int32_t) * nb));
    }

    ikpso_solver_desc desc;
    memset(&desc, 0, sizeof(desc));
    desc.chain = chain;
    desc.node_count = 8;
    desc.particles = P;
    desc.pso.inertia = 0.5f;
    desc.pso.local = 0.5f;
    desc.pso.global = 1.25f;
    desc.pso.iterations = iters;
    desc.fit.angle_weight = 3.0f;
    desc.fit.error_threshold = 0.1f;
    ikpso_solver *s, *loop;
    CHECK_IK(ikpso_solver_create(&desc, &s));
    CHECK_IK(ikpso_solver_create(&desc, &loop));
    CHECK_IK(ikpso_solver_seed(s, B, 0, 0, NULL));
    CHECK_IK(ikpso_solver_seed(loop, B, 0, 0, NULL));

    /* the whole track in one call */
    CHECK_IK(ikpso_solve_track(s, d_tg, NULL, B, T, iters, stop, d_ang[0], d_fit[0], d_res[0], d_it[0], NULL));
    /* the loop it replaces: frame t starts from frame t - 1's answers */
    for (int t = 0; t < T; ++t)
        CHECK_IK(ikpso_solve_batch_until(loop, d_tg + t * frame, t ? d_ang[1] + (size_t)(t - 1) * B * D : NULL, B,
                                         iters, stop, d_ang[1] + (size_t)t * B * D, d_fit[1] + (size_t)t * B,
                                         d_res[1] + (size_t)t * B, d_it[1] + (size_t)t * B, NULL));
    CHECK_HIP(hipDeviceSynchronize());

    float* h_ang[2];
    float* h_fit[2];
    float* h_res[2];
    int32_t* h_it[2];
    for (int i = 0; i < 2; ++i) {
        h_ang[i] = (float*)malloc(sizeof(float) * nb * D);
        h_fit[i] = (float*)malloc(sizeof(float) * nb);
        h_res[i] = (float*)malloc(sizeof(float) * nb);
        h_it[i] = (int32_t*)malloc(sizeof(int32_t) * nb);
        CHECK_HIP(hipMemcpy(h_ang[i], d_ang[i], sizeof(float) * nb * D, hipMemcpyDeviceToHost));
        CHECK_HIP(hipMemcpy(h_fit[i], d_fit[i], sizeof(float) * nb, hipMemcpyDeviceToHost));
        CHECK_HIP(hipMemcpy(h_res[i], d_res[i], sizeof(float) * nb, hipMemcpyDeviceToHost));
        CHECK_HIP(hipMemcpy(h_it[i], d_it[i], sizeof(int32_t) * nb, hipMemcpyDeviceToHost));
    }
    const int same = !memcmp(h_ang[0], h_ang[1], sizeof(float) * nb * D) &&
                     !memcmp(h_fit[0], h_fit[1], sizeof(float) * nb) &&
                     !memcmp(h_res[0], h_res[1], sizeof(float) * nb) &&
                     !memcmp(h_it[0], h_it[1], sizeof(int32_t) * nb);
    double f0 = 0, fl = 0, its = 0;
    int finite = 1;
    for (size_t i = 0; i < nb; ++i) {
        its += h_it[0][i];
        finite &= isfinite(h_fit[0][i]) && isfinite(h_res[0][i]);
    }
    for (int b = 0; b < B; ++b) {
        f0 += h_fit[0][b];
        fl += h_fit[0][(size_t)(T - 1) * B + b];
    }
    printf("kernel %s: %d arms x %d frames x <= %d iterations, stop at fitness %.3f\n", ikpso_solver_kernel_name(s),
           B, T, iters, stop);
    printf("mean fitness frame 0 %.6f, frame %d %.6f, mean iterations per frame %.2f, finite %d, matches loop %d\n",
           f0 / B, T - 1, fl / B, its / (double)nb, finite, same);
    ikpso_solver_destroy(s);
    ikpso_solver_destroy(loop);
    return finite && same ? 0 : 2;
}
