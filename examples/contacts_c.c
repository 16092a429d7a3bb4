/* contacts_c.c -- ikpso_solver_evaluate_contacts from plain C: B copies of the reference tree (four elbows,
 * three wrist effectors) among the four unit boxes of the reference's initColliders are solved for wrist
 * targets by a few PSO iterations, warm-started from a pose that stands clear of the boxes (the chain's own
 * rest pose lies in one, and a swarm started inside a box stays there, as in the reference).  The collider
 * term keeps the answers out of the boxes, and the contacts entry says so: no (node, collider) pair for an
 * answer whose fitness is finite.  Then every answer has its
 * first joint turned to (0, 0, 0), which lays the first link along +x into the box centred at (1, 0, 0):
 * the entry names the pairs that now touch -- (node 1, collider 0) among them -- where the fitness says
 * FLT_MAX and no more.
 * usage: contacts_c [B] [PSO iterations] */
#include <hip/hip_runtime_api.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
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
#define JOINTS 7
#define EFF 3
#define DOF 21
#define BOXES 4

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

/* the reference's initColliders: four unit cubes around the origin, the second one turned */
static void reference_boxes(ikpso_collider* b)
{
    static const float pos[BOXES][3] = {{1, 0, 0}, {0, 0, -1}, {-1, 0, 0}, {0, 0, 1}};
    static const float quat[BOXES][4] = {{0, 0, 0, 1}, {-0.403f, -0.819f, 0.273f, 0.304f}, {0, 0, 0, 1}, {0, 0, 0, 1}};
    memset(b, 0, sizeof(ikpso_collider) * BOXES);
    for (int i = 0; i < BOXES; ++i) {
        b[i].x = b[i].y = b[i].z = 1.0f;
        memcpy(b[i].pos, pos[i], sizeof(pos[i]));
        memcpy(b[i].quat, quat[i], sizeof(quat[i]));
    }
}

/* Print the (node, collider) pairs of B rows of contact words; returns how many there are, and through
 * `has` whether (node, collider) is among them in every row. */
static int print_pairs(const char* what, const uint32_t* words, const float* fit, int B, int node, int collider,
                       int* has)
{
    int total = 0;
    *has = 1;
    for (int b = 0; b < B; ++b) {
        int count = 0;
        printf("swarm %d fitness %s\n", b, fit[b] == FLT_MAX ? "FLT_MAX" : "finite");
        printf("%s:", what);
        for (int c = 0; c < BOXES; ++c)
            for (int k = 1; k <= JOINTS; ++k)
                if ((words[(size_t)b * BOXES + c] >> (k - 1)) & 1u) {
                    printf(" (node %d, collider %d)", k, c);
                    ++count;
                }
        if (!count) printf(" no contact");
        printf("\n");
        *has &= (int)((words[(size_t)b * BOXES + collider] >> (node - 1)) & 1u);
        total += count;
    }
    return total;
}

int main(int argc, char** argv)
{
    const int B = argc > 1 ? atoi(argv[1]) : 8;
    const int iters = argc > 2 ? atoi(argv[2]) : 100;
    const int P = 256, D = DOF;
    if (B <= 0 || iters < 0) return 1;
    ikpso_node chain[NODES];
    ikpso_collider boxes[BOXES];
    reference_arm(chain);
    reference_boxes(boxes);

    /* wrist targets above the boxes, a little apart per swarm */
    float* h_tg = (float*)malloc(sizeof(float) * B * EFF * 3);
    for (int b = 0; b < B; ++b)
        for (int e = 0; e < EFF; ++e) {
            float* t = h_tg + ((size_t)b * EFF + e) * 3;
            t[0] = 0.6f * (float)(e - 1) + 0.1f * (float)sin(0.9 * b);
            t[1] = 2.5f + 0.2f * (float)cos(1.3 * b);
            t[2] = 0.4f * (float)sin(0.7 * b + e);
        }
    /* the warm start: the first joint turned about z so that the arm stands straight up, clear of the boxes */
    float* h_start = (float*)calloc((size_t)B * D, sizeof(float));
    for (int b = 0; b < B; ++b) h_start[(size_t)b * D + 2] = 1.57f;
    float *d_tg, *d_ang, *d_fit, *d_start;
    CHECK_HIP(hipMalloc((void**)&d_start, sizeof(float) * B * D));
    CHECK_HIP(hipMemcpy(d_start, h_start, sizeof(float) * B * D, hipMemcpyHostToDevice));
    uint32_t* d_words;
    CHECK_HIP(hipMalloc((void**)&d_tg, sizeof(float) * B * EFF * 3));
    CHECK_HIP(hipMemcpy(d_tg, h_tg, sizeof(float) * B * EFF * 3, hipMemcpyHostToDevice));
    CHECK_HIP(hipMalloc((void**)&d_ang, sizeof(float) * B * D));
    CHECK_HIP(hipMalloc((void**)&d_fit, sizeof(float) * B));
    CHECK_HIP(hipMalloc((void**)&d_words, sizeof(uint32_t) * B * BOXES));

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
    desc.colliders = boxes;
    desc.collider_count = BOXES;
    ikpso_solver* s;
    CHECK_IK(ikpso_solver_create(&desc, &s));
    CHECK_IK(ikpso_solver_seed(s, B, 0, 0, NULL));
    CHECK_IK(ikpso_solve_batch(s, d_tg, d_start, B, iters, d_ang, NULL, NULL, NULL));
    printf("kernel %s: %d trees x %d iterations among %d boxes (%d within reach)\n", ikpso_solver_kernel_name(s), B,
           iters, BOXES, ikpso_solver_collider_count(s));

    float* q = (float*)malloc(sizeof(float) * B * D);
    float* fit = (float*)malloc(sizeof(float) * B);
    uint32_t* words = (uint32_t*)malloc(sizeof(uint32_t) * B * BOXES);
    int ok = 1, has;

    /* the answers: the fitness and the contacts behind it */
    CHECK_IK(ikpso_solver_evaluate(s, d_ang, d_tg, NULL, (int64_t)B, d_fit, NULL, NULL));
    CHECK_IK(ikpso_solver_evaluate_contacts(s, d_ang, (int64_t)B, d_words, NULL, NULL));
    CHECK_HIP(hipMemcpy(fit, d_fit, sizeof(float) * B, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(words, d_words, sizeof(uint32_t) * B * BOXES, hipMemcpyDeviceToHost));
    const int before = print_pairs("answers", words, fit, B, 1, 0, &has);
    for (int b = 0; b < B; ++b) ok &= fit[b] != FLT_MAX; /* the solve kept every tree out of the boxes */
    ok &= before == 0;

    /* the same answers, the first joint turned so that its link lies in box 0 */
    CHECK_HIP(hipMemcpy(q, d_ang, sizeof(float) * B * D, hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b) q[(size_t)b * D + 0] = q[(size_t)b * D + 1] = q[(size_t)b * D + 2] = 0.0f;
    CHECK_HIP(hipMemcpy(d_ang, q, sizeof(float) * B * D, hipMemcpyHostToDevice));
    CHECK_IK(ikpso_solver_evaluate(s, d_ang, d_tg, NULL, (int64_t)B, d_fit, NULL, NULL));
    CHECK_IK(ikpso_solver_evaluate_contacts(s, d_ang, (int64_t)B, d_words, NULL, NULL));
    CHECK_HIP(hipMemcpy(fit, d_fit, sizeof(float) * B, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(words, d_words, sizeof(uint32_t) * B * BOXES, hipMemcpyDeviceToHost));
    const int after = print_pairs("pushed", words, fit, B, 1, 0, &has);
    for (int b = 0; b < B; ++b) ok &= fit[b] == FLT_MAX;
    ok &= has;
    printf("%d pairs before, %d after; answers free, pushed poses report (node 1, collider 0): %d\n", before, after, ok);
    ikpso_solver_destroy(s);
    return ok ? 0 : 2;
}
