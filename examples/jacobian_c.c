/* jacobian_c.c -- ikpso_solver_evaluate_jacobian from plain C: B copies of the reference tree (four
 * elbows, three wrist effectors) are solved for reachable wrist targets, then the answers are polished by
 * two Gauss-Newton steps on the host.  Each step reads the node positions and the Jacobian of the three
 * wrists at the current angles from the device, stacks the linear rows into the 9 x 21 matrix A and the
 * positional residual into r = t - p (9 values), and takes the minimum-norm step of the dual system,
 *   dq = A^T (A A^T + lambda I)^-1 r     (9 x 9, solved by Gaussian elimination with pivoting),
 * with a small damping lambda, since the three wrists hang off one elbow and A is ill-conditioned near
 * the rest pose.  PSO stops near 1e-3; two such steps take the residual well below it.  The angle term of the
 * solver's objective is left out on purpose: this polishes the positions alone.  A demonstration, not a
 * refine entry: the sum over the wrists of |p_e - t_e| is printed before and after.
 * usage: jacobian_c [B] [PSO iterations] */
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
#define JOINTS (NODES - 1)
#define EFF 3
#define DOF 21
#define ROWS (3 * EFF)
#define STEPS 2
#define LAMBDA 1e-4 /* damping: the tree is ill-conditioned near its rest pose (smallest singular value ~0.01) */

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

/* x <- M^-1 x for the ROWS x ROWS matrix M (destroyed); 0 if a pivot vanishes */
static int solve9(double M[ROWS][ROWS], double x[ROWS])
{
    for (int c = 0; c < ROWS; ++c) {
        int piv = c;
        for (int r = c + 1; r < ROWS; ++r)
            if (fabs(M[r][c]) > fabs(M[piv][c])) piv = r;
        if (M[piv][c] == 0.0) return 0;
        for (int k = 0; k < ROWS; ++k) {
            const double t = M[c][k];
            M[c][k] = M[piv][k], M[piv][k] = t;
        }
        const double t = x[c];
        x[c] = x[piv], x[piv] = t;
        for (int r = c + 1; r < ROWS; ++r) {
            const double f = M[r][c] / M[c][c];
            for (int k = c; k < ROWS; ++k) M[r][k] -= f * M[c][k];
            x[r] -= f * x[c];
        }
    }
    for (int c = ROWS - 1; c >= 0; --c) {
        for (int k = c + 1; k < ROWS; ++k) x[c] -= M[c][k] * x[k];
        x[c] /= M[c][c];
    }
    return 1;
}

/* mean over the trees of sum_e |p_e - t_e|, from the device's node positions [B][JOINTS][3] */
static double mean_residual(const float* pos, const float* tg, int B)
{
    double sum = 0.0;
    for (int b = 0; b < B; ++b)
        for (int e = 0; e < EFF; ++e) {
            double d2 = 0.0;
            for (int c = 0; c < 3; ++c) {
                const double d = (double)pos[((size_t)b * JOINTS + 4 + e) * 3 + c] - (double)tg[((size_t)b * EFF + e) * 3 + c];
                d2 += d * d;
            }
            sum += sqrt(d2);
        }
    return sum / B;
}

int main(int argc, char** argv)
{
    const int B = argc > 1 ? atoi(argv[1]) : 8;
    const int iters = argc > 2 ? atoi(argv[2]) : 100;
    const int P = 1024, D = DOF;
    if (B <= 0 || iters < 0) return 1;
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
    const size_t jac_count = (size_t)B * EFF * 6 * D, pos_count = (size_t)B * JOINTS * 3;
    float *d_tg, *d_ang, *d_fit, *d_pos, *d_jac;
    CHECK_HIP(hipMalloc((void**)&d_tg, sizeof(float) * B * EFF * 3));
    CHECK_HIP(hipMemcpy(d_tg, h_tg, sizeof(float) * B * EFF * 3, hipMemcpyHostToDevice));
    CHECK_HIP(hipMalloc((void**)&d_ang, sizeof(float) * B * D));
    CHECK_HIP(hipMalloc((void**)&d_fit, sizeof(float) * B));
    CHECK_HIP(hipMalloc((void**)&d_pos, sizeof(float) * pos_count));
    CHECK_HIP(hipMalloc((void**)&d_jac, sizeof(float) * jac_count));

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
    CHECK_IK(ikpso_solve_batch(s, d_tg, NULL, B, iters, d_ang, d_fit, NULL, NULL));

    float* h_ang = (float*)malloc(sizeof(float) * B * D);
    float* h_pos = (float*)malloc(sizeof(float) * pos_count);
    float* h_jac = (float*)malloc(sizeof(float) * jac_count);
    CHECK_HIP(hipMemcpy(h_ang, d_ang, sizeof(float) * B * D, hipMemcpyDeviceToHost)); /* waits for the solve */
    printf("kernel %s: %d trees x %d iterations, then %d Gauss-Newton steps on the host\n", ikpso_solver_kernel_name(s),
           B, iters, STEPS);
    int finite = 1;
    for (int step = 0; step <= STEPS; ++step) {
        CHECK_IK(ikpso_solver_evaluate_jacobian(s, d_ang, (int64_t)B, d_pos, d_jac, NULL));
        CHECK_HIP(hipMemcpy(h_pos, d_pos, sizeof(float) * pos_count, hipMemcpyDeviceToHost));
        CHECK_HIP(hipMemcpy(h_jac, d_jac, sizeof(float) * jac_count, hipMemcpyDeviceToHost));
        const double res = mean_residual(h_pos, h_tg, B);
        finite &= isfinite(res) != 0;
        printf("residual after %d steps: %.3e\n", step, res);
        if (step == STEPS) break;
        for (int b = 0; b < B; ++b) {
            double A[ROWS][DOF], M[ROWS][ROWS], y[ROWS];
            for (int e = 0; e < EFF; ++e)
                for (int c = 0; c < 3; ++c) {
                    for (int d = 0; d < D; ++d) A[3 * e + c][d] = h_jac[(((size_t)b * EFF + e) * 6 + c) * D + d];
                    y[3 * e + c] = (double)h_tg[((size_t)b * EFF + e) * 3 + c] - (double)h_pos[((size_t)b * JOINTS + 4 + e) * 3 + c];
                }
            for (int i = 0; i < ROWS; ++i)
                for (int j = 0; j < ROWS; ++j) {
                    M[i][j] = i == j ? LAMBDA : 0.0;
                    for (int d = 0; d < D; ++d) M[i][j] += A[i][d] * A[j][d];
                }
            if (!solve9(M, y)) continue; /* leave this tree's answer as it is */
            for (int d = 0; d < D; ++d) {
                double dq = 0.0;
                for (int i = 0; i < ROWS; ++i) dq += A[i][d] * y[i];
                h_ang[(size_t)b * D + d] += (float)dq;
            }
        }
        CHECK_HIP(hipMemcpy(d_ang, h_ang, sizeof(float) * B * D, hipMemcpyHostToDevice));
    }
    printf("finite %d\n", finite);
    ikpso_solver_destroy(s);
    return finite ? 0 : 2;
}
