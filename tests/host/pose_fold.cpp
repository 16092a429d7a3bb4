// pose_fold.cpp -- the folded chain's effector frame on the CPU: parses arms given on stdin with
// the chain parser (csrc/ikpso_chain.cpp, linked alone as in chain_dump.cpp), folds them
// (build_dh) and replays the fold in fp64 from the ChainHost the parser produced:
//   R = C_1 Rz(t_1) C_2 Rz(t_2) ... C_N Rz(t_N) G
// with C_j the fp32 constants of aux + dh_off and G = ChainHost::tip_rot.  tests/test_pose_fold.py
// compares R with the Euler definition of the effector node's frame, computed independently.
//
// stdin:  arms
//         per arm: node_count poses
//                  node_count lines: type parent length rot[3] lo[3] hi[3] pos[3] mask
//                  poses lines: N free angles
// stdout: per arm "arm N" + the nine entries of G; per pose the nine entries of R (row-major, %.17g)
#include <math.h>
#include <stdio.h>

#include <vector>

#include "ikpso_chain.h"

using namespace ikpso;

namespace {

struct M3 {
    double m[3][3];
};

M3 mul(const M3& a, const M3& b)
{
    M3 r{};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            for (int x = 0; x < 3; ++x) r.m[i][j] += a.m[i][x] * b.m[x][j];
    return r;
}

M3 from9(const float* p)
{
    M3 r{};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r.m[i][j] = (double)p[3 * i + j];
    return r;
}

M3 rz(double t)
{
    M3 r{};
    r.m[0][0] = cos(t), r.m[0][1] = -sin(t), r.m[1][0] = sin(t), r.m[1][1] = cos(t), r.m[2][2] = 1.0;
    return r;
}

void print9(const M3& a)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) printf("%.17g%c", a.m[i][j], i == 2 && j == 2 ? '\n' : ' ');
}

}  // namespace

int main()
{
    int arms = 0;
    if (scanf("%d", &arms) != 1) return 2;
    for (int a = 0; a < arms; ++a) {
        int n = 0, poses = 0;
        if (scanf("%d %d", &n, &poses) != 2 || n < 2 || n - 1 > kMaxJoints) return 2;
        std::vector<ikpso_node> nodes(n);
        std::vector<uint8_t> mask(n);
        for (int k = 0; k < n; ++k) {
            ikpso_node nd{};
            int m = 0;
            if (scanf("%d %d %f %f %f %f %f %f %f %f %f %f %f %f %f %d", &nd.node_type, &nd.parent_index, &nd.length,
                      &nd.rotation[0], &nd.rotation[1], &nd.rotation[2], &nd.min_rotation[0], &nd.min_rotation[1],
                      &nd.min_rotation[2], &nd.max_rotation[0], &nd.max_rotation[1], &nd.max_rotation[2],
                      &nd.position[0], &nd.position[1], &nd.position[2], &m) != 16)
                return 2;
            nd.effector_weight = nd.node_type == IKPSO_NODE_EFFECTOR ? 1.0f : 0.0f;
            nodes[k] = nd;
            mask[k] = (uint8_t)m;
        }
        Extras ex;
        ex.axis_mask = mask.data();
        const ikpso_pso_config pso{0.5f, 0.5f, 1.25f, 15};
        const ikpso_fitness_config fit{3.0f, 0.0f, 0.1f};
        ChainHost eu, dh;
        if (parse_chain(nodes, pso, fit, ex, eu) != IKPSO_OK || !build_dh(nodes, eu, ex, dh)) {
            fprintf(stderr, "arm %d does not fold\n", a);
            return 3;
        }
        const int N = dh.J;
        const M3 G = from9(dh.tip_rot);
        printf("arm %d\n", N);
        print9(G);
        const float* dc = dh.aux.data() + dh.dh_off;
        for (int p = 0; p < poses; ++p) {
            M3 W{};
            W.m[0][0] = W.m[1][1] = W.m[2][2] = 1.0;
            for (int j = 0; j < N; ++j) {
                float t = 0.0f;
                if (scanf("%f", &t) != 1) return 2;
                W = mul(mul(W, from9(dc + 12 * j)), rz((double)t));
            }
            print9(mul(W, G));
        }
    }
    return 0;
}
