// aim_fold.cpp -- ikpso_solve_track_aim's axis in the folded chain's frame on the CPU: parses arms
// given on stdin with the chain parser (csrc/ikpso_chain.cpp, linked alone as in pose_fold.cpp),
// folds them (build_dh) and prints G = ChainHost::tip_rot and, for every axis given,
// aim_axis_folded's flag and a' = G a / |a|.  tests/test_aim_fold.py checks both against float64.
//
// stdin:  arms
//         per arm: node_count axes
//                  node_count lines: type parent length rot[3] lo[3] hi[3] pos[3] mask
//                  axes lines: 3 floats (nan and inf are read as such)
// stdout: per arm "arm N" + the nine entries of G; per axis "axis <valid> a'[3]" (%.9g; zeros when invalid)
#include <math.h>
#include <stdio.h>

#include <vector>

#include "ikpso_chain.h"

using namespace ikpso;

int main()
{
    int arms = 0;
    if (scanf("%d", &arms) != 1) return 2;
    for (int a = 0; a < arms; ++a) {
        int n = 0, axes = 0;
        if (scanf("%d %d", &n, &axes) != 2 || n < 2 || n - 1 > kMaxJoints) return 2;
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
        printf("arm %d\n", dh.J);
        for (int i = 0; i < 9; ++i) printf("%.9g%c", (double)dh.tip_rot[i], i == 8 ? '\n' : ' ');
        for (int x = 0; x < axes; ++x) {
            float axis[3], out[3] = {0.0f, 0.0f, 0.0f};
            if (scanf("%f %f %f", &axis[0], &axis[1], &axis[2]) != 3) return 2;
            const bool ok = aim_axis_folded(dh, axis, out);
            printf("axis %d %.9g %.9g %.9g\n", ok ? 1 : 0, (double)out[0], (double)out[1], (double)out[2]);
        }
    }
    return 0;
}
