// Host check of the free expression's arithmetic (csrc/fdc_keypoints.h; tests/test_expression_cpu.py), in the kernel's order.
// Reads numbers from a text file:  parents[55] JE[55 3][10] psi[10] A[55][12] dAp[55][12] dJw[23][3] W[9]
// and prints one named line of numbers per result:
//   delta [55 3], dt [55 3] (Dt_j), A [55][12] (corrected), dA [55][12] (d loss / d A' plus the rotation addends),
//   ddelta [55 3], dpsi [10] (JE^T d delta)
// for the loss sum(dAp . A') + sum_{j < 23} dJw_j . (W Dt_j).
#include <stdio.h>

#include <fstream>
#include <string>
#include <vector>

#include "fdc_host_setup.h"
#include "fdc_keypoints.h"

using namespace fdc;

static void print_arr(const char* name, const float* v, int n) {
    printf("%s", name);
    for (int i = 0; i < n; ++i) printf(" %.9g", (double)v[i]);
    printf("\n");
}
static bool rd(std::ifstream& in, float* v, int n) {
    for (int i = 0; i < n; ++i) { std::string s; if (!(in >> s)) return false; v[i] = strtof(s.c_str(), nullptr); }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3 || std::string(argv[1]) != "chain") return 2;
    std::ifstream in(argv[2]);
    std::vector<float> pf(NJ), JE(NJ * 3 * NEXPR), psi(NEXPR), A(NJ * 12), dAp(NJ * 12), dJw(NJW * 3), W(9);
    if (!rd(in, pf.data(), NJ) || !rd(in, JE.data(), NJ * 3 * NEXPR) || !rd(in, psi.data(), NEXPR) || !rd(in, A.data(), NJ * 12) ||
        !rd(in, dAp.data(), NJ * 12) || !rd(in, dJw.data(), NJW * 3) || !rd(in, W.data(), 9))
        return 3;
    std::vector<int> parents(NJ), child_start(NJ + 1), child_list;
    for (int j = 0; j < NJ; ++j) parents[j] = (int)pf[j];
    for (int p = 0; p < NJ; ++p) {                          // (host_pose_setup's lists)
        child_start[p] = (int)child_list.size();
        for (int j = 0; j < NJ; ++j) if (parents[j] == p) child_list.push_back(j);
    }
    child_start[NJ] = (int)child_list.size();
    child_list.push_back(0);
    std::vector<int> depth(NJ, 0);
    int nlevels = 1;
    for (int j = 1; j < NJ; ++j) { depth[j] = depth[parents[j]] + 1; nlevels = std::max(nlevels, depth[j] + 1); }

    std::vector<float> delta(NJ * 3), dt(NJ * 3), own(NJ * 3), S(NJ * 3), dd(NJ * 3), dA(NJ * 12), dpsi(NEXPR);
    for (int e = 0; e < NJ * 3; ++e) delta[e] = expr_delta_entry(JE.data(), psi.data(), e);
    for (int j = 0; j < NJ; ++j) {
        const V3 t = expr_forward(A.data(), parents.data(), delta.data(), j);
        dt[3 * j] = t.x; dt[3 * j + 1] = t.y; dt[3 * j + 2] = t.z;
    }
    for (int j = 0; j < NJ; ++j)
        for (int c = 0; c < 3; ++c) {
            float o = dAp[12 * j + 4 * c + 3];
            if (j < NJW) o += (W[c] * dJw[3 * j] + W[3 + c] * dJw[3 * j + 1]) + W[6 + c] * dJw[3 * j + 2];
            own[3 * j + c] = o;
        }
    for (int L = nlevels - 1; L >= 0; --L)                  // (the kernel's order: joints by level, the deepest first)
        for (int j = 0; j < NJ; ++j)
            if (depth[j] == L) {
                const V3 s = expr_subtree_children(child_start.data(), child_list.data(), own.data(), S.data(), j);
                S[3 * j] = s.x; S[3 * j + 1] = s.y; S[3 * j + 2] = s.z;
            }
    for (int j = 0; j < NJ; ++j) {
        const V3 d = expr_backward_delta(A.data(), parents.data(), own.data(), S.data(), dAp.data(), j);
        dd[3 * j] = d.x; dd[3 * j + 1] = d.y; dd[3 * j + 2] = d.z;
    }
    for (int q = 0; q < NJ * 12; ++q) {
        const int j = q / 12, e = q - 12 * j, i = e >> 2, c = e & 3;
        dA[q] = dAp[q];
        if (c < 3) dA[q] += expr_backward_rot_entry(child_start.data(), child_list.data(), delta.data(), own.data(), S.data(), dAp.data(), j, i, c);
    }
    for (int l = 0; l < NEXPR; ++l) {
        float acc = 0.f;
        for (int e = 0; e < NJ * 3; ++e) acc += JE[e * NEXPR + l] * dd[e];
        dpsi[l] = acc;
    }
    print_arr("delta", delta.data(), NJ * 3); print_arr("dt", dt.data(), NJ * 3); print_arr("A", A.data(), NJ * 12);
    print_arr("dA", dA.data(), NJ * 12); print_arr("ddelta", dd.data(), NJ * 3); print_arr("dpsi", dpsi.data(), NEXPR);
    return 0;
}
