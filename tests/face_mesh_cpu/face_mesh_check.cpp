// Host check of the full mesh's face arithmetic (csrc/fdc_face_mesh.h; tests/test_face_mesh_cpu.py): the per-frame functions the two
// per-frame kernels follow, and the two reductions' frame forms.
//   face_mesh_check frame FILE    numbers: has_psi has_jaw has_gJ has_dAp parents[55] JE[55 3][10] Jt[55 3] Jd[55 3][10] betas[10] psi[10]
//                                          jaw[3] A[55][12] dAp[55][12] gJ[55 3] dpsi_v[10]
//       prints  A2 [55][12], pf9 [9], dt [55 3], dA [55][12], dpsi [10], R9 [9], dbeta [10]
//   face_mesh_check sums FILE     numbers: ncol E[10][ncol] psi[10] Voff[ncol] dV[ncol]
//       prints  Voff [ncol] (+= E psi), dpsi_v [10] (= E^T dV in expr_dpsi_kernel's order)
#include <stdio.h>

#include <fstream>
#include <string>
#include <vector>

#include "fdc_host_setup.h"
#include "fdc_face_mesh.h"

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

static int run_frame(std::ifstream& in) {
    float flags[4];
    std::vector<float> pf(NJ), JE(NJ * 3 * NEXPR), Jt(NJ * 3), Jd(NJ * 3 * NBETA), betas(NBETA), psi(NEXPR), jaw(3), A(NJ * 12), dAp(NJ * 12),
        gJ(NJ * 3), dpv(NEXPR);
    if (!rd(in, flags, 4) || !rd(in, pf.data(), NJ) || !rd(in, JE.data(), NJ * 3 * NEXPR) || !rd(in, Jt.data(), NJ * 3) ||
        !rd(in, Jd.data(), NJ * 3 * NBETA) || !rd(in, betas.data(), NBETA) || !rd(in, psi.data(), NEXPR) || !rd(in, jaw.data(), 3) ||
        !rd(in, A.data(), NJ * 12) || !rd(in, dAp.data(), NJ * 12) || !rd(in, gJ.data(), NJ * 3) || !rd(in, dpv.data(), NEXPR))
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
    const FaceTabs t{JE.data(), Jt.data(), Jd.data(), parents.data(), child_start.data(), child_list.data(), depth.data(), nlevels};
    const float* const p = flags[0] != 0.f ? psi.data() : nullptr;
    const float* const w = flags[1] != 0.f ? jaw.data() : nullptr;
    std::vector<float> A2 = A, pf9(9, 0.f), dt(NJ * 3), dA(NJ * 12), dpsi(NEXPR, 0.f), R9(9, 0.f), dbeta(NBETA, 0.f);
    face_forward_frame(t, betas.data(), p, w, A2.data(), pf9.data(), dt.data());
    face_backward_frame(t, betas.data(), p, w, A.data(), flags[3] != 0.f ? dAp.data() : nullptr, flags[2] != 0.f ? gJ.data() : nullptr,
                        dpv.data(), dA.data(), dpsi.data(), R9.data(), dbeta.data());
    print_arr("A2", A2.data(), NJ * 12); print_arr("pf9", pf9.data(), 9); print_arr("dt", dt.data(), NJ * 3);
    print_arr("dA", dA.data(), NJ * 12); print_arr("dpsi", dpsi.data(), NEXPR); print_arr("R9", R9.data(), 9);
    print_arr("dbeta", dbeta.data(), NBETA);
    return 0;
}

static int run_sums(std::ifstream& in) {
    float nf;
    if (!rd(in, &nf, 1) || nf < 1.f) return 3;
    const int ncol = (int)nf, lde = (ncol + 3) & ~3;
    std::vector<float> E((size_t)NEXPR * lde, 0.f), psi(NEXPR), Voff(ncol), dV(ncol), dpv(NEXPR);
    for (int l = 0; l < NEXPR; ++l) if (!rd(in, E.data() + (size_t)l * lde, ncol)) return 3;
    if (!rd(in, psi.data(), NEXPR) || !rd(in, Voff.data(), ncol) || !rd(in, dV.data(), ncol)) return 3;
    face_offsets_frame(E.data(), lde, ncol, psi.data(), Voff.data());
    face_dpsi_frame(E.data(), lde, ncol, dV.data(), dpv.data());
    print_arr("Voff", Voff.data(), ncol); print_arr("dpsi_v", dpv.data(), NEXPR);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::ifstream in(argv[2]);
    if (!in) return 2;
    const std::string mode = argv[1];
    if (mode == "frame") return run_frame(in);
    if (mode == "sums") return run_sums(in);
    return 2;
}
