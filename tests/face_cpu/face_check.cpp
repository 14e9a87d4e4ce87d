// Host checks of the free jaw's and the bending prior's arithmetic (csrc/fdc_keypoints.h, csrc/fdc_fit2d.h; tests/test_face_cpu.py).
// Reads numbers from a text file and prints one named line of numbers per result:
//   "jaw":   w[3] J22[3] A22[12] dAp[12] gP[9] w_jaw[3]      -> A' pf9 dRw dA22 dJ22 grad (jaw_forward, jaw_backward, jaw_grad)
//   "bend":  items of  R[9] axis sign w                        -> per item: val, dR[9] (fit2d_bend_term)
//   "terms": w n joint[n] axis[n] sign[n]                      -> fit2d_bend_check's result
#include <stdio.h>

#include <fstream>
#include <string>
#include <vector>

#include "fdc_keypoints.h"

using namespace fdc;

static void print_arr(const char* name, const float* v, int n) {
    printf("%s", name);
    for (int i = 0; i < n; ++i) printf(" %.9g", (double)v[i]);
    printf("\n");
}
static bool rd(std::ifstream& in, float* v, int n) {
    for (int i = 0; i < n; ++i) { std::string s; if (!(in >> s)) return false; v[i] = strtof(s.c_str(), nullptr); }     // (strtof reads "nan" and "inf")
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const std::string mode = argv[1];
    std::ifstream in(argv[2]);
    if (mode == "jaw") {
        float w[3], J[3], A[12], dAp[12], gP[9], wj[3];
        if (!rd(in, w, 3) || !rd(in, J, 3) || !rd(in, A, 12) || !rd(in, dAp, 12) || !rd(in, gP, 9) || !rd(in, wj, 3)) return 3;
        float pf9[9];
        const JawFwd f = jaw_forward(v3(w[0], w[1], w[2]), v3(J[0], J[1], J[2]), A, pf9);
        const JawBwd b = jaw_backward(f, dAp);
        const V3 g = jaw_grad(v3(w[0], w[1], w[2]), b.dRw.m, gP, wj);
        const float dJ[3] = {b.dJ22.x, b.dJ22.y, b.dJ22.z}, gg[3] = {g.x, g.y, g.z};
        print_arr("A", A, 12); print_arr("pf9", pf9, 9); print_arr("dRw", b.dRw.m, 9); print_arr("dA22", b.dA22, 12);
        print_arr("dJ22", dJ, 3); print_arr("grad", gg, 3);
        return 0;
    }
    if (mode == "bend") {
        float it[12];
        int k = 0;
        while (rd(in, it, 12)) {
            M3 R, dR;
            for (int e = 0; e < 9; ++e) R.m[e] = it[e];
            const float val = fit2d_bend_term(it[11], (int)it[9], it[10], R, &dR);
            float out[10] = {val};
            for (int e = 0; e < 9; ++e) out[1 + e] = dR.m[e];
            print_arr(("item" + std::to_string(k++)).c_str(), out, 10);
        }
        return 0;
    }
    if (mode == "terms") {
        float w;
        int n;
        if (!rd(in, &w, 1) || !(in >> n)) return 3;
        const int m = n > 0 && n < 64 ? n : 0;
        std::vector<int32_t> joint(m), axis(m);
        std::vector<float> sign(m);
        for (auto& x : joint) in >> x;
        for (auto& x : axis) in >> x;
        if (!rd(in, sign.data(), m)) return 3;
        printf("result %d\n", fit2d_bend_check(w, n, joint.data(), axis.data(), sign.data()));
        return 0;
    }
    return 2;
}
