// Host checks of the inner fit's start from keypoints alone (csrc/fdc_fit2d_init.h; tests/test_fit2d_init_cpu.py).
// Reads numbers from a text file and prints one named line of numbers per result.  Slots are joints here (the 23-joint layout's rule,
// n_kp given), lists are padded to their longest form:
//   "depth":  fx fy n_kp n_edge edge[4][2] shoulder[2] conf_thr default_depth side_view_px G[55*12] kp[n_kp*3]   -> z valid side
//   "camera": fx fy cx cy n_kp n_torso torso[8] conf_thr w_data w_depth G[55*12] x_setup[78] x[78] kp[n_kp*3]    -> setup loss g9
//             (fit2d_camera_offset and the set-up's layout, then fit2d_camera_frame)
//   "flip":   items of aa[3]                                                                                     -> per item: once[3] twice[3]
//   "select": items of loss_first loss_twin                                                                      -> per item: 0 / 1
//   "build":  n_kp n_edge edge[4][2] n_torso torso[8] shoulder[2] conf_thr default_depth side_view_px w_data w_depth surface_slot
//             -> fit2d_init_build's result (slot `surface_slot`, if >= 0, is a surface point)
#include <stdio.h>

#include <fstream>
#include <string>
#include <vector>

#include "fdc_fit2d_init.h"

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
static bool rdi(std::ifstream& in, int32_t* v, int n) {
    for (int i = 0; i < n; ++i) if (!(in >> v[i])) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const std::string mode = argv[1];
    std::ifstream in(argv[2]);
    std::vector<int32_t> ident(64);
    for (int k = 0; k < 64; ++k) ident[k] = k < NJ ? k : -1;
    if (mode == "depth") {
        float f[2], set[3];
        int32_t n_kp, n_edge, edge[INIT_MAX_EDGE][2], sh[2];
        const int32_t torso[1] = {0};
        if (!rd(in, f, 2) || !rdi(in, &n_kp, 1) || !rdi(in, &n_edge, 1) || !rdi(in, &edge[0][0], 8) || !rdi(in, sh, 2) || !rd(in, set, 3)) return 3;
        if (n_kp < 1 || n_kp > 64) return 3;
        std::vector<float> G(NJ * 12), kp((size_t)n_kp * 3);
        if (!rd(in, G.data(), NJ * 12) || !rd(in, kp.data(), n_kp * 3)) return 3;
        Fit2dInit c;
        if (fit2d_init_build(n_edge, edge, 1, torso, sh, set[0], set[1], set[2], 1.f, 1.f, n_kp, ident.data(), &c)) return 4;
        int valid = -1;
        const float z = fit2d_depth_guess(c, f[0], f[1], G.data(), kp.data(), &valid);
        const float out[3] = {z, (float)valid, (float)fit2d_side_view(c, kp.data())};
        print_arr("guess", out, 3);
        return 0;
    }
    if (mode == "camera") {
        float f[4], set[3], xs[XDIM], x[XDIM];
        int32_t n_kp, n_torso, torso[INIT_MAX_TORSO];
        const int32_t edge[1][2] = {{0, 1}}, sh[2] = {0, 1};
        if (!rd(in, f, 4) || !rdi(in, &n_kp, 1) || !rdi(in, &n_torso, 1) || !rdi(in, torso, INIT_MAX_TORSO) || !rd(in, set, 3)) return 3;
        if (n_kp < 2 || n_kp > 64) return 3;
        std::vector<float> G(NJ * 12), kp((size_t)n_kp * 3);
        if (!rd(in, G.data(), NJ * 12) || !rd(in, xs, XDIM) || !rd(in, x, XDIM) || !rd(in, kp.data(), n_kp * 3)) return 3;
        Fit2dInit c;
        if (fit2d_init_build(1, edge, n_torso, torso, sh, set[0], 2.5f, 25.f, set[1], set[2], n_kp, ident.data(), &c)) return 4;
        float setup[CAM_SETUP_LD] = {};                      // (fit2d_camera_setup_kernel's layout)
        for (int k = 0; k < c.n_torso; ++k) {
            const V3 q = fit2d_camera_offset(G.data(), c.torso_joint[k]);
            setup[3 * k] = q.x; setup[3 * k + 1] = q.y; setup[3 * k + 2] = q.z;
        }
        const V3 b = g_trn(G.data()) + v3(xs[X_TRANSL], xs[X_TRANSL + 1], xs[X_TRANSL + 2]);
        setup[3 * INIT_MAX_TORSO] = b.x; setup[3 * INIT_MAX_TORSO + 1] = b.y; setup[3 * INIT_MAX_TORSO + 2] = b.z;
        setup[3 * INIT_MAX_TORSO + 3] = xs[X_CAMT + 2];
        const Fit2dStage s = {f[0], f[1], f[2], f[3], 100.f, 1.f, 0.f, 0.f, 0.f};
        float g9[9];
        const float loss = fit2d_camera_frame(s, c, setup, x, kp.data(), g9);
        print_arr("setup", setup, CAM_SETUP_LD); print_arr("loss", &loss, 1); print_arr("g9", g9, 9);
        return 0;
    }
    if (mode == "flip") {
        float a[3];
        int k = 0;
        while (rd(in, a, 3)) {
            const V3 once = fit2d_flip_orient(v3(a[0], a[1], a[2])), twice = fit2d_flip_orient(once);
            const float out[6] = {once.x, once.y, once.z, twice.x, twice.y, twice.z};
            print_arr(("item" + std::to_string(k++)).c_str(), out, 6);
        }
        return 0;
    }
    if (mode == "select") {
        float l[2];
        int k = 0;
        while (rd(in, l, 2)) {
            const float out = (float)fit2d_select_twin(l[0], l[1]);
            print_arr(("item" + std::to_string(k++)).c_str(), &out, 1);
        }
        return 0;
    }
    if (mode == "build") {
        int32_t n_kp, n_edge, edge[INIT_MAX_EDGE][2], n_torso, torso[INIT_MAX_TORSO], sh[2], surface;
        float set[5];
        if (!rdi(in, &n_kp, 1) || !rdi(in, &n_edge, 1) || !rdi(in, &edge[0][0], 8) || !rdi(in, &n_torso, 1) || !rdi(in, torso, INIT_MAX_TORSO) ||
            !rdi(in, sh, 2) || !rd(in, set, 5) || !rdi(in, &surface, 1))
            return 3;
        if (n_kp < 0 || n_kp > 64) return 3;
        if (surface >= 0 && surface < 64) ident[surface] = -1;
        Fit2dInit c;
        printf("result %d\n", fit2d_init_build(n_edge, edge, n_torso, torso, sh, set[0], set[1], set[2], set[3], set[4], n_kp, ident.data(), &c));
        return 0;
    }
    return 2;
}
