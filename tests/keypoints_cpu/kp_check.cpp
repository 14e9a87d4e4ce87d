// Host checks of csrc/fdc_keypoints.h (tests/test_keypoints_cpu.py): the keypoint map's validation and de-duplication, and the
// per-keypoint math -- combination, projection, GMoF, gradient scatter -- in the kernel's order.  Reads numbers from a text file:
//   V n_kp  joint[n_kp]  tri[3 n_kp]  bary[3 n_kp]          ("map": stops here)
//   stage[9]  J55[55 * 3]  verts[V * 3]  kp[3 n_kp]          ("math")
// "blend": the file holds pairs "frames columns"; prints kp_blend_by_panels of each
#include <stdio.h>

#include <fstream>
#include <string>
#include <vector>

#include "fdc_keypoints.h"

using namespace fdc;

template <class T>
static void print_vec(const char* name, const std::vector<T>& v) {
    printf("%s", name);
    for (const T& x : v) printf(" %.9g", (double)x);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const std::string mode = argv[1];
    std::ifstream in(argv[2]);
    if (mode == "blend") {
        int frames, ncol;
        while (in >> frames >> ncol) printf("%d\n", kp_blend_by_panels(frames, ncol) ? 1 : 0);
        return 0;
    }
    int V = 0, n = 0;
    in >> V >> n;
    const int m = n > 0 ? n : 0;
    std::vector<int32_t> joint(m), tri(3 * m);
    std::vector<float> bary(3 * m);
    for (auto& x : joint) in >> x;
    for (auto& x : tri) in >> x;
    for (auto& x : bary) { std::string s; in >> s; x = strtof(s.c_str(), nullptr); }       // (strtof reads "nan" and "inf")
    KeypointTables t;
    if (keypoint_map_build(n, joint.data(), tri.data(), bary.data(), V, &t)) { printf("err\n"); return 0; }
    printf("ok %d %d %d\n", t.n_kp, t.nr, t.np);
    print_vec("real_ids", t.real_ids); print_vec("pseudo_joint", t.pseudo_joint); print_vec("kjoint", t.kjoint);
    print_vec("kref", t.kref); print_vec("kbary", t.kbary); print_vec("vl_start", t.vl_start); print_vec("vl_k", t.vl_k);
    print_vec("vl_w", t.vl_w); print_vec("jl_start", t.jl_start); print_vec("jl_k", t.jl_k);
    if (mode != "math") return 0;
    float sg[9];
    for (float& x : sg) in >> x;
    const Fit2dStage s = {sg[0], sg[1], sg[2], sg[3], sg[4], sg[5], sg[6], sg[7], sg[8]};
    std::vector<float> J(55 * 3), verts((size_t)V * 3), kp(3 * m);
    for (auto& x : J) in >> x;
    for (auto& x : verts) in >> x;
    for (auto& x : kp) in >> x;
    if (!in) return 3;
    const int nu = t.nu();
    std::vector<float> vw(3 * (size_t)nu + 3), pos(3 * m), dkp(3 * m), gvw(3 * (size_t)nu + 3), dJw(23 * 3);
    for (int u = 0; u < nu; ++u)
        for (int c = 0; c < 3; ++c) vw[3 * u + c] = u < t.nr ? verts[3 * (size_t)t.real_ids[u] + c] : J[3 * t.pseudo_joint[u - t.nr] + c];
    const float data = kp_frame_host(s, t, J.data(), vw.data(), kp.data(), pos.data(), dkp.data(), gvw.data(), dJw.data());
    printf("data %.9g\n", (double)data);
    gvw.resize(3 * (size_t)nu);
    print_vec("pos", pos); print_vec("gvw", gvw); print_vec("dJw", dJw);
    return 0;
}
