// Host checks of csrc/fdc_collide.h (tests/test_collision_cpu.py, and the host side of tests/test_gpu_collision.py): the header's
// own predicate, penalty and face-order builder, compiled by plain g++ -ffp-contract=off.  Reads one binary file of 32-bit words:
//   sat      N | N x 18 floats (s0 s1 s2 t0 t1 t2)                       -> N lines "hit" (coll_tri_sat, usable faces only) as 0 / 1 / 2 (unusable)
//   pairs    V F has_part has_ign | verts [V,3] | faces [F,3] | part [F] (as int32) | ign [64] as 128 words
//                                                                        -> lines "i j" (i < j by face id), every pair through coll_pair_test
//   penalty  N sigma | N x 18 floats                                      -> N lines "e g[18]" (coll_pair_backward), then N lines "e" (coll_pair_forward)
//   order    V F leaf_want has_part | vt [V,3] | faces [F,3] | part [F]   -> "err", or "ok leaf NL NLp" and the order
//   params   sigma w capacity                                             -> 0 / 1 (coll_params_ok)
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <string>
#include <vector>

#include "fdc_collide.h"

using namespace fdc;

static std::vector<uint32_t> slurp(const char* fn) {
    std::ifstream in(fn, std::ios::binary);
    std::vector<char> b((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    std::vector<uint32_t> w(b.size() / 4);
    memcpy(w.data(), b.data(), w.size() * 4);
    return w;
}
static float as_f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const std::string mode = argv[1];
    const std::vector<uint32_t> w = slurp(argv[2]);
    size_t at = 0;
    auto geti = [&]() { return (int32_t)w.at(at++); };
    auto getf = [&]() { return as_f(w.at(at++)); };
    if (mode == "sat") {
        const int N = geti();
        for (int i = 0; i < N; ++i) {
            float s[3][3], t[3][3];
            for (auto& r : s) for (float& x : r) x = getf();
            for (auto& r : t) for (float& x : r) x = getf();
            printf("%d\n", !coll_face_ok(s) || !coll_face_ok(t) ? 2 : coll_tri_sat(s, t) ? 1 : 0);
        }
        return 0;
    }
    if (mode == "penalty") {
        const int N = geti();
        const float sigma = getf();
        std::vector<float> fwd;
        for (int i = 0; i < N; ++i) {
            float P[6][3], g[6][3];
            for (auto& r : P) for (float& x : r) x = getf();
            printf("%.9g", (double)coll_pair_backward(P, sigma, g));
            for (auto& r : g) for (float x : r) printf(" %.9g", (double)x);
            printf("\n");
            fwd.push_back(coll_pair_forward(P, sigma));
        }
        for (float e : fwd) printf("%.9g\n", (double)e);
        return 0;
    }
    if (mode == "params") {
        const float sigma = getf(), wc = getf();
        const int cap = geti();
        printf("%d\n", coll_params_ok(sigma, wc, cap) ? 1 : 0);
        return 0;
    }
    if (mode == "pairs") {
        const int V = geti(), F = geti(), has_part = geti(), has_ign = geti();
        std::vector<float> verts((size_t)3 * V);
        std::vector<int32_t> faces((size_t)3 * F), part((size_t)F);
        for (float& x : verts) x = getf();
        for (auto& x : faces) x = geti();
        for (auto& x : part) x = geti();
        unsigned long long ign[64] = {0}, sym[64] = {0};
        for (auto& x : ign) { const uint64_t lo = w.at(at++); const uint64_t hi = w.at(at++); x = lo | (hi << 32); }
        if (has_ign)
            for (int a = 0; a < 64; ++a)
                for (int b = 0; b < 64; ++b)
                    if ((ign[a] >> b) & 1ull) { sym[a] |= 1ull << b; sym[b] |= 1ull << a; }
        for (int i = 0; i < F; ++i)
            for (int j = i + 1; j < F; ++j) {
                float s[3][3], t[3][3];
                for (int c = 0; c < 3; ++c)
                    for (int k = 0; k < 3; ++k) { s[c][k] = verts[3 * (size_t)faces[3 * i + c] + k]; t[c][k] = verts[3 * (size_t)faces[3 * j + c] + k]; }
                if (coll_pair_test(s, &faces[3 * i], has_part ? part[i] : 0, t, &faces[3 * j], has_part ? part[j] : 0, sym)) printf("%d %d\n", i, j);
            }
        return 0;
    }
    if (mode == "order") {
        const int V = geti(), F = geti(), leaf_want = geti(), has_part = geti();
        const int Vn = V > 0 ? V : 0, Fn = F > 0 ? F : 0;
        std::vector<float> vt((size_t)3 * Vn);
        std::vector<int32_t> faces((size_t)3 * Fn);
        std::vector<uint8_t> part((size_t)Fn);
        for (float& x : vt) x = getf();
        for (auto& x : faces) x = geti();
        for (auto& x : part) x = (uint8_t)geti();
        CollTables t;
        if (coll_mesh_build(F, faces.data(), has_part ? part.data() : nullptr, nullptr, V, vt.data(), leaf_want, &t)) { printf("err\n"); return 0; }
        printf("ok %d %d %d\n", t.leaf, t.NL, t.NLp);
        for (int32_t f : t.order) printf("%d ", f);
        printf("\n");
        for (size_t p = 0; p < t.order.size(); ++p) printf("%d %d %d %d ", t.tri[4 * p], t.tri[4 * p + 1], t.tri[4 * p + 2], t.tri[4 * p + 3]);
        printf("\n");
        return 0;
    }
    return 2;
}
