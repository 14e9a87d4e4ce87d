// TEST INFRASTRUCTURE ONLY (tests/test_contact_diet_cpu.py): what skin_bwd_vec_kernel forms instead of staging (csrc/fdc_skin.h,
// csrc/fdc_math.h), compiled for the host as a stand-alone program.  Built with -fsanitize=address,undefined and -ffp-contract=off.
//   * skin_world_vertex, the one helper the forward kernels and the backward share, equals the forward's expression written out
//     (sv = s vb, then the three rows of M), bit for bit: random inputs, NaN and infinities in every argument; and
//     skin_forward_vertex's vw is the helper's value of its vb
//   * the distance a search leaves for a query without a neighbour is NN_NO_NEIGHBOUR_D2: +infinity, which no distance of a NaN
//     query is better than (nn_exact_d2, nn_better) and every finite distance is
//   * rows [0, ja_hi) of A cover every joint id of random padded weight lists (skin_ja_hi on the transposed lists, built the way
//     build_skin_set builds them)
// Exit status 0 and "all checks hold" when everything holds.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <vector>

#include "../../4dcapture-fpv_amd/csrc/fdc_skin.h"

using namespace fdc;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_bad; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static bool same_bits(float a, float b) { return bits(a) == bits(b) || (a != a && b != b); }   // (any NaN equals any NaN: payloads are the host's)

// the forward's source expression, written out (skin_fwd_kernel / blend_skin_fwd_kernel before they shared the helper)
static V3 world_written_out(V3 vb, float s, const float* M) {
    const V3 sv = s * vb;
    V3 o;
    o.x = M[0] * sv.x + M[1] * sv.y + M[2] * sv.z + M[3];
    o.y = M[4] * sv.x + M[5] * sv.y + M[6] * sv.z + M[7];
    o.z = M[8] * sv.x + M[9] * sv.y + M[10] * sv.z + M[11];
    return o;
}

static void check_helper(std::mt19937& rng) {
    std::normal_distribution<float> nd(0.f, 1.f);
    const float special[] = {NAN, INFINITY, -INFINITY, 0.f, -0.f, 1e-42f, 3.4e38f};
    const int nspecial = (int)(sizeof(special) / sizeof(special[0]));
    int n = 0;
    for (int it = 0; it < 20000; ++it) {
        float M[12], s = 1.8f + 0.2f * nd(rng);
        V3 vb = v3(nd(rng), nd(rng), 2.f * nd(rng));
        for (int e = 0; e < 12; ++e) M[e] = nd(rng);
        if (it >= 10000) {                                  // one special value in one of the 16 arguments, each in turn
            const int slot = it % 16;
            const float v = special[(it / 16) % nspecial];
            if (slot < 12) M[slot] = v; else if (slot == 12) s = v; else if (slot == 13) vb.x = v; else if (slot == 14) vb.y = v; else vb.z = v;
        }
        const V3 a = skin_world_vertex(vb, s, M), b = world_written_out(vb, s, M);
        CHECK(same_bits(a.x, b.x) && same_bits(a.y, b.y) && same_bits(a.z, b.z), "helper != written-out expression at case %d", it);
        ++n;
    }
    // the whole per-vertex forward: its vw is the helper's value of its vb
    for (int it = 0; it < 2000; ++it) {
        const int V = 5, K = 4;
        std::vector<float> vt(3 * V), ww(V * K), A(55 * 12);
        std::vector<int> wj(V * K);
        for (auto& x : vt) x = nd(rng);
        for (auto& x : A) x = nd(rng);
        for (int i = 0; i < V * K; ++i) { wj[i] = (int)(rng() % 55); ww[i] = 0.25f; }
        SkinModel sm{};
        sm.vt = vt.data(); sm.S = nullptr; sm.wj = wj.data(); sm.ww = ww.data(); sm.K = K;
        float M[12], voff[3] = {nd(rng), nd(rng), nd(rng)}, beta[10] = {0};
        for (int e = 0; e < 12; ++e) M[e] = nd(rng);
        const float s = 1.8f + 0.2f * nd(rng);
        const SkinFwd f = skin_forward_vertex(sm, (int)(rng() % V), beta, voff, A.data(), v3(nd(rng), nd(rng), nd(rng)), M, s);
        const V3 b = world_written_out(f.vb, s, M);
        CHECK(same_bits(f.vw.x, b.x) && same_bits(f.vw.y, b.y) && same_bits(f.vw.z, b.z), "skin_forward_vertex's vw at case %d", it);
    }
    printf("helper: %d cases\n", n);
}

static void check_no_neighbour(std::mt19937& rng) {
    std::normal_distribution<float> nd(0.f, 3.f);
    CHECK(bits(NN_NO_NEIGHBOUR_D2) == 0x7f800000u, "the constant is not +infinity");
    for (int it = 0; it < 10000; ++it) {
        const float px = nd(rng), py = nd(rng), pz = nd(rng);
        float q[3] = {nd(rng), nd(rng), nd(rng)};
        // a finite query: any scene point replaces the initial value, so a query with a neighbour never keeps the constant
        const float d = nn_exact_d2(q[0], q[1], q[2], px, py, pz);
        CHECK(d >= 0.f && d < INFINITY && nn_better(d, (int)(rng() % 1000), NN_NO_NEIGHBOUR_D2, -1), "finite distance not better than the constant");
        // a NaN coordinate: no point is ever better, the running minimum stays the constant
        q[it % 3] = NAN;
        const float dn = nn_exact_d2(q[0], q[1], q[2], px, py, pz);
        CHECK(dn != dn, "a NaN query's distance is not NaN");
        CHECK(!nn_better(dn, 0, NN_NO_NEIGHBOUR_D2, -1) && !nn_better(dn, 0, NN_NO_NEIGHBOUR_D2, 0x7fffffff), "a NaN distance replaced the constant");
    }
    // ... whose robustifier has a zero derivative: such a query adds no gradient whichever way the distance reached the backward
    float dterm = 1.f;
    (void)contact_term(NN_NO_NEIGHBOUR_D2, &dterm);
    CHECK(dterm == 0.f, "d contact_term / d dist at the constant is %g", dterm);
}

static void check_ja_hi(std::mt19937& rng) {
    const int NJ_ = 55;
    for (int it = 0; it < 3000; ++it) {
        const int V = 1 + (int)(rng() % 40), K = 1 + (int)(rng() % 12);
        const int top = 1 + (int)(rng() % NJ_);            // joints below `top` may carry weight
        std::vector<float> lbs((size_t)V * NJ_, 0.f);
        for (int v = 0; v < V; ++v) {
            const int nz = 1 + (int)(rng() % K);
            for (int k = 0; k < nz; ++k) lbs[(size_t)v * NJ_ + rng() % top] = 0.1f + 0.01f * (float)(rng() % 50);
        }
        // per-vertex lists, padded with (joint 0, weight 0); transposed lists per joint
        std::vector<int> wj((size_t)V * K, 0), csc_start(NJ_ + 1, 0);
        std::vector<float> ww((size_t)V * K, 0.f);
        for (int v = 0; v < V; ++v) {
            int k = 0;
            for (int j = 0; j < NJ_ && k < K; ++j) if (lbs[(size_t)v * NJ_ + j] != 0.f) { wj[(size_t)v * K + k] = j; ww[(size_t)v * K + k] = lbs[(size_t)v * NJ_ + j]; ++k; }
        }
        int run = 0;
        for (int j = 0; j < NJ_; ++j) {
            csc_start[j] = run;
            for (int v = 0; v < V; ++v) if (lbs[(size_t)v * NJ_ + j] != 0.f) ++run;
        }
        csc_start[NJ_] = run;
        const int ja = skin_ja_hi(csc_start.data(), NJ_);
        CHECK(ja >= 1 && ja <= NJ_ && ja <= top, "ja_hi %d out of range (top %d)", ja, top);
        for (size_t i = 0; i < wj.size(); ++i) CHECK(wj[i] < ja, "joint id %d at or above ja_hi %d", wj[i], ja);
        // (the rows staged: reading A through every id stays inside [0, ja_hi) rows -- the sanitizer watches the buffer)
        std::vector<float> A((size_t)ja * 12, 1.f);
        float acc = 0.f;
        for (size_t i = 0; i < wj.size(); ++i) for (int e = 0; e < 12; ++e) acc += ww[i] * A[(size_t)wj[i] * 12 + e];
        CHECK(acc == acc, "NaN from the staged rows");
    }
}

int main() {
    std::mt19937 rng(20260114u);
    check_helper(rng);
    check_no_neighbour(rng);
    check_ja_hi(rng);
    if (g_bad) { printf("%d checks FAILED\n", g_bad); return 1; }
    printf("all checks hold\n");
    return 0;
}
