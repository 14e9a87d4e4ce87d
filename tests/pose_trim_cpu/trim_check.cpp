// TEST INFRASTRUCTURE ONLY (tests/test_pose_trim_cpu.py, tests/test_gpu_pose_trim.py): the per-frame pose math of csrc/fdc_frame.h
// compiled for the host, the way tests/cpu_harness does, as a stand-alone program.
//   trim_check                      pose_forward + pose_backward limited to joint sets (jn, jr) against the full sets on SMPL-X's
//                                   tree and random rows, then the rules of plan_pose_joints (csrc/fdc_forms.h); exit status 0 = all hold
//   trim_check plan JA C W T        the plan for ja_hi = JA, contact_state = C, need_world = W, trim = T on SMPL-X's tree: "jn jr nlev world"
// Whatever the limited run must not touch is NaN when it starts: the scratch, every output row, the rows >= jn of the forward
// state it is handed and of dA.  Built with -fsanitize=address,undefined.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "../../4dcapture-fpv_amd/csrc/fdc_forms.h"
#include "../../4dcapture-fpv_amd/csrc/fdc_frame.h"
#include "../../4dcapture-fpv_amd/csrc/fdc_host_setup.h"

using namespace fdc;

static_assert(POSE_NJ == NJ && POSE_NJW == NJW, "fdc_forms.h restates the two joint counts");

struct NoSync { void operator()() const {} };

// SMPL-X's kinematic tree: pelvis, 21 body joints, jaw and eyes, 15 joints per hand
static const int PARENTS[NJ] = {-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15,
                                20, 25, 26, 20, 28, 29, 20, 31, 32, 20, 34, 35, 20, 37, 38,
                                21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53};

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_bad; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
// equal as floats and the same bits, the sign of a zero excepted
static bool same(float a, float b) { return a == b && (bits(a) == bits(b) || (a == 0.f && b == 0.f)); }
static void fill_nan(void* p, size_t bytes) { memset(p, 0xff, bytes); }          // (0xffffffff is a NaN)
static bool is_fill(float f) { return bits(f) == 0xffffffffu; }

struct Model {
    HostPoseSetup hs;
    std::vector<float> hand_comp, hand_mean;
    PoseModel pm() const {
        PoseModel m;
        m.Jt = hs.Jt.data(); m.Jd = hs.Jd.data(); m.parents = hs.parents.data(); m.order = hs.order.data();
        m.level_start = hs.level_start.data(); m.child_start = hs.child_start.data(); m.child_list = hs.child_list.data();
        m.depth = hs.depth.data();
        m.hand_comp = hand_comp.data(); m.hand_mean = hand_mean.data(); m.nlevels = hs.nlevels;
        return m;
    }
};

static bool make_model(Model* m, std::mt19937& rng) {
    const int V = 48;
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<float> vt(V * 3), S(V * 3 * NBETA), Jreg((size_t)NJ * V, 0.f);
    for (float& v : vt) v = 0.5f * nd(rng);
    for (float& v : S) v = 0.05f * nd(rng);
    for (int j = 0; j < NJ; ++j) {                          // three vertices per joint, weights summing to one
        float w[3] = {0.5f, 0.3f, 0.2f};
        for (int k = 0; k < 3; ++k) Jreg[(size_t)j * V + (7 * j + 11 * k) % V] += w[k];
    }
    if (!host_pose_setup(V, vt.data(), S.data(), Jreg.data(), PARENTS, &m->hs)) return false;
    m->hand_comp.resize(2 * 12 * 45); m->hand_mean.resize(90);
    for (float& v : m->hand_comp) v = 0.1f * nd(rng);
    for (float& v : m->hand_mean) v = 0.1f * nd(rng);
    return true;
}

struct FwdOut {
    std::vector<float> Rm, PF, Jrest, G, A, M, Jw;
    FwdOut() : Rm(NJ * 9), PF(NPF), Jrest(NJ * 3), G(NJ * 12), A(NJ * 12), M(12), Jw(NJW * 3) {}
    void nan_all() { for (auto* v : {&Rm, &PF, &Jrest, &G, &A, &M, &Jw}) fill_nan(v->data(), v->size() * 4); }
};
struct BwdOut { float dx[XDIM], dO[ODIM], dcam[16], dscale; };

static int levels_of(const Model& m, int jn) {
    int n = 0;
    for (int j = 0; j < jn; ++j) n = std::max(n, m.hs.depth[j] + 1);
    return n;
}

static void run_case(const Model& m, int jn, int jr, unsigned seed) {
    std::mt19937 rng(seed);
    std::normal_distribution<float> nd(0.f, 1.f);
    const PoseModel pm = m.pm();
    const int nlev = levels_of(m, jn);
    const bool contact = jr == NJ, world = jn >= NJW;       // which inputs reach the chain: dA / dPF with the contact state, dJw with the world joints
    static PoseScratch sc;
    for (int row = 0; row < 4; ++row) {
        float x[XDIM], o[ODIM], cam[16];
        for (float& v : x) v = 0.3f * nd(rng);
        for (float& v : o) v = nd(rng);
        for (float& v : cam) v = nd(rng);
        const float scale = 0.8f + 0.1f * row;
        // ---- forward
        FwdOut F, T;
        memset(&sc, 0, sizeof(sc));
        pose_forward(pm, x, o, cam, scale, sc, F.Rm.data(), F.PF.data(), F.Jrest.data(), F.G.data(), F.A.data(), F.M.data(), F.Jw.data(),
                     0, 1, NoSync());
        T.nan_all();
        fill_nan(&sc, sizeof(sc));
        pose_forward(pm, x, o, cam, scale, sc, T.Rm.data(), contact ? T.PF.data() : nullptr, T.Jrest.data(), T.G.data(),
                     contact ? T.A.data() : nullptr, T.M.data(), world ? T.Jw.data() : nullptr, 0, 1, NoSync(), nullptr, 0, jn, jr, nlev);
        for (int j = 0; j < NJ; ++j) {
            for (int e = 0; e < 12; ++e) {
                if (j < jn) {
                    CHECK(same(T.G[12 * j + e], F.G[12 * j + e]), "(%d,%d) G[%d][%d]", jn, jr, j, e);
                    if (contact) CHECK(same(T.A[12 * j + e], F.A[12 * j + e]), "(%d,%d) A[%d][%d]", jn, jr, j, e);
                } else {
                    CHECK(is_fill(T.G[12 * j + e]) && is_fill(T.A[12 * j + e]), "(%d,%d) row %d of G / A was written", jn, jr, j);
                }
            }
            for (int c = 0; c < 3; ++c) {
                if (j < jn) CHECK(same(T.Jrest[3 * j + c], F.Jrest[3 * j + c]), "(%d,%d) Jrest[%d][%d]", jn, jr, j, c);
                else CHECK(is_fill(T.Jrest[3 * j + c]), "(%d,%d) row %d of Jrest was written", jn, jr, j);
            }
            for (int e = 0; e < 9; ++e) {
                if (j < jr) CHECK(same(T.Rm[9 * j + e], F.Rm[9 * j + e]), "(%d,%d) Rm[%d][%d]", jn, jr, j, e);
                else CHECK(is_fill(T.Rm[9 * j + e]), "(%d,%d) row %d of Rm was written", jn, jr, j);
                if (contact && j >= 1) CHECK(same(T.PF[9 * (j - 1) + e], F.PF[9 * (j - 1) + e]), "(%d,%d) PF[%d][%d]", jn, jr, j, e);
            }
        }
        for (int e = 0; e < 12; ++e) CHECK(same(T.M[e], F.M[e]), "(%d,%d) M[%d]", jn, jr, e);
        if (world) for (int e = 0; e < NJW * 3; ++e) CHECK(same(T.Jw[e], F.Jw[e]), "(%d,%d) Jw[%d]", jn, jr, e);
        // ---- backward: the full run gets the same dA with the rows >= jn zeroed, the limited run NaN in their place
        std::vector<float> dA_full(NJ * 12, 0.f), dA_trim(NJ * 12), dPF(NPF), dJw(NJW * 3);
        fill_nan(dA_trim.data(), dA_trim.size() * 4);
        for (int i = 0; i < jn * 12; ++i) dA_full[i] = dA_trim[i] = nd(rng);
        for (float& v : dPF) v = nd(rng);
        for (float& v : dJw) v = nd(rng);
        float dMv[12], dsv = nd(rng), dbeta_v[NBETA], dtransl_v[3], dx0[XDIM];
        for (float& v : dMv) v = nd(rng);
        for (float& v : dbeta_v) v = nd(rng);
        for (float& v : dtransl_v) v = nd(rng);
        for (float& v : dx0) v = nd(rng);
        BwdOut bf, bt;
        memcpy(bf.dx, dx0, sizeof(dx0));
        memset(&sc, 0, sizeof(sc));
        pose_backward(pm, x, o, cam, scale, F.Rm.data(), F.Jrest.data(), F.G.data(), contact ? dA_full.data() : nullptr,
                      contact ? dPF.data() : nullptr, world ? dJw.data() : nullptr, dMv, &dsv, dbeta_v, dtransl_v, sc, bf.dx, bf.dO, bf.dcam,
                      &bf.dscale, 0, 1, NoSync());
        memcpy(bt.dx, dx0, sizeof(dx0));
        fill_nan(bt.dO, sizeof(bt.dO)); fill_nan(bt.dcam, sizeof(bt.dcam)); fill_nan(&bt.dscale, 4);
        fill_nan(&sc, sizeof(sc));
        pose_backward(pm, x, o, cam, scale, (const float*)nullptr, T.Jrest.data(), T.G.data(), contact ? dA_trim.data() : nullptr,
                      contact ? dPF.data() : nullptr, world ? dJw.data() : nullptr, dMv, &dsv, dbeta_v, dtransl_v, sc, bt.dx, bt.dO, bt.dcam,
                      &bt.dscale, 0, 1, NoSync(), nullptr, nullptr, nullptr, 0, jn, jr, nlev);
        for (int e = 0; e < XDIM; ++e) CHECK(same(bt.dx[e], bf.dx[e]), "(%d,%d) dx[%d]: %.9g vs %.9g", jn, jr, e, bt.dx[e], bf.dx[e]);
        for (int e = 0; e < ODIM; ++e) CHECK(same(bt.dO[e], bf.dO[e]), "(%d,%d) dO[%d]: %.9g vs %.9g", jn, jr, e, bt.dO[e], bf.dO[e]);
        for (int e = 0; e < 16; ++e) CHECK(same(bt.dcam[e], bf.dcam[e]), "(%d,%d) dcam_ext[%d]: %.9g vs %.9g", jn, jr, e, bt.dcam[e], bf.dcam[e]);
        CHECK(same(bt.dscale, bf.dscale), "(%d,%d) dscale: %.9g vs %.9g", jn, jr, bt.dscale, bf.dscale);
    }
}

static void check_plans(const Model& m) {
    const int* par = m.hs.parents.data();
    const int* dep = m.hs.depth.data();
    const int nlevels = m.hs.nlevels;
    auto is = [](const PoseJoints& p, int jn, int jr, int nlev, bool world) { return p.jn == jn && p.jr == jr && p.nlev == nlev && p.world == world; };
    CHECK(nlevels == 11, "SMPL-X's tree has 11 levels, not %d", nlevels);
    // phase 1, a leg-only contact set (skinned to joints below 12), no logging
    CHECK(is(plan_pose_joints(par, dep, 12, true, false), 12, NJ, 5, false), "legs, phase 1");
    // the same iteration when it logs, or with anything else that reads the world joints
    CHECK(is(plan_pose_joints(par, dep, 12, true, true), NJW, NJ, 8, true), "legs, logging");
    // phase 2: no contact state, the world joints
    CHECK(is(plan_pose_joints(par, dep, 0, false, true), NJW, NJW, 8, true), "phase 2");
    CHECK(is(plan_pose_joints(par, dep, 12, false, true), NJW, NJW, 8, true), "phase 2: ja_hi does not count without the contact state");
    // a contact set that reaches a joint in 12..22, and one beyond the world joints
    CHECK(is(plan_pose_joints(par, dep, 17, true, false), 17, NJ, 6, false), "ja_hi = 17");
    CHECK(is(plan_pose_joints(par, dep, 17, true, true), NJW, NJ, 8, true), "ja_hi = 17, logging");
    CHECK(is(plan_pose_joints(par, dep, 30, true, true), 30, NJ, 11, true), "ja_hi = 30");
    // nothing reaches the chain: the root alone
    CHECK(is(plan_pose_joints(par, dep, 0, false, false), 1, 1, 1, false), "no contact, no world");
    // every joint skinned to (every vertex a contact): the full plan, world joints included
    CHECK(is(plan_pose_joints(par, dep, NJ, true, false), NJ, NJ, nlevels, true), "ja_hi = 55");
    // the switch: the full plan whatever the rest says
    for (int ja : {0, 12, 17, NJ})
        for (int cs = 0; cs < 2; ++cs)
            for (int nw = 0; nw < 2; ++nw) CHECK(is(plan_pose_joints(par, dep, ja, cs != 0, nw != 0, false), NJ, NJ, nlevels, true), "trim off: %d %d %d", ja, cs, nw);
    // the prefix form needs parents[j] < j below jn: a tree numbered otherwise gets the full plan
    {
        std::vector<int> p2(par, par + NJ), d2(dep, dep + NJ);
        p2[4] = 7; p2[7] = 1; d2[7] = 2; d2[4] = 3; d2[10] = 4;       // 1 -> 7 -> 4 (-> nothing), 7 -> 10: joint 4's parent has a higher number
        CHECK(is(plan_pose_joints(p2.data(), d2.data(), 12, true, false), NJ, NJ, nlevels, true), "prefix violated below jn");
        CHECK(is(plan_pose_joints(p2.data(), d2.data(), 4, true, false), 4, NJ, 2, false), "violation at or above jn does not matter");
    }
}

int main(int argc, char** argv) {
    std::mt19937 rng(1234);
    Model m;
    if (!make_model(&m, rng)) { printf("FAILED: host_pose_setup\n"); return 2; }
    if (argc == 6 && !strcmp(argv[1], "plan")) {
        const PoseJoints p = plan_pose_joints(m.hs.parents.data(), m.hs.depth.data(), atoi(argv[2]), atoi(argv[3]) != 0, atoi(argv[4]) != 0, atoi(argv[5]) != 0);
        printf("%d %d %d %d\n", p.jn, p.jr, p.nlev, p.world ? 1 : 0);
        return 0;
    }
    const int cases[5][2] = {{12, NJ}, {NJW, NJW}, {17, NJ}, {NJ, NJ}, {1, 1}};     // (1, 1): neither a contact term nor the world joints
    for (int k = 0; k < 5; ++k) run_case(m, cases[k][0], cases[k][1], 99 + k);
    check_plans(m);
    printf(g_bad ? "%d checks FAILED\n" : "all checks hold\n", g_bad);
    return g_bad ? 1 : 0;
}
