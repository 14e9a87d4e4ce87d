// TEST INFRASTRUCTURE ONLY (tests/test_reproj_cpu.py): what the clip-level reprojection term (fdcap_opt_set_reproj) adds to the
// host-testable headers, compiled for the host as a stand-alone program; exit status 0 = all hold.
//   * plan_pose_joints (csrc/fdc_forms.h) with the new argument: jn >= 23 in every iteration -- phase 1 with the legs alone, a fit
//     with no contact set at all -- jr as without it; the old results without it
//   * reproj_joint (csrc/fdc_fit2d.h): exact zeros at conf = 0 whatever the coordinates and the depth hold; fit2d_joint's value and
//     gradient, the gradient times wn, at a detected keypoint; a finite-difference check of the gradient
//   * reproj_params_check: what fdcap_opt_set_reproj refuses
// Built with -fsanitize=address,undefined.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>

#include "../../4dcapture-fpv_amd/csrc/fdc_fit2d.h"
#include "../../4dcapture-fpv_amd/csrc/fdc_forms.h"

using namespace fdc;

static const int PARENTS[NJ] = {-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15,
                                20, 25, 26, 20, 28, 29, 20, 31, 32, 20, 34, 35, 20, 37, 38,
                                21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53};

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_bad; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static bool is(const PoseJoints& p, int jn, int jr, int nlev, bool world) { return p.jn == jn && p.jr == jr && p.nlev == nlev && p.world == world; }

int main() {
    int dep[NJ];
    int nlevels = 0;
    for (int j = 0; j < NJ; ++j) { dep[j] = j ? dep[PARENTS[j]] + 1 : 0; nlevels = dep[j] + 1 > nlevels ? dep[j] + 1 : nlevels; }
    const int* par = PARENTS;
    // with the term: the body-frame joints 0..22 in every iteration
    CHECK(is(plan_pose_joints(par, dep, 12, true, false, true, true), NJW, NJ, 8, false), "legs, phase 1, with the term");
    CHECK(is(plan_pose_joints(par, dep, 0, false, false, true, true), NJW, NJW, 8, false), "no contact, no world, with the term");
    CHECK(is(plan_pose_joints(par, dep, 12, true, true, true, true), NJW, NJ, 8, true), "legs, logging, with the term");
    CHECK(is(plan_pose_joints(par, dep, 0, false, true, true, true), NJW, NJW, 8, true), "phase 2, with the term");
    CHECK(is(plan_pose_joints(par, dep, 30, true, false, true, true), 30, NJ, 11, false), "ja_hi = 30, with the term");
    CHECK(is(plan_pose_joints(par, dep, 12, true, false, false, true), NJ, NJ, nlevels, true), "trim off, with the term");
    // without it: the results tests/pose_trim_cpu/trim_check.cpp pins, with the argument left out and with it false
    for (int k = 0; k < 2; ++k) {
        CHECK(is(k ? plan_pose_joints(par, dep, 12, true, false, true, false) : plan_pose_joints(par, dep, 12, true, false), 12, NJ, 5, false), "legs, phase 1");
        CHECK(is(k ? plan_pose_joints(par, dep, 0, false, false, true, false) : plan_pose_joints(par, dep, 0, false, false), 1, 1, 1, false), "no contact, no world");
        CHECK(is(k ? plan_pose_joints(par, dep, 0, false, true, true, false) : plan_pose_joints(par, dep, 0, false, true), NJW, NJW, 8, true), "phase 2");
        CHECK(is(k ? plan_pose_joints(par, dep, 17, true, false, true, false) : plan_pose_joints(par, dep, 17, true, false), 17, NJ, 6, false), "ja_hi = 17");
    }

    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const ReprojIn rp = {nullptr, 692.f, 673.f, 640.f, 360.f, 100.f, 0.25f, nullptr};
    // conf = 0: exact zeros (positive ones) whatever else the keypoint and the joint hold
    const V3 pts[4] = {v3(0.1f, -0.2f, 3.5f), v3(0.1f, -0.2f, 0.f), v3(nan, nan, nan), v3(1.f, 1.f, -1e-30f)};
    const float coords[4] = {nan, inf, -inf, 1e30f};
    for (const V3& p : pts)
        for (float c : coords)
            for (float conf : {0.f, -0.f}) {
                V3 d = v3(nan, nan, nan);
                const float val = reproj_joint(rp, p, c, c, conf, &d);
                CHECK(bits(val) == 0 && bits(d.x) == 0 && bits(d.y) == 0 && bits(d.z) == 0, "conf = 0: %g (%g %g %g)", val, d.x, d.y, d.z);
            }
    // a detected keypoint: fit2d_joint at w_data = 1, the gradient times wn, the value without it
    {
        const Fit2dStage s = {rp.fx, rp.fy, rp.cx, rp.cy, rp.rho, 1.f, 0.f, 0.f, 0.f};
        const V3 p = v3(0.31f, -0.42f, 3.3f);
        const float ku = 720.f, kv = 250.f, conf = 0.7f;
        V3 d0, d1;
        const float v0 = fit2d_joint(s, p, ku, kv, conf, &d0), v1 = reproj_joint(rp, p, ku, kv, conf, &d1);
        CHECK(bits(v0) == bits(v1), "value %g %g", v0, v1);
        CHECK(d1.x == d0.x * rp.wn && d1.y == d0.y * rp.wn && d1.z == d0.z * rp.wn, "gradient");
        CHECK(v1 > 0.f && d1.x != 0.f && d1.y != 0.f && d1.z != 0.f, "a live keypoint");
        // central differences of wn * value in double steps of 1e-3 (the value is smooth there: error ~ h^2)
        const float h = 1e-3f;
        const float g[3] = {d1.x, d1.y, d1.z};
        for (int c = 0; c < 3; ++c) {
            V3 a = p, b = p, t;
            (c == 0 ? a.x : c == 1 ? a.y : a.z) += h;
            (c == 0 ? b.x : c == 1 ? b.y : b.z) -= h;
            const double fd = ((double)reproj_joint(rp, a, ku, kv, conf, &t) - (double)reproj_joint(rp, b, ku, kv, conf, &t)) / (2.0 * h) * rp.wn;
            CHECK(fabs(fd - g[c]) <= 2e-3 * fabs(g[c]) + 1e-3, "d/d%c: %g vs %g", "xyz"[c], fd, g[c]);
        }
    }
    // what fdcap_opt_set_reproj refuses with FDCAP_E_ARG
    CHECK(reproj_params_check(692.f, 692.f, 640.f, 360.f, 100.f, 1.f) == 0, "the defaults");
    CHECK(reproj_params_check(692.f, 692.f, 640.f, 360.f, 100.f, 0.f) == 0, "weight 0");
    const float badf[4] = {0.f, -1.f, nan, inf};
    for (float b : badf) {
        CHECK(reproj_params_check(b, 692.f, 640.f, 360.f, 100.f, 1.f) != 0, "fx %g", b);
        CHECK(reproj_params_check(692.f, b, 640.f, 360.f, 100.f, 1.f) != 0, "fy %g", b);
        CHECK(reproj_params_check(692.f, 692.f, 640.f, 360.f, b, 1.f) != 0, "rho %g", b);
    }
    CHECK(reproj_params_check(692.f, 692.f, 640.f, 360.f, 100.f, -1.f) != 0 && reproj_params_check(692.f, 692.f, 640.f, 360.f, 100.f, nan) != 0 &&
          reproj_params_check(692.f, 692.f, 640.f, 360.f, 100.f, inf) != 0, "weight");
    CHECK(reproj_params_check(692.f, 692.f, nan, 360.f, 100.f, 1.f) != 0 && reproj_params_check(692.f, 692.f, 640.f, inf, 100.f, 1.f) != 0, "cx, cy");
    if (g_bad) { printf("%d checks failed\n", g_bad); return 1; }
    printf("ok\n");
    return 0;
}
