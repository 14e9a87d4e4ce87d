// Host program of tests/test_forms_cpu.py: the plans of csrc/fdc_forms.h over the sweep of sweep_driver.h, as text.  The vertex
// sets are the synthetic models': K weights per vertex, nnz = K x vertices, the packed layouts while K <= 12, the permuted forward
// operand for sets of <= 512 vertices with K <= 4, the MFMA-fragment weights for sets of more than 512 (SkinSet, fdc_state.h).
#include "fdc_forms.h"
#include "sweep_driver.h"

using namespace fdc;

static const int NPFX = 496;                 // columns of the blend operand [pose feature | betas] (fdc_frame.h)
#ifndef FORMS_NP
#define FORMS_NP 2                           // planes of the default operand format (PnH2)
#endif
static const int NP = FORMS_NP;

static std::string name_of(Form f) { const char* n = form_name(f); return n ? n : (f == F_NONE ? "none" : "unnamed"); }
static Rec panel_rec(const PanelPlan& p) {
    return Rec{fmt("form=%s nw=%d T=%d cs=%d ks=%d block=%d lds=%zu max_lds=%zu two_partials=%d", name_of(p.form).c_str(), p.nw, p.T, p.cs, p.ks,
                   p.block, p.lds, p.max_lds, (int)p.two_partials),
               fmt("grid=%d mp=%d,%d,%d,%d,%d,%d", p.grid, p.mp.nrb, p.mp.ncb, p.mp.xc, p.mp.rpg, p.mp.cpg, p.mp.rfast)};
}
static Rec skin_rec(const SkinBwdPlan& p) {
    return Rec{fmt("form=%s G=%d vpt=%d kc=%d nch=%d block=%d lds=%zu ja_rows=%d", name_of(p.form).c_str(), p.G, p.vpt, p.kc, p.nch, p.block, p.lds,
                   (int)p.ja_rows),
               fmt("grid=%d", p.grid)};
}

Rec ev_pfwd(int rows, int nv) { return panel_rec(plan_panel3(rows, NPFX, (3 * nv + 15) / 16, (NPFX + 31) / 32, NP, forms_read_env())); }
Rec ev_bwd(int rows, int nv, bool may_split) {
    const int K = 3 * nv;
    return panel_rec(plan_blend_backward(rows, K, (NPFX + 15) / 16, (K + 31) / 32, NP, may_split, forms_read_env()));
}
Rec ev_cfwd(int rows, int nv, int wpv, int ja) {
    const ContactFwdPlan p = plan_contact_forward(rows, nv, NPFX, NP, false, nv <= 512 && wpv <= 4, wpv <= 12 && nv <= 65535, wpv, ja, forms_read_env());
    return Rec{fmt("form=%s block=%d lds=%zu max_lds=%zu", name_of(p.form).c_str(), p.block, p.lds, p.max_lds), fmt("grid=%d,%d", p.grid, p.grid_y)};
}
Rec ev_skin(int rows, int nv, int wpv) {
    const bool packed = wpv <= 12 && nv <= 65535;
    return skin_rec(plan_contact_skin_bwd(rows, nv, wpv * nv, wpv, packed, packed, true, nv > 512, forms_read_env().skin_vec));
}
Rec ev_skinany(int rows, int nv) { return skin_rec(plan_skin_bwd_any(rows, nv, nv > 512)); }
Rec ev_nn(int rows, int nv, int ns) {
    const FormSwitches sw = forms_read_env();
    const int nq = rows * nv;
    const bool culled = sw.nn_seed && sw.nn_cull;
    const int nsplit = nn_pick_nsplit(nq, ns, culled), nsplit_bf = nn_pick_nsplit(nq, ns, false);
    const NNPlan p = plan_nn_search(nq, ns, culled, sw.nn_cull, sw.nn_seed, nsplit, g_nn_mode, sw);
    return Rec{fmt("form=%s wpg=%d nq_blocks=%d block=%d", name_of(p.form).c_str(), p.wpg, p.nq_blocks, p.block),
               fmt("grid=%d groups=%d nsplit=%d nsplit_bf=%d", p.grid, p.groups, nsplit, nsplit_bf)};
}
