"""The yardsticks of tests/test_gpu_local2_bars.py evaluated with the oracle alone (tests/local2_bars.py, tests/dct_bars.py): the
conditions under which the two precisions' difference is a rounding yardstick hold for every case; every alternative form of
cal_loss2 and of cal_dctloss (MUTANTS) leaves at least one block's bar by FACTOR = 20 wherever it applies; and the case that is
the reason for these files stays on record -- the whole-matrix bar accepts a gradient without the blend products' backward.

Worst max|mutant - g64| / bar over the cases and splits where the mutant applies (x86-64, torch 2 CPU kernels):
  second loop   zero_product 1.9e+04   no_posedirs_bwd 7.4e+03   J_no_betas 7.1e+03   vs_tail 5.6e+02   fs_tail 1.1e+03
                w_i 2.1e+04   one_den 5.6e+04   no_thresh 3.8e+04
  DCT term      den 1.2e+05   basis_row 1.3e+04   tail_window 6.9e+04   mean_69 5.2e+05"""
import numpy as np
import pytest
import torch

import tests.dct_bars as db
import tests.gradient_bars as gb
import tests.local2_bars as lb
import tests.test_settings_cpu as sc

FACTOR = sc.FACTOR
OLD_RTOL, OLD_ATOL = 3e-3, 3e-4            # test_gpu_parity.py::test_local_mode_second_loop_gradient_matches_autograd: atol = 3e-4 max|g|


def test_the_restated_loss_is_cal_loss2():
    """lb.loss2_terms without a mutant against FittingOracle.cal_loss2, both precisions, case C at an unequal split: the four values
    bit for bit; the gradient of their sum to 4 units of roundoff of max|g| (the helper shares one forward among all splits and
    mutants, so autograd adds the rows' three contributions up in another order than in cal_loss2's own graph)."""
    case, dup = lb.CASES["C"]
    for dtype in (torch.float64, torch.float32):
        f, verts, x0, idx1, w = lb._forward(case, dup, dtype)
        mine, _ = lb.loss2_terms(f, verts, x0, idx1, w, 1)
        l_rec, l_loc, l_sm, l_cs = f.cal_loss2(x0, idx1, w, 1)
        for a, b in zip(mine, (l_rec, l_loc, l_sm, l_cs)):
            assert torch.equal(a.detach(), b.detach())
        (ga,) = torch.autograd.grad(mine[2] + mine[1] + mine[0] + mine[3], f.body_rotation_rec)
        (gb_,) = torch.autograd.grad(l_sm + l_loc + l_rec + l_cs, f.body_rotation_rec)
        err, eps = float((ga - gb_).abs().max()), torch.finfo(dtype).eps
        print(dtype, "max |difference of the gradients|", err, "max|g|", float(gb_.abs().max()))
        assert err <= 4 * eps * float(gb_.abs().max()) and float(ga.abs().max()) > 0


def test_the_weight_pattern_decides_alike_in_both_precisions():
    """`w < 0.5` and `1 - w < 0.5` fall the same way in fp32 and fp64 for every weight of the pattern.  (1 - w itself is not exact
    in fp32 for 0.3 and for the float below 0.5 -- 1 - (0.5 - 2^-25) rounds to 0.5, which stays on the kept side as 0.5 + 2^-25
    does -- the decisions are what has to agree.)  The pattern has weights on both sides of the threshold next to it, on it, and at
    0 and 1, and each side of it is taken by a left and by a right weight."""
    w = lb.WEIGHT_PATTERN
    l32, l64 = np.float32(1) - w, 1.0 - w.astype(np.float64)
    assert l32.dtype == np.float32 and np.array_equal(l32 < 0.5, l64 < 0.5)
    assert np.array_equal(w < np.float32(0.5), w.astype(np.float64) < 0.5)
    assert (l32 < 0.5).tolist() == [False, True, False, False, True, True, False]
    assert (w < 0.5).tolist() == [False, False, True, True, False, False, True]
    assert lb.LO < 0.5 < lb.HI and float(lb.HI) - float(lb.LO) == 2.0 ** -24 + 2.0 ** -25
    assert {0.0, 0.5, 1.0, float(lb.LO), float(lb.HI)} <= set(map(float, w))
    assert lb.weights(9).shape == (9,) and np.array_equal(lb.weights(9)[7:], w[:2])


@pytest.mark.parametrize("name", sorted(lb.CASES))
def test_conditions_hold_and_every_mutant_leaves_a_bar(name):
    """Per case and split n_left in (1, nc // 2, nc - 1): reference() asserts the conditions while it builds the bars; then every
    mutant that applies leaves at least one block's bar by FACTOR, and `one_den` changes nothing where the parts are equal."""
    case, dup = lb.CASES[name]
    nc = len(sc.make_case(*case)[4])
    assert (3 * case[1], 3 * nc) == {"A": (255, 12), "B": (258, 18), "C": (1023, 258), "D": (1026, 300), "E": (2100, 72), "F": (2100, 900)}[name]
    for n_left in lb.n_lefts(case):
        ref = lb.reference(case, dup, n_left)
        print(f"{name} {case} n_left {n_left}: smallest |dd64| {ref['margin'][0]:.3g}, max|dd32 - dd64| {ref['margin'][1]:.3g}; bars",
              " ".join(f"{k} {v:.2g}" for k, v in ref["bar"].items()))
        assert all(v > 0 for v in ref["bar"].values())
        for mutant in lb.MUTANTS:
            g = lb.mutant_gradient(case, dup, n_left, mutant)
            if not lb.applies(mutant, case, n_left):
                if mutant == "one_den":
                    assert all(np.array_equal(g[k], ref["g64"][k]) for k in g)
                continue
            r = gb.ratios(g, ref["g64"], ref["bar"])
            print(f"   {mutant}: worst {max(r.values()):.3g} |", " ".join(f"{k} {v:.2g}" for k, v in r.items()))
            assert max(r.values()) >= FACTOR, (name, n_left, mutant, r)


@pytest.mark.parametrize("name", sorted(lb.BATCHES))
def test_conditions_hold_for_every_clip_of_the_batches(name):
    """The clips of a batch are cases of their own on case C's models, weighted by the pattern from their first row on: the
    conditions hold (asserted by reference()), the pair weight and the denominators are observed in each clip alone, the threshold
    in at least one clip of each batch."""
    batch = lb.BATCHES[name]
    assert lb.batch_offsets(batch) == {"ragged": (0, 5, 8), "equal": (0, 4)}[name]
    models = [lb.make_case(c) for c in batch]
    for m in models[1:]:
        assert np.array_equal(m[0].posedirs, models[0][0].posedirs) and np.array_equal(m[1].fc2_w, models[0][1].fc2_w)
        assert np.array_equal(m[4], models[0][4]) and np.array_equal(m[3], models[0][3])
    assert len({m[2].body_params.tobytes() for m in models}) == len(batch)
    thresh = []
    for case, off in zip(batch, lb.batch_offsets(batch)):
        for n_left in lb.BATCH_N_LEFTS:
            ref = lb.reference(case, None, n_left, off)
            assert np.array_equal(ref["w"], np.resize(lb.WEIGHT_PATTERN, off + case[0])[off:])
            for mutant in ("w_i", "one_den", "no_thresh"):
                f64 = lb._forward_pair(case, None, off)[0]
                r = gb.ratios(gb.blocks(rows=lb._gradient(f64, n_left, mutant)[0]), ref["g64"], ref["bar"])
                print(f"{name} {case} n_left {n_left} {mutant}: worst {max(r.values()):.3g}")
                if mutant == "no_thresh":                        # (the second clip of (4, 4) has the pair weights 1, 0 and 0.5: nothing to cut)
                    thresh.append(max(r.values()))
                else:
                    assert max(r.values()) >= FACTOR, (case, n_left, mutant, r)
    assert sum(v >= FACTOR for v in thresh) >= len(lb.BATCH_N_LEFTS)


def test_every_mutant_applies_somewhere():
    for mutant in lb.MUTANTS:
        assert any(lb.applies(mutant, case, nl) for case, _ in lb.CASES.values() for nl in lb.n_lefts(case)), mutant
    for mutant in db.MUTANTS:
        assert any(db.applies(mutant, n) for n in db.CASES), mutant


def _old_tests_vertex_term(case, mutant):
    """d l_sm / d rows in fp64 at the state of the old second-loop test: the fp64 start rows + 0.01 randn of seed 6."""
    from oracle import rotrepr
    from oracle.fitting import FittingOracle
    bm, vp, clip, scene, vid, n = sc.make_case(*case)
    dt = torch.float64
    body_cls, vposer_cls = gb._models(mutant, vid, 0)
    f = FittingOracle(body_cls(bm, dt), vposer_cls.from_data(vp, dt), scene, vid, clip.camerapose_lines, n, dtype=dt)
    x78 = rotrepr.convert_to_6D_rot(torch.tensor(clip.body_params, dtype=dt)).detach()
    idx1 = f.init(x78)
    f.body_rotation_rec.data += 0.01 * torch.randn((n, 78), generator=torch.Generator().manual_seed(6), dtype=dt)
    l_sm = f.cal_loss2(x78, idx1, torch.full((n,), 0.5, dtype=dt), len(vid) // 2)[2]
    return gb.blocks(rows=torch.autograd.grad(l_sm, f.body_rotation_rec)[0].numpy())


def test_the_whole_matrix_bar_accepts_a_gradient_without_the_blend_products_backward():
    """Why tests/local2_bars.py exists.  Case (7, 777, 801, 7, 12), the vertex-smoothing term ALONE, at the state the old test
    differentiates at (test_local_mode_second_loop_gradient_matches_autograd: fp64 start rows + 0.01 randn of seed 6): with v_posed
    detached (`zero_product`: the whole backward through the blend products missing) the latent, lh and rh blocks move by less than
    atol = 3e-4 max|g| -- measured 0.92, 0.97 and 0.94 of it -- so the old bar accepts the mutant there.  (At the state of
    tests/local2_bars.py, perturbation seed 5, the same figures are 1.10, 1.11 and 0.87, and in the full loss 3.9, 2.7 and 5.5: the
    old bar sees the mutant by a small factor at best.)  Against the per-block bars of the full loss the mutant is out by 8e+02
    (latent) to 5e+04 (betas)."""
    case, n_left = gb.PARITY_CASES[2], 7
    assert case == (7, 777, 801, 7, 12)
    g, m = _old_tests_vertex_term(case, None), _old_tests_vertex_term(case, "zero_product")
    atol = OLD_ATOL * max(np.abs(v).max() for v in g.values())
    for k in ("latent", "lh", "rh"):
        moved = np.abs(m[k] - g[k])
        print(f"vertex term alone, {k}: the mutant moves max {moved.max() / atol:.3g} atol")
        assert 0 < moved.max() < atol
    # the full loss at the state the new GPU tests use: old atol and new bars
    full, mfull = lb.term_gradient(case, None, n_left, ("sm", "loc", "rec", "cs")), lb.mutant_gradient(case, None, n_left, "zero_product")
    atol_full = OLD_ATOL * max(np.abs(v).max() for v in full.values())
    print("full loss: the mutant leaves the old atol by", {k: f"{np.abs(mfull[k] - full[k]).max() / atol_full:.3g}" for k in full})
    ref = lb.reference(case, None, n_left)
    r = gb.ratios(mfull, ref["g64"], ref["bar"])
    print("full loss: the mutant against the per-block bars", {k: f"{v:.3g}" for k, v in r.items()})
    for k in ("betas", "latent", "lh", "rh"):
        assert r[k] >= FACTOR, (k, r[k])


@pytest.mark.parametrize("n", db.CASES)
def test_dct_mutants_leave_a_bar(n):
    """The DCT term alone at cpu_state(n): the hand blocks are exactly zero in both precisions (bar 0: the GPU must match them
    exactly), the tail rows carry no gradient, and each alternative form of cal_dctloss leaves a bar by FACTOR where it applies."""
    state = db.cpu_state(n)
    ref = db.reference(n, state)
    print(f"n = {n}: l_dct {ref['l_dct']:.6g}; bars", " ".join(f"{k} {v:.2g}" for k, v in ref["bar"].items()))
    assert ref["bar"]["lh"] == 0 and ref["bar"]["rh"] == 0
    assert all(v > 0 for k, v in ref["bar"].items() if k not in ("lh", "rh"))
    rows64 = np.concatenate([ref["g64"][k] for k in gb.ROW_BLOCKS], axis=1)
    assert not rows64[db.T * (n // db.T):].any() and rows64[:db.T * (n // db.T)].any(axis=1).all()
    for mutant in db.MUTANTS:
        g = db.mutant_gradient(n, state, mutant)
        if not db.applies(mutant, n):
            assert all(np.array_equal(g[k], ref["g64"][k]) for k in g), mutant
            continue
        r = gb.ratios(g, ref["g64"], ref["bar"])
        print(f"   {mutant}: worst {max(r.values()):.3g} |", " ".join(f"{k} {v:.2g}" for k, v in r.items()))
        assert max(r.values()) >= FACTOR, (n, mutant, r)
