"""Gradient bars cut per loss term and per column block, derived from the oracle's own two precisions (no GPU needed).

The project's older gradient comparison (rtol 2e-3, atol 2e-4 max|g| over the whole [n, 78] matrix, at the default phase-1 mix
0.1 l_con + l_sm + l_rec) is blind to most of the body-model chain: the two L1 terms put a sign gradient of constant size into every
column and set max|g|, while everything that reaches a row through the contact term is a few per cent of it -- the latent block
5 %, betas 0.4 %, the hands 0.1 % -- so whole factors of the chain (the backward through the blend products, the joint regressor's
dependence on betas) can be missing inside atol.  The zero switches isolate a term (weight_loss_rec = 0 with PHASE1_SMOOTH = 0
leaves l_con, with PHASE2_SMOOTH = 0 leaves l_ws), and then a bar can be as tight as fp32 arithmetic allows:

    bar_b = M * max( max|g32_b - g64_b| , 2^-24 max|g64_b| )        per block b, elementwise absolute, no rtol

g32 / g64: the oracle's autograd in fp32 / fp64 at the SAME fp32-rounded state (as_the_gpu_holds_it), so the bar comes from the
reference's arithmetic and never from the kernels.  M = 32: the dense products are pinned at 1e-6 sum|a||b| (tests/test_gpu_panel.py)
against fp32's unit roundoff 2^-24 = 6e-8 -- a ratio of 16.8 -- doubled for a different summation order.

tests/test_gradient_bars_cpu.py evaluates, with the oracle alone, that gradients with a part of the chain missing (MUTANTS: the
oracle's graph with a tensor detached, values unchanged) leave these bars by a factor, so the GPU tests that use them
(tests/test_gpu_gradient_bars.py, tests/test_gpu_panel.py) cannot pass vacuously."""
import functools

import numpy as np
import torch

import tests.test_settings_cpu as sc
from oracle import rotrepr
from oracle.chamfer import nn_direct
from oracle.fitting import find_outliers_and_sources
from oracle.smplx import SMPLXOracle
from oracle.vposer import VPoserDecoder

M = 32.0
EPS32 = 2.0 ** -24
ROW_BLOCKS = {"transl": slice(0, 3), "sixd": slice(3, 9), "betas": slice(9, 19), "latent": slice(19, 51), "lh": slice(51, 63),
              "rh": slice(63, 75), "camt": slice(75, 78)}
# coefficient of the unweighted term in the loss total when the other terms are switched off (fdcap_amd.fitting's defaults:
# weight_contact x PHASE1_CONTACT, PHASE2_WORLD)
COEFF = {"con": 0.1 * 0.1, "ws": 1.0}
# n, V, scene points, contact vertices per part, seed: tests/test_gpu_parity.py test_optimiser_gradients_match_autograd and its ragged shapes
PARITY_CASES = [(12, 300, 800, 20, 0), (4, 120, 50, 1, 11), (7, 777, 801, 7, 12), (19, 300, 5000, 40, 13), (33, 150, 333, 3, 14),
                (65, 512, 2049, 17, 15), (130, 240, 1000, 9, 16)]
TAIL = 11                                  # contact vertices whose blend offsets `drop_tail` detaches: 33 K-columns, one 32-column ring step
MUTANTS = ("zero_product", "drop_tail", "no_posedirs_bwd", "no_hand_posedirs_bwd", "J_no_betas", "vposer_part")
# the blocks each mutant must leave in the isolated contact term (tests/test_gradient_bars_cpu.py)
TARGETS = {"zero_product": ("betas", "latent", "lh", "rh"), "drop_tail": ("betas", "latent", "lh", "rh"),
           "no_posedirs_bwd": ("latent", "lh", "rh"), "no_hand_posedirs_bwd": ("lh", "rh"), "J_no_betas": ("betas",),
           "vposer_part": ("latent",)}


def blocks(rows=None, dscale=None, dcam=None):
    """-> {block name: array} of a row gradient [n, 78], d scale and d camera_ext [n, 16] (row-major 4 x 4: the 3 x 3 rotation
    part, the translation column, the bottom row)."""
    out = {}
    if rows is not None:
        rows = np.asarray(rows, dtype=np.float64)
        out.update({k: rows[:, s] for k, s in ROW_BLOCKS.items()})
    if dscale is not None:
        out["dscale"] = np.asarray(dscale, dtype=np.float64).reshape(1)
    if dcam is not None:
        c = np.asarray(dcam, dtype=np.float64).reshape(-1, 4, 4)
        out.update({"cam_rot": c[:, :3, :3], "cam_transl": c[:, :3, 3], "cam_bottom": c[:, 3, :]})
    return out


def bars(b32, b64):
    """The bar of every block from the oracle's two precisions."""
    return {k: M * max(float(np.abs(b32[k] - b64[k]).max()), EPS32 * float(np.abs(b64[k]).max())) for k in b64}


def ratios(got, want, bar):
    """max|got - want| / bar per block; a block whose bar is 0 (the camera's bottom row) must be matched exactly: 0 or inf."""
    out = {}
    for k in want:
        err = float(np.abs(np.asarray(got[k], dtype=np.float64) - want[k]).max())
        out[k] = err / bar[k] if bar[k] > 0 else (0.0 if err == 0 else float("inf"))
    return out


def _models(mutant, vid, part):
    """The oracle's body model and decoder with the mutant's tensor detached (tap() of oracle/smplx.py, oracle/vposer.py)."""
    if mutant is None:
        return SMPLXOracle, VPoserDecoder
    assert mutant in MUTANTS, mutant
    tail = torch.as_tensor(np.asarray(vid)[-TAIL:], dtype=torch.long)

    def cut(v, mask):                                           # the same values, no gradient where mask
        return torch.where(mask, v.detach(), v)

    class Body(SMPLXOracle):
        def tap(self, point, v):
            if point == "v_posed" and mutant == "zero_product":                 # v_posed - v_template of all vertices
                return v.detach()
            if point == "v_posed" and mutant == "drop_tail":                    # ... of the last contact vertices
                mask = torch.zeros(v.shape[1], dtype=torch.bool)
                mask[tail] = True
                return cut(v, mask[None, :, None])
            if point == "pose_feature" and mutant == "no_posedirs_bwd":
                return v.detach()
            if point == "pose_feature" and mutant == "no_hand_posedirs_bwd":    # joints 25 .. 54: columns 9 (j - 1) ..
                return cut(v, (torch.arange(v.shape[1]) >= 9 * 24)[None, :])
            if point == "v_shaped_to_joints" and mutant == "J_no_betas":
                return v.detach()
            return v

    class Decoder(VPoserDecoder):
        def tap(self, point, v):
            # vposer_bwd_*_kernel (csrc/fdc_panel.h): workgroup q of a row block owns columns 128 q .. 128 q + 127 of the second
            # hidden layer -- dH2[:, quarter] = dO x W3[:, quarter], down to its own partial latent gradient
            if point == "hidden2" and mutant == "vposer_part":
                c = torch.arange(v.shape[1])
                return cut(v, ((c >= 128 * part) & (c < 128 * part + 128))[None, :])
            return v

    return Body, Decoder


def _term_blocks(t):
    return {"con": blocks(rows=t["g"]["con"][0], dscale=t["g"]["con"][1]), "ws": blocks(rows=t["g"]["ws"][0], dcam=t["g"]["ws"][2])}


def _neighbours(f, vid):
    with torch.no_grad():
        _, verts, _ = f.forward_world()
        return np.stack([nn_direct(verts[b, vid], f.s_verts_batch[b])[1].numpy() for b in range(verts.shape[0])])


def start_state(case, edit=None):
    """What the GPU is given and then holds: the fp32 start rows `x78` for init(), `rows` after init() (outlier rows replaced) and
    `+= fp32(perturbation)`, and the start scale.  edit: sc.term_gradients' (None: the clip as it is)."""
    c = sc.make_case(*case)
    body_params = c[2].body_params if edit is None else edit.clip(c[2].body_params)
    x78 = rotrepr.convert_to_6D_rot(torch.tensor(body_params, dtype=torch.float64)).detach().float()
    if edit is not None:
        x78 = edit.rows(x78)
    idx1, pos = find_outliers_and_sources(x78)
    rows = x78.clone()
    if len(idx1) and len(pos):
        rows[idx1] = x78[pos]
    rows += sc.perturbation(c[5]).float()
    return {"x78": x78.numpy(), "rows": rows.numpy(), "scale": np.float32(sc.DEFAULTS["scale_init"])}


@functools.lru_cache(maxsize=None)
def isolated_terms(case, edit=None):
    """case = (n, V, scene points, contact vertices per part, seed), the models of tests/test_gpu_parity.py _make_fop.
    -> {"g64", "g32": {term: {block: array}}, "bar": {term: {block: float}}, "x78", "rows", "scale"}: the oracle's gradients of
    l_con alone (d rows, d scale) and of l_ws alone (d rows, d camera_ext), unweighted, in both precisions at the state the GPU holds
    (start rows rounded to fp32, + fp32(0.01 randn, seed 5), scale fp32(1.8)), and the bars.  Multiply all three by COEFF[term].
    "l1": the fp64 row gradient of l_rec + l_sm, for the default phase-1 mix.
    edit: sc.term_gradients' (None: the clip as it is; the existing cases)."""
    c = sc.make_case(*case)
    vid = c[4]
    t64 = sc.term_gradients(c, sc.DEFAULTS["scale_init"], torch.float64, ("rec", "sm", "con", "ws"), as_the_gpu_holds_it=True, edit=edit)
    t32 = sc.term_gradients(c, sc.DEFAULTS["scale_init"], torch.float32, ("con", "ws"), as_the_gpu_holds_it=True, edit=edit)
    start = start_state(case, edit)
    assert np.array_equal(t64["rows"].numpy(), start["rows"].astype(np.float64)) and np.array_equal(t32["rows"].numpy(), start["rows"])
    # a bar that contained a nearest-neighbour flip between the two precisions would be no rounding yardstick
    assert np.array_equal(_neighbours(t64["oracle"], vid), _neighbours(t32["oracle"], vid)), f"nearest neighbours differ between fp32 and fp64: take another seed than {case}"
    g64, g32 = _term_blocks(t64), _term_blocks(t32)
    return dict(start, g64=g64, g32=g32, bar={k: bars(g32[k], g64[k]) for k in g64}, l1=t64["g"]["rec"][0] + t64["g"]["sm"][0])


@functools.lru_cache(maxsize=None)
def mutant_terms(case, mutant, part=0, terms=("con",)):
    """The fp64 gradients of isolated_terms with the mutant's contribution missing -> {term: {block: array}}."""
    c = sc.make_case(*case)
    body_cls, vposer_cls = _models(mutant, c[4], part)
    t = sc.term_gradients(c, sc.DEFAULTS["scale_init"], torch.float64, terms, as_the_gpu_holds_it=True, body_cls=body_cls, vposer_cls=vposer_cls)
    out = {}
    if "con" in terms:
        out["con"] = blocks(rows=t["g"]["con"][0], dscale=t["g"]["con"][1])
    if "ws" in terms:
        out["ws"] = blocks(rows=t["g"]["ws"][0], dcam=t["g"]["ws"][2])
    return out


def check(got, want, bar, coeff, label):
    """Every block of `got` against coeff x bar around coeff x want: prints max|err| / bar per block
    -> the blocks outside their bar, {block: (err / bar, bar, max|g|)}; the caller asserts that there are none."""
    want = {k: coeff * v for k, v in want.items()}
    bar = {k: coeff * v for k, v in bar.items()}
    r = ratios(got, want, bar)
    print(label, "max|err| / bar:", " ".join(f"{k} {v:.3g}" for k, v in r.items()))
    return {k: (v, bar[k], float(np.abs(want[k]).max())) for k, v in r.items() if not v <= 1.0}
