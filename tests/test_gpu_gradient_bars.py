"""The in-loop backward chain with ONE loss term switched on, every column block held to a bar of its own (tests/gradient_bars.py:
bar = 32 x max(fp32 oracle - fp64 oracle, 2^-24 max|g|) per block, from the oracle's two precisions; tests/test_gradient_bars_cpu.py
shows on the CPU that a gradient with the blend products' backward, a ring step, a VPoser partial sum or the joint regressor's
dependence on betas missing leaves these bars by a factor).

  phase 1, weight_loss_rec = 0 and PHASE1_SMOOTH = 0: the contact term alone -- d rows, d scale;
  phase 2, weight_loss_rec = 0 and PHASE2_SMOOTH = 0: the world-joint term alone -- d rows, d camera_ext (bottom row exactly zero).

Each case runs with the default products (two fp16 planes) in this process and with the exact-fp32 products (FDCAP_GEMM_SPLIT3=0,
read once per process) in a child; both forms are held to the same bars.

Worst measured max|err| / bar per block over the seven cases (MI355X), fp16 planes / exact fp32:
  contact term   transl 0.042 / 0.069   sixd 0.053 / 0.063   betas 0.044 / 0.060   latent 0.042 / 0.105   lh 0.061 / 0.089
                 rh 0.037 / 0.048   camt 0.042 / 0.068   dscale 0.18 / 0.20
  world term     transl 0.116 / 0.116   sixd 0.063 / 0.072   betas 0.031 / 0.074   latent 0.027 / 0.055   lh, rh 0 / 0 (exact zeros)
                 camt 0.031 / 0.031   cam_rot 0.044 / 0.044   cam_transl 0.031 / 0.031   cam_bottom 0 / 0 (exact zeros)
The sixteen ring and fused-VPoser cases of tests/test_gpu_panel.py (contact term, fp16 planes): at most 0.080 (betas) in a row
block, 0.44 in dscale."""
import os

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
import tests.gradient_bars as gb
import tests.test_settings_cpu as sc
from fdcap_amd import capi
from fdcap_amd import fitting as fit_mod
from fdcap_amd.fitting import FittingOP
from fdcap_amd.io import read_camerapose

pytestmark = pytest.mark.gpu
BIG = 10 ** 6
CASES = gb.PARITY_CASES


def isolated_backward(case, term, it=None):
    """fdcap_opt_backward with one term switched on, at the state of gb.isolated_terms (`it`; None: only its start, without the
    oracle's gradients).  term "con": phase 1 with the data and smoothing terms at zero weight -> blocks of d rows and d scale;
    "ws": phase 2 likewise -> blocks of d rows and d camera_ext.  -> (blocks, the kernel forms the backward's launches took)"""
    import ctypes
    bm, vp, clip, scene, vid, n = sc.make_case(*case)
    start = gb.start_state(case) if it is None else it
    forms = ctypes.create_string_buffer(4096)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(fit_mod, "PHASE1_SMOOTH" if term == "con" else "PHASE2_SMOOTH", 0.0)
        fop = FittingOP({"num_iter": 500}, {"weight_contact": 0.1, "weight_loss_rec": 0.0}, n, body_model=bm, vposer=vp, scene_verts=scene,
                        contact_ids=vid, camera_ext=read_camerapose(clip.camerapose_lines))
        try:
            fop.init(torch.tensor(start["x78"]).cuda())
            fop._rows_x[2:2 + n] += sc.perturbation(n).float().cuda()
            # the oracle differentiates at exactly the state the device holds
            assert np.array_equal(fop._rows_x[2:2 + n].cpu().numpy(), start["rows"])
            assert np.float32(fop._scale.cpu().numpy()[0]) == start["scale"]
            lib, h = fop.ctx.lib, fop.ctx.handle
            capi.check(lib.fdcap_debug_kernel_forms(forms, len(forms), 1), "kernel_forms")      # (reset)
            # (a logging backward: d loss / d scale is summed over the frames right here, not by the step that would follow)
            capi.check(lib.fdcap_opt_backward(h, 5, BIG if term == "con" else 0, 1, capi.current_stream()), "backward")
            dx = torch.empty(n, 78, device="cuda")
            dcam = torch.empty(n, 16, device="cuda")
            capi.check(lib.fdcap_opt_get_grads(h, capi.dptr(dx), capi.dptr(dcam), capi.current_stream()), "grads")
            torch.cuda.synchronize()
            capi.check(lib.fdcap_debug_kernel_forms(forms, len(forms), 0), "kernel_forms")
            if term == "con":
                out = gb.blocks(rows=dx.cpu().numpy(), dscale=float(fop._dscale.cpu()))
            else:
                out = gb.blocks(rows=dx.cpu().numpy(), dcam=dcam.cpu().numpy())
        finally:
            fop.close()
    return out, forms.value.decode().split(";")


def check_isolated(case, term, got, label):
    """Prints max|err| / bar per block, -> the blocks outside their bar"""
    it = gb.isolated_terms(case)
    return gb.check(got, it["g64"][term], it["bar"][term], gb.COEFF[term], f"{label} {case} {'contact' if term == 'con' else 'world'} term")


_CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
from tests.test_gpu_gradient_bars import CASES, isolated_backward
out = {}
for i, case in enumerate(CASES):
    for term in ("con", "ws"):
        for k, v in isolated_backward(case, term)[0].items():
            out["%%d/%%s/%%s" %% (i, term, k)] = v
np.savez(sys.argv[1], **out)
print("RESULT ok")
"""


@pytest.fixture(scope="module")
def exact_fp32(tmp_path_factory):
    """All cases in ONE child process with the exact-fp32 products -> {(case index, term): blocks}"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path_factory.mktemp("exact_fp32") / "grads.npz")
    p = subprocess.run([sys.executable, "-c", _CHILD % root, path], env=dict(os.environ, FDCAP_GEMM_SPLIT3="0"), capture_output=True, text=True,
                       timeout=600, cwd=root)
    assert p.returncode == 0 and "RESULT ok" in p.stdout, p.stderr[-2000:]
    out = {}
    with np.load(path) as z:
        for key in z.files:
            i, term, block = key.split("/")
            out.setdefault((int(i), term), {})[block] = z[key]
    return out


@pytest.mark.parametrize("index", range(len(CASES)), ids=["-".join(map(str, c)) for c in CASES])
def test_isolated_term_gradients_within_their_per_block_bars(index, exact_fp32):
    """n = 12 / V = 300 / 800 points / 2 x 20 contact vertices and the ragged shapes of
    test_optimiser_gradients_match_autograd_at_ragged_shapes (frames no multiple of the 16-row blocks, one contact vertex per
    leg, ...): the isolated contact gradient (rows, d scale) and the isolated world gradient (rows, d camera_ext), both product
    forms, every block within its bar."""
    case = CASES[index]
    bad = {}
    for term in ("con", "ws"):
        got, _ = isolated_backward(case, term, gb.isolated_terms(case))
        for form, blocks in (("fp16 planes", got), ("exact fp32", exact_fp32[(index, term)])):
            b = check_isolated(case, term, blocks, form)
            if b:
                bad[(form, term)] = b
    assert not bad, f"blocks outside their bar {{block: (err / bar, bar, max|g|)}}: {bad}"
