"""tests/forms_table.json (what csrc/fdc_forms.h must select, pinned on the CPU by tests/test_forms_cpu.py) against the device: after a
one-iteration fit, fdcap_debug_kernel_forms lists exactly the forms the table gives for the fit's sizes -- the contact forward (and
the blend product's own launch where the two are not fused), the blend product's data gradient, the contact set's skinning backward
and the in-loop search."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, synth
from fdcap_amd.fitting import FittingOP
from fdcap_amd.io import read_camerapose

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, NS = 10475, 20_000

with open(os.path.join(ROOT, "tests", "forms_table.json")) as _f:
    _TABLE = json.load(_f)["settings"]["default"]


def _form(key, rows):
    (run,) = [r for r in _TABLE[key] if r[0] <= rows <= r[1]]
    return re.split(r" (?=[A-Za-z_]+=)", run[2])[0][len("form="):]          # (the first field; a form's name may hold blanks)


def expected_forms(rows, nv, ja_hi):
    """The names the table gives for a fit of `rows` frames with nv contact vertices (4 weights each, reaching ja_hi joints) against
    the 20 k-point scene."""
    contact = _form(f"cfwd nv={nv} wpv=4 ja={37 if ja_hi <= 37 else 38}", rows)
    names = {contact, _form(f"bwd nv={nv} may_split=1", rows), _form(f"skin nv={nv} wpv=4", rows), _form(f"nn nv={nv} ns={NS}", rows)}
    if contact == "skin_fwd_kernel":
        names.add(_form(f"pfwd nv={nv}", rows))          # two launches: the blend product has its own
    return names


@pytest.fixture(scope="module")
def model():
    bm = synth.make_body_model(V, seed=0)
    left, right = synth.make_contact_ids(bm.v_template, per_part=250, seed=4)
    return bm, synth.make_vposer(seed=1), synth.make_scene(NS, seed=2), np.concatenate([left, right])


def _fit_forms(model, rows, vid):
    bm, vp, scene, _ = model
    clip = synth.make_clip(rows, seed=3)
    lib = capi.load_library()
    buf = ctypes.create_string_buffer(4096)
    lib.fdcap_debug_kernel_forms(buf, 4096, 1)          # (reset)
    fop = FittingOP({"num_iter": 1}, {}, rows, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid,
                    camera_ext=read_camerapose(clip.camerapose_lines))
    fop.fitting(torch.tensor(clip.body_params).cuda(), "global")
    torch.cuda.synchronize()
    lib.fdcap_debug_kernel_forms(buf, 4096, 0)
    fop.close()
    ja_hi = 1 + int(np.nonzero(np.asarray(bm.lbs_weights)[vid].any(axis=0))[0].max())
    return set(buf.value.decode().split(";")), ja_hi


@pytest.mark.parametrize("rows", [128, 160, 256, 257, 300, 335, 336, 384, 1024])
def test_a_fit_launches_the_forms_the_table_gives(model, rows):
    got, ja_hi = _fit_forms(model, rows, model[3])
    want = expected_forms(rows, 500, ja_hi)
    print(rows, "rows: launched", sorted(got), "| table", sorted(want), "| joints", ja_hi)
    assert got == want


def test_an_all_vertices_fit_launches_the_forms_the_table_gives(model):
    got, ja_hi = _fit_forms(model, 64, np.arange(V))
    want = expected_forms(64, V, ja_hi)
    print("64 rows, all vertices: launched", sorted(got), "| table", sorted(want))
    assert got == want
