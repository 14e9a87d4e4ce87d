"""The query order's sort (csrc/fdc_scene.h nn_query_order: keys + histogram, row prefixes, scatter, row prefixes, scatter) through
fdcap_debug_nn_query_sort, which runs it on neighbour positions given by the caller and returns the permutation and the headers.

The order is fully specified -- stable, by the 16-bit key min(pos >> 7, 0xFFFF) (0xFFFF without a neighbour), ties by query index --
so the reference is numpy's stable argsort and the comparison is exact.  Sizes: a single ragged block (1, 12, 255), the tile and the
tile + 1 for both tile sizes the kernels have been built with (2048, 4096), several ragged tiles (20 012) and 300 001, which has
more than 64 tiles per digit row, so that the row kernel carries its total from one 64-counter step to the next.  The rebuild
resets hdr[0 .. groups) to -1 and must leave what lies behind untouched."""
import ctypes

import numpy as np
import pytest

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, synth

SIZES = (1, 12, 255, 2048, 2049, 4096, 4097, 20012, 300001)
PATTERNS = ("uniform", "all_equal", "descending", "missing_5pct", "clamped", "low_byte", "high_byte")
TAIL = 37                                             # header entries behind the groups


def _positions(pattern, nq):
    rng = np.random.default_rng(1000 * PATTERNS.index(pattern) + nq % 997)
    if pattern == "uniform":                          # quarters 0 .. 3906: both digits populated
        pos = rng.integers(0, 500000, nq)
    elif pattern == "all_equal":                      # stability alone: the identity
        pos = np.full(nq, 123456)
    elif pattern == "descending":                     # quarters descend (strictly up to 65 536 queries, then in runs of equal length)
        step = (nq + 65535) // 65536
        pos = ((nq - 1 - np.arange(nq)) // step) << 7
    elif pattern == "missing_5pct":                   # -1 lands last, in index order
        pos = rng.integers(0, 500000, nq)
        pos[rng.random(nq) < 0.05] = -1
    elif pattern == "clamped":                        # quarters up to 131 071: those from 0xFFFF on clamp and tie with the -1 sentinel
        pos = rng.integers(0, 1 << 24, nq)
        pos[rng.random(nq) < 0.02] = -1
    elif pattern == "low_byte":                       # pass 0 does all the work
        pos = (rng.integers(0, 256, nq) << 7) + rng.integers(0, 128, nq)
    else:                                             # high_byte: pass 1 does all the work
        pos = (rng.integers(0, 256, nq) << 15) + rng.integers(0, 128, nq)
    return np.ascontiguousarray(pos, dtype=np.int32)


def _reference(pos):
    key = np.where(pos >= 0, np.minimum(pos >> 7, 0xFFFF), 0xFFFF)
    return key, np.argsort(key, kind="stable").astype(np.int32)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("nq", SIZES)
def test_reference_has_the_properties_the_patterns_are_for(nq, pattern):
    pos = _positions(pattern, nq)
    key, ref = _reference(pos)
    assert np.array_equal(np.sort(ref), np.arange(nq))
    sk = key[ref]
    assert (np.diff(sk) >= 0).all() and (np.diff(ref)[np.diff(sk) == 0] > 0).all()
    if pattern == "all_equal":
        assert np.array_equal(ref, np.arange(nq))
    if pattern == "descending" and nq > 1:
        assert key[0] == key.max() and key[-1] == 0 and (np.diff(key) <= 0).all() and (nq > 65536 or (np.diff(key) < 0).all())
    if pattern in ("missing_5pct", "clamped"):
        last = np.flatnonzero(key == 0xFFFF)
        assert np.array_equal(ref[nq - len(last):], last)
        if nq >= 255:
            assert (pos < 0).any()
        if pattern == "clamped" and nq >= 255:
            assert ((pos >> 7) > 0xFFFF).any()
    if pattern == "low_byte":
        assert key.max() < 256
    if pattern == "high_byte":
        assert not (key & 255).any()
    if pattern == "uniform" and nq >= 4096:
        assert len(np.unique(key & 255)) == 256 and len(np.unique(key >> 8)) > 8


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(synth.make_body_model(400, seed=0), synth.make_vposer(seed=1))
    yield c
    c.close()


def _sort(ctx, pos, groups, hdr):
    perm = np.full(len(pos), -7, np.int32)
    code = ctx.lib.fdcap_debug_nn_query_sort(ctx.handle, pos.ctypes.data_as(ctypes.c_void_p), len(pos), groups, len(hdr),
                                             hdr.ctypes.data_as(ctypes.c_void_p), perm.ctypes.data_as(ctypes.c_void_p), None)
    return code, perm


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("nq", SIZES)
def test_sort_gives_the_stable_order_and_resets_the_group_headers(ctx, nq, pattern):
    pos = _positions(pattern, nq)
    _, ref = _reference(pos)
    groups = (nq + 31) // 32
    fill = (7 * np.arange(groups + TAIL) + 3).astype(np.int32)
    hdr = fill.copy()
    code, perm = _sort(ctx, pos, groups, hdr)
    capi.check(code, "fdcap_debug_nn_query_sort")
    bad = np.flatnonzero(perm != ref)
    assert not len(bad), f"{len(bad)} of {nq} slots differ, first at slot {bad[0]}: {perm[bad[0]]} for {ref[bad[0]]}"
    assert (hdr[:groups] == -1).all()
    assert np.array_equal(hdr[groups:], fill[groups:])


@pytest.mark.gpu
def test_sort_with_no_header_room_behind_the_groups_and_repeated(ctx):
    """hdr_len == groups, and the same call twice: the counters the first scatter adds into are zeroed by every rebuild."""
    nq = 20012
    pos = _positions("uniform", nq)
    _, ref = _reference(pos)
    groups = (nq + 31) // 32
    for _ in range(2):
        hdr = np.arange(groups, dtype=np.int32)
        code, perm = _sort(ctx, pos, groups, hdr)
        capi.check(code, "fdcap_debug_nn_query_sort")
        assert np.array_equal(perm, ref) and (hdr == -1).all()


@pytest.mark.gpu
def test_sort_refuses_bad_calls(ctx):
    pos = np.zeros(64, np.int32)
    hdr = np.zeros(2, np.int32)
    perm = np.zeros(64, np.int32)
    p, h, q = (a.ctypes.data_as(ctypes.c_void_p) for a in (pos, hdr, perm))
    f = ctx.lib.fdcap_debug_nn_query_sort
    assert f(ctx.handle, p, 0, 0, 2, h, q, None) == -1                 # FDCAP_E_ARG: nothing to sort
    assert f(ctx.handle, p, 64, 3, 2, h, q, None) == -1                # fewer headers than groups
    assert f(ctx.handle, None, 64, 2, 2, h, q, None) == -1
    assert f(ctx.handle, p, 64, 2, 2, None, q, None) == -1
    assert f(ctx.handle, p, 64, 2, 2, h, None, None) == -1
    assert f(None, p, 64, 2, 2, h, q, None) == -1
    assert not hdr.any() and not perm.any()
