"""The vocabulary entry points exist at every layer (header, library, binding,
Python mirror) and their argument checks answer on the host: every malformed
vocabulary is refused before a device is looked for, so these cases give the
same codes on a machine without a GPU. A context cannot exist without a device;
the transform and score calls carry a NULL context here and
tests/test_gpu_bow.py repeats their checks on a live one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sqrtlm import _lib, orb, orb_scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sqlm_voc_create", "sqlm_voc_destroy", "sqlm_voc_info", "sqlm_bow_transform", "sqlm_bow_score"]
INVALID, UNSUPPORTED = -1, -8


def test_header_binding_and_library_carry_the_names():
    hdr = open(os.path.join(ROOT, "include", "sqrtlm_orb.h")).read()
    declared = set(re.findall(r"\b(sqlm_[A-Za-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for n in NAMES:
        assert n in declared and n in _lib.ORB_EXPORTS and hasattr(L, n), n
    assert declared == set(_lib.ORB_EXPORTS)
    assert "typedef struct sqlm_voc sqlm_voc;" in hdr
    assert "uninitialised" in hdr  # the early-leaf node is this library's choice, and the header says so


def test_signatures_are_bound():
    L = _lib.lib()
    assert len(L.sqlm_voc_create.argtypes) == 11 and L.sqlm_voc_create.argtypes[5] is C.c_int32
    assert len(L.sqlm_voc_destroy.argtypes) == 1 and len(L.sqlm_voc_info.argtypes) == 2
    assert len(L.sqlm_bow_transform.argtypes) == 11
    assert len(L.sqlm_bow_score.argtypes) == 10 and L.sqlm_bow_score.argtypes[1] is C.c_int64


def _create(v, **over):
    a = dict(v, scoring=0, weighting=0, n_nodes=len(v["parent"]))
    a.update(over)
    p = _lib.ptr
    h = C.c_void_p()
    r = _lib.lib().sqlm_voc_create(0, a["k"], a["L"], a["scoring"], a["weighting"], a["n_nodes"], p(a["parent"]),
                                   p(a["is_word"]), p(a["desc"]), p(a["weight"]), C.byref(h))
    if r == 0:  # a machine with a device: the sound vocabulary was built
        _lib.lib().sqlm_voc_destroy(h)
    else:
        assert not h.value
    return r


@pytest.fixture(scope="module")
def voc():
    return S.make_vocabulary(3, 2, seed=4)  # 1 + 3 + 9 nodes, pre-order: node 1's children are 2, 3, 4


def _edit(v, name, index, value):
    a = v[name].copy()
    a[index] = value
    return {name: a}


def test_a_sound_vocabulary_passes_the_host_checks(voc):
    # without a device the call gets as far as looking for one: NO_DEVICE (-6) or a HIP error (-2)
    assert _create(voc) in (0, -6, -2)


@pytest.mark.parametrize("k", [0, -1, 21])
def test_k_outside_the_loaders_limits(voc, k):
    assert _create(voc, k=k) == INVALID


@pytest.mark.parametrize("L", [0, -3, 11])
def test_L_outside_the_loaders_limits(voc, L):
    assert _create(voc, L=L) == INVALID


def test_structure_errors(voc):
    assert voc["parent"].tolist()[:6] == [0, 0, 1, 1, 1, 0]
    assert _create(voc, **_edit(voc, "parent", 2, 2)) == INVALID    # parent[i] == i
    assert _create(voc, **_edit(voc, "parent", 2, 7)) == INVALID    # parent[i] > i
    assert _create(voc, **_edit(voc, "parent", 2, -1)) == INVALID   # no parent at all
    assert _create(voc, **_edit(voc, "parent", 5, 1)) == INVALID    # node 1 gets a fourth child, k = 3
    assert _create(voc, k=2) == INVALID                              # the same tree under k = 2
    assert _create(voc, **_edit(voc, "is_word", 1, 1)) == INVALID   # a word with children
    assert _create(voc, **_edit(voc, "is_word", 0, 1)) == INVALID   # the root as a word
    assert _create(voc, **_edit(voc, "is_word", 2, 0)) == INVALID   # a childless node that is no word
    assert _create(voc, n_nodes=1) == INVALID and _create(voc, n_nodes=0) == INVALID
    assert _create(voc, n_nodes=2) == INVALID                        # the cut leaves node 1 childless and no word
    for name in ("parent", "is_word", "desc", "weight"):
        assert _create(voc, **{name: None}) == INVALID, name
    L = _lib.lib()
    p = _lib.ptr
    assert L.sqlm_voc_create(0, 3, 2, 0, 0, 13, p(voc["parent"]), p(voc["is_word"]), p(voc["desc"]), p(voc["weight"]),
                             None) == INVALID


@pytest.mark.parametrize("scoring,weighting", [(1, 0), (0, 1), (5, 3), (2, 2)])
def test_other_scoring_and_weighting_are_unsupported(voc, scoring, weighting):
    assert _create(voc, scoring=scoring, weighting=weighting) == UNSUPPORTED


def test_null_handles():
    L = _lib.lib()
    p = _lib.ptr
    out = np.zeros(8, np.int32)
    assert L.sqlm_voc_destroy(None) == INVALID
    assert L.sqlm_voc_info(None, p(out)) == INVALID and not out.any()
    off = np.array([0, 2], np.int64)
    d = np.zeros((2, 32), np.uint8)
    i32 = np.zeros(4, np.int32)
    f64 = np.zeros(4)
    # no context and no vocabulary, otherwise well-formed
    assert L.sqlm_bow_transform(None, None, 1, p(off), p(d), 4, p(i32), p(i32), p(off.copy()), p(i32), p(f64)) == INVALID
    assert L.sqlm_bow_transform(None, None, 0, p(off), None, 4, None, None, p(off.copy()), None, None) == INVALID
    w = np.array([1, 5], np.int32)
    assert L.sqlm_bow_score(None, 2, p(w), p(f64), 1, p(off), p(w), p(f64), p(f64.copy()), p(i32)) == INVALID
    assert L.sqlm_bow_score(None, 0, None, None, 0, p(off), None, None, None, None) == INVALID
    # and beside each malformed argument
    down = np.array([5, 1], np.int32)
    for bad in ((2, down, 1, off, w), (2, w, 1, off, down), (2, w, 1, np.array([0, -1], np.int64), w),
                (-1, w, 1, off, w), (2, w, -1, off, w), (2, w, 1, None, w), (2, None, 1, off, w)):
        nq, qw, n_db, o, dw = bad
        assert L.sqlm_bow_score(None, nq, p(qw), p(f64), n_db, p(o), p(dw), p(f64), p(f64.copy()), p(i32)) == INVALID


def test_python_mirror():
    for fn in (orb.ORBVocabulary.load_text, orb.ORBVocabulary.save_text, orb.ORBVocabulary.transform,
               orb.ORBVocabulary.transform_many, orb.ORBVocabulary.score, orb.ORBVocabulary.score_many,
               orb.load_vocabulary_text, orb.save_vocabulary_text, S.make_vocabulary):
        assert callable(fn)
    v = S.make_vocabulary(2, 2, seed=1)
    assert set(v) == {"k", "L", "parent", "is_word", "desc", "weight"}
    assert v["parent"].dtype == np.int32 and v["is_word"].dtype == np.uint8 and v["weight"].dtype == np.float64
    assert v["desc"].dtype == np.uint8 and v["desc"].shape == (7, 32)
    host = orb.ORBVocabulary(**v, upload=False)
    assert not host._h and host.k == 2 and host.L == 2
    with pytest.raises(ValueError):
        orb.ORBVocabulary(2, 2, v["parent"], v["is_word"][:-1], v["desc"], v["weight"], upload=False)
    # a malformed vocabulary is refused by the library, not by Python, and by its status
    bad = dict(v, is_word=np.zeros(7, np.uint8))
    with pytest.raises(_lib.SqlmError) as e:
        orb.ORBVocabulary(**bad)
    assert e.value.status == INVALID
