"""The product's OBJ importer (host/ObjLoader.cpp) and the oracle's (oracle/orc_obj.h) against the REFERENCE's own importer,
XUSG::ObjLoader.  This is the one row of the hot path where the reference's code itself can be run: vertex and
index arrays are compared bit for bit -- on the three meshes the reference ships (Bin/Assets, regenerated from
tests/golden/assets/) and on generated files covering every face syntax the importer parses.

The reference's answers are recorded under tests/golden/ (obj_import.json: SHA-256 of the raw arrays of the shipped meshes;
obj_import_generated.npz: the whole output for every generated file), written by tests/golden/make_obj_golden.py with the
reference's importer built into oracle/_ref/libobjloader_ref.so (oracle/Makefile target `ref`).  Both importers are checked
against the recorded answers everywhere; where that library has been built, they are also compared with it directly, and the
recorded answers with what it says today."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import assets
from oracle import oracle as O
from oracle import ref_obj

HERE = os.path.dirname(os.path.abspath(__file__))

SYNTAXES = ["v", "v/vt", "v//vn", "v/vt/vn"]
GENERATED_FILES = 12         # files per case of test_generated_files_import_like_the_reference


@functools.lru_cache(maxsize=None)
def _known_shipped():
    with open(os.path.join(HERE, "golden", "obj_import.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def _known_generated():
    with np.load(os.path.join(HERE, "golden", "obj_import_generated.npz")) as z:
        return {k: z[k] for k in z.files}


def _digests(a):
    """SHA-256 of the raw vertex, index and AABB arrays, as make_obj_golden.py records them for the reference's output."""
    return (hashlib.sha256(np.ascontiguousarray(a[0]).view(np.uint32).tobytes()).hexdigest(),
            hashlib.sha256(np.ascontiguousarray(a[1], np.uint32).tobytes()).hexdigest(),
            hashlib.sha256(np.ascontiguousarray(a[2]).view(np.uint32).tobytes()).hexdigest())


def _same(a, b, what):
    np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32), err_msg=what + ": vertices")
    np.testing.assert_array_equal(a[1], b[1], err_msg=what + ": indices")
    np.testing.assert_array_equal(a[2].view(np.uint32), b[2].view(np.uint32), err_msg=what + ": AABB")


@pytest.mark.parametrize("name", ["bunny", "dragon", "TuringBowl"])
def test_shipped_meshes_import_like_the_reference(built, name):
    """bunny / dragon: no normals in the file (face-normal synthesis, XUSGObjLoader.cpp:337-384); TuringBowl: v//vn faces with
    per-corner normals and vertex splitting (:300-335; Bin/TuringBowl.bat)."""
    from raytracedggx_amd import app
    path = assets.path(name + ".obj")
    f = _known_shipped()[name]
    known = (f["sha256_verts"], f["sha256_indices"], f["sha256_aabb"])
    got = {"product": app.obj_import(path), "oracle": O.obj_import(path)}
    if ref_obj.available():
        ref = ref_obj.obj_import(path)
        for who, a in got.items():
            _same(a, ref, who + " " + name)
        # and the committed known answers are what the reference's importer says today (tests/golden/make_obj_golden.py)
        assert ref[0].shape == (f["num_verts"], 6) and ref[1].size == f["num_indices"]
        assert "%08x" % assets.fnv1a32(ref[0].tobytes()) == f["fnv_verts"] and "%08x" % assets.fnv1a32(ref[1].tobytes()) == f["fnv_indices"]
        assert _digests(ref) == known, "%s: the reference's importer no longer gives the recorded answer" % name
    for who, a in got.items():
        assert a[0].shape == (f["num_verts"], 6) and a[1].size == f["num_indices"], "%s %s: array sizes" % (who, name)
        assert "%08x" % assets.fnv1a32(a[0].tobytes()) == f["fnv_verts"] and "%08x" % assets.fnv1a32(a[1].tobytes()) == f["fnv_indices"], \
            "%s %s: FNV-1a of the arrays" % (who, name)
        assert _digests(a) == known, "%s %s: vertices, indices or AABB differ from the reference's (SHA-256 of the raw arrays)" % (who, name)


def _generated_obj(rng, syntax, polygons, negative):
    """A random mesh as OBJ text: `syntax` in {"v", "v/vt", "v//vn", "v/vt/vn"}; faces are triangles, or polygons of 3-6
    corners (fan triangulation, :267-297); indices 1-based or negative (relative, :243)."""
    nv, nn, nt = int(rng.integers(6, 40)), int(rng.integers(1, 12)), int(rng.integers(1, 9))
    lines = ["# generated", "o thing"]
    lines += ["v %.6f %.6f %.6f" % tuple(rng.uniform(-5, 5, 3)) for _ in range(nv)]
    if "vt" in syntax:
        lines += ["vt %.4f %.4f" % tuple(rng.uniform(0, 1, 2)) for _ in range(nt)]
    if "vn" in syntax:
        for _ in range(nn):
            n = rng.standard_normal(3)
            lines.append("vn %.6f %.6f %.6f" % tuple(n / np.linalg.norm(n) * rng.uniform(0.5, 2.0)))
    lines.append("s 1")
    for _ in range(int(rng.integers(1, 30))):
        k = int(rng.integers(3, 7)) if polygons else 3
        corners = []
        for c in rng.choice(nv, k, replace=False):
            v = int(c) - nv if negative else int(c) + 1
            t = int(rng.integers(0, nt)); t = t - nt if negative else t + 1
            n = int(rng.integers(0, nn)); n = n - nn if negative else n + 1
            corners.append({"v": "%d" % v, "v/vt": "%d/%d" % (v, t), "v//vn": "%d//%d" % (v, n), "v/vt/vn": "%d/%d/%d" % (v, t, n)}[syntax])
        lines.append("f " + " ".join(corners))
    return "\n".join(lines) + "\n"


def generated_cases():
    """(case, rng, syntax, polygons, negative) for every case of the test below, each with its own freshly seeded generator."""
    for syntax in SYNTAXES:
        for polygons in (False, True):
            for negative in (False, True):
                case = SYNTAXES.index(syntax) * 4 + polygons * 2 + negative
                yield case, np.random.default_rng(case), syntax, polygons, negative


def generated_key(case, k):
    return "c%02d_f%02d" % (case, k)


@pytest.mark.parametrize("syntax", SYNTAXES)
@pytest.mark.parametrize("polygons", [False, True], ids=["triangles", "polygons"])
@pytest.mark.parametrize("negative", [False, True], ids=["absolute", "relative"])
def test_generated_files_import_like_the_reference(built, tmp_path, syntax, polygons, negative):
    from raytracedggx_amd import app
    case, rng = next((c, r) for c, r, s, p, n in generated_cases() if (s, p, n) == (syntax, polygons, negative))
    known = _known_generated()
    for k in range(GENERATED_FILES):
        p = tmp_path / ("g%d.obj" % k)
        text = _generated_obj(rng, syntax, polygons, negative)
        p.write_text(text)
        key = generated_key(case, k)
        assert hashlib.sha256(text.encode()).digest() == known[key + "_text_sha256"].tobytes(), \
            "%s #%d: the generator no longer writes the file the reference's answer was recorded for" % (syntax, k)
        rec = (known[key + "_v"], known[key + "_i"], known[key + "_aabb"])
        assert rec[1].size >= 3
        if ref_obj.available():
            _same(ref_obj.obj_import(str(p)), rec, "reference today vs recorded, %s #%d" % (syntax, k))
        _same(app.obj_import(str(p)), rec, "product %s #%d" % (syntax, k))
        _same(O.obj_import(str(p)), rec, "oracle %s #%d" % (syntax, k))
