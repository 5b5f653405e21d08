"""Pins the yardstick of the fb_fem_surface tests (tests/surfref.py) without a GPU: the literal restatement of
SurfaceMesh::setupFromTetMesh against the vectorised one, and properties of a boundary surface that use neither."""
import functools

import numpy as np
import pytest

import cut_inputs as ci
import cutref as cr
import surface_inputs as si
import surfref as sr

# Under cut_inputs.smooth_displacement the Delaunay meshes and the disc hold elements that turn inside out relative to their neighbours
# (measured: enclosed volume off by 11 % to 79 % of the elements' on the Delaunay cases and 25 % on the disc, 1e-15 everywhere else), so the
# restatement itself fails the orientation properties there; those cases assert literal == vectorised only.
INVERTING = ("delaunay", "disc")


@functools.lru_cache(maxsize=None)
def _rest_cases():
    return {c[0]: c for c in si.rest_cases()}


def _cut_cases(name):
    """(label, deformed, old node count, vertices, tets) of the case's cuts that were made"""
    _, v, t, _ = _rest_cases()[name]
    out = []
    for label, strip in si.blades(name, v):
        for q in (None, ci.smooth_displacement(v)):
            r = cr.cut(v, t, strip, q=q)
            if r["status"] != 1:
                continue
            x2, t2 = ci.cut_mesh(v if q is None else v + q, t, r)
            out.append((label, q is not None, len(v), x2, t2))
    return out


NAMES = ["cube5", "cube7"] + list(ci.SHIPPED) + ["delaunay%d" % c[0] for c in ci.DELAUNAY_CASES]


def _same(v, t):
    a, at = sr.literal(v, t)
    b, bt = sr.vectorised(v, t)
    assert np.array_equal(a, b) and np.array_equal(at, bt)
    return a, at


def _properties(v, t, faces, n_bodies):
    assert sr.closed_and_oriented(faces)
    vol = sr.element_volume(v, t)
    assert abs(sr.enclosed_volume(v, faces) - vol) <= 1e-12 * vol
    assert sr.euler(faces) == 2 * n_bodies


@pytest.mark.parametrize("name", NAMES)
def test_literal_equals_vectorised_and_properties_at_rest(name):
    _, v, t, _ = _rest_cases()[name]
    faces, face_tets = _same(v, t)
    n_bodies = ci.SHIPPED_BODIES.get(name, 624 if name == "implicit_sphere" else 1)
    assert si.bodies(t) == n_bodies
    _properties(v, t, faces, n_bodies)
    if name == "implicit_sphere":
        assert sr.euler(faces) == 1248
    # every face belongs to the element it names, in that element's winding
    det = sr.determinants(v, t)
    for f, e in zip(faces[:50], face_tets[:50]):
        local = sr.FACES_POS if det[e] >= 0 else sr.FACES_NEG
        assert tuple(f) in [tuple(int(t[e][k]) for k in loc) for loc in local]


@pytest.mark.parametrize("name", NAMES)
def test_after_a_cut(name):
    cases = _cut_cases(name)
    assert len(cases) >= 2, "every mesh is cut at rest and deformed at least once"
    for label, deformed, n_old, x2, t2 in cases:
        faces, _ = _same(x2, t2)
        assert np.isin(np.arange(n_old, len(x2)), sr.vertex_ids(faces)).all(), "every new node lies on the surface"
        if deformed and name.startswith(INVERTING):
            continue
        _properties(x2, t2, faces, si.bodies(t2))


def test_a_face_of_three_elements_keeps_the_third_winding():
    v, t = si.three_on_a_face()
    faces, face_tets = _same(v, t)
    k = [i for i, f in enumerate(faces) if sorted(f) == [0, 1, 2]]
    assert len(k) == 1 and face_tets[k[0]] == 2
    det = sr.determinants(v, t)
    local = sr.FACES_POS if det[2] >= 0 else sr.FACES_NEG
    assert tuple(faces[k[0]]) in [tuple(int(t[2][c]) for c in loc) for loc in local]
    assert len(faces) == 3 * 3 + 1


def test_a_duplicated_element_contributes_nothing():
    v, t = si.duplicated_element()
    faces, face_tets = _same(v, t)
    assert not (face_tets == 7).any()   # (a face it shares with a neighbour occurs three times and is left by the later copy)
    once, _ = sr.vectorised(v, np.delete(t[:-1], 7, axis=0))
    assert np.array_equal(np.sort(np.sort(faces, 1), 0), np.sort(np.sort(once, 1), 0)), "the surface of the mesh without the element"


@pytest.mark.parametrize("n,count", [(5, 192), (7, 432), (56, 36300)])
def test_cube_face_count(n, count):
    v, t = si.cube(n)
    faces, _ = sr.vectorised(v, t)
    assert len(faces) == count == 12 * (n - 1) ** 2


def test_normals_and_box_of_a_cube_at_rest():
    v, t = si.cube(5)
    faces, _ = sr.literal(v, t)
    ids = sr.vertex_ids(faces)
    n, length = sr.normals(v, faces)
    assert length.min() >= 1.7
    lo, hi = v.min(0), v.max(0)
    on = (v[ids] == lo) | (v[ids] == hi)
    inside_face = on.sum(1) == 1          # on one side of the cube only
    k = np.argmax(on[inside_face], axis=1)
    expect = np.zeros((inside_face.sum(), 3))
    expect[np.arange(len(k)), k] = np.where(v[ids][inside_face][np.arange(len(k)), k] == lo[k], -1.0, 1.0)
    assert np.array_equal(n[inside_face], expect)
    box = sr.aabb(np.float32(v[ids]))
    assert np.array_equal(box, np.float32([lo, hi]))
