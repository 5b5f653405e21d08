"""The meshes of the fb_fem_surface tests: what tests/test_fem_surface_ref.py pins the restatement (tests/surfref.py) on without a GPU and
tests/test_fem_surface_gpu.py runs the device on."""
import numpy as np

from fembrain_amd import meshgen

import cut_inputs as ci
import cutref as cr


def cube(n):
    v, t = meshgen.truth_cube(n, n, n)[:2]
    return np.asarray(v, np.float64).reshape(-1, 3), np.ascontiguousarray(np.asarray(t).reshape(-1, 4), np.int32)


def cube_fixed(v):
    """the DOFs of the x = min face"""
    fv = np.nonzero(v[:, 0] == v[:, 0].min())[0]
    return (3 * fv[:, None] + np.arange(3)[None, :]).reshape(-1).astype(np.int32)


def cube_blade(v):
    """a plane near the middle of a cube that passes through no node"""
    return cr.plane_strip(v.mean(0) + [0.013, 0.007, 0.003], (1.0, 0.21, 0.13))


def rest_cases(cubes=(5, 7)):
    """(name, vertices, tets, fixed DOFs) of every uncut mesh: cubes, the shipped meshes, the Delaunay cases"""
    out = []
    for n in cubes:
        v, t = cube(n)
        out.append(("cube%d" % n, v, t, cube_fixed(v)))
    for name in ci.SHIPPED:
        v, t, fd = ci.shipped(name)
        out.append((name, v, t, fd))
    for (n, seed, _, _) in ci.DELAUNAY_CASES:
        v, t, fd = ci.delaunay(n, seed)
        out.append(("delaunay%d" % n, v, t, fd))
    return out


def blades(name, v):
    """the blades a case is cut with: (label, strip)"""
    if name.startswith("cube"):
        return [("mid", cube_blade(v))]
    if name.startswith("delaunay"):
        n = int(name[len("delaunay"):])
        (_, _, ps, k), = [c for c in ci.DELAUNAY_CASES if c[0] == n]
        return [("p%d" % i, s) for i, (_, _, s) in enumerate(ci.random_planes(ps, k))]
    return [("p%d" % i, s) for i, (_, _, s) in enumerate(ci.shipped_planes(name, v, 2))]


def is_delaunay(name):
    return name.startswith("delaunay")


def bodies(tets):
    return len(np.unique(cr.face_components(tets)))


def three_on_a_face():
    """three elements on the face (0, 1, 2): it survives with the third's winding.  Apices 3, 4 above, 5 below."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.2, 0.2, 1.0], [0.3, 0.3, 0.6], [0.2, 0.2, -1.0]], np.float64)
    t = np.array([[0, 1, 2, 3], [0, 1, 2, 4], [2, 1, 0, 5]], np.int32)
    return v, t


def duplicated_element():
    """a cube 3^3 whose element 7 is listed twice: the pair contributes nothing, so its neighbours' faces towards it surface"""
    v, t = cube(3)
    return v, np.ascontiguousarray(np.concatenate([t, t[7:8]]), np.int32)
