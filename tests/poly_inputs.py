"""The trees, grids and comparisons of the polygonizer parity tests (tests/test_poly_gpu.py), kept apart so that
tests/test_poly_word_edges.py can check the grid list on the oracle alone, without a GPU.

Every OrcPoly stage after the sweep reads ``OrcPoly.xyzf``.  Handing the oracle the device's own grid therefore makes everything
downstream of the field a bit-exact comparison whatever the field values are: a sample within rounding of the iso value classifies
the same way on both sides, because both sides read the same number."""
import functools

import numpy as np

from fembrain_amd.blobtree import make_tree, sphere_blob
from oracle.pyfield import OrcPoly

from meshchecks import surface_mesh_checks

ISO = np.float32(0.5)
OF_RIGHT_OP, OF_LEFT_OP, OF_RANGE, OF_UNARY = 1, 2, 4, 8


def trees():
    pts = [(0, (0.1 * i - 0.3, 0.05 * i, 0.02 * i * i), (0, 0, 0), (0, 0, 0)) for i in range(6)]
    mixed = [(0, (0, 0, 0), (0, 0, 0), (0, 0, 0)), (1, (-0.5, 0.2, 0), (0.6, 0.3, 0.1), (0, 0, 0)), (5, (0.3, -0.4, 0.2), (0, 0, 0), (0.25, 0, 0)),
             (2, (0, 0, -0.6), (0, 1, 0), (0.2, 0.7, 0)), (3, (0.5, 0.5, 0.5), (0, 0, 1), (0.3, 0, 0)), (4, (-0.5, -0.5, 0.4), (1, 0, 0), (0.3, 0, 0)),
             (7, (0.2, 0.7, -0.3), (1.0, 0.8, 0.64), (1.0 / 0.8 ** 4, -2.0 / 0.64, 1.0))]
    return {
        "sphere": sphere_blob(),
        "blend6_noops": make_tree(pts),
        "range_blend": make_tree(pts, [(4, 0, 5, OF_RANGE, 0, 0)]),
        # op0 = union(op1, op2); op1 = dif(prim0, prim1); op2 = smoothdif(op3, prim2); op3 = range(3..6)
        "nested": make_tree(mixed, [(0, 1, 2, OF_LEFT_OP | OF_RIGHT_OP, 0, 0), (2, 0, 1, 0, 0, 0), (3, 3, 2, OF_LEFT_OP, 0, 0), (4, 3, 6, OF_RANGE, 0, 0)]),
        # two range operators under an intersection: the second range inherits the first one's running field
        "two_ranges": make_tree(pts, [(1, 1, 2, OF_LEFT_OP | OF_RIGHT_OP, 0, 0), (4, 0, 2, OF_RANGE, 0, 0), (4, 3, 5, OF_RANGE, 0, 0)]),
        "ricci": make_tree(pts[:2], [(5, 0, 1, 0, 2.0, 0.5)]),
    }


def sqrt_free(blob):
    """untransformed point primitives under operators that only add, subtract and compare: the trees whose device field the tests demand
    equal to the oracle's bit for bit"""
    plain_ops = blob.n_ops == 0 or bool(np.isin(blob.ops[:, 0], (0, 1, 2, 3, 4)).all())
    return bool((blob.prims[:, 0] == 0).all() and (blob.prims[:, 1] == 0).all()) and plain_ops


# ---- grids at the edges of the 64-point words the classification works on ---------------------------------------------------------------
# fewer than 64 points; a plane below / of exactly one word (the z neighbour in the same / the next word); one, two and "two and a bit" words
# per row; 16|17 words (k_tet_vertices' workgroup), 62|63 (the tet kernels' prefetch run), 256|257 (k_ranks' workgroup), 4096|4097 (the
# surface pass's scan chunk); n_points a multiple of 64 with gx not one
WORD_EDGE_SHAPES = (
    (2, 2, 2), (3, 2, 2), (2, 2, 70), (2, 70, 2), (70, 2, 2), (63, 3, 3), (64, 3, 3), (65, 3, 3), (127, 2, 5), (128, 2, 2), (129, 3, 2),
    (8, 8, 2), (8, 8, 9), (16, 4, 5), (32, 2, 17), (4, 16, 5), (6, 32, 3), (8, 8, 16), (8, 8, 17), (8, 8, 62), (8, 8, 63),
    (64, 16, 16), (63, 17, 16), (64, 16, 17), (64, 64, 64), (65, 64, 64))
PLACEMENTS = {"first": 0.07, "last": 0.93}
# a point inside the body of the tree: the grid corner next to it is inside, the surface leaves the grid through its faces
CENTRES = {"blend6_noops": (-0.05, 0.12, 0.13), "nested": (0.2, 0.7, -0.3)}
NESTED_SHAPES = ((3, 2, 2), (64, 3, 3), (8, 8, 9), (8, 8, 17), (128, 2, 2), (63, 17, 16), (64, 16, 17), (65, 64, 64))
WORD_EDGE_CASES = tuple(("blend6_noops", d, w) for d in WORD_EDGE_SHAPES for w in PLACEMENTS) + \
    tuple(("nested", d, w) for d in NESTED_SHAPES for w in PLACEMENTS)
# (dims, ranks) of the z-slab runs at the same edges
SLAB_CASES = (((8, 8, 17), 2), ((8, 8, 17), 3), ((8, 8, 63), 2), ((8, 8, 63), 3), ((2, 2, 70), 5), ((64, 16, 17), 2))


def case_id(case):
    return "%s-%s-%s" % (case[0], "x".join(str(d) for d in case[1]), case[2])


def place(tree, dims, where):
    """(lower corner fp32, cellsize) of the grid `dims` whose first / last corner lies next to the tree's centre: the longest axis spans 2.2"""
    d = np.asarray(dims, np.float64)
    cell = 2.2 / (d.max() - 1)
    ext = cell * (d - 1)
    return (np.asarray(CENTRES[tree], np.float64) - PLACEMENTS[where] * ext).astype(np.float32), float(cell)


@functools.lru_cache(maxsize=None)
def oracle_case(tree, dims, where):
    """the oracle's own sweep of a word-edge case, computed once per process and read-only: (blob, lower, cellsize, xyzf)"""
    blob = trees()[tree]
    lower, cell = place(tree, dims, where)
    xyzf = OrcPoly(blob).sweep_grid(lower, cell, dims)
    xyzf.setflags(write=False)
    lower.setflags(write=False)
    return blob, lower, cell, xyzf


def oracle_on_grid(blob, lower, cellsize, dims, xyzf):
    o = OrcPoly(blob)
    o.lo, o.g, o.cellsize = np.asarray(lower, np.float32), np.asarray(dims, np.int32), cellsize
    o.xyzf = np.ascontiguousarray(xyzf, np.float32)
    return o


def oracle_on_device_grid(blob, g, own=None):
    """An OrcPoly whose grid is the one the device swept (``g``: a GpuPoly after sweep / sweep_grid), after holding that grid against the
    oracle's own sweep `own` (computed here when not given): positions bit for bit, field values to 2e-6 and bit for bit for sqrt-free trees."""
    grid = g.read_grid()
    if own is None:
        own = OrcPoly(blob).sweep_grid(g.lower, g.cellsize, g.dims)
    assert grid.shape == own.shape
    assert np.array_equal(grid[:, :3], own[:, :3])
    if sqrt_free(blob):
        assert np.array_equal(grid[:, 3], own[:, 3])
    else:
        assert np.abs(grid[:, 3] - own[:, 3]).max() <= 2e-6
    return oracle_on_grid(blob, g.lower, g.cellsize, g.dims, grid)


def run_pipeline(g):
    """classify -> tetrahedralize -> surface on a swept GpuPoly"""
    g.classify()
    g.tetrahedralize()
    return g.surface()


def normals_tol(blob, exact_field=True):
    """1e-6 where the field at the surface vertices is the oracle's bit for bit; an ulp of difference in a sqrt / pow primitive is amplified 1e4-fold
    by the forward difference over delta = 1e-4, so those trees are held to 2e-2"""
    return 1e-6 if exact_field and sqrt_free(blob) else 2e-2


def assert_pipeline_equals(g, o, normals_tol, mesh_checks=None):
    """Everything a GpuPoly that ran classify, tetrahedralize and surface holds, against the oracle `o` on the same grid samples: bit for bit but
    for the normals.  mesh_checks: keyword arguments of meshchecks.surface_mesh_checks, None = do not run it.  Returns the device's outputs."""
    oc = o.classify()
    c = g.counts
    flags, cnt, cfg = g.read_classification()
    assert (c.n_points, c.n_cells) == (len(o.xyzf), len(o.config))
    assert np.array_equal(flags, o.edge_flags) and np.array_equal(cnt, o.edge_count) and np.array_equal(cfg, o.config)
    counts = (c.n_crossed_edges, c.n_surface_cells, c.n_included_cells, c.n_tet_vertices)
    assert counts == (oc["n_crossed_edges"], oc["n_surface_cells"], oc["n_included_cells"], oc["n_tet_vertices"])
    xyz, tets = g.read_tetmesh()
    oxyz, otets = o.tetrahedralize()
    assert c.n_tets == len(otets)
    assert np.array_equal(tets, otets) and np.array_equal(xyz, oxyz)
    sx, sn, st = g.read_surface()
    ox, on, ot = o.surface()
    assert c.n_surface_vertices == len(ox) == c.n_crossed_edges and c.n_surface_indices == 3 * len(ot)
    assert np.array_equal(st, ot) and np.array_equal(sx, ox)
    # a vertex where the field is flat has no normal on either side (0 / 0); everywhere else the two agree
    assert np.array_equal(np.isnan(sn), np.isnan(on))
    if len(sn):
        assert np.nan_to_num(np.abs(sn - on)).max() <= normals_tol
    pairs, w = g.read_surface_binding()
    opairs, ow = o.surface_binding()
    assert np.array_equal(pairs, opairs) and np.array_equal(w, ow)
    if mesh_checks is not None:
        surface_mesh_checks(sx, sn, st, **mesh_checks)
    return flags, cnt, cfg, xyz, tets, sx, sn, st, pairs, w, counts


def assert_runs_identical(a, b):
    """two returns of assert_pipeline_equals, bit for bit (a normal that does not exist compares equal to one that does not exist)"""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)


def unclamped_flags(inside, dims):
    """crossed-edge bits of a classifier that forgets the last-plane masks: inside[p] ^ inside[p + step], the neighbour read past the row /
    plane / grid end as the bit array holds it (zero past the end).  Returns (x, y, z) bit arrays."""
    gx, gy, _ = dims
    out = []
    for step in (1, gx, gx * gy):
        nb = np.zeros_like(inside)
        nb[:-step] = inside[step:]
        out.append(inside ^ nb)
    return out
