#!/usr/bin/env python3
"""Same decisions, same bits: what the polygonizer of a library compiles, computes and refuses on the fixture models and a few seeded inputs.

    python tools/same_decisions_poly.py TREE OUT.json      one process per tree: imports fembrain_amd (and tests/poly_inputs.py) from TREE
    python tools/same_decisions_poly.py --compare A.json B.json [TABLE.txt]

Per model (tests/golden/blob/*.blob and the trees of tests/poly_inputs.py) and per field semantics: the steps and slots of
fb_poly_compile_info (default semantics), and under every semantics the handle accepts the sha256 of fb_poly_field_array at 4,096 seeded
points, of the grid, the classification arrays, the counts, the tet mesh, the surface (positions, normals, indices, binding),
fb_poly_off_surface, both displacement entry points and the three slab pieces of a world of 3, on a grid of (64, 19, 23) points
(k_classify<true>) and one of (37, 21, 18) (k_classify<false>); under the default semantics also the two colour entry points.  A refusal
is recorded as its return code and the text of fb_last_error.  The order and argument checks of tests/test_poly_gpu.py
(test_poly_error_paths_and_order, test_slab_argument_checks) and a handle switched CPU -> OPENCL -> CPU_BOX -> CPU are cases of their own."""
import glob
import hashlib
import json
import os
import sys

GRIDS = ((64, 19, 23), (37, 21, 18))
SEMANTICS = (("cpu", 0), ("cpu_box", 1), ("opencl", 2))


def sha(*arrays):
    import numpy as np
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def refusal(e):
    return "refused %d: %s" % (e.code, str(e).split(": ", 1)[1])


def attempt(fn):
    """fn()'s value, or the refusal as the table shows it"""
    from fembrain_amd import lib as fl
    try:
        return fn()
    except fl.FbError as e:
        return refusal(e)


def grid_for(blob, dims):
    """a grid of `dims` points around the model's box, a cell beyond it on every side"""
    import numpy as np
    lo, hi = np.asarray(blob.bbox[0], np.float64)[:3], np.asarray(blob.bbox[1], np.float64)[:3]
    cell = float(max((hi - lo) / (np.array(dims) - 3)))
    return (lo - cell).astype(np.float32), cell


def counts_row(c):
    return [int(x) for x in (c.n_points, c.n_cells, c.n_crossed_edges, c.n_surface_cells, c.n_included_cells, c.n_tet_vertices, c.n_tets, c.n_surface_vertices,
                             c.n_surface_indices)]


def on_grid(g, blob, dims, colours):
    import numpy as np
    from fembrain_amd.poly import MESH_SURFACE, MESH_TET
    lower, cell = grid_for(blob, dims)
    out = {}
    g.sweep_grid(lower, cell, dims)
    out["grid"] = sha(g.read_grid())
    g.classify()
    out["classification"] = sha(*g.read_classification())
    g.tetrahedralize()
    xyz, tets = g.read_tetmesh()
    out["tetmesh"] = sha(xyz, tets)
    c = g.surface()
    out["counts"] = counts_row(c)
    sx, sn, st = g.read_surface()
    out["surface"], out["normals"], out["indices"], out["binding"] = sha(sx), sha(sn), sha(st), sha(*g.read_surface_binding())
    if colours:
        out["surface_colors"] = attempt(lambda: sha(g.read_surface_colors()))
    out["off_surface"] = attempt(lambda: sha(g.compute_off_surface_points_and_fields(0.01)))
    rng = np.random.default_rng(11)
    u_tet, u_surf = rng.normal(size=3 * len(xyz)) * 0.01, rng.normal(size=3 * len(sx)) * 0.01
    out["displaced_tet"] = attempt(lambda: sha(g.apply_fem_displacements(u_tet, MESH_TET)))
    out["displaced_surface"] = attempt(lambda: sha(g.apply_fem_displacements(u_surf, MESH_SURFACE)))
    out["interpolated"] = attempt(lambda: sha(g.interpolate_displacements(u_tet)))
    pieces, sizes = [], []
    for rank in range(3):
        piece = attempt(lambda: g.run_tetrahedralizer_slab(lower, cell, dims, rank, 3, lambda nv: (sizes.append(nv), list(sizes))[1]))
        pieces.append(piece if isinstance(piece, str) else sha(*piece))
    out["slabs"] = pieces
    return out


def model_row(blob):
    import ctypes as C
    import numpy as np
    from fembrain_amd import lib as fl
    from fembrain_amd.poly import GpuPoly
    row = {}
    a, b = C.c_int(0), C.c_int(0)
    rc = fl.lib().fb_poly_compile_info(blob.n_ops, fl.fptr(blob.ops), blob.n_prims, fl.fptr(blob.prims), C.byref(a), C.byref(b))
    row["compile_info"] = [a.value, b.value] if rc == 0 else "refused %d: %s" % (rc, fl.lib().fb_last_error().decode())
    lo, hi = np.asarray(blob.bbox[0], np.float64)[:3], np.asarray(blob.bbox[1], np.float64)[:3]
    pts = np.zeros((4096, 4), np.float32)
    pts[:, :3] = np.random.default_rng(5).uniform(lo - 0.1, hi + 0.1, size=(4096, 3)).astype(np.float32)
    for name, sem in SEMANTICS:
        try:
            g = GpuPoly(blob)
            if sem:
                g.set_field_semantics(sem)
        except (fl.FbError, ValueError) as e:
            row[name] = refusal(e) if isinstance(e, fl.FbError) else "no primitive boxes"
            continue
        r = {"field_array": sha(g.compute_field_array(pts))}
        if sem == 0:
            r["field_color_array"] = attempt(lambda: sha(*g.field_color_array(pts)))
        for dims in GRIDS:
            r["%dx%dx%d" % dims] = on_grid(g, blob, dims, sem == 0)
        g.close()
        row[name] = r
    return row


def refusals():
    """the order and argument checks, each as its return code and message"""
    import numpy as np
    from fembrain_amd import lib as fl
    from fembrain_amd.blobtree import make_tree, sphere_blob
    from fembrain_amd.poly import GpuPoly
    out = {}
    g = GpuPoly(sphere_blob())
    out["classify before a sweep"] = attempt(g.classify)
    out["read_grid before a sweep"] = attempt(lambda: fl.check(g._L.fb_poly_read_grid(g.h, None)))
    out["sweep below the reference's minimum cell size"] = attempt(lambda: g.sweep(0.001))
    out["sweep_grid with one point on an axis"] = attempt(lambda: g.sweep_grid((0, 0, 0), 0.1, (4, 1, 4)))
    out["sweep_grid with a cell size of zero"] = attempt(lambda: g.sweep_grid((0, 0, 0), 0.0, (4, 4, 4)))
    g.sweep(0.2)
    out["tetrahedralize before classify"] = attempt(g.tetrahedralize)
    out["surface before classify"] = attempt(g.surface)
    g.classify()
    out["read_tetmesh before tetrahedralize"] = attempt(lambda: fl.check(g._L.fb_poly_read_tetmesh(g.h, None, None)))
    out["read_surface before surface"] = attempt(lambda: fl.check(g._L.fb_poly_read_surface(g.h, None, None, None)))
    out["time_pipeline before tetrahedralize"] = attempt(lambda: g.time_pipeline(1))
    out["time_surface before surface"] = attempt(lambda: g.time_surface(1))
    out["displacements before a mesh"] = attempt(lambda: g.apply_fem_displacements(np.zeros(3)))
    g.tetrahedralize()
    out["displacements of the wrong length"] = attempt(lambda: g.apply_fem_displacements(np.zeros(3), 1))
    out["displacements of an unknown mesh"] = attempt(lambda: g.apply_fem_displacements(np.zeros(3), 2))
    out["empty field array"] = attempt(lambda: list(g.compute_field_array(np.zeros((0, 4), np.float32)).shape))
    out["unknown semantics"] = attempt(lambda: g.set_field_semantics(7))
    out["CPU_BOX without boxes"] = attempt(lambda: fl.check(g._L.fb_poly_set_field_semantics(g.h, 1, None)))
    out["null handle"] = attempt(lambda: fl.check(g._L.fb_poly_classify(None, None)))
    bad = sphere_blob()
    bad.prims[0, 1] = 7
    out["matrix index out of range"] = attempt(lambda: GpuPoly(bad))
    loop = make_tree([(0, (0, 0, 0), (0, 0, 0), (0, 0, 0))] * 2, [(0, 0, 0, 2, 0, 0)])
    out["operator is its own child"] = attempt(lambda: GpuPoly(loop))
    blob = sphere_blob()
    s = GpuPoly(blob)
    dims = (12, 12, 12)
    out["slab past the grid"] = attempt(lambda: s.sweep_slab(blob.bbox[0], 0.1, dims, 5, 8))
    s.sweep_slab(blob.bbox[0], 0.1, dims, 4, 6)
    out["slab_counts before tetrahedralize"] = attempt(lambda: s.slab_counts(5, 3, 3))
    s.classify()
    s.tetrahedralize()
    out["slab without the plane below"] = attempt(lambda: s.slab_counts(4, 2, 2))
    out["slab without the planes above"] = attempt(lambda: s.slab_counts(5, 4, 4))
    out["slab planes outside"] = attempt(lambda: s.slab_counts(2, 3, 3))
    out["slab that fits"] = attempt(lambda: list(s.slab_counts(5, 3, 3)))
    return out


def switched(blob):
    """one handle through CPU -> OPENCL -> CPU_BOX -> CPU, recorded at each stop (results of the semantics before are void each time)"""
    import numpy as np
    from fembrain_amd.poly import GpuPoly
    g = GpuPoly(blob)
    pts = np.zeros((4096, 4), np.float32)
    pts[:, :3] = np.random.default_rng(5).uniform(-1.5, 1.5, size=(4096, 3)).astype(np.float32)
    out = {}
    for k, (name, sem) in enumerate((("cpu", 0), ("opencl", 2), ("cpu_box", 1), ("cpu", 0))):
        if k:
            out["%d %s: switch" % (k, name)] = attempt(lambda: g.set_field_semantics(sem))
            out["%d %s: classify without a new sweep" % (k, name)] = attempt(lambda: counts_row(g.classify()))
        out["%d %s: semantics" % (k, name)] = int(g._L.fb_poly_field_semantics(g.h))
        out["%d %s: field_array" % (k, name)] = sha(g.compute_field_array(pts))
        out["%d %s: 37x21x18" % (k, name)] = on_grid(g, blob, GRIDS[1], sem == 0)
    return out


def run_cases(tree, out):
    from fembrain_amd.blobtree import read_blob
    import poly_inputs as pi

    def case(name, fn):
        out[name] = fn()
        print(name, json.dumps(out[name], default=str), flush=True)

    for path in sorted(glob.glob(os.path.join(tree, "tests", "golden", "blob", "*.blob"))):
        case(os.path.basename(path), lambda: model_row(read_blob(path)))
    for name, blob in pi.trees().items():
        case("tree " + name, lambda: model_row(blob))
    case("refusals", refusals)
    case("switched peanutInstanced.blob", lambda: switched(read_blob(os.path.join(tree, "tests", "golden", "blob", "peanutInstanced.blob"))))
    case("switched complex.blob (OPENCL refuses it)", lambda: switched(read_blob(os.path.join(tree, "tests", "golden", "blob", "complex.blob"))))


HEADER = """Polygonizer: the library of the first tree (A.json, the parent commit's) and of the second (B.json, this commit's) on the same inputs, one process per
library (tools/same_decisions_poly.py).  Per model and field semantics: steps and slots of fb_poly_compile_info, and the first 16 hex digits of the sha256 of
fb_poly_field_array at 4,096 seeded points, and on grids of 64x19x23 (k_classify<true>) and 37x21x18 points (k_classify<false>) around the model's box of the grid samples,
the classification arrays, the tet mesh, the surface's positions, normals, indices and binding, fb_poly_off_surface, fb_poly_apply_displacements on both meshes,
fb_poly_interpolate_displacements and the three slab pieces of a world of 3, with the counts; the colour entry points under the default semantics.  "refused <code>: <text>" is
the return code and fb_last_error of a call that was refused.  A row shows the parent's values, a grid's record as its counts and one hash over all of its hashes (every
field is compared on its own); the last column says whether this commit's are the same in every field.
"""


def flat(row, prefix=""):
    if not isinstance(row, dict):
        return ["%s %s" % (prefix, json.dumps(row))]
    res = []
    for k, v in row.items():
        res += flat(v, (prefix + " / " + k) if prefix else k)
    return res


def digest(v):
    """one table entry of a value: a grid's record as its counts and one hash over all of its hashes"""
    if isinstance(v, dict) and "grid" in v:
        return "counts %s all %d fields %s" % (v["counts"], len(flat(v)), hashlib.sha256(json.dumps(v, sort_keys=True).encode()).hexdigest()[:16])
    return json.dumps(v)


def compare(a_path, b_path, table_path=None):
    """a: the parent's file, b: this commit's.  Every field is compared; the table folds a grid's hashes into one"""
    a, b = json.load(open(a_path)), json.load(open(b_path))
    lines, same_all, n_fields = [HEADER], list(a) == list(b), 0
    for name, row in a.items():
        fa, fb_ = flat(row), flat(b.get(name, {}))
        same = fa == fb_
        same_all = same_all and same
        n_fields += len(fa)
        lines.append("%s | %d fields | %s" % (name, len(fa), "this commit: identical in every field" if same else "this commit DIFFERS"))
        for k, v in row.items():
            lines.append("    %s: %s" % (k, " | ".join("%s %s" % (kk, digest(vv)) for kk, vv in v.items()) if isinstance(v, dict) and "grid" not in v else digest(v)))
        if not same:
            lines += ["    DIFFERS, this commit: " + x for x in fb_ if x not in fa]
    lines.append("all %d cases, %d fields, identical in every field (hashes bit for bit, refusals word for word): %s" % (len(a), n_fields, same_all))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text if not same_all else lines[-1] + "\n")
    if table_path:
        open(table_path, "w").write(text)
    return 0 if same_all else 1


def main():
    if sys.argv[1] == "--compare":
        sys.exit(compare(*sys.argv[2:5]))
    tree, out_path = os.path.abspath(sys.argv[1]), sys.argv[2]
    sys.path[:0] = [tree, os.path.join(tree, "tests")]
    from fembrain_amd import lib as fl
    assert os.path.abspath(fl.__file__).startswith(tree + os.sep), fl.__file__
    out = {}
    run_cases(tree, out)
    json.dump(out, open(out_path, "w"), indent=1, default=str)


if __name__ == "__main__":
    main()
