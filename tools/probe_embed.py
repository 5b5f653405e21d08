"""fb_fem_embed / fb_fem_embed_update at size, on one GPU.

    python tools/probe_embed.py [--out profiles/embed_probe.json] [--reps 10] [--n 56] [--cell 0.01]

The n^3 cantilever (56: 998,250 tets) with the marching-cubes surface of sphere.blob, polygonized at --cell, scaled into it.  The
polygonizer takes no cell below 0.01, which is a 102^3 grid over the sphere's box and 38,958 vertices: the 256^3 grid and 250 k vertices
one would like to measure are out of its reach, and the probe says which surface it got.  Measured: the full search by phase -- grid
build, search through the grid, external pass with weights and counts (HIP events inside fb_fem_time_embed_search, on a scratch copy
of the points; medians of --reps) -- and the update with its copy (fb_fem_time_embed); the same after a cut through mid-span; and the
eager re-bind inside fb_fem_cut: wall clock of a FIRST cut and of a SECOND cut (another blade, the handle warm) on a handle with the
embedding live and on a twin without.  FEMBRAIN_TIMING=1 prints the laps of the re-sync inside the cut.

The way back (fb_fem_embed_add_forces / pick_ray / pick_point / embed_stress), before the cuts, each the median of --reps wall-clock
timings of the call followed by a device synchronise, every shape warmed first: the first add of a fresh embedding (table build +
dense add; one sample per spare slot), a dense add, a 3-point add, a ray pick, a point pick, embed_stress -- and, in the same run, the
host route they replace: fb_fem_read_embedding + np.add.at + fb_fem_set_external_forces, and a numpy Moeller-Trumbore pass over the
positions fb_fem_embed_update reads back.

    python tools/probe_embed.py --outside [--out profiles/embed_probe_outside.json] [--reps 10] [--n 56]

The enclosing case alone: the same surface scaled to ENCLOSE the cantilever, every vertex outside the tets.  The closest-centre pass by
path (fb_fem_time_embed_closest: the scan, the ring through the centre grid, the grid's build) for the first 1 .. 16,384 vertices of a
shuffle and for all of them, at n^3 and at the 27^3 cube (105,456 tets), with what the automatic rule chose and the search info."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from fembrain_amd import lib as fl  # noqa: E402
from fembrain_amd.blobtree import sphere_blob  # noqa: E402
from fembrain_amd.fem import FemIntegrator  # noqa: E402
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube  # noqa: E402
from fembrain_amd.poly import GpuPoly  # noqa: E402
import cutref as cr  # noqa: E402


def mid_blade(v, frac=0.5):
    xs = np.unique(v[:, 0])
    k = int(len(xs) * frac)
    p = np.array([0.5 * (xs[k - 1] + xs[k]), 0.5 * (v[:, 1].min() + v[:, 1].max()), 0.5 * (v[:, 2].min() + v[:, 2].max())])
    return cr.plane_strip(p, (1.0, 0.013, 0.007), half=20.0)


def _median_wall(fn, reps, sync):
    fn()
    sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(time.perf_counter() - t0)
    return float(np.median(out))


def touch_row(g, eid, pts, tri, reps):
    """the calls that go from the drawn mesh back to the tets, and the host route they replace"""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    sync = hip.hipDeviceSynchronize
    n = len(pts)
    rng = np.random.default_rng(1)
    f_all, f3 = rng.standard_normal((n, 3)), rng.standard_normal((3, 3))
    ids3 = np.sort(tri[len(tri) // 2]).astype(np.int32)
    g.set_uniform_force(1, -300.0)
    # the first add of a fresh embedding builds its table: one sample per spare slot (the first of them also warms the sort's storage)
    firsts = []
    for _ in range(5):
        e = g.embed(pts, tri)
        sync()
        t0 = time.perf_counter()
        g.embed_add_forces(e, f_all)
        sync()
        firsts.append(time.perf_counter() - t0)
        g.embed_release(e)
    dense = _median_wall(lambda: g.embed_add_forces(eid, f_all), reps, sync)
    three = _median_wall(lambda: g.embed_add_forces(eid, f3, ids3), reps, sync)
    info = g.embed_forces_info(eid)
    # a ray through the middle of the drawn surface, from outside the body
    c = pts.mean(axis=0)
    o, d = c + [0.03, 0.05, 10.0], np.array([0.0, 0.0, -1.0])
    hit = g.embed_pick_ray(eid, o, d)
    assert hit["triangle"] >= 0, hit
    ray = _median_wall(lambda: g.embed_pick_ray(eid, o, d), reps, sync)
    point = _median_wall(lambda: g.embed_pick_point(eid, c + [0.3, 0.1, 0.2]), reps, sync)
    g.stress()
    stress = _median_wall(lambda: g.embed_stress(eid), reps, sync)

    # the host route: the binding comes back, the scatter runs on the host, a 3 n_nodes vector goes up
    def host_add():
        b = g.embedding(eid)
        f = g.external_forces().reshape(-1, 3)
        np.add.at(f, b["vertices"].ravel(), (b["weights"][:, :, None] * f_all[:, None, :]).reshape(-1, 3))
        g.set_external_forces(f)

    def host_add3():
        b = g.embedding(eid)
        f = g.external_forces().reshape(-1, 3)
        np.add.at(f, b["vertices"][ids3].ravel(), (b["weights"][ids3][:, :, None] * f3[:, None, :]).reshape(-1, 3))
        g.set_external_forces(f)

    def host_ray():
        p = g.embed_update(eid, normals=False)[0].astype(np.float64)
        a, b, cc = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
        e1, e2 = b - a, cc - a
        pv = np.cross(d[None, :], e2)
        det = (e1 * pv).sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            tv = o[None, :] - a
            u = (tv * pv).sum(axis=1) / det
            qv = np.cross(tv, e1)
            w = (qv * d[None, :]).sum(axis=1) / det
            t = (e2 * qv).sum(axis=1) / det
            ok = (det != 0) & (u >= 0) & (w >= 0) & (u + w <= 1) & (t >= 0)
        k = np.nonzero(ok)[0]
        return int(k[np.argmin(t[k])]) if len(k) else -1

    assert host_ray() == hit["triangle"], (host_ray(), hit)
    out = dict(case="touch", n_points=n, n_triangles=len(tri), n_nodes=g.r // 3, longest_run=info["longest_run"], n_nodes_touched=info["n_nodes_touched"],
               seconds_first_add_samples=firsts, seconds_first_add=float(np.median(firsts[1:])), seconds_dense_add=dense, seconds_3_point_add=three,
               seconds_pick_ray=ray, seconds_pick_point=point, seconds_embed_stress=stress,
               host_seconds_dense_add=_median_wall(host_add, reps, sync), host_seconds_3_point_add=_median_wall(host_add3, reps, sync),
               host_seconds_pick_ray=_median_wall(host_ray, reps, sync),
               bytes_host_route_add=52 * n + 2 * 24 * (g.r // 3), bytes_dense_add=24 * n, bytes_3_point_add=3 * 28)
    out["seconds_table_build"] = out["seconds_first_add"] - dense
    return out


def outside_rows(n, sx, tri, reps):
    """--outside: the sphere scaled to ENCLOSE the n^3 cantilever, every vertex outside the tets.  The external pass alone, by path
    (fb_fem_time_embed_closest: HIP events, medians, on a scratch copy), for all vertices and for the first k of a shuffle of them (the
    crossover of the two paths); what the automatic rule chose for the embedding; the search info under either path."""
    v, t = truth_cube(n, n, n, 0.1)
    v = np.asarray(v, np.float64).reshape(-1, 3)
    fixed = fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n))
    lo, hi = v.min(0), v.max(0)
    radius = np.linalg.norm(sx.astype(np.float64), axis=1)
    pts = 0.5 * (lo + hi) + sx.astype(np.float64) * (1.05 * 0.5 * np.linalg.norm(hi - lo) / radius.min())
    order = np.random.default_rng(0).permutation(len(pts))
    g = FemIntegrator(v, t, fixed)
    rows = []
    counts = [k for k in (1, 4, 12, 16, 64, 256, 1024, 4096, 16384) if k < len(pts)] + [len(pts)]
    for name in ("FEMBRAIN_EMBED_CLOSEST", "FEMBRAIN_EMBED_RING_BUDGET"):
        os.environ.pop(name, None)
    # what the rule chooses on a mesh generation without a centre grid: ascending counts, so that the first grid is one the rule asked for
    auto_path = {}
    for k in counts:
        e = g.embed(pts[order[:k]])
        auto_path[k] = g.embed_search_info(e)["path"]
        g.embed_release(e)
    for k in counts:
        whole = k == len(pts)
        eid, info = g.embed(pts if whole else pts[order[:k]], tri if whole else None, info=True)
        auto = dict(path=auto_path[k])
        assert info["n_external"] == k, info
        r_scan = max(1, min(reps, 3)) if k * len(t) > 1 << 33 else reps  # (seconds per repetition up there)
        scan = g.time_embed_closest(eid, fl.FB_EMBED_CLOSEST_SCAN, r_scan)
        ring = g.time_embed_closest(eid, fl.FB_EMBED_CLOSEST_RING, reps)
        g.embed_release(eid)
        by_path = {}
        for path in ("scan", "ring"):  # the same points bound under either path: the counters, and the same binding
            os.environ["FEMBRAIN_EMBED_CLOSEST"] = path
            e = g.embed(pts if whole else pts[order[:k]])
            by_path[path] = (g.embed_search_info(e), g.embedding(e))
            g.embed_release(e)
        os.environ.pop("FEMBRAIN_EMBED_CLOSEST")
        same = all(by_path["scan"][1][key].tobytes() == by_path["ring"][1][key].tobytes() for key in ("elements", "vertices", "weights"))
        out = dict(case="outside%d" % n, n_tets=len(t), n_outside=k, grid=list(info["grid"]), auto_path=auto["path"], seconds_scan=scan[1], reps_scan=r_scan,
                   seconds_ring=ring[1], seconds_centre_grid_build=ring[0], ring_plus_build_over_scan=(ring[0] + ring[1]) / scan[1],
                   same_binding=same, info_ring=by_path["ring"][0], info_scan=by_path["scan"][0])
        print(json.dumps(out), flush=True)
        rows.append(out)
    g.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=56)
    ap.add_argument("--cell", type=float, default=0.01)
    ap.add_argument("--outside", action="store_true", help="the enclosing-surface case only: every vertex outside the tets (profiles/embed_probe_outside.json)")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "embed_probe_outside.json" if a.outside else "embed_probe.json")
    v, t = truth_cube(a.n, a.n, a.n, 0.1)
    v = np.asarray(v, np.float64).reshape(-1, 3)
    fixed = fixed_vertices_to_dofs(cube_fixed_plane_i0(a.n, a.n))
    # the drawn surface: the sphere, 90 % of the body's width, about its centre
    poly = GpuPoly(sphere_blob())
    box = poly.sweep(a.cell)
    poly.classify()
    poly.surface()
    sx, _, st = poly.read_surface()
    lo, hi = v.min(0), v.max(0)
    r = np.abs(sx).max()
    pts = 0.5 * (lo + hi) + sx.astype(np.float64) * (0.45 * (hi - lo).min() / r)
    tri = st.astype(np.int32)
    poly.close()
    if a.outside:
        rows = outside_rows(a.n, sx, tri, a.reps) + outside_rows(27, sx, tri, a.reps)  # 998,250 tets at the default n | the 105,456-tet cube
        with open(a.out, "w") as fh:
            json.dump(dict(tool="tools/probe_embed.py --outside", reps=a.reps, timer="HIP events inside fb_fem_time_embed_closest (medians; the ring's figure includes its host wait)", rows=rows), fh, indent=1)
            fh.write("\n")
        return
    rows = []

    def row(name, g, eid, **extra):
        info = g.embed_update(eid)[2]
        loc, upd = g.time_embed(eid, a.reps)
        phases = g.time_embed_search(eid, a.reps)
        out = dict(case=name, n_tets=int(g.num_tets()), n_points=info["n_points"], n_triangles=info["n_triangles"], grid=list(info["grid"]), n_wide=info["n_wide"],
                   n_external=info["n_external"], n_rebound=info["n_rebound"], seconds_locate=loc, seconds_grid_build=phases[0],
                   seconds_search=phases[1], seconds_external_pass=phases[2], seconds_update=upd,
                   bytes_out_update=24 * info["n_points"] + 24, **extra)
        print(json.dumps(out), flush=True)
        rows.append(out)

    g = FemIntegrator(v, t, fixed, expect_cuts=True)
    t0 = time.perf_counter()
    eid = g.embed(pts, tri)
    first = time.perf_counter() - t0
    row("cube%d" % a.n, g, eid, first_embed_wall_s=first, sweep_dims=[int(x) for x in box] if box is not None else None)
    rows.append(touch_row(g, eid, pts, tri, a.reps))
    print(json.dumps(rows[-1]), flush=True)

    def two_cuts(h):
        out = []
        for frac in (0.5, 0.75):
            t0 = time.perf_counter()
            info, _ = h.cut(mid_blade(v, frac), mode="carry", track=False)
            out.append(time.perf_counter() - t0)
            assert info["status"] == fl.FB_CUT_DONE, info
        return out

    with_e = two_cuts(g)
    row("cube%d_after_cuts" % a.n, g, eid)
    g.close()
    g = FemIntegrator(v, t, fixed, expect_cuts=True)
    without = two_cuts(g)
    g.close()
    rows.append(dict(case="cube%d_cuts" % a.n, first_cut_wall_s_with_embedding=with_e[0], first_cut_wall_s_without=without[0],
                     second_cut_wall_s_with_embedding=with_e[1], second_cut_wall_s_without=without[1]))
    print(json.dumps(rows[-1]), flush=True)
    with open(a.out, "w") as fh:
        json.dump(dict(tool="tools/probe_embed.py", reps=a.reps, timer="HIP events inside fb_fem_time_embed / fb_fem_time_embed_search (medians); time.perf_counter around fb_fem_cut; the touch row: time.perf_counter around the call and a hipDeviceSynchronize (medians)", rows=rows), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
