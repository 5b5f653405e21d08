"""fb_fem_surface / fb_fem_surface_update against the host route they replace, on one GPU.

    python tools/probe_fem_surface.py [--out profiles/fem_surface_probe.json] [--reps 20] [--rounds 5] [--trace]

Cases: the 27^3 and 56^3 cantilevers (998,250 tets), the 56^3 one after a cut through mid-span, the 606k-tet Delaunay mesh of a jittered
grid.  Per case: build and update on the device (HIP events inside fb_fem_time_surface, warm, the median of --reps repetitions; --rounds
such medians give the spread), and beside each what it replaces, measured in the same run: read_mesh() + the vectorised restatement
(tests/surfref.py) for the build; get_q_state() + numpy positions and normals for the update (wall clock).  --trace: one warm build and
update of the 56^3 case only (for a kernel-trace run of its own)."""
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
from fembrain_amd.fem import FemIntegrator  # noqa: E402
from fembrain_amd.meshgen import cube_fixed_plane_i0, delaunay_jittered, fixed_vertices_to_dofs, truth_cube  # noqa: E402
import cutref as cr  # noqa: E402
import surfref as sr  # noqa: E402


def cube(n):
    v, t = truth_cube(n, n, n, 0.1)
    return np.asarray(v, np.float64).reshape(-1, 3), t, fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n))


def mid_blade(v):
    xs = np.unique(v[:, 0])
    k = len(xs) // 2
    p = np.array([0.5 * (xs[k - 1] + xs[k]), 0.5 * (v[:, 1].min() + v[:, 1].max()), 0.5 * (v[:, 2].min() + v[:, 2].max())])
    return cr.plane_strip(p, (1.0, 0.013, 0.007), half=20.0)


def spread(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1], n=len(xs))


def measure(name, g, load, reps, rounds):
    steps = "2 loaded steps"
    try:
        for _ in range(2):
            g.set_uniform_force(1, load)
            g.do_timestep()
    except fl.FbError as e:        # (thin pieces after a cut: the solver's matter; the surface is measured at whatever state there is)
        steps = "a step failed: %s" % e
    s = g.surface()
    g.surface_update()
    dev = [g.time_surface(reps) for _ in range(rounds)]
    # the host route of the build: the whole mesh back, four faces per element sorted on the host
    t0 = time.perf_counter()
    x0, t = g.read_mesh()
    t1 = time.perf_counter()
    faces, _ = sr.vectorised(x0, t)
    t2 = time.perf_counter()
    assert np.array_equal(faces, s["faces"])
    ids = s["vertex_ids"]
    host_update = []
    for _ in range(3):
        t3 = time.perf_counter()
        q = g.get_q_state()[0].reshape(-1, 3)
        t4 = time.perf_counter()
        pos = x0 + q
        xyz = np.float32(pos)[ids]
        nrm, _ = sr.normals(pos, faces, ids)
        box = sr.aabb(xyz)
        host_update.append((t4 - t3, time.perf_counter() - t4))
    xyz_d, _, box_d = g.surface_update()
    assert np.array_equal(xyz_d, xyz) and np.array_equal(box_d, box)
    t5 = time.perf_counter()
    g.surface_update()
    wall_update = time.perf_counter() - t5
    row = dict(case=name, state=steps, n_nodes=int(len(x0)), n_tets=int(len(t)), n_faces=int(len(faces)), n_vertices=int(len(ids)),
               device_build_s=spread([b for b, _ in dev]), device_update_s=spread([u for _, u in dev]), device_update_wall_s=wall_update,
               host_build_s=dict(read_mesh=t1 - t0, faces_numpy=t2 - t1, total=t2 - t0),
               host_update_s=dict(get_q_state=spread([a for a, _ in host_update]), numpy=spread([b for _, b in host_update]),
                                  total=spread([a + b for a, b in host_update])),
               bytes_out_update=int(24 * len(ids) + 24), bytes_host_route_update=int(8 * 3 * len(x0)))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fem_surface_probe.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    if a.trace:
        v, t, fixed = cube(56)
        g = FemIntegrator(v, t, fixed, expect_cuts=True)
        g.surface()
        g.time_surface(1)
        g.close()
        return
    rows = []
    for n in (27, 56):
        v, t, fixed = cube(n)
        g = FemIntegrator(v, t, fixed, expect_cuts=True)
        rows.append(measure("cube%d" % n, g, -10000.0, a.reps, a.rounds))
        g.close()
        if n == 56:   # cut at rest (under the load above the beam sags away from a blade placed in the rest frame), a warm second handle
            g = FemIntegrator(v, t, fixed, expect_cuts=True)
            g.surface()
            t0 = time.perf_counter()
            info, _ = g.cut(mid_blade(v), track=False)
            cut_s = time.perf_counter() - t0
            assert info["status"] == fl.FB_CUT_DONE, info
            t0 = time.perf_counter()
            g.surface()
            first = time.perf_counter() - t0
            row = measure("cube56_after_cut", g, -300.0, a.reps, a.rounds)
            row["cut_wall_s"], row["first_build_after_cut_wall_s"] = cut_s, first
            rows.append(row)
            g.close()
    pts, tt, fxd = delaunay_jittered(48)
    g = FemIntegrator(pts, tt, fxd)
    rows.append(measure("delaunay_jittered48", g, -200.0, a.reps, a.rounds))
    g.close()
    with open(a.out, "w") as fh:
        json.dump(dict(tool="tools/probe_fem_surface.py", reps=a.reps, rounds=a.rounds, timer="HIP events inside fb_fem_time_surface (device), time.perf_counter (host route)",
                       rows=rows), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
