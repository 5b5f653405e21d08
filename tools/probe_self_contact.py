"""What fb_fem_self_contact costs at 1M tets, against the two routes a caller had before it.

    python tools/probe_self_contact.py [--out profiles/self_contact_probe.json] [--n 56] [--reps 5]

The n^3 cantilever is cut through mid-span (fb_fem_cut, carry) and stays ONE handle; the free half is pressed 0.3 of a cell into the
clamped one, off its sides by fractions of a cell.  Mode FB_SELF_CONTACT_OTHER_PARTS.  For FEMBRAIN_SELF_CONTACT=ring and =scan:
  stages   fb_fem_time_self_contact's five stages (positions and box | point grid and containment | face grid | closest faces |
           scatter), means of --reps with their host waits
  call     one fb_fem_self_contact by wall clock, the median of --reps
Yardsticks, measured in the same run:
  host     the route without any contact call on the device: the state (get_q_state) and the mesh (read_mesh) down, one force vector
           up, timed without any arithmetic in between
  detach   fb_fem_body_contact on the same two halves at the same positions after detach_part(remove=True): two handles, the call and
           its stages (default path)
Also written: the point grid's cell count by the library's grid rule and the elements per cell, the first thing to tune where the
containment stage is what costs.

    python tools/probe_self_contact.py --friction [--out profiles/self_contact_friction_probe.json]

--friction: the same pressed handle with the free half moving at (0.2, -0.1, 0.05); one call by wall clock, the median of --reps, WITHOUT
and WITH friction and damping (fb_fem_self_contact against fb_fem_self_contact_friction, mu 0.5, slip speed 0.15, damping 40) in the same
run, default path.  The pair goes into a JSON of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cutref as cr  # noqa: E402
import selfcontactref as S  # noqa: E402
from fembrain_amd import lib as fl  # noqa: E402
from fembrain_amd.fem import FemIntegrator  # noqa: E402
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube  # noqa: E402

K = 5000.0
SELF_STAGES = ("positions_and_box", "point_grid_and_containment", "face_grid", "closest", "scatter")
BODY_STAGES = ("boxes", "tet_grid_and_containment", "face_grid", "closest", "scatter")


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--friction", action="store_true")
    ap.add_argument("--n", type=int, default=56)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "self_contact_friction_probe.json" if a.friction else "self_contact_probe.json")
    n, h = a.n, 0.1
    v, t = truth_cube(n, n, n, h)
    v = np.asarray(v, np.float64).reshape(-1, 3)
    g = FemIntegrator(v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n)), expect_cuts=True)
    xs = np.unique(v[:, 0])
    k = len(xs) // 2
    p = np.array([0.5 * (xs[k - 1] + xs[k]), 0.5 * (v[:, 1].min() + v[:, 1].max()), 0.5 * (v[:, 2].min() + v[:, 2].max())])
    surface_before = len(g.surface()["vertex_ids"])
    info, _ = g.cut(cr.plane_strip(p, (1.0, 0.013, 0.007), half=4.0 * n * h), mode="carry", track=False)
    assert info["status"] == fl.FB_CUT_DONE and g.parts()["n_parts"] == 2, info
    n_nodes, n_tets = int(g._L.fb_fem_num_nodes(g.h)), int(g.num_tets())
    g.r = 3 * n_nodes
    free = 1 - int(g.element_parts()[0])
    in_free = g.node_parts() == free
    press = np.array([-0.3 * h, 0.37 * h, 0.41 * h])   # the free half sits at larger x: into the clamped half, and off its sides
    q = np.where(in_free[:, None], press[None, :], 0.0)
    g.set_q_state(q.reshape(-1))
    surf = g.surface()
    nv, nf = len(surf["vertex_ids"]), len(surf["faces"])
    print("one handle: %d tets on %d nodes, %d surface vertices (%d before the cut), %d boundary faces" % (n_tets, n_nodes, nv, surface_before, nf), flush=True)
    out = {}
    if a.friction:
        mu, slip, damping = 0.5, 0.15, 40.0
        g.set_q_state(q.reshape(-1), np.where(in_free[:, None], np.array([0.2, -0.1, 0.05])[None, :], 0.0).reshape(-1))
        for name, kw in (("frictionless", {}), ("friction", dict(mu=mu, slip_speed=slip, damping=damping))):
            g.set_external_forces_to_zero()
            c = g.self_contact(K, mode="other_parts", **kw)   # (warm)
            walls = []
            for _ in range(a.reps):
                g.set_external_forces_to_zero()
                t0 = time.perf_counter()
                c = g.self_contact(K, mode="other_parts", **kw)
                walls.append(time.perf_counter() - t0)
            out[name] = dict(call_seconds=median(walls), call_all=walls, path=c["path"], n_contacts=c["n_contacts"], faces_tested=c["faces_tested"])
            for key in ("n_sticking", "n_sliding", "n_separating", "max_slip_speed", "max_normal_force", "max_stick_rate"):
                if key in c:
                    out[name][key] = list(c[key]) if isinstance(c[key], tuple) else c[key]
            print("  %-12s call %.3f ms (%s); %d contacts" % (name, 1e3 * out[name]["call_seconds"], " ".join("%.3f" % (1e3 * w) for w in walls), c["n_contacts"]), flush=True)
        out["friction_over_frictionless"] = out["friction"]["call_seconds"] / out["frictionless"]["call_seconds"]
        g.close()
        res = dict(tool="tools/probe_self_contact.py --friction", mesh="cube %d^3 after a mid-span cut, one handle, the free half pressed 0.3 of a cell into the clamped one" % n,
                   mode="other_parts", reps=a.reps, stiffness=K, mu=mu, slip_speed=slip, damping=damping,
                   sizes=dict(n_tets=n_tets, n_nodes=n_nodes, surface_vertices=nv, faces=nf), results=out, kernel_sources_sha256=fl.source_sha256("fem"))
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", a.out)
        return
    for path in ("ring", "scan"):
        os.environ["FEMBRAIN_SELF_CONTACT"] = path
        g.set_external_forces_to_zero()
        c = g.self_contact(K, mode="other_parts")   # (warm: buffers, code objects, the labels)
        walls = []
        for _ in range(a.reps):
            g.set_external_forces_to_zero()
            t0 = time.perf_counter()
            c = g.self_contact(K, mode="other_parts")
            walls.append(time.perf_counter() - t0)
        stages = g.time_self_contact(K, mode="other_parts", reps=a.reps)
        out[path] = dict(stages_seconds=dict(zip(SELF_STAGES, [float(x) for x in stages])), stages_total_seconds=float(stages.sum()), call_seconds=median(walls),
                         call_all=walls, path=c["path"], n_points=c["n_points"], n_contacts=c["n_contacts"], n_degenerate=c["n_degenerate"],
                         faces_tested=c["faces_tested"], faces_tested_per_contact=c["faces_tested"] / max(c["n_contacts"], 1), max_depth=c["max_depth"])
        print("  %-4s call %.2f ms; stages (ms) %s; %d contacts, %.0f faces tested per contact" % (
            path, 1e3 * out[path]["call_seconds"], " ".join("%.2f" % (1e3 * x) for x in stages), c["n_contacts"], out[path]["faces_tested_per_contact"]), flush=True)
    del os.environ["FEMBRAIN_SELF_CONTACT"]
    x, _ = g.read_mesh()
    cur = x + q
    dim = [int(d) for d in S.point_grid(cur, nv)[2]]   # (the library's grid rule, restated for the tests)
    cells = dim[0] * dim[1] * dim[2]
    out["point_grid"] = dict(dim=dim, cells=cells, elements_per_cell=n_tets / cells, points_per_cell=nv / cells)
    # the host route: state and mesh down, one force vector up, nothing computed
    host = []
    zero = np.zeros(3 * n_nodes)
    for _ in range(a.reps):
        t0 = time.perf_counter()
        g.get_q_state()
        g.read_mesh()
        t1 = time.perf_counter()
        g.set_external_forces(zero)
        t2 = time.perf_counter()
        host.append((t2 - t0, t1 - t0, t2 - t1))
    hm = sorted(host)[len(host) // 2]
    out["host_route"] = dict(seconds=hm[0], read_back_seconds=hm[1], upload_seconds=hm[2])
    print("  host route %.2f ms: read back %.2f, upload %.2f (no arithmetic)" % (1e3 * hm[0], 1e3 * hm[1], 1e3 * hm[2]), flush=True)
    # the two-handle route on the same halves at the same positions
    t0 = time.perf_counter()
    piece, _, _ = g.detach_part(free, remove=True, track=False)
    t_detach = time.perf_counter() - t0
    g.r, piece.r = 3 * int(g._L.fb_fem_num_nodes(g.h)), 3 * int(piece._L.fb_fem_num_nodes(piece.h))
    g.set_q_state(np.zeros(g.r))
    piece.set_q_state(np.tile(press, piece.r // 3))
    for b in (g, piece):
        b.set_external_forces_to_zero()
    bc = piece.body_contact(g, K)
    walls = []
    for _ in range(a.reps):
        for b in (g, piece):
            b.set_external_forces_to_zero()
        t0 = time.perf_counter()
        bc = piece.body_contact(g, K)
        walls.append(time.perf_counter() - t0)
    stages = piece.time_body_contact(g, K, reps=a.reps)
    out["detached_body_contact"] = dict(detach_seconds=t_detach, stages_seconds=dict(zip(BODY_STAGES, [float(s) for s in stages])), stages_total_seconds=float(stages.sum()),
                                        call_seconds=median(walls), call_all=walls, path=bc["path"], n_contacts=list(bc["n_contacts"]),
                                        faces_tested=bc["faces_tested"], max_depth=bc["max_depth"])
    print("  two handles: detach %.2f ms once, then fb_fem_body_contact %.2f ms a call; stages (ms) %s; %d + %d contacts" % (
        1e3 * t_detach, 1e3 * median(walls), " ".join("%.2f" % (1e3 * s) for s in stages), bc["n_contacts"][0], bc["n_contacts"][1]), flush=True)
    piece.close()
    g.close()
    res = dict(tool="tools/probe_self_contact.py", mesh="cube %d^3 after a mid-span cut, one handle, the free half pressed 0.3 of a cell into the clamped one" % n,
               mode="other_parts", reps=a.reps, stiffness=K, sizes=dict(n_tets=n_tets, n_nodes=n_nodes, surface_vertices=nv, surface_vertices_before_cut=surface_before, faces=nf),
               results=out, kernel_sources_sha256=fl.source_sha256("fem"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
