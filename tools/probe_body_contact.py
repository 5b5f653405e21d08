"""What contact between two bodies costs on the device beside the host route it replaces, on one GPU.

    python tools/probe_body_contact.py [--out profiles/body_contact_probe.json] [--n 56] [--reps 5] [--host-points 128]

The n^3 cantilever (56: 998,250 tets) after its mid-span cut (FB_CUT_CARRY); the free half is detached with removal.  Two cases:
  resting  the detached half laid onto the top of the stump, sunk in by 0.3 of a cell: a thin overlap, contacts in both directions
  deep     a small cube (8^3 nodes, half the cell size) in the middle of the stump: few points, each far from every boundary face
Per case, for FEMBRAIN_BODY_CONTACT=ring and =scan:
  stages   fb_fem_time_body_contact's five stages (boxes | element grid and containment | face grid | closest faces | scatter), host waits included
  call     one fb_fem_body_contact by wall clock, the median of --reps
  counts   candidates, contacts, grids built, faces tested per contact
and once per case:
  filter   the elements of each searched body whose current box meets the overlap box (what the element grid bins; counted here on the
           host by the same rule) against the elements of the mesh
  host     the route the call replaces: both states and surfaces read back, tests/bodycontactref.py's brute force on the elements the
           filter keeps and ALL faces, two force vectors uploaded.  The brute force runs on --host-points candidates per direction, evenly
           spaced, and `scaled_seconds` scales its time to all of them: it is an estimate and labelled so.

    python tools/probe_body_contact.py --friction [--out profiles/body_contact_friction_probe.json]

--friction: the resting case only, the piece moving at (0.2, -0.1, 0.05); one call by wall clock, the median of --reps, WITHOUT and WITH
friction and damping (fb_fem_body_contact against fb_fem_body_contact_friction, mu 0.5, slip speed 0.15, damping 40) in the same run,
default path.  The pair goes into a JSON of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bodycontactref as R  # noqa: E402
import cutref as cr  # noqa: E402
from fembrain_amd import lib as fl  # noqa: E402
from fembrain_amd.fem import FemIntegrator  # noqa: E402
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube  # noqa: E402

K = 5000.0


def median(xs):
    return sorted(xs)[len(xs) // 2]


def current(g):
    x, t = g.read_mesh()
    return x, t, x + g.get_q_state()[0].reshape(-1, 3)


def filtered(cur_p, vids_p, cur_t, tets_t):
    """ids of the elements of T whose current box meets the overlap of P's surface box and T's node box"""
    lo = np.maximum(cur_p[vids_p].min(axis=0), cur_t.min(axis=0))
    hi = np.minimum(cur_p[vids_p].max(axis=0), cur_t.max(axis=0))
    if not (lo <= hi).all():
        return np.zeros(0, np.int64)
    pad = 2.0 ** -30 * float((cur_t.max(axis=0) - cur_t.min(axis=0)).max())
    v = cur_t[tets_t]
    return np.nonzero(((v.min(axis=1) - pad <= hi) & (v.max(axis=1) + pad >= lo)).all(axis=1))[0]


def host_route(ga, gb, points):
    """seconds of the host route's three parts, and what it found on its sample"""
    t0 = time.perf_counter()
    xa, ta, ca = current(ga)
    xb, tb, cb = current(gb)
    sa, sb = ga.surface(), gb.surface()
    t_read = time.perf_counter() - t0
    t_ref, scaled, found, kept = 0.0, 0.0, [], []
    for (cp, vp), (ct, tt, ft) in (((ca, sa["vertex_ids"]), (cb, tb, sb["faces"])), ((cb, sb["vertex_ids"]), (ca, ta, sa["faces"]))):
        t0 = time.perf_counter()
        keep = filtered(cp, vp, ct, tt)
        kept.append((int(len(keep)), int(len(tt))))
        inside = ((cp[vp] >= ct.min(axis=0)) & (cp[vp] <= ct.max(axis=0))).all(axis=1)
        cand = vp[inside]
        t_pre = time.perf_counter() - t0
        if not len(cand) or not len(keep):
            t_ref += t_pre
            scaled += t_pre
            found.append((int(len(cand)), 0, 0))
            continue
        sample = cand[np.unique(np.linspace(0, len(cand) - 1, min(points, len(cand))).astype(np.int64))]
        t0 = time.perf_counter()
        r = R.direction(cp, sample, ct, tt[keep], ft, K)
        dt = time.perf_counter() - t0
        t_ref += t_pre + dt
        scaled += t_pre + dt * len(cand) / len(sample)
        found.append((int(len(cand)), int(len(sample)), int(len(r["node"]))))
    t0 = time.perf_counter()
    ga.set_external_forces(np.zeros(3 * len(xa)))
    gb.set_external_forces(np.zeros(3 * len(xb)))
    t_up = time.perf_counter() - t0
    return dict(read_back_seconds=t_read, reference_seconds_on_sample=t_ref, reference_scaled_seconds=scaled, upload_seconds=t_up,
                scaled_seconds=t_read + scaled + t_up, candidates_sample_contacts=found), kept


def measure(ga, gb, reps, points):
    out = {}
    for path in ("ring", "scan"):
        os.environ["FEMBRAIN_BODY_CONTACT"] = path
        for g in (ga, gb):
            g.set_external_forces_to_zero()
        info = ga.body_contact(gb, K)   # (warm: buffers, code objects, both surfaces)
        walls = []
        for _ in range(reps):
            for g in (ga, gb):
                g.set_external_forces_to_zero()
            t0 = time.perf_counter()
            info = ga.body_contact(gb, K)
            walls.append(time.perf_counter() - t0)
        stages = ga.time_body_contact(gb, K, reps=reps)
        n = sum(info["n_contacts"])
        out[path] = dict(stages_seconds=dict(zip(("boxes", "tet_grid_and_containment", "face_grid", "closest", "scatter"), [float(x) for x in stages])),
                         stages_total_seconds=float(stages.sum()), call_seconds=median(walls), call_all=walls, path=int(info["path"]),
                         n_candidates=list(info["n_candidates"]), n_contacts=list(info["n_contacts"]), n_degenerate=list(info["n_degenerate"]),
                         n_tet_grid_builds=info["n_tet_grid_builds"], n_face_grid_builds=info["n_face_grid_builds"], faces_tested=info["faces_tested"],
                         faces_tested_per_contact=info["faces_tested"] / max(n, 1), max_depth=info["max_depth"])
        print("  %-4s call %.2f ms; stages (ms) %s; %d contacts, %.0f faces tested per contact" % (
            path, 1e3 * out[path]["call_seconds"], " ".join("%.2f" % (1e3 * x) for x in stages), n, out[path]["faces_tested_per_contact"]), flush=True)
    del os.environ["FEMBRAIN_BODY_CONTACT"]
    host, kept = host_route(ga, gb, points)
    out["host_route"] = host
    out["filter"] = dict(elements_binned_and_elements=[list(k) for k in kept],
                         faces=[len(gb.surface()["faces"]), len(ga.surface()["faces"])])
    print("  host route (scaled from %d points per direction) %.1f ms: read back %.1f, reference %.1f, upload %.1f; elements the filter keeps %s" % (
        points, 1e3 * host["scaled_seconds"], 1e3 * host["read_back_seconds"], 1e3 * host["reference_scaled_seconds"], 1e3 * host["upload_seconds"], kept), flush=True)
    return out


MU, SLIP, DAMPING = 0.5, 0.15, 40.0


def measure_friction(ga, gb, reps):
    """one call by wall clock without and with friction, from the same state"""
    out = {}
    for name, kw in (("frictionless", {}), ("friction", dict(mu=MU, slip_speed=SLIP, damping=DAMPING))):
        for g in (ga, gb):
            g.set_external_forces_to_zero()
        info = ga.body_contact(gb, K, **kw)   # (warm)
        walls = []
        for _ in range(reps):
            for g in (ga, gb):
                g.set_external_forces_to_zero()
            t0 = time.perf_counter()
            info = ga.body_contact(gb, K, **kw)
            walls.append(time.perf_counter() - t0)
        out[name] = dict(call_seconds=median(walls), call_all=walls, path=int(info["path"]), n_contacts=list(info["n_contacts"]), faces_tested=info["faces_tested"])
        for key in ("n_sticking", "n_sliding", "n_separating", "max_slip_speed", "max_normal_force", "max_stick_rate"):
            if key in info:
                out[name][key] = list(info[key]) if isinstance(info[key], tuple) else info[key]
        print("  %-12s call %.3f ms (%s); %d contacts" % (name, 1e3 * out[name]["call_seconds"], " ".join("%.3f" % (1e3 * w) for w in walls), sum(info["n_contacts"])), flush=True)
    out["friction_over_frictionless"] = out["friction"]["call_seconds"] / out["frictionless"]["call_seconds"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--friction", action="store_true")
    ap.add_argument("--n", type=int, default=56)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-points", type=int, default=128)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "body_contact_friction_probe.json" if a.friction else "body_contact_probe.json")
    n, h = a.n, 0.1
    v, t = truth_cube(n, n, n, h)
    v = np.asarray(v, np.float64).reshape(-1, 3)
    stump = FemIntegrator(v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n)), expect_cuts=True)
    xs = np.unique(v[:, 0])
    k = len(xs) // 2
    p = np.array([0.5 * (xs[k - 1] + xs[k]), 0.5 * (v[:, 1].min() + v[:, 1].max()), 0.5 * (v[:, 2].min() + v[:, 2].max())])
    info, _ = stump.cut(cr.plane_strip(p, (1.0, 0.013, 0.007), half=4.0 * n * h), mode="carry", track=False)
    assert info["status"] == fl.FB_CUT_DONE and stump.parts()["n_parts"] == 2, info
    free = 1 - int(stump.element_parts()[0])
    piece, _, _ = stump.detach_part(free, remove=True, track=False)
    sizes = dict(stump=dict(n_tets=int(stump.num_tets()), n_nodes=int(stump._L.fb_fem_num_nodes(stump.h))),
                 piece=dict(n_tets=int(piece.num_tets()), n_nodes=int(piece._L.fb_fem_num_nodes(piece.h))))
    stump.r, piece.r = 3 * sizes["stump"]["n_nodes"], 3 * sizes["piece"]["n_nodes"]
    print("stump %(n_tets)d tets on %(n_nodes)d nodes" % sizes["stump"], "| piece %(n_tets)d tets on %(n_nodes)d nodes" % sizes["piece"], flush=True)
    cases = {}
    # resting: the piece onto the stump's top, 0.3 of a cell deep, off the stump's sides by fractions of a cell
    x = piece.read_mesh()[0]
    lift = np.array([v[:, 0].min() + 0.37 * h - x[:, 0].min(), v[:, 1].max() - 0.3 * h - x[:, 1].min(), 0.41 * h])
    piece.set_q_state(np.tile(lift, len(x)))
    if a.friction:
        piece.set_q_state(np.tile(lift, len(x)), np.tile([0.2, -0.1, 0.05], len(x)))
        print("resting, without and with friction:", flush=True)
        pair = measure_friction(piece, stump, a.reps)
        piece.close()
        stump.close()
        out = dict(tool="tools/probe_body_contact.py --friction", mesh="cube %d^3 after a mid-span cut, the free half detached and laid onto the stump" % n, reps=a.reps,
                   stiffness=K, mu=MU, slip_speed=SLIP, damping=DAMPING, sizes=sizes, resting=pair, kernel_sources_sha256=fl.source_sha256("fem"))
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", a.out)
        return
    print("resting:", flush=True)
    cases["resting"] = measure(piece, stump, a.reps, a.host_points)
    piece.close()
    # deep: a small cube in the middle of the stump
    vc, tc = truth_cube(8, 8, 8, 0.5 * h)
    stump_x = stump.read_mesh()[0][np.unique(stump.read_mesh()[1])]
    centre = 0.5 * (stump_x.min(axis=0) + stump_x.max(axis=0)) + np.array([0.013, 0.029, 0.017])
    vc = vc + (centre - 0.5 * (vc.min(axis=0) + vc.max(axis=0)))[None, :]
    small = FemIntegrator(vc, tc)
    sizes["small"] = dict(n_tets=len(tc), n_nodes=len(vc))
    print("deep:", flush=True)
    cases["deep"] = measure(small, stump, a.reps, a.host_points)
    small.close()
    stump.close()
    out = dict(tool="tools/probe_body_contact.py", mesh="cube %d^3 after a mid-span cut, the free half detached" % n, reps=a.reps, host_points=a.host_points,
               stiffness=K, sizes=sizes, cases=cases, kernel_sources_sha256=fl.source_sha256("fem"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
