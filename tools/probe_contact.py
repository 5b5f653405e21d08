"""The probe's box contact on the device against the host route it replaces, on one GPU.

    python tools/probe_contact.py [--out profiles/contact_probe.json] [--reps 9] [--n 56] [--patches 12,20,32]

Case: the n^3 cantilever (default 56: 998,250 tets) after two lightly loaded steps, a tool box pressed half a cell into a square patch of
p x p nodes in the middle of its top face (p = 12: 144 nodes, what fb_fem_add_haptic_forces still takes; 20 and 32: 400 and 1024 nodes,
beyond it).  Per patch:

  move      contact_move (fb_fem_contact_move: eight launches, one 64-byte copy back) with the set already touched -- the per-frame case
            host: get_q_state read-back, ProbeContact.move on the positions (numpy)
  apply     set_uniform_force + contact_apply (fb_fem_contact_apply) at neighbourhood sizes 3 and 5, with the path it took and its records
            host: zero-fill + gravity, spread_haptic_forces on the handle's pattern (the Python walk), set_external_forces
            at most FB_HAPTIC_MAX_SOURCES entries: also set_uniform_force + add_haptic_forces fed the same list, pick_box(capacity 0) as its
            synchronising call
  pick_box  the read-back the host route starts from (ids and positions of the touched nodes)

Wall clock (time.perf_counter) around calls that end in a device synchronise, warm, the median of --reps repetitions with min and max."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fembrain_amd import lib as fl  # noqa: E402
from fembrain_amd.fem import FemIntegrator, ProbeContact, spread_haptic_forces  # noqa: E402
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube  # noqa: E402

GRAVITY = -10000.0
COEFF = 200000.0   # DEFAULT_HAPTIC_FORCE_COEFF of the reference's probe


def spread(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1], n=len(xs))


def timed(fn, reps, sync=None):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        out.append(time.perf_counter() - t0)
    return spread(out)


def measure(n_side, patches, reps):
    v, t = truth_cube(n_side, n_side, n_side, 0.1)
    v = np.asarray(v, np.float64).reshape(-1, 3)
    g = FemIntegrator(v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(n_side, n_side)), expect_cuts=True)
    for _ in range(2):   # (a light load: q != 0, and the top stays where a box half a cell deep holds its top layer alone)
        g.set_uniform_force(1, GRAVITY / 1000.0)
        g.do_timestep()
    bptr, bcol = g.pattern()[:2]
    rows = []
    for p in patches:
        pos = v + g.get_q_state()[0].reshape(-1, 3)
        top = np.nonzero(v[:, 1] == v[:, 1].max())[0]
        c = pos[top].mean(0)
        half = 0.05 * p + 0.04   # p nodes of spacing 0.1 around the middle, the box's sides farther from them than its bottom
        sel = top[(np.abs(pos[top, 0] - c[0]) <= half) & (np.abs(pos[top, 2] - c[2]) <= half)]
        lo = np.array([c[0] - half, pos[sel, 1].min() - 0.05, c[2] - half])   # (the loaded beam sags: the count below says what the box holds)
        hi = np.array([c[0] + half, pos[sel, 1].max() + 1.0, c[2] + half])
        g.contact_reset(keep_face=False)
        probe = ProbeContact()
        dev, host = g.contact_move(lo, hi, COEFF), probe.move(pos, lo, hi, COEFF)
        assert all(dev[k] == host[k] for k in ("status", "n_touched", "face", "closest_node", "n_pushing", "contact_dist")), (dev, host)
        n = dev["list_size"]
        assert 0 < n <= 2 * p * p, "the box holds %d nodes, not a patch of %d x %d: the Python walk below would take minutes" % (n, p, p)
        row = dict(patch=p, sources=n, pushing=dev["n_pushing"], face=dev["face"])
        row["move"] = dict(device_s=timed(lambda: g.contact_move(lo, hi, COEFF), reps),
                           host_s=timed(lambda: probe.move(v + g.get_q_state()[0].reshape(-1, 3), lo, hi, COEFF), min(reps, 5)))
        row["pick_box_readback_s"] = timed(lambda: g.pick_box(lo, hi), reps)
        row["apply"] = []
        tuples = [tuple(x) for x in probe.forces]
        ids = [int(i) for i in probe.ids]
        for size in (3, 5):
            def dev_apply():
                g.set_uniform_force(1, GRAVITY)
                return g.contact_apply(size)
            info = dev_apply()
            f = np.zeros(g.r)
            f[1::3] += GRAVITY
            spread_haptic_forces(bptr, bcol, ids, tuples, size, f)
            assert np.array_equal(g.external_forces(), f), (p, size)
            parts = dict(fill=[], walk=[], upload=[])
            for _ in range(3):
                t0 = time.perf_counter()
                f = np.zeros(g.r)
                f[1::3] += GRAVITY
                t1 = time.perf_counter()
                spread_haptic_forces(bptr, bcol, ids, tuples, size, f)
                t2 = time.perf_counter()
                g.set_external_forces(f)
                t3 = time.perf_counter()
                parts["fill"].append(t1 - t0); parts["walk"].append(t2 - t1); parts["upload"].append(t3 - t2)
            a = dict(size=size, path="records" if info["path"] == fl.FB_CONTACT_SPREAD_RECORDS else "levels", n_records=info["n_records"], n_targets=info["n_targets"],
                     device_s=timed(dev_apply, reps), host_fill_s=spread(parts["fill"]), host_walk_python_s=spread(parts["walk"]), host_upload_s=spread(parts["upload"]))
            if n <= fl.FB_HAPTIC_MAX_SOURCES:
                def dev_haptic():
                    g.set_uniform_force(1, GRAVITY)
                    g.add_haptic_forces(ids, probe.forces, size)
                dev_haptic()
                a["add_haptic_forces_s"] = timed(dev_haptic, reps, lambda: g.pick_box(lo, hi, capacity=0))
            row["apply"].append(a)
        print(json.dumps(row), flush=True)
        rows.append(row)
    g.close()
    return dict(case="cube%d" % n_side, n_nodes=int(len(v)), n_tets=int(len(t)), force_coeff=COEFF, patches=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contact_probe.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--n", type=int, default=56)
    ap.add_argument("--patches", default="12,20,32")
    a = ap.parse_args()
    row = measure(a.n, [int(p) for p in a.patches.split(",")], a.reps)
    with open(a.out, "w") as fh:
        json.dump(dict(tool="tools/probe_contact.py", reps=a.reps, timer="time.perf_counter around calls that end in a device synchronise",
                       max_sources_of_add_haptic_forces=fl.FB_HAPTIC_MAX_SOURCES, rows=[row]), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
