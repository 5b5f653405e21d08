"""fb_fem_cut at 1M tets: the 56^3-node cantilever (998,250 tets), cut through at mid-span, at rest and after 5 steps.

    python tools/probe_fem_cut.py [--out profiles/fem_cut_probe.json] [--reps 3] [--trace]

Reports per case: the subdivision stage alone (a dry run: cut codes, compaction, unique cut edges, pieces -- steps 1-4), the whole
fb_fem_cut (a fresh handle per repetition), fb_fem_resync_delta fed the same delta from the host on a twin handle, the host route
(the numpy restatement of tests/cutref.py + fb_fem_resync_delta), and which re-sync path each took.  Wall-clock seconds of the
calls, which synchronise before they return.  --trace: one cut only (for a kernel-trace run of its own)."""
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
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube  # noqa: E402
import cutref as cr  # noqa: E402

N = 56


def mesh():
    v, t = truth_cube(N, N, N, 0.1)
    return v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(N, N))


def strip_for(v):
    xs = np.unique(v[:, 0])
    k = len(xs) // 2
    p = np.array([0.5 * (xs[k - 1] + xs[k]), 0.5 * (v[:, 1].min() + v[:, 1].max()), 0.5 * (v[:, 2].min() + v[:, 2].max())])
    return cr.plane_strip(p, (1.0, 0.013, 0.007), half=20.0)


def handle(v, t, fixed, steps):
    g = FemIntegrator(v, t, fixed, expect_cuts=True)
    for _ in range(steps):
        g.set_uniform_force(1, -10000.0)
        g.do_timestep()
    return g


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fem_cut_probe.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    v, t, fixed = mesh()
    strip = strip_for(v)
    if a.trace:
        g = handle(v, t, fixed, 0)
        info, _ = g.cut(strip, modify=False, track=False)
        info, _ = g.cut(strip, track=False)
        print(json.dumps(info))
        return
    rec = {"mesh": "truth_cube %d^3 nodes, %d tets, cantilever clamped at x = 0" % (N, len(t)), "cases": []}
    for steps in (0, 5):
        case = {"steps_before_cut": steps, "dry_s": [], "cut_s": [], "resync_delta_s": [], "host_route_s": [], "host_restatement_s": []}
        for rep in range(a.reps):
            g = handle(v, t, fixed, steps)
            g.cut(strip, modify=False, track=False)  # (the first launch of the cut kernels in the process)
            dt, (info, d) = timed(lambda: g.cut(strip, modify=False, track=False))
            case["dry_s"].append(dt)
            dt, (info, d) = timed(lambda: g.cut(strip, track=False))
            case["cut_s"].append(dt)
            case["cut_path"] = g.resync_path()
            case["info"] = info
            # the same delta from the host on a twin (the rest shape baked from its state, as the cut does)
            twin = handle(v, t, fixed, steps)
            x0, tt = twin.read_mesh()
            q = twin.get_q_state()[0].reshape(-1, 3)
            twin.resync(x0 + q, tt, fixed)  # (the state is reset: the delta below starts from the baked rest shape)
            dt, _ = timed(lambda: twin.resync_delta(d, fixed, track=False))
            case["resync_delta_s"].append(dt)
            case["resync_delta_path"] = twin.resync_path()
            twin.close()
            # the host route: restatement + fb_fem_resync_delta
            host = handle(v, t, fixed, steps)
            t0 = time.perf_counter()
            x0, tt = host.read_mesh()
            q = host.get_q_state()[0]
            e = cr.cut(x0, tt, strip, q)
            t1 = time.perf_counter()
            host.resync(x0 + q.reshape(-1, 3), tt, fixed)
            t2 = time.perf_counter()
            host.resync_delta(e, fixed, track=False)
            t3 = time.perf_counter()
            case["host_restatement_s"].append(t1 - t0)
            case["host_route_s"].append((t1 - t0) + (t3 - t2))
            host.close()
            g.close()
        for k in ("dry_s", "cut_s", "resync_delta_s", "host_route_s", "host_restatement_s"):
            case[k.replace("_s", "_ms_median")] = 1e3 * float(np.median(case[k]))
        rec["cases"].append(case)
        print(json.dumps({k: case[k] for k in case if not k.endswith("_s")}))
    rec["source_sha256"] = fl.source_sha256()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
