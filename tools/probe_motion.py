"""What constrained motion (fb_fem_set_constrained_motion / fb_fem_grasp) costs at 1M tets.

    python tools/probe_motion.py [--out profiles/motion_probe.json] [--n 56] [--reps 9] [--bench LABEL=FILE ...]

The n^3 cantilever (n = 56: 998,250 tets), clamped at plane i = 0, gravity as a uniform force, with two grasps of its far plane:
  patch    the 8 x 8 nodes in the middle of the far plane (64 nodes)
  plane    the whole far plane (n^2 nodes)
For each: the element table (listed elements, touched nodes, longest run of one node), fb_fem_time_motion's four stages (table build |
right-hand-side correction | reactions | write of the moved DOFs; means of --reps, a host wait each), and the time of fb_fem_step
with the grasp held still against the same handle before the grasp -- medians of --reps steps by wall clock around the call, which ends
in a wait for the device, warmed, in the same process.  The held nodes sit at their targets, so the set costs its kernels and changes
nothing else about the solve.
--bench LABEL=FILE: the JSON result line of a ``bench.py`` run is copied into the output under ``bench[LABEL]`` (the headline workload has
no motion set and runs no kernel of motion.hip: its runs on this commit and on its parent belong in the same file)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fembrain_amd import lib as fl  # noqa: E402
from fembrain_amd.fem import FemIntegrator  # noqa: E402
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube  # noqa: E402

STAGES = ("table_build", "correction", "reactions", "apply")


def median(xs):
    return sorted(xs)[len(xs) // 2]


def step_times(g, reps):
    out = []
    for _ in range(reps):
        g.set_uniform_force(1, -100.0)
        t0 = time.perf_counter()
        g.do_timestep()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_probe.json"))
    ap.add_argument("--n", type=int, default=56)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--bench", action="append", default=[], metavar="LABEL=FILE")
    a = ap.parse_args()
    n = a.n
    v, t = truth_cube(n, n, n, 0.1)
    far = np.arange(n * n * (n - 1), n ** 3, dtype=np.int32).reshape(n, n)
    lo = max(0, n // 2 - 4)
    grasps = {"patch": np.sort(far[lo:lo + 8, lo:lo + 8].reshape(-1)), "plane": far.reshape(-1)}
    g = FemIntegrator(v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n)))
    for _ in range(3):   # warm, and a state that is not the rest state
        g.set_uniform_force(1, -100.0)
        g.do_timestep()
    out = {}
    for name, nodes in grasps.items():
        before = step_times(g, a.reps)
        builds0 = g.motion_info()["table_builds"]
        info = g.grasp(nodes)
        g.set_uniform_force(1, -100.0)
        g.do_timestep()   # (builds the table, loads the kernels)
        held = step_times(g, a.reps)
        stages = g.time_motion(reps=a.reps)
        mi = g.motion_info()
        lam, s3 = g.reactions()
        out[name] = dict(nodes=int(len(nodes)), n_dofs=mi["n_dofs"], listed_elements=mi["n_listed_elements"], touched_nodes=mi["n_touched_nodes"], longest_run=mi["longest_run"],
                         table_builds=mi["table_builds"] - builds0, stages_seconds=dict(zip(STAGES, [float(x) for x in stages])),
                         step_seconds_without=median(before), step_seconds_with=median(held), step_all_without=before, step_all_with=held,
                         iterations_last=int(g.last.cg_iterations), reaction_sum=[float(x) for x in s3], n_dofs_at_grasp=info["n_dofs"])
        print("  %-5s %5d nodes: %d elements listed, %d nodes touched, longest run %d; stages (ms) %s; step %.3f ms held, %.3f ms before" % (
            name, len(nodes), mi["n_listed_elements"], mi["n_touched_nodes"], mi["longest_run"], " ".join("%.3f" % (1e3 * x) for x in stages),
            1e3 * median(held), 1e3 * median(before)), flush=True)
        g.release()
    sizes = dict(n_tets=int(g.num_tets()), n_nodes=int(len(v)))
    g.close()
    bench = {}
    for item in a.bench:
        label, path = item.split("=", 1)
        with open(path) as f:
            lines = [w for w in f.read().splitlines() if w.startswith("{")]
        bench[label] = json.loads(lines[-1])
    res = dict(tool="tools/probe_motion.py", mesh="cube %d^3, clamped at plane i = 0, the far plane grasped and held still" % n, reps=a.reps, sizes=sizes, results=out, bench=bench,
               kernel_sources_sha256=fl.source_sha256("fem"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
