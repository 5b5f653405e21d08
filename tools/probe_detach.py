"""What detaching a part on the device costs beside the host route it replaces, on one GPU.

    python tools/probe_detach.py [--out profiles/detach_probe.json] [--n 56] [--reps 5]

The n^3 cantilever (56: 998,250 tets) with a two-material map, loaded, stepped and cut at mid-span with FB_CUT_CARRY: two parts.  By wall
clock, the median of --reps each, every piece destroyed before the next is made:
  keep     fb_fem_detach_part(FB_DETACH_KEEP) of the free part
  remove   fb_fem_detach_part(FB_DETACH_REMOVE) of it (a fresh cut parent per repetition: the removal changes it)
  host     the route it replaces: read_part + fb_fem_create + set_state + set_materials / set_element_materials + set_external_forces
  build    the floor of all three: the piece built again from its own device mesh by the full builder (an empty fb_fem_resync_delta under
           FEMBRAIN_RESYNC_DELTA=rebuild), i.e. the plan build without the hand-over"""
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
import detachref as dr  # noqa: E402
from fembrain_amd import lib as fl  # noqa: E402
from fembrain_amd.fem import FemIntegrator  # noqa: E402
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube  # noqa: E402

MATS = ([1e7, 3e6], [0.46, 0.40], [1000.0, 1200.0])


def median(xs):
    return sorted(xs)[len(xs) // 2]


def cut_parent(v, t, fixed, n):
    g = FemIntegrator(v, t, fixed, expect_cuts=True)
    g.set_materials(*MATS, element_ids=np.arange(len(t)) % 2)
    g.set_uniform_force(1, -3000.0)
    g.do_timestep()
    xs = np.unique(v[:, 0])
    k = len(xs) // 2
    p = np.array([0.5 * (xs[k - 1] + xs[k]), 0.5 * (v[:, 1].min() + v[:, 1].max()), 0.5 * (v[:, 2].min() + v[:, 2].max())])
    info, _ = g.cut(cr.plane_strip(p, (1.0, 0.013, 0.007), half=4.0 * n * 0.1), mode="carry", track=False)
    assert info["status"] == fl.FB_CUT_DONE, info
    assert g.parts()["n_parts"] == 2
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detach_probe.json"))
    ap.add_argument("--n", type=int, default=56)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n = a.n
    v, t = truth_cube(n, n, n, 0.1)
    v = np.asarray(v, np.float64).reshape(-1, 3)
    fixed = fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n))
    g = cut_parent(v, t, fixed, n)
    free = 1 - int(g.element_parts()[0])
    fext = np.zeros(g.r)
    fext[1::3] = -3000.0
    g.set_external_forces(fext)
    keep, host, build = [], [], []
    for _ in range(a.reps + 1):   # (the first repetition warms the allocator and the kernels up and is dropped)
        t0 = time.perf_counter()
        piece, ids, nodes = g.detach_part(free, track=False)
        keep.append(time.perf_counter() - t0)
        os.environ["FEMBRAIN_RESYNC_DELTA"] = "rebuild"
        pf = piece.constrained_dofs()
        t0 = time.perf_counter()
        piece.resync_delta({}, fixed_dofs=pf, track=False)
        build.append(time.perf_counter() - t0)
        del os.environ["FEMBRAIN_RESYNC_DELTA"]
        sizes = dict(n_tets=int(piece.num_tets()), n_nodes=int(piece._L.fb_fem_num_nodes(piece.h)))
        piece.close()
        t0 = time.perf_counter()
        ids, nodes, xyz, tl = g.read_part(free)
        q, qv, _ = g.get_q_state()
        ref = dr.detach(ids, nodes, xyz, tl, fixed_dofs=fixed, vectors=dict(q=q, qvel=qv, fext=fext), material_ids=g.element_materials())
        twin = FemIntegrator(ref["xyz"], ref["tets"], ref["fixed"], expect_cuts=True)
        twin.set_q_state(ref["q"], ref["qvel"])
        twin.set_materials(*MATS)
        twin.set_element_materials(ref["materials"])
        twin.set_external_forces(ref["fext"])
        host.append(time.perf_counter() - t0)
        twin.close()
    g.close()
    remove, paths = [], []
    for _ in range(a.reps):
        g = cut_parent(v, t, fixed, n)
        g.set_external_forces(fext)
        t0 = time.perf_counter()
        piece, _, _ = g.detach_part(free, remove=True, track=False)
        remove.append(time.perf_counter() - t0)
        paths.append(piece.detach_info["parent_resync_path"])
        piece.close()
        g.close()
    out = dict(tool="tools/probe_detach.py", mesh="cube %d^3 after a mid-span cut, the free part" % n, reps=a.reps, piece=sizes,
               keep_seconds=median(keep[1:]), remove_seconds=median(remove), host_route_seconds=median(host[1:]), plan_build_seconds=median(build[1:]),
               all=dict(keep=keep, remove=remove, host=host, build=build), parent_resync_paths=paths, kernel_sources_sha256=fl.source_sha256("fem"))
    print("piece of %d tets on %d nodes: detach keep %.1f ms, remove %.1f ms, host route %.1f ms; the plan build alone %.1f ms (%.0f %% of keep)"
          % (sizes["n_tets"], sizes["n_nodes"], 1e3 * out["keep_seconds"], 1e3 * out["remove_seconds"], 1e3 * out["host_route_seconds"],
             1e3 * out["plan_build_seconds"], 100.0 * out["plan_build_seconds"] / out["keep_seconds"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
