"""What a per-element material map costs, on one GPU.

    python tools/probe_materials.py [--out profiles/materials_probe.json] [--n 56] [--reps 20] [--rounds 5]

The n^3 cantilever (56: 998,250 tets), one handle without a map and one with three materials by region (the region function of
tests/matref.py), in the same run.  Per handle: fb_fem_time_assembly (k_tet_warp + the element-major assembly of a step; HIP events, warm)
and one rebuild of the mass entries (mass(): k_mass_blocks' sums through the slot-major kernel, with the read-back, wall clock) -- the
median of --reps repetitions, --rounds such medians as the spread."""
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


def three_materials():
    """[(E, nu, rho)] * 3: the `default` and `soft_damped` sets of tests/fem_params.py and a stiff light one (tests/matref.py)"""
    return [(1e7, 0.46, 1000.0), (2.5e5, 0.30, 1200.0), (5e7, 0.2, 800.0)]


def region_ids(verts, tets):
    """ids = min(2, [cx > mean] + 2 [cy > mean and cz > mean]) over element centroids (tests/matref.py)"""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    c, m = v[np.asarray(tets).reshape(-1, 4)].mean(axis=1), v.mean(axis=0)
    return np.minimum(2, (c[:, 0] > m[0]).astype(np.int64) + 2 * ((c[:, 1] > m[1]) & (c[:, 2] > m[2]))).astype(np.uint8)


def spread(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1], n=len(xs))


def measure(g, reps, rounds):
    g.set_uniform_force(1, -1000.0)
    g.do_timestep()
    asm, mass = [], []
    for _ in range(rounds):
        asm.append(sorted(g.time_assembly(1) for _ in range(reps))[reps // 2])
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            g.mass()
            ts.append(time.perf_counter() - t0)
        mass.append(sorted(ts)[reps // 2])
    return dict(assembly_seconds=spread(asm), mass_rebuild_seconds=spread(mass), assembly_kernel=int(fl.lib().fb_fem_assembly_kernel(g.h)),
                element_map_bytes=g.element_map_bytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "materials_probe.json"))
    ap.add_argument("--n", type=int, default=56)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    v, t = truth_cube(a.n, a.n, a.n, 0.1)
    fixed = fixed_vertices_to_dofs(cube_fixed_plane_i0(a.n, a.n))
    mats = three_materials()
    ids = region_ids(v, t)
    out = dict(n=a.n, tets=int(len(t)), nodes=int(len(v)), reps=a.reps, rounds=a.rounds, materials=mats, elements_per_material=np.bincount(ids).tolist(),
               source_sha256=fl.source_sha256("fem"), cases={})
    for name in ("uniform", "three_materials", "uniform_again"):   # (the uniform handle before and after: drift of the machine shows)
        g = FemIntegrator(v, t, fixed, E=mats[0][0], nu=mats[0][1], rho=mats[0][2], matrix_precision=fl.FB_MATRIX_F32)
        if name == "three_materials":
            g.set_materials(*zip(*mats), element_ids=ids)
        out["cases"][name] = measure(g, a.reps, a.rounds)
        g.close()
        print(name, json.dumps(out["cases"][name]))
    u, m = out["cases"]["uniform"], out["cases"]["three_materials"]
    out["assembly_ratio"] = m["assembly_seconds"]["median"] / u["assembly_seconds"]["median"]
    out["mass_ratio"] = m["mass_rebuild_seconds"]["median"] / u["mass_rebuild_seconds"]["median"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("assembly x%.3f, mass rebuild x%.3f -> %s" % (out["assembly_ratio"], out["mass_ratio"], a.out))


if __name__ == "__main__":
    main()
