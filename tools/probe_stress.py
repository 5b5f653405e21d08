"""What element stress on the device costs beside the host route it replaces, on one GPU.

    python tools/probe_stress.py [--out profiles/stress_probe.json] [--n 27 56] [--reps 20] [--rounds 5] [--steps 3]

The n^3 cantilevers (27: 105,456 tets, 56: 998,250) after a few loaded steps, one handle without an element map and one with three
materials by region, in the same run.  Per handle: fb_fem_time_stress -- the median of --reps HIP-event timings of fb_fem_stress (the
element kernel, the fold and the 48-byte copy) without and with FB_STRESS_TENSORS, and of fb_fem_surface_stress (the vertex kernel and
its 4 n_vertices bytes) -- --rounds such medians as the spread.  And, by wall clock in the same run, the host route: get_q_state() +
read_mesh() + the numpy restatement of the same tensors (vectorised over the elements: F, the rotation from numpy's SVD, H, the stress of
every element's own material, von Mises, psi, J), with the transfer share of it."""
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
    return [(1e7, 0.46, 1000.0), (2.5e5, 0.30, 1200.0), (5e7, 0.2, 800.0)]


def region_ids(verts, tets):
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    c, m = v[np.asarray(tets).reshape(-1, 4)].mean(axis=1), v.mean(axis=0)
    return np.minimum(2, (c[:, 0] > m[0]).astype(np.int64) + 2 * ((c[:, 1] > m[1]) & (c[:, 2] > m[2]))).astype(np.uint8)


def lame(E, nu):
    return (nu * E) / ((1 + nu) * (1 - 2 * nu)), E / (2 * (1 + nu))


def host_stress(x, t, q, lam, mu):
    """the tensors of include/fembrain_hip.h for every element at once (rotation: U V^T of the SVD of F, negated where det F < 0, as
    the assembly's flipped rotation).  Returns (von Mises, psi, J)."""
    X = x[t]                                              # (m, 4, 3)
    P = X + q.reshape(-1, 3)[t]
    Dm = np.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0], X[:, 3] - X[:, 0]], axis=2)
    Di = np.linalg.inv(Dm)                                # rows: b_1, b_2, b_3
    b = np.concatenate([-Di.sum(axis=1, keepdims=True), Di], axis=1)     # (m, 4, 3)
    F = np.einsum("mki,mkj->mij", P, b)
    U, _, Vt = np.linalg.svd(F)
    R = U @ Vt
    R[np.linalg.det(F) < 0] *= -1.0                       # (U V^T has determinant -1 there; the assembly's flipped R has +1)
    y = np.einsum("mia,mki->mka", R, P) - X               # R^T P_k - X_k
    H = np.einsum("mka,mkc->mac", y, b)
    tr = np.trace(H, axis1=1, axis2=2)
    Hs = H + np.swapaxes(H, 1, 2)
    S = mu[:, None, None] * Hs + (lam * tr)[:, None, None] * np.eye(3)
    d = np.stack([S[:, 0, 0] - S[:, 1, 1], S[:, 1, 1] - S[:, 2, 2], S[:, 2, 2] - S[:, 0, 0]], axis=1)
    vm = np.sqrt(0.5 * (d ** 2).sum(axis=1) + 3.0 * (S[:, 0, 1] ** 2 + S[:, 1, 2] ** 2 + S[:, 2, 0] ** 2))
    psi = 0.25 * np.einsum("mac,mac->m", S, Hs)
    return vm, psi, np.linalg.det(F)


def spread(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1], n=len(xs))


def measure(g, mats, ids, reps, rounds, steps):
    for _ in range(steps):
        g.set_uniform_force(1, -1000.0)
        g.do_timestep()
    plain, tens, surf = [], [], []
    for _ in range(rounds):
        a, s = g.time_stress(reps)
        b, _ = g.time_stress(reps, tensors=True)
        plain.append(a); tens.append(b); surf.append(s)
    # the host route, same run
    lam, mu = (np.array([lame(m[0], m[1])[k] for m in mats])[ids] for k in (0, 1))
    total, moved = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        q = g.get_q_state()[0]
        x, t = g.read_mesh()
        t1 = time.perf_counter()
        vm, psi, J = host_stress(x, t, q, lam, mu)
        t2 = time.perf_counter()
        total.append(t2 - t0); moved.append(t1 - t0)
    info = g.stress()
    dev = g.element_stress()
    scale = (3 * lam + 2 * mu)
    return dict(n_tets=int(info["n_elements"]), n_surface_vertices=int(len(g.surface()["vertex_ids"])), element_map_bytes=g.element_map_bytes(),
                stress_seconds=spread(plain), stress_tensors_seconds=spread(tens), surface_stress_seconds=spread(surf),
                host_route_seconds=spread(total), host_route_transfer_seconds=spread(moved),
                host_route_bytes=int(q.nbytes * 3 + x.nbytes + t.nbytes),    # get_q_state brings q, qvel and qaccel
                device_against_host=dict(von_mises_over_scale=float((np.abs(dev["von_mises"] - vm) / scale).max()),
                                         J_relative=float((np.abs(dev["J"] - J) / np.abs(J)).max()),
                                         psi_of_largest=float(np.abs(dev["energy_density"] - psi).max() / np.abs(psi).max())),
                summary={k: info[k] for k in ("max_von_mises", "max_element", "min_J", "min_J_element", "n_inverted", "energy")})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stress_probe.json"))
    ap.add_argument("--n", type=int, nargs="+", default=[27, 56])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    name = fl.C.create_string_buffer(128)
    arch = fl.C.create_string_buffer(64)
    cus = fl.C.c_int(0)
    fl.lib().fb_device_info(0, name, 128, arch, 64, fl.C.byref(cus))
    out = dict(tool="tools/probe_stress.py", device=name.value.decode(), arch=arch.value.decode(), reps=a.reps, rounds=a.rounds, loaded_steps=a.steps,
               kernel_sources_sha256=fl.source_sha256("fem"), meshes=[])
    for n in a.n:
        v, t = truth_cube(n, n, n, 0.1)
        fixed = fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n))
        rec = dict(mesh="cube %d^3" % n)
        g = FemIntegrator(v, t, fixed)
        rec["uniform"] = measure(g, [(1e7, 0.46, 1000.0)], np.zeros(len(t), np.uint8), a.reps, a.rounds, a.steps)
        g.close()
        mats, ids = three_materials(), region_ids(v, t)
        g = FemIntegrator(v, t, fixed)
        g.set_materials(*zip(*mats), element_ids=ids)
        rec["three_materials"] = measure(g, mats, ids, a.reps, a.rounds, a.steps)
        g.close()
        for k in ("uniform", "three_materials"):
            r = rec[k]
            print("%s %s: stress %.1f us, with tensors %.1f us, surface %.1f us; host route %.1f ms (%.1f ms of it transfers)"
                  % (rec["mesh"], k, 1e6 * r["stress_seconds"]["median"], 1e6 * r["stress_tensors_seconds"]["median"],
                     1e6 * r["surface_stress_seconds"]["median"], 1e3 * r["host_route_seconds"]["median"], 1e3 * r["host_route_transfer_seconds"]["median"]), flush=True)
        out["meshes"].append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
