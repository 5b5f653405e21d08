"""What fb_fem_tool_contact costs at 1M tets, against the route a caller had before it.

    python tools/probe_tool_contact.py [--out profiles/tool_contact_probe.json] [--n 56] [--reps 9]

The n^3 cantilever at a state that is not zero, and a tool of a capsule with a sphere at its tip and an oriented box, pressed into the
top face.  For the surface vertices and for all nodes, without and with friction:
  stages   fb_fem_time_tool_contact's three stages (points against shapes | compaction and the host wait | forces and the records' way
           back), means of --reps
  call     one fb_fem_tool_contact by wall clock, the median of --reps
Yardstick, measured in the same run (frictionless, surface vertices):
  host     surface() + get_q_state() + the rule in vectorised numpy (the operations of tests/toolref.py in the same order, array-wise) +
           set_external_forces: what a caller did before the call existed.  Its force vector is compared with the call's, bit for bit."""
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

K = 5000.0
STAGES = ("points_against_shapes", "compaction_and_wait", "forces_and_records")


def median(xs):
    return sorted(xs)[len(xs) // 2]


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _sphere(P, c, r):
    u = [P[:, k] - c[k] for k in range(3)]
    l2 = _dot(u, u)
    held = l2 <= r * r
    l = np.sqrt(l2)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.stack([u[k] / l for k in range(3)], axis=1)
    return held, np.where(l == 0, r, r - l), np.where((l == 0)[:, None], 0.0, n), l == 0


def shape_numpy(shape, P):
    """(held, depth, normal, degenerate) of one shape at the points P, the rule's operations array-wise"""
    a = np.asarray(shape[1], np.float64)
    if shape[0] == "sphere":
        return _sphere(P, a, float(shape[2]))
    if shape[0] == "capsule":
        b, r = np.asarray(shape[2], np.float64), float(shape[3])
        d = b - a
        dd = _dot(d, d)
        u = [P[:, k] - a[k] for k in range(3)]
        t = np.minimum(np.maximum(_dot(u, d) / dd, 0.0), 1.0) if dd > 0 else np.zeros(len(P))
        c = [a[k] + t * d[k] for k in range(3)]
        return _sphere(P, c, r)
    half = np.asarray(shape[2], np.float64)
    R = np.eye(3) if len(shape) < 4 or shape[3] is None else np.asarray(shape[3], np.float64).reshape(3, 3)
    u = [P[:, k] - a[k] for k in range(3)]
    l = np.stack([_dot(R[i], u) for i in range(3)], axis=1)
    e = half[None, :] - np.abs(l)
    held = (np.abs(l) <= half[None, :]).all(axis=1)
    axis = np.argmin(e, axis=1)     # (the first of equal ones)
    rows = np.arange(len(P))
    n = np.where((l[rows, axis] < 0)[:, None], -R[axis], R[axis])
    return held, e[rows, axis], n, np.zeros(len(P), bool)


def host_rule(x, q, vids, shapes, stiffness, f):
    """the frictionless rule on the surface vertices, added into f (3 n); returns the number of contacts"""
    P = x[vids] + q.reshape(-1, 3)[vids]
    best = np.full(len(P), -1.0)
    found = np.zeros(len(P), bool)
    normal, degenerate = np.zeros((len(P), 3)), np.zeros(len(P), bool)
    for shape in shapes:
        held, depth, n, deg = shape_numpy(shape, P)
        take = held & (~found | (depth > best))
        best[take], normal[take], degenerate[take] = depth[take], n[take], deg[take]
        found |= held
    push = found & ~degenerate
    F = (stiffness * best[push])[:, None] * normal[push]
    f.reshape(-1, 3)[vids[push]] += F
    return int(found.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tool_contact_probe.json"))
    ap.add_argument("--n", type=int, default=56)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    n, h = a.n, 0.1
    v, t = truth_cube(n, n, n, h)
    v = np.asarray(v, np.float64).reshape(-1, 3)
    g = FemIntegrator(v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n)))
    n_nodes, n_tets = len(v), int(g.num_tets())
    rng = np.random.default_rng(2)
    g.set_q_state(0.002 * rng.standard_normal(3 * n_nodes), 0.2 * rng.standard_normal(3 * n_nodes))
    top, mid = v[:, 1].max(), 0.5 * (v.min(0) + v.max(0))
    cz, sz = np.cos(0.3), np.sin(0.3)
    tip = np.array([mid[0], top + 0.45, mid[2]])
    shapes = [("sphere", tuple(tip), 0.6), ("capsule", tuple(tip), tuple(tip + [-0.4, 1.5, 0.2]), 0.4),
              ("box", (mid[0] + 1.2, top + 0.1, mid[2] - 0.8), (0.5, 0.25, 0.4), [[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])]
    frame = dict(origin=tuple(tip), velocity=(0.3, -0.2, 0.1), omega=(0.5, 1.0, -0.7))
    nv = len(g.surface()["vertex_ids"])
    print("%d tets on %d nodes, %d surface vertices" % (n_tets, n_nodes, nv), flush=True)
    out = {}
    for points in ("surface", "all_nodes"):
        for name, kw in (("frictionless", {}), ("friction", dict(mu=0.4, slip_speed=0.3, damping=20.0))):
            g.set_external_forces_to_zero()
            c = g.tool_contact(shapes, K, points=points, **frame, **kw)   # (warm: buffers, code objects, the surface)
            walls = []
            for _ in range(a.reps):
                g.set_external_forces_to_zero()
                t0 = time.perf_counter()
                c = g.tool_contact(shapes, K, points=points, **frame, **kw)
                walls.append(time.perf_counter() - t0)
            stages = g.time_tool_contact(shapes, K, points=points, reps=a.reps, **frame, **kw)
            key = "%s_%s" % (points, name)
            out[key] = dict(call_seconds=median(walls), call_all=walls, stages_seconds=dict(zip(STAGES, [float(s) for s in stages])), stages_total_seconds=float(stages.sum()),
                            n_points=c["n_points"], n_contacts=c["n_contacts"], contacts_by_shape=[int(k) for k in c["contacts_by_shape"]], max_depth=c["max_depth"])
            print("  %-24s call %.3f ms; stages (ms) %s; %d contacts of %d points" % (key, 1e3 * median(walls), " ".join("%.3f" % (1e3 * s) for s in stages), c["n_contacts"],
                                                                                        c["n_points"]), flush=True)
    # the host route, and its vector against the call's
    g.set_external_forces_to_zero()
    g.tool_contact(shapes, K, **frame)
    f_call = g.external_forces()
    host = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        vids = g.surface()["vertex_ids"]
        q = g.get_q_state()[0]
        t1 = time.perf_counter()
        f = np.zeros(3 * n_nodes)
        n_host = host_rule(v, q, vids, shapes, K, f)
        t2 = time.perf_counter()
        g.set_external_forces(f)
        t3 = time.perf_counter()
        host.append((t3 - t0, t1 - t0, t2 - t1, t3 - t2))
    same = bool(np.array_equal(f.view(np.uint64), f_call.view(np.uint64)))
    hm = sorted(host)[len(host) // 2]
    out["host_route"] = dict(seconds=hm[0], read_back_seconds=hm[1], numpy_seconds=hm[2], upload_seconds=hm[3], n_contacts=n_host, same_bits_as_the_call=same)
    out["host_over_call"] = hm[0] / out["surface_frictionless"]["call_seconds"]
    print("  host route %.3f ms: read back %.3f, numpy %.3f, upload %.3f; %d contacts, same bits %s; %.1f x the call" % (
        1e3 * hm[0], 1e3 * hm[1], 1e3 * hm[2], 1e3 * hm[3], n_host, same, out["host_over_call"]), flush=True)
    g.close()
    res = dict(tool="tools/probe_tool_contact.py", mesh="cube %d^3, a sphere-tipped capsule and an oriented box pressed into the top face" % n, reps=a.reps, stiffness=K,
               sizes=dict(n_tets=n_tets, n_nodes=n_nodes, surface_vertices=nv), results=out, kernel_sources_sha256=fl.source_sha256("fem"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)
    assert same and n_host == out["surface_frictionless"]["n_contacts"]


if __name__ == "__main__":
    main()
