"""The haptic probe's device entry points against the host routes they replace, on one GPU.

    python tools/probe_haptic.py [--out profiles/haptic_probe.json] [--reps 20] [--cases 27,56]

Cases: the 27^3 and 56^3 cantilevers (cube27; 998,250 tets).  Per case, after two loaded steps:

  force set-up of one probed step, for 1, 8, 64 and 256 sources at neighbourhood size 5
    device: set_uniform_force + add_haptic_forces (fb_fem_add_haptic_forces), then pick_box with capacity 0 as the synchronising call (its
            4-byte copy waits for the stream; its own time is reported beside it as sync_call_s and is INCLUDED in device_s)
    host:   zero-fill + gravity, spread_haptic_forces on the handle's pattern (the Python walk Deformable falls back to), set_external_forces
            (which waits for its upload); the three parts are reported apart, since the upload alone bounds any host walk from below
  pick_vertex, pick_box, volume: the device call (which ends in its own small copy) against get_q_state + numpy

Wall clock (time.perf_counter) around synchronised sections, warm, the median of --reps repetitions with min and max beside it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fembrain_amd import lib as fl  # noqa: E402
from fembrain_amd.fem import FemIntegrator, spread_haptic_forces  # noqa: E402
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube  # noqa: E402

SIZE = 5
GRAVITY = -10000.0


def element_volumes(p, t):
    """|u . (v x w)| / 6 per element in fb_fem_volume's operation order"""
    u, v, w = p[t[:, 0]] - p[t[:, 3]], p[t[:, 1]] - p[t[:, 3]], p[t[:, 2]] - p[t[:, 3]]
    return np.abs((u[:, 0] * (v[:, 1] * w[:, 2] - v[:, 2] * w[:, 1]) + u[:, 1] * (v[:, 2] * w[:, 0] - v[:, 0] * w[:, 2])) + u[:, 2] * (v[:, 0] * w[:, 1] - v[:, 1] * w[:, 0])) / 6.0


def box_ids(p, lo, hi):
    return np.nonzero(((p >= lo) & (p <= hi)).all(axis=1))[0].astype(np.int32)


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


def sources(v, n):
    """n surface nodes of the free end around its middle: what a probe box touches"""
    end = np.nonzero(v[:, 0] == v[:, 0].max())[0]
    c = v[end].mean(0)
    order = end[np.argsort(((v[end] - c) ** 2).sum(1), kind="stable")]
    return [int(i) for i in order[:n]]


def measure(n_side, reps):
    v, t = truth_cube(n_side, n_side, n_side, 0.1)
    v = np.asarray(v, np.float64).reshape(-1, 3)
    g = FemIntegrator(v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(n_side, n_side)), expect_cuts=True)
    for _ in range(2):
        g.set_uniform_force(1, GRAVITY)
        g.do_timestep()
    lo, hi = v.min(0) + 0.45 * (v.max(0) - v.min(0)), v.min(0) + 0.55 * (v.max(0) - v.min(0))

    def device_sync():
        g.pick_box(lo, hi, capacity=0)
    device_sync()
    row = dict(case="cube%d" % n_side, n_nodes=int(len(v)), n_tets=int(len(t)), neighbourhood_size=SIZE, force_setup=[])
    t0 = time.perf_counter()
    bptr, bcol = g.pattern()
    row["host_pattern_fetch_s"] = time.perf_counter() - t0      # paid again after every cut by the host route
    row["sync_call_s"] = timed(device_sync, reps)
    for n in (1, 8, 64, 256):
        ids = sources(v, n)
        if len(ids) < n:
            continue
        frc = np.tile(np.array([[30.0, 2500.0, -40.0]]), (n, 1))
        tuples = [tuple(x) for x in frc]

        def dev():
            g.set_uniform_force(1, GRAVITY)
            g.add_haptic_forces(ids, frc, SIZE)
        dev()
        device_sync()
        d = timed(dev, reps, device_sync)
        parts = dict(fill=[], walk=[], upload=[])
        for _ in range(max(2, min(reps, 5 if n >= 64 else reps))):
            t0 = time.perf_counter()
            f = np.zeros(g.r)
            f[1::3] += GRAVITY
            t1 = time.perf_counter()
            spread_haptic_forces(bptr, bcol, ids, tuples, SIZE, f)
            t2 = time.perf_counter()
            g.set_external_forces(f)
            t3 = time.perf_counter()
            parts["fill"].append(t1 - t0); parts["walk"].append(t2 - t1); parts["upload"].append(t3 - t2)
        reached = int(np.count_nonzero(f[0::3]))
        row["force_setup"].append(dict(sources=n, nodes_reached=reached, device_s=d, host_fill_s=spread(parts["fill"]), host_walk_python_s=spread(parts["walk"]),
                                       host_upload_s=spread(parts["upload"]),
                                       host_total_s=spread([a + b + c for a, b, c in zip(parts["fill"], parts["walk"], parts["upload"])])))
        print(json.dumps(row["force_setup"][-1]), flush=True)
    # picking and volume at the loaded state
    w = (10.0, 0.2, 10.0)

    def host_positions():
        return v + g.get_q_state()[0].reshape(-1, 3)

    def host_pick():
        p = host_positions()
        dx = p - np.asarray(w)
        d2 = (dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1]) + dx[:, 2] * dx[:, 2]
        return int(np.argmin(d2))

    def host_box():
        return box_ids(host_positions(), lo, hi)

    def host_volume():
        return float(np.sum(element_volumes(host_positions(), t)))
    assert g.pick_vertex(w)[0] == host_pick()
    n_box, ids_d, _ = g.pick_box(lo, hi, capacity=4096)
    assert n_box == len(host_box()) and n_box <= 4096 and np.array_equal(ids_d, host_box())
    assert abs(g.volume() - host_volume()) <= 1e-9
    row["pick_vertex"] = dict(device_s=timed(lambda: g.pick_vertex(w), reps), host_s=timed(host_pick, min(reps, 10)))
    row["pick_box"] = dict(hits=n_box, device_s=timed(lambda: g.pick_box(lo, hi, capacity=4096), reps), host_s=timed(host_box, min(reps, 10)))
    row["volume"] = dict(device_s=timed(g.volume, reps), device_with_elements_s=timed(lambda: g.volume(per_element=True), reps), host_s=timed(host_volume, min(reps, 10)))
    row["get_q_state_s"] = timed(lambda: g.get_q_state(), min(reps, 10))
    g.close()
    print(json.dumps({k: row[k] for k in ("case", "pick_vertex", "pick_box", "volume", "get_q_state_s")}), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "haptic_probe.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cases", default="27,56")
    a = ap.parse_args()
    rows = [measure(int(n), a.reps) for n in a.cases.split(",")]
    with open(a.out, "w") as fh:
        json.dump(dict(tool="tools/probe_haptic.py", reps=a.reps, timer="time.perf_counter around synchronised sections", max_sources=fl.FB_HAPTIC_MAX_SOURCES, rows=rows),
                  fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
