"""What labelling the disjoint parts on the device costs beside the host route it replaces, on one GPU.

    python tools/probe_parts.py [--out profiles/parts_probe.json] [--n 56] [--reps 20] [--rounds 5] [--trace]

The n^3 cantilever (56: 998,250 tets) after a mid-span cut: two parts.  fb_fem_time_parts -- the median of --reps HIP-event timings of
a forced labelling (face sort, hooking, flatten, per-part table, node labels; host waits included) and of a split's device work --
--rounds such medians as the spread, beside fb_fem_time_surface's build figure on the same handle (the same face sort).  And, by wall
clock in the same run, once: the host route, read_mesh() + tests/cutref.py face_components(), with the transfer share of it.
--trace: the cut and two labellings (the second warm) and nothing else, for a kernel-trace run of its own; tools/show_parts_trace.py
lists the dispatches of the last labelling from that run's kernel trace."""
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
from fembrain_amd import lib as fl  # noqa: E402
from fembrain_amd.fem import FemIntegrator  # noqa: E402
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1], n=len(xs))


def mid_span_strip(v, n):
    """a blade across mid-span, in the middle of a grid cell and tilted too little to reach a node plane"""
    xs = np.unique(v[:, 0])
    k = len(xs) // 2
    p = np.array([0.5 * (xs[k - 1] + xs[k]), 0.5 * (v[:, 1].min() + v[:, 1].max()), 0.5 * (v[:, 2].min() + v[:, 2].max())])
    return cr.plane_strip(p, (1.0, 0.013, 0.007), half=4.0 * n * 0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parts_probe.json"))
    ap.add_argument("--n", type=int, nargs="+", default=[56])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="leave the host route out (a profiler run)")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    if a.trace:
        n = a.n[0]
        v, t = truth_cube(n, n, n, 0.1)
        g = FemIntegrator(v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n)))
        info, _ = g.cut(mid_span_strip(v, n), track=False)
        assert info["status"] == fl.FB_CUT_DONE, info
        g.parts()
        print("labelling", g.time_parts(1)[0], "s;", g.parts(), flush=True)
        g.close()
        return
    name, arch, cus = fl.C.create_string_buffer(128), fl.C.create_string_buffer(64), fl.C.c_int(0)
    fl.lib().fb_device_info(0, name, 128, arch, 64, fl.C.byref(cus))
    device = name.value.decode() or arch.value.decode()   # (a runtime that reports no marketing name: the architecture string says what it ran on)
    if not device:
        raise RuntimeError("the device reports neither a name nor an architecture: the profile would not say what it was taken on")
    out = dict(tool="tools/probe_parts.py", device=device, arch=arch.value.decode(), reps=a.reps, rounds=a.rounds,
               kernel_sources_sha256=fl.source_sha256("fem"), meshes=[])
    for n in a.n:
        v, t = truth_cube(n, n, n, 0.1)
        g = FemIntegrator(v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n)))
        t0 = time.perf_counter()
        info, _ = g.cut(mid_span_strip(v, n), track=False)
        cut_s = time.perf_counter() - t0
        assert info["status"] == fl.FB_CUT_DONE, info
        parts = g.parts()
        label, split, build = [], [], []
        for _ in range(a.rounds):
            la, sp = g.time_parts(a.reps)
            b, _ = g.time_surface(a.reps)
            label.append(la); split.append(sp); build.append(b)
        rec = dict(mesh="cube %d^3 after a mid-span cut" % n, n_tets=int(fl.lib().fb_fem_num_tets(g.h)), n_nodes=int(fl.lib().fb_fem_num_nodes(g.h)),
                   parts=parts, part_elements=g.part_table()["elements"].tolist(), cut_wall_seconds=cut_s,
                   label_seconds=spread(label), split_seconds=spread(split), surface_build_seconds=spread(build))
        if not a.no_host:
            t0 = time.perf_counter()
            x, tt = g.read_mesh()
            t1 = time.perf_counter()
            roots = cr.face_components(tt)
            t2 = time.perf_counter()
            assert len(np.unique(roots)) == parts["n_parts"]
            rec.update(host_route_seconds=t2 - t0, host_route_transfer_seconds=t1 - t0, host_route_bytes=int(x.nbytes + tt.nbytes))
        g.close()
        print("%s: %d tets, %d parts %s; labelling %.1f us, split %.1f us, surface build %.1f us%s"
              % (rec["mesh"], rec["n_tets"], parts["n_parts"], rec["part_elements"], 1e6 * rec["label_seconds"]["median"], 1e6 * rec["split_seconds"]["median"],
                 1e6 * rec["surface_build_seconds"]["median"],
                 "" if a.no_host else "; host route %.2f s (%.1f ms of it transfers)" % (rec["host_route_seconds"], 1e3 * rec["host_route_transfer_seconds"])), flush=True)
        out["meshes"].append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
