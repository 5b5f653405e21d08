"""Records what the persistent one-row kernels with an LDS window (k_pcg_pipe<float,c16|c32,12,6|7>) compute, bit for bit, on small
meshes confined to one XCD (FEMBRAIN_CU_MASK=0:32: 32 workgroups, so ~20k nodes are 9..12 slices per workgroup).

Run on an MI355X at the commit whose bits are to be kept (`python tests/golden/make_pipe_onchip_bits.py [file]`): writes
tests/golden/pipe_onchip_bits.json (or `file`) -- per case the kernel name, persist_info(), persist_mirror(), the iteration count of
pcg(rhs, eps=1e-6, max_iter=20000) under the reference load and the SHA-256 of the solution's bytes; for the first case also the
iteration counts and q hashes of three do_timestep() calls.  tests/test_pipe_onchip_gpu.py runs the same cases (run_case below) and
compares: a change of the product's schedule that keeps the order of the additions keeps every hash.

The file in the repository was written by the C++ loops over the on-chip slots (one basic block per slot, the commit before the
hand-scheduled on-chip run)."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
OUT = os.path.join(HERE, "pipe_onchip_bits.json")

# (name, nodes per edge, 16-bit columns, launches cut into these many iterations as well, steps recorded)
CASES = [
    ("cube28_c16", 28, True, (1, 7, 30), 3),   # (12, 6): 343 slices, 10 and 11 per workgroup, service wavefront
    ("cube28_c32", 28, False, (), 0),          # the 384-byte mirror table
    ("cube26_c16", 26, True, (), 0),           # (12, 7): 9 per workgroup, one workgroup without mirrors
    ("cube29_c16", 29, True, (), 0),           # 12 per workgroup (no spare wavefront), slices of width 8
    ("cube29_c32", 29, False, (), 0),          # only some workgroups keep mirrors
]
# the cut mesh: the first of these (cube edge, plane) after which the handle still runs a 12-wavefront one-row kernel
CUT_CANDIDATES = [(27, 0.45), (28, 0.45), (27, 0.3), (26, 0.45)]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _set(env, name, value):
    if value is None:
        env.pop(name, None)
    else:
        env[name] = value


def make_handle(n, c16, cut=None, env=os.environ):
    """The case's handle on CUs 0..31 (and the kernel it reports); cut = the plane of a synthetic_cut(stride=3) applied by a delta re-sync."""
    from fembrain_amd.fem import FemIntegrator
    from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, synthetic_cut, truth_cube
    v, t = truth_cube(n, n, n, 0.1)
    fixed = fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n))
    old = {k: env.get(k) for k in ("FEMBRAIN_CU_MASK", "FEMBRAIN_SPMV_C16")}
    env["FEMBRAIN_CU_MASK"] = "0:32"
    _set(env, "FEMBRAIN_SPMV_C16", None if c16 else "0")
    try:
        g = FemIntegrator(v, t, fixed)
        if cut is not None:
            _, _, d = synthetic_cut(v, t, axis=1, where=cut, stride=3)
            g.resync_delta(d, fixed)
    finally:
        for k, val in old.items():
            _set(env, k, val)
    return g


def run_case(n, c16, runs=(), steps=0, cut=None, env=os.environ):
    """What a case records (see the module text)."""
    g = make_handle(n, c16, cut, env)
    try:
        g.set_uniform_force(1, -10000.0)
        _, rhs = g.system()
        it, x = g.pcg(rhs, eps=1e-6, max_iter=20000)
        path = g.pcg_path()
        rec = dict(n=n, c16=bool(c16), cut=cut, kernel=path["kernel"], path=path["path"], fallbacks=path["fallbacks"], persist_info=list(g.persist_info()),
                   persist_mirror=list(g.persist_mirror()), iterations=it, x_sha256=_sha(x), runs={}, steps=[])
        for run in runs:
            env["FEMBRAIN_PERSIST_MAX_RUN"] = str(run)
            try:
                itc, xc = g.pcg(rhs, eps=1e-6, max_iter=20000)
            finally:
                env.pop("FEMBRAIN_PERSIST_MAX_RUN", None)
            rec["runs"][str(run)] = dict(iterations=itc, x_sha256=_sha(xc))
        for _ in range(steps):
            its = g.do_timestep()
            rec["steps"].append(dict(iterations=its, q_sha256=_sha(g.get_q_state()[0])))
        rec["fallbacks"] = g.pcg_path()["fallbacks"]
    finally:
        g.close()
    return rec


def main():
    out = {}
    for name, n, c16, runs, steps in CASES:
        out[name] = run_case(n, c16, runs, steps)
        print(name, json.dumps(out[name]), flush=True)
    for n, where in CUT_CANDIDATES:
        g = make_handle(n, True, where)
        kernel = g.pcg_path()["kernel"]
        g.close()
        print("cut candidate", n, where, kernel, flush=True)
        if kernel.startswith("k_pcg_pipe<float,c16,12,"):
            out["cut_c16"] = run_case(n, True, (), 0, cut=where)
            print("cut_c16", json.dumps(out["cut_c16"]), flush=True)
            break
    else:
        raise SystemExit("no cut candidate keeps a 12-wavefront one-row kernel")
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
