"""Records what two instantiations of the persistent one-row kernel compute, bit for bit, that tests/golden/pipe_onchip_bits.json has no
bits for and that run with a service wavefront (one wavefront more than slices: the launch form whose wavefronts run ahead of the
barrier behind the sums, pcg_pipe.hip.h "Run-ahead form"), each confined to one XCD (FEMBRAIN_CU_MASK=0:32: 32 workgroups):
  cube14_c16  k_pcg_pipe<float,c16,8,8>: 43 slices, 1 and 2 per workgroup -- the first of CUBE88 that selects (8, 8) with a wavefront to spare
  cube28_bj   k_pcg_pipe<float,c16,12,6,bj> (FB_PCG_BLOCK_JACOBI): 343 slices, 10 and 11 per workgroup

Run on an MI355X at the commit whose bits are to be kept (`python tests/golden/make_pipe_runahead_bits.py [file]`): writes
tests/golden/pipe_runahead_bits.json (or `file`) -- per case the kernel name, persist_info(), the iteration count of
pcg(rhs, eps=1e-6, max_iter=20000) under the reference load and the SHA-256 of the solution's bytes, uncut and with the launches cut into
1 and 7 iterations (FEMBRAIN_PERSIST_MAX_RUN).  tests/test_pipe_runahead_gpu.py runs the same cases (run_case below) and compares.

The file in the repository was written at the commit before the run-ahead form: every launch form with all its barriers."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
OUT = os.path.join(HERE, "pipe_runahead_bits.json")

RUNS = (1, 7)
CUBE88 = (14, 15, 13, 16, 12)  # cube edges tried for the (8, 8) case, nearest to 14 first
KERNEL88 = "k_pcg_pipe<float,c16,8,8>"
KERNEL_BJ = "k_pcg_pipe<float,c16,12,6,bj>"


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def make_handle(n, bj, env=os.environ):
    """The case's handle on CUs 0..31, 16-bit columns."""
    from fembrain_amd import lib as fl
    from fembrain_amd.fem import FemIntegrator
    from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube
    v, t = truth_cube(n, n, n, 0.1)
    fixed = fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n))
    old = {k: env.get(k) for k in ("FEMBRAIN_CU_MASK", "FEMBRAIN_SPMV_C16")}
    env["FEMBRAIN_CU_MASK"] = "0:32"
    env.pop("FEMBRAIN_SPMV_C16", None)
    try:
        return FemIntegrator(v, t, fixed, pcg_variant=fl.FB_PCG_BLOCK_JACOBI if bj else fl.FB_PCG_MERGED)
    finally:
        for k, val in old.items():
            if val is None:
                env.pop(k, None)
            else:
                env[k] = val


def run_case(n, bj, runs=RUNS, env=os.environ):
    """What a case records (see the module text)."""
    g = make_handle(n, bj, env)
    try:
        g.set_uniform_force(1, -10000.0)
        _, rhs = g.system()
        it, x = g.pcg(rhs, eps=1e-6, max_iter=20000)
        path = g.pcg_path()
        rec = dict(n=n, bj=bool(bj), kernel=path["kernel"], path=path["path"], persist_info=list(g.persist_info()), iterations=it, x_sha256=_sha(x), runs={})
        for run in runs:
            env["FEMBRAIN_PERSIST_MAX_RUN"] = str(run)
            try:
                itc, xc = g.pcg(rhs, eps=1e-6, max_iter=20000)
            finally:
                env.pop("FEMBRAIN_PERSIST_MAX_RUN", None)
            rec["runs"][str(run)] = dict(iterations=itc, x_sha256=_sha(xc))
        rec["fallbacks"] = g.pcg_path()["fallbacks"]
    finally:
        g.close()
    return rec


def main():
    out = {}
    for n in CUBE88:
        g = make_handle(n, False)
        kernel, info = g.pcg_path()["kernel"], g.persist_info()
        g.close()
        print("(8, 8) candidate", n, kernel, info, flush=True)
        if kernel == KERNEL88 and info[0] and info[1] < 8:  # fewer slices than wavefronts: a service wavefront
            out["cube%d_c16" % n] = run_case(n, False)
            print(json.dumps(out["cube%d_c16" % n]), flush=True)
            break
    else:
        raise SystemExit("no candidate selects (8, 8) with a wavefront to spare")
    out["cube28_bj"] = run_case(28, True)
    print("cube28_bj", json.dumps(out["cube28_bj"]), flush=True)
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
