#!/usr/bin/env python3
"""Same decisions, same bits: what the assembly and SpMV host side of a library decides and computes on a set of small seeded cases.

    python tools/same_decisions_asm_spmv.py TREE OUT.json      one process per tree: imports fembrain_amd (and tests/product_inputs.py) from TREE
    python tools/same_decisions_asm_spmv.py --compare A.json B.json [TABLE.txt]

Per case: fb_fem_assembly_kernel, fb_fem_assembly_wide_slices, fb_fem_pcg_path, spmv_bytes, the PCG iterations of three steps and the
sha256 of Keff, rhs (system() at a seeded live state), mass(), spmv(x) for a seeded x and q after the steps.  The sharded case runs two
ranks on the local communicator in FB_XCH_P2P_FUSED and reports per rank (its owned DOFs of q; no inspection entry points)."""
import ctypes as C
import hashlib
import json
import os
import sys

KNOBS = ("FEMBRAIN_ASM_KERNEL", "FEMBRAIN_SPMV_C16", "FEMBRAIN_SPMV_NT")


def sha(a):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def meshes():
    import numpy as np
    import product_inputs as pi
    from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube
    n = 14
    v, t = truth_cube(n, n, n, 0.1)
    hv, ht, hf = pi.hub(100)
    return {"cube14": (v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n))), "hub": (hv, ht, fixed_vertices_to_dofs(hf))}


def cases():
    from fembrain_amd import lib as fl
    F32, F64 = fl.FB_MATRIX_F32, fl.FB_MATRIX_F64
    out = [("cube14 fp32", "cube14", dict(matrix_precision=F32), {}, None),
           ("cube14 fp64", "cube14", dict(matrix_precision=F64), {}, None),
           ("cube14 fp64 exact tangent", "cube14", dict(matrix_precision=F64, exact_tangent=True), {}, None),
           ("cube14 fp32 exact tangent", "cube14", dict(matrix_precision=F32, exact_tangent=True), {}, None),
           ("cube14 fp32 Newmark", "cube14", dict(matrix_precision=F32, integrator=fl.FB_INTEGRATOR_NEWMARK), {}, None),
           ("cube14 fp64 Newmark", "cube14", dict(matrix_precision=F64, integrator=fl.FB_INTEGRATOR_NEWMARK), {}, None),
           ("cube14 fp32 block-Jacobi", "cube14", dict(matrix_precision=F32, pcg_variant=fl.FB_PCG_BLOCK_JACOBI), {}, None)]
    for c16 in "01":
        for nt in "01":
            out.append(("cube14 fp32 rows C16=%s NT=%s" % (c16, nt), "cube14", dict(matrix_precision=F32, spmv_kernel=fl.FB_SPMV_ROWS),
                        dict(FEMBRAIN_SPMV_C16=c16, FEMBRAIN_SPMV_NT=nt), None))
    out.append(("cube14 fp64 rows C16=1 NT=1", "cube14", dict(matrix_precision=F64, spmv_kernel=fl.FB_SPMV_ROWS), dict(FEMBRAIN_SPMV_C16="1", FEMBRAIN_SPMV_NT="1"), None))
    out.append(("cube14 fp32 split", "cube14", dict(matrix_precision=F32, spmv_kernel=fl.FB_SPMV_SPLIT), {}, None))
    out.append(("cube14 fp64 split", "cube14", dict(matrix_precision=F64, spmv_kernel=fl.FB_SPMV_SPLIT), {}, None))
    for k in ("tets1", "rows"):
        out.append(("cube14 fp32 ASM_KERNEL=%s" % k, "cube14", dict(matrix_precision=F32), dict(FEMBRAIN_ASM_KERNEL=k), None))
    for prec, pn in ((F32, "fp32"), (F64, "fp64")):
        for mat in (None, "map", "map set after a step"):
            out.append(("hub %s %s" % (pn, mat or "no map"), "hub", dict(matrix_precision=prec), {}, mat))
    return out


def run_case(mesh, kw, env, mat):
    import numpy as np
    from fembrain_amd import lib as fl
    from fembrain_amd.fem import FemIntegrator
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    v, t, fixed = mesh
    L = fl.lib()
    g = FemIntegrator(v, t, fixed, timestep=0.01, damping_mass=0.4, damping_stiffness=0.003, **kw)
    r = 3 * len(v)
    rng = np.random.default_rng(7)
    q, qv, x = rng.normal(size=r) * 0.002, rng.normal(size=r) * 0.1, rng.normal(size=r)
    q[fixed] = 0
    qv[fixed] = 0
    f = np.zeros(r)
    f[1::3] = -1000.0
    ids = (1 + (np.arange(len(t)) % 2)).astype(np.uint8)
    mats = ([1e7, 2e6, 5e7], [0.46, 0.3, 0.4], [1000.0, 900.0, 1200.0])
    if mat == "map":
        g.set_materials(*mats, element_ids=ids)
    elif mat:   # the plan was built, and used, without a map
        g.set_external_forces(f)
        g.do_timestep()
        g.reset_to_rest()
        g.set_materials(*mats, element_ids=ids)
    g.set_q_state(q, qv)
    g.set_external_forces(f)
    Keff, rhs = g.system()
    y = g.spmv(x)
    mass = g.mass()
    g.reset_to_rest()
    its = []
    for _ in range(3):
        g.set_external_forces(f)
        its.append(int(g.do_timestep()))
    path = g.pcg_path()
    out = dict(assembly_kernel=int(L.fb_fem_assembly_kernel(g.h)), wide_slices=int(L.fb_fem_assembly_wide_slices(g.h)), pcg_path=[path["path"], path["kernel"]],
               spmv_bytes=g.spmv_bytes(), iterations=its, Keff=sha(Keff), rhs=sha(rhs), mass=sha(mass), spmv=sha(y), q=sha(g.get_q_state()[0]))
    g.close()
    return out


def shard_worker(tree, rank, world, shm, queue):
    try:
        os.environ.update(FEMBRAIN_P2P="1", FEMBRAIN_XCH_MODE="4", FEMBRAIN_P2P_TIMEOUT_MS="20000")
        sys.path[:0] = [tree, os.path.join(tree, "tests")]
        import numpy as np
        from fembrain_amd import lib as fl
        from fembrain_amd.fem import FemIntegrator
        L = fl.lib()
        comm = C.c_void_p()
        fl.check(L.fb_comm_create_local(C.byref(comm), rank, world, shm.encode(), 8 << 20, 0))
        v, t, fixed = meshes()["cube14"]
        n = 14
        splits = np.array([(n * r // world) * n * n for r in range(world + 1)], np.int32)
        g = FemIntegrator(v, t, fixed, shard=(world, rank, splits, comm))
        f = np.zeros(g.r)
        f[1::3] = -10000.0
        f[0::3] = 300.0 * np.sin(np.arange(len(v)))
        its = []
        for _ in range(3):
            g.set_external_forces(f)
            its.append(int(g.do_timestep()))
        own = g.owned_nodes()
        dofs = (3 * own[:, None].astype(np.int64) + np.arange(3)[None, :]).reshape(-1)
        path = g.pcg_path()
        queue.put((rank, dict(transport=int(L.fb_fem_transport(g.h)), assembly_kernel=int(L.fb_fem_assembly_kernel(g.h)), wide_slices=int(L.fb_fem_assembly_wide_slices(g.h)),
                              pcg_path=[path["path"], path["kernel"]], spmv_bytes=g.spmv_bytes(), iterations=its, q=sha(g.get_q_state()[0][dofs]))))
        g.close()
        L.fb_comm_destroy(comm)
    except Exception as e:   # surface the failure instead of hanging the peer
        queue.put((rank, dict(error=repr(e))))
        queue.close()
        queue.join_thread()
        os._exit(1)


def run_sharded(tree):
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    queue = ctx.Queue()
    shm = "/fembrain_same_decisions_%d" % os.getpid()
    procs = [ctx.Process(target=shard_worker, args=(tree, r, 2, shm, queue)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(queue.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    return got


HEADER = """Assembly and SpMV launches through one resolved kernel table each: the parent commit's library (bbc4100) and this commit's on the same seeded inputs, one process per
library on one MI355X (tools/same_decisions_asm_spmv.py).  Per case: fb_fem_assembly_kernel (0 slot-major, 1 element-major, 2 its staged form), fb_fem_assembly_wide_slices,
fb_fem_pcg_path (path of the last solve, persistent kernel name: none on meshes this small), fb_fem_spmv_bytes, PCG iterations of three steps, first 24 hex digits of the sha256
of Keff and rhs (system() at a seeded live state), mass(), spmv(x) for a seeded x, and q after the steps.  The sharded case: two ranks on the local communicator in
FB_XCH_P2P_FUSED, per rank, q on its owned DOFs.  The row shows the parent's values; the last column says whether this commit's are the same in every field (hashes: bit for bit).
"hub ... map set after a step": the plan was built and stepped without a map, which then arrives (fb_fem_set_element_materials resolves the material-aware rows).
"""


def compare(a_path, b_path, table_path=None):
    """a: the parent's file, b: this commit's"""
    a, b = json.load(open(a_path)), json.load(open(b_path))
    lines, same_all = [HEADER], list(a) == list(b)
    for name, row in a.items():
        same = b.get(name) == row
        same_all = same_all and same
        h = " ".join("%s %s" % (k, row[k]) for k in ("Keff", "rhs", "mass", "spmv", "q") if k in row)
        lines.append("%-34s asm %s wide %s path %s bytes %.0f its %s %s | %s" % (name, row.get("assembly_kernel"), row.get("wide_slices"), row.get("pcg_path"),
                                                                                row.get("spmv_bytes", 0), row.get("iterations"), h,
                                                                                "this commit: identical in every field" if same else "this commit DIFFERS: %s" % b.get(name)))
    lines.append("all %d cases identical in every field (hashes bit for bit): %s" % (len(a), same_all))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if table_path:
        open(table_path, "w").write(text)
    return 0 if same_all else 1


def main():
    if sys.argv[1] == "--compare":
        sys.exit(compare(*sys.argv[2:5]))
    tree, out_path = os.path.abspath(sys.argv[1]), sys.argv[2]
    sys.path[:0] = [tree, os.path.join(tree, "tests")]
    from fembrain_amd import lib as fl
    assert os.path.abspath(fl.__file__).startswith(tree + os.sep), fl.__file__
    ms = meshes()
    out = {}
    for name, mesh, kw, env, mat in cases():
        out[name] = run_case(ms[mesh], kw, env, mat)
        print(name, json.dumps(out[name]), flush=True)
    for k in KNOBS:
        os.environ.pop(k, None)
    for rank, row in sorted(run_sharded(tree).items()):
        out["cube14 two ranks P2P_FUSED, rank %d" % rank] = row
        print("rank", rank, json.dumps(row), flush=True)
    json.dump(out, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
