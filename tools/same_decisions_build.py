#!/usr/bin/env python3
"""Same decisions, same bits: what the handle's life cycle (plan build, creation, the three re-syncs, the cut) of a library decides and
computes on a set of small seeded cases.

    python tools/same_decisions_build.py TREE OUT.json      one process per tree: imports fembrain_amd (and tests/cutref.py) from TREE
    python tools/same_decisions_build.py --compare A.json B.json [TABLE.txt]

Per case: fb_fem_resync_path, fb_fem_renumbering (flag and both spans), fb_fem_plan_on_device, fb_fem_matrix_precision,
fb_fem_assembly_kernel, and the sha256 of every fb_fem_device_plan_get array, of fb_fem_pattern, of Keff and rhs (system() at a seeded
state), of mass() and of q after three steps.  The sharded cases run two ranks on the local communicator in FB_XCH_P2P_FUSED and report
per rank (q on its owned DOFs)."""
import ctypes as C
import hashlib
import json
import os
import sys

KNOBS = ("FEMBRAIN_PLAN_DEVICE", "FEMBRAIN_RESYNC_DELTA", "FEMBRAIN_FRESH_ORDER_PERCENT", "FEMBRAIN_PARTITION_DEVICE")
ARRAYS = ("slice_off", "colidx", "slot_coff", "slot_ccnt", "contrib", "bptr", "bcol", "blk_slot")
N = 14


def sha(a):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def cube(n, scrambled=False):
    import numpy as np
    from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube
    v, t = truth_cube(n, n, n, 0.1)
    fixed = cube_fixed_plane_i0(n, n)
    if scrambled:
        m = np.random.default_rng(4).permutation(len(v))
        v2 = np.empty_like(v)
        v2[m] = v
        v, t, fixed = v2, np.ascontiguousarray(m[t].astype(np.int32)), np.sort(m[fixed])
    return v, t, fixed_vertices_to_dofs(fixed)


def strip_for(v):
    import numpy as np
    import cutref as cr
    xs = np.unique(v[:, 0])
    k = len(xs) // 2
    p = np.array([0.5 * (xs[k - 1] + xs[k]), 0.5 * (v[:, 1].min() + v[:, 1].max()), 0.5 * (v[:, 2].min() + v[:, 2].max())])
    return cr.plane_strip(p, (1.0, 0.013, 0.007), half=20.0)


def record(g, dofs=None):
    """everything the table holds of a handle as it stands; dofs: the entries of q that are this rank's"""
    import numpy as np
    from fembrain_amd import lib as fl
    L = fl.lib()
    out = dict(path=g.resync_path(), renumbering=[int(x) for x in g.renumbering()], plan_on_device=int(L.fb_fem_plan_on_device(g.h)),
               precision=int(g.matrix_precision()), assembly_kernel=int(L.fb_fem_assembly_kernel(g.h)))
    for name in ARRAYS:
        n = int(L.fb_fem_device_plan_get(g.h, name.encode(), None, 0))
        if n < 0:
            out[name] = "none"   # (a host-built plan keeps no pattern on the device)
            continue
        buf = np.zeros(max(n, 1), np.int32)
        assert int(L.fb_fem_device_plan_get(g.h, name.encode(), fl.iptr(buf), n)) == n
        out[name] = sha(buf[:n])
    r = 3 * int(L.fb_fem_num_nodes(g.h))
    rng = np.random.default_rng(7)
    q, qv = rng.normal(size=r) * 0.002, rng.normal(size=r) * 0.1
    f = np.zeros(r)
    f[1::3] = -1000.0
    try:
        out["pattern"] = sha(np.concatenate(g.pattern()))
        g.set_q_state(q, qv)
        g.set_external_forces(f)
        Keff, rhs = g.system()
        out["Keff"], out["rhs"], out["mass"] = sha(Keff), sha(rhs if dofs is None else rhs[dofs]), sha(g.mass())
    except fl.FbError as e:
        out["inspection"] = str(e)
    g.reset_to_rest()
    its = []
    for _ in range(3):
        g.set_external_forces(f)
        its.append(int(g.do_timestep()))
    qq = g.get_q_state()[0]
    out["iterations"], out["q"] = its, sha(qq if dofs is None else qq[dofs])
    return out


def run_cases(out):
    import numpy as np
    from fembrain_amd import lib as fl
    from fembrain_amd.fem import FemIntegrator
    OFF, AUTO, ON = fl.FB_RENUMBER_OFF, fl.FB_RENUMBER_AUTO, fl.FB_RENUMBER_ON

    def case(name, fn, env=None):
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env or {})
        out[name] = fn()
        print(name, json.dumps(out[name]), flush=True)

    def created(mesh, **kw):
        g = FemIntegrator(*mesh, **kw)
        row = record(g)
        g.close()
        return row

    plain, scrambled = cube(N), cube(N, True)
    for mode, mn in ((OFF, "OFF"), (AUTO, "AUTO"), (ON, "ON")):
        case("create cube14 renumber %s" % mn, lambda: created(plain, renumber=mode))
        case("create scrambled cube14 renumber %s" % mn, lambda: created(scrambled, renumber=mode))
    case("create cube14 FEMBRAIN_PLAN_DEVICE=0", lambda: created(plain), dict(FEMBRAIN_PLAN_DEVICE="0"))
    case("create cube14 Newmark", lambda: created(plain, integrator=fl.FB_INTEGRATOR_NEWMARK))

    def from_poly():
        from fembrain_amd.blobtree import sphere_blob
        from fembrain_amd.meshgen import fixed_vertices_to_dofs
        from fembrain_amd.poly import GpuPoly
        poly = GpuPoly(sphere_blob())
        xyz, _ = poly.run_tetrahedralizer(0.1)
        g = FemIntegrator.from_poly(poly, fixed_vertices_to_dofs(np.nonzero(xyz[:, 1] < xyz[:, 1].min() + 0.15)[0].astype(np.int32)))
        row = record(g)
        g.close()
        poly.close() if hasattr(poly, "close") else None
        return row
    case("fb_fem_create_from_poly sphere", from_poly)

    def full_resync(n_to, **kw):
        g = FemIntegrator(*plain, **kw)
        g.set_uniform_force(1, -1000.0)
        g.do_timestep()
        g.resync(*cube(n_to))
        row = record(g)
        g.close()
        return row
    case("full re-sync cube14 -> cube16", lambda: full_resync(16))
    case("FB_MATRIX_AUTO across a re-sync cube14 -> cube26", lambda: full_resync(26, matrix_precision=fl.FB_MATRIX_AUTO))

    def delta(**kw):
        """the delta of a dry cut at rest, fed from the host"""
        g = FemIntegrator(*plain, **kw)
        info, d = g.cut(strip_for(plain[0]), modify=False)
        assert info["status"] == fl.FB_CUT_DRY, info
        g.resync_delta(d, plain[2])
        row = record(g)
        g.close()
        return row
    case("delta, caller's order (merged)", lambda: delta(renumber=OFF))
    case("delta, FEMBRAIN_RESYNC_DELTA=rebuild", lambda: delta(renumber=OFF), dict(FEMBRAIN_RESYNC_DELTA="rebuild"))
    case("delta, renumbered, past the fresh-order rule", lambda: delta(renumber=ON))
    case("delta, renumbered, FEMBRAIN_FRESH_ORDER_PERCENT=100", lambda: delta(renumber=ON), dict(FEMBRAIN_FRESH_ORDER_PERCENT="100"))

    def cut(mode, ids=False, **kw):
        g = FemIntegrator(*plain, expect_cuts=True, **kw)
        if ids:
            g.set_materials([1e7, 2e6, 5e7], [0.46, 0.3, 0.4], [1000.0, 900.0, 1200.0], element_ids=(1 + (np.arange(len(plain[1])) % 2)).astype(np.uint8))
        g.set_uniform_force(1, -1000.0)
        for _ in range(2):
            g.do_timestep()
        info, _ = g.cut(strip_for(plain[0]), mode=mode)
        assert info["status"] == fl.FB_CUT_DONE, info
        row = record(g)
        if ids:
            row["element_map"] = sha(g.element_materials())
        g.close()
        return row
    case("expect_cuts (prewarm), cut bake", lambda: cut("bake"))
    case("expect_cuts (prewarm), cut carry", lambda: cut("carry"))
    case("expect_cuts, element map through a cut", lambda: cut("bake", ids=True))
    merged = dict(FEMBRAIN_FRESH_ORDER_PERCENT="100")   # (the cut's nodes are merged into the order the handle has)
    case("expect_cuts, cut bake, merged", lambda: cut("bake"), merged)
    case("expect_cuts, cut carry, merged", lambda: cut("carry"), merged)
    case("expect_cuts, element map through a merged cut", lambda: cut("bake", ids=True), merged)
    for k in KNOBS:
        os.environ.pop(k, None)


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

        def splits(n):
            return np.array([(n * r // world) * n * n for r in range(world + 1)], np.int32)

        def own(g):
            ids = g.owned_nodes()
            return (3 * ids[:, None].astype(np.int64) + np.arange(3)[None, :]).reshape(-1)
        rows = {}
        for name, env, kw, mesh, sp, then in (("creation", {}, {}, cube(N), splits(N), None),
                                              ("FEMBRAIN_PARTITION_DEVICE=0", dict(FEMBRAIN_PARTITION_DEVICE="0"), {}, cube(N), splits(N), None),
                                              ("FB_RENUMBER_ON, scrambled", {}, dict(renumber=fl.FB_RENUMBER_ON), cube(N, True), None, None),
                                              ("collective re-sync cube14 -> cube16", {}, {}, cube(N), splits(N), 16)):
            for k in KNOBS:
                os.environ.pop(k, None)
            os.environ.update(env)
            g = FemIntegrator(*mesh, shard=(world, rank, sp, comm), **kw)
            if then:
                g.set_uniform_force(1, -1000.0)
                g.do_timestep()
                g.resync(*cube(then), node_splits=splits(then))
            rows[name] = dict(record(g, own(g)), transport=int(L.fb_fem_transport(g.h)), halo=[int(x) for x in g.halo_info()])
            g.close()
        queue.put((rank, rows))
        L.fb_comm_destroy(comm)
    except Exception as e:   # surface the failure instead of hanging the peer
        import traceback
        queue.put((rank, dict(error=repr(e) + traceback.format_exc())))
        queue.close()
        queue.join_thread()
        os._exit(1)


def run_sharded(tree):
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    queue = ctx.Queue()
    shm = "/fembrain_same_decisions_build_%d" % os.getpid()
    procs = [ctx.Process(target=shard_worker, args=(tree, r, 2, shm, queue)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = dict(queue.get(timeout=300) for _ in procs)
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    return got


HEADER = """Handle build and re-sync host side in a unit of its own (fem_build.hip), each step written once: the parent commit's library (3693b8e) and this commit's on the same seeded
inputs, one process per library on one MI355X (tools/same_decisions_build.py).  Per case: fb_fem_resync_path (0 full, 1 delta merged, 2 delta rebuilt), fb_fem_renumbering (flag,
widest element in the caller's and in the internal order), fb_fem_plan_on_device, fb_fem_matrix_precision (0 fp32, 1 fp64), fb_fem_assembly_kernel, PCG iterations of three steps,
and the first 16 hex digits of the sha256 of every fb_fem_device_plan_get array (slice_off colidx slot_coff slot_ccnt contrib bptr bcol blk_slot; "none": a host-built plan keeps
no pattern on the device), of fb_fem_pattern, of Keff and rhs (system() at a seeded state), of mass() and of q after the steps.  The sharded cases: two ranks on the local
communicator in FB_XCH_P2P_FUSED, per rank, rhs and q on its owned DOFs, with fb_fem_transport and fb_fem_halo_info.  The row shows the parent's values; the last column says
whether this commit's are the same in every field (hashes: bit for bit).
"""


def compare(a_path, b_path, table_path=None):
    """a: the parent's file, b: this commit's"""
    a, b = json.load(open(a_path)), json.load(open(b_path))
    lines, same_all = [HEADER], list(a) == list(b)
    for name, row in a.items():
        same = b.get(name) == row
        same_all = same_all and same
        plan = " ".join(str(row.get(k)) for k in ARRAYS)
        rest = " ".join("%s %s" % (k, row[k]) for k in ("pattern", "Keff", "rhs", "mass", "q", "element_map", "transport", "halo", "inspection", "error") if k in row)
        lines.append("%-58s path %s ren %s dev %s prec %s asm %s its %s plan %s %s | %s" % (
            name, row.get("path"), row.get("renumbering"), row.get("plan_on_device"), row.get("precision"), row.get("assembly_kernel"), row.get("iterations"), plan, rest,
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
    out = {}
    run_cases(out)
    for rank, rows in sorted(run_sharded(tree).items()):
        if "error" in rows:
            rows = {"sharded": rows}
        for name, row in rows.items():
            out["two ranks P2P_FUSED, %s, rank %d" % (name, rank)] = row
            print("rank", rank, name, json.dumps(row), flush=True)
    json.dump(out, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
