"""GPU: the sharded FEM handle run by several PROCESSES on the one GPU of the box.  The ranks talk through the
host-staged shared-memory communicator (fb_comm_create_local), which drives exactly the code path of the RCCL
communicator -- per-rank plans, halo packing and exchange of q / qvel / the PCG search direction / x, rank-ordered
all-reduce of the merged PCG sums, identical termination on every rank -- so the N > 1 solver is exercised on hardware
even though RCCL itself refuses two ranks on one device.  The gathered state must match the unsharded handle."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _mesh(n, world):
    """n > 0: truth cube split into i-plane slabs; n < 0: Delaunay tetrahedra of |n| random points in RANDOM node order split
    into equal index ranges -- every rank neighbours every other and the halos are large and irregular."""
    from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube
    if n > 1000:   # the (n - 1000)^3 cube with its node ids randomly permuted, equal index ranges: every rank neighbours every other
        v, t, fixed = _scrambled_cube(n - 1000)
        return v, t, fixed, np.array([len(v) * r // world for r in range(world + 1)], np.int32)
    if n > 0:
        v, t = truth_cube(n, n, n, 0.1)
        fixed = fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n))
        planes = [n * r // world for r in range(world + 1)]
        return v, t, fixed, np.array([p * n * n for p in planes], np.int32)
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(77)
    v = rng.uniform(0, 1, size=(-n, 3))
    t = Delaunay(v).simplices.astype(np.int32)
    vol = np.einsum("ij,ij->i", v[t[:, 1]] - v[t[:, 0]], np.cross(v[t[:, 2]] - v[t[:, 0]], v[t[:, 3]] - v[t[:, 0]])) / 6
    t = np.ascontiguousarray(t[np.abs(vol) > 1e-7])
    fixed = fixed_vertices_to_dofs(np.nonzero(v[:, 0] < 0.12)[0])
    return v, t, fixed, np.array([(-n) * r // world for r in range(world + 1)], np.int32)


def _worker(rank, world, shm_name, n, variant, steps, q, p2p=0, quit_early=False, spmv=0, renumber=0):
    """p2p: 0 = host-staged test communicator, else the peer-to-peer exchange mode (lib.FB_XCH_P2P / _SUMS / _FUSED).
    renumber: FB_RENUMBER_* of the handle (0 = AUTO: the ranks vote on the node order before they build)."""
    try:
        if p2p:
            os.environ["FEMBRAIN_P2P"] = "1"
            os.environ["FEMBRAIN_XCH_MODE"] = str(p2p)
            os.environ["FEMBRAIN_P2P_TIMEOUT_MS"] = "1500" if quit_early else "20000"
        from fembrain_amd import lib as fl
        from fembrain_amd.fem import FemIntegrator
        from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube
        L = fl.lib()
        comm = C.c_void_p()
        fl.check(L.fb_comm_create_local(C.byref(comm), rank, world, shm_name.encode(), 8 << 20, 0))
        v, t, fixed, splits = _mesh(n, world)
        g = FemIntegrator(v, t, fixed, shard=(world, rank, splits, comm), pcg_variant=variant, spmv_kernel=spmv, renumber=renumber)
        assert L.fb_fem_transport(g.h) == (p2p if p2p else 1), L.fb_fem_transport(g.h)
        if quit_early and rank == world - 1:   # a rank that stops taking part: the others must time out, not hang
            q.put((rank, "left", None, None, 0, 0))
            q.close()
            q.join_thread()   # flush the feeder thread before leaving without cleanup
            os._exit(0)
        f = np.zeros(g.r)
        f[1::3] = -10000.0 if n > 0 else -200.0
        f[0::3] = (300.0 if n > 0 else 20.0) * np.sin(np.arange(len(v)))   # not symmetric across the slabs (a function of the caller's ids)
        its = []
        for _ in range(steps):
            g.set_external_forces(f)
            its.append(g.do_timestep())
        qq, vv, _ = g.get_q_state()
        # the nodes this rank owns: its range of the caller's ids, or -- when the ranks voted for the internal order -- whatever
        # fb_fem_owned_nodes lists
        own = g.owned_nodes()
        dofs = (3 * own[:, None].astype(np.int64) + np.arange(3)[None, :]).reshape(-1)
        info = (bool(g.renumbering()[0]),) + tuple(g.halo_info())
        if os.environ.get("FEMBRAIN_TEST_REPORT_WIDE") == "1":    # (test_sharded_mesh_with_hull_slices_wider_than_the_element_major_kernel_takes)
            info = info + (int(L.fb_fem_assembly_kernel(g.h)), int(L.fb_fem_assembly_wide_slices(g.h)))
        q.put((rank, its, qq[dofs].copy(), vv[dofs].copy(), dofs, info))
        g.close()
        L.fb_comm_destroy(comm)
    except Exception as e:  # surface the failure instead of hanging the peers' barrier forever
        q.put((rank, repr(e), None, None, 0, 0))
        q.close()
        q.join_thread()
        os._exit(1)


@pytest.mark.parametrize("world,variant,p2p", [(2, 0, 0), (3, 0, 0), (2, 1, 0), (4, 1, 0),
                                               (2, 0, 2), (3, 0, 3), (2, 0, 4), (4, 0, 4), (3, 1, 4), (4, 1, 2)])
def test_sharded_ranks_on_one_gpu_match_the_unsharded_handle(gpu, world, variant, p2p):
    _run_sharded(world, variant, p2p, 12)


def _own_dofs(g):
    own = g.owned_nodes()
    return (3 * own[:, None].astype(np.int64) + np.arange(3)[None, :]).reshape(-1)


def _put(qg, qq, lo, hi):
    """a rank's values into the gathered vector: a range, or (hi None) the DOFs fb_fem_owned_nodes listed"""
    if hi is None:
        qg[lo] = qq
    else:
        qg[lo:hi] = qq


def _scrambled_cube(n):
    from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube
    v0, t0 = truth_cube(n, n, n, 0.1)
    m = np.random.default_rng(4).permutation(len(v0))
    v = np.empty_like(v0)
    v[m] = v0
    t = np.ascontiguousarray(m[t0].astype(np.int32))
    return v, t, fixed_vertices_to_dofs(np.sort(m[cube_fixed_plane_i0(n, n)]))


def _renumbered_worker(rank, world, shm_name, n, p2p, q, subset):
    try:
        if p2p:
            os.environ["FEMBRAIN_P2P"] = "1"
            os.environ["FEMBRAIN_XCH_MODE"] = str(p2p)
        from fembrain_amd import lib as fl
        from fembrain_amd.fem import FemIntegrator
        L = fl.lib()
        comm = C.c_void_p()
        fl.check(L.fb_comm_create_local(C.byref(comm), rank, world, shm_name.encode(), 8 << 20, 0))
        v, t, fixed = _scrambled_cube(n)
        if subset and rank == world - 1:
            t = np.ascontiguousarray(t[: len(t) // 2])      # NOT the whole mesh on this rank: the ranks must notice
            v = v * np.array([1.0, 1.0, 0.5])
        try:
            g = FemIntegrator(v, t, fixed, shard=(world, rank, None, comm), renumber=fl.FB_RENUMBER_ON)
        except fl.FbError as e:
            q.put((rank, "refused: %s" % e, None, None, None, None))
            return
        on, sc, si = g.renumbering()
        halo, nbr = g.halo_info()
        own = g.owned_nodes()
        f = np.zeros(g.r)
        f[1::3] = -10000.0
        f[0::3] = 300.0 * np.sin(v[:, 2] * 7.0)   # (a function of the position, not of the caller's id)
        its = []
        for _ in range(2):
            g.set_external_forces(f)
            its.append(g.do_timestep())
        qq = g.get_q_state()[0]
        bptr, bcol = g.pattern()
        q.put((rank, its, (on, sc, si, halo, nbr), own, qq, (bptr, bcol)))
        g.close()
        L.fb_comm_destroy(comm)
    except Exception as e:
        q.put((rank, repr(e), None, None, None, None))
        q.close()
        q.join_thread()
        os._exit(1)


@pytest.mark.parametrize("world,p2p,sigma", [(2, 0, 0), (3, 4, 0), (4, 2, 0), (3, 4, 1)])
def test_renumbered_shards_of_a_scrambled_cube_are_slabs_with_two_neighbours(gpu, monkeypatch, world, p2p, sigma):
    """SURVEY 8e / VERDICT r3 item 1: a cube whose node ids are a random permutation, cut into equal index ranges, makes every rank a
    neighbour of every other with half the mesh as halo.  With FB_RENUMBER_ON every rank derives the same slab order from the whole
    mesh and owns a contiguous range of THAT: at most two neighbour ranks, a halo of one or two grid planes, the ranks' owned nodes
    partition the caller's ids, patterns come back in the caller's ids (ascending), and two steps gathered over the ranks equal the
    unsharded handle's on the same caller mesh.  sigma = 1: with the second stage of the node order forced on (FEMBRAIN_SIGMA=1: rows sorted
    by element count inside windows of 256), the same, the slabs a window thicker at most."""
    import multiprocessing as mp
    from fembrain_amd.fem import FemIntegrator
    n = 12
    if sigma:
        monkeypatch.setenv("FEMBRAIN_SIGMA", "1")   # (the workers inherit it)
    slack = 512 if sigma else 0   # (two nodes of an element may move a window each, apart)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = "/fembrain_test_%d_renum_%d_%d_%d" % (os.getpid(), world, p2p, sigma)
    procs = [ctx.Process(target=_renumbered_worker, args=(r, world, name, n, p2p, q, False)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(world):
            res.append(q.get(timeout=240))
            assert res[-1][2] is not None, res[-1]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    v, t, fixed = _scrambled_cube(n)
    g = FemIntegrator(v, t, fixed, renumber=0)
    f = np.zeros(g.r)
    f[1::3] = -10000.0
    f[0::3] = 300.0 * np.sin(v[:, 2] * 7.0)
    its = []
    for _ in range(2):
        g.set_external_forces(f)
        its.append(g.do_timestep())
    qs = g.get_q_state()[0]
    gb, gc = g.pattern()
    qg = np.zeros_like(qs)
    seen = np.zeros(len(v), int)
    for rank, rits, info, own, qq, (bptr, bcol) in res:
        on, sc, si, halo, nbr = info
        assert on and si <= n * n + n + 1 + slack < sc
        assert nbr <= 2 and halo <= 2 * (n * n + n + 1 + slack), (rank, halo, nbr)      # a slab: one neighbour below, one above
        assert rits == res[0][1] and all(abs(a - b) <= max(2, 0.01 * b) for a, b in zip(rits, its))
        seen[own] += 1
        dofs = (3 * own[:, None] + np.arange(3)[None, :]).reshape(-1)
        qg[dofs] = qq[dofs]
        outside = np.setdiff1d(np.arange(3 * len(v)), dofs)
        assert not qq[outside].any()                                         # a rank fills the entries of its own nodes only
        for k, node in enumerate(own):                                       # its rows of the pattern, in the caller's ids, ascending
            assert np.array_equal(bcol[bptr[k]:bptr[k + 1]], gc[gb[node]:gb[node + 1]])
    assert (seen == 1).all()
    assert np.abs(qg - qs).max() <= 1e-6 * np.abs(qs).max()
    g.close()


def _other_plane_dofs(v, fixed):
    """list B of the constraint tests: the face of the cube opposite the constrained one, in the caller's ids, ascending"""
    from fembrain_amd.meshgen import fixed_vertices_to_dofs
    a = v[np.unique(np.asarray(fixed) // 3)]
    axis = int(np.argmin(np.ptp(a, axis=0)))   # the constrained face is flat along it
    far = v[:, axis].max() if a[0, axis] == v[:, axis].min() else v[:, axis].min()
    return fixed_vertices_to_dofs(np.nonzero(v[:, axis] == far)[0])


def _set_constraints_worker(rank, world, shm_name, n, q, set_later):
    try:
        from fembrain_amd import lib as fl
        from fembrain_amd.fem import FemIntegrator
        L = fl.lib()
        comm = C.c_void_p()
        fl.check(L.fb_comm_create_local(C.byref(comm), rank, world, shm_name.encode(), 8 << 20, 0))
        v, t, fixed_a = _scrambled_cube(n)
        fixed_b = _other_plane_dofs(v, fixed_a)
        assert len(fixed_b) == len(fixed_a) and not np.intersect1d(fixed_a, fixed_b).size and (np.diff(fixed_b) > 0).all()
        g = FemIntegrator(v, t, fixed_a if set_later else fixed_b, shard=(world, rank, None, comm), renumber=fl.FB_RENUMBER_ON)
        assert g.renumbering()[0]
        f = np.zeros(g.r)
        f[1::3] = -10000.0
        f[0::3] = 300.0 * np.sin(v[:, 2] * 7.0)
        refusals = []
        if set_later:
            g.set_constrained_dofs(fixed_b)
        its = []
        for bad in (np.append(fixed_b, 3 * len(v)).astype(np.int32), np.ascontiguousarray(fixed_b[::-1])):
            if set_later:   # (rank-local: a refused list leaves the handle as it was, and the step that follows is the reference's)
                try:
                    g.set_constrained_dofs(bad)
                    refusals.append(None)
                except fl.FbError as e:
                    refusals.append(str(e))
            g.set_external_forces(f)
            its.append(g.do_timestep())
        dofs = _own_dofs(g)
        q.put((rank, set_later, its, dofs, g.get_q_state()[0][dofs].copy(), refusals))
        g.close()
        L.fb_comm_destroy(comm)
    except Exception as e:
        import traceback
        q.put((rank, set_later, "EXC " + repr(e) + traceback.format_exc(), None, None, None))
        q.close()
        q.join_thread()
        os._exit(1)


def test_constrained_dofs_set_on_a_renumbered_shard_equal_those_it_was_created_with(gpu):
    """fb_fem_set_constrained_dofs on a renumbered shard takes the list in the caller's ids, checks it, maps it to internal ids and sorts it
    again -- the steps creation takes.  Two ranks under FB_RENUMBER_ON on the scrambled 10^3 cube, created with the plane i = 0 constrained
    and then given the opposite face, step twice to the bits of two ranks created with that face: each rank's owned DOFs of q.  A list with
    an id out of range and a descending one are refused with the messages creation has, before each of the two steps, which stay the
    reference's."""
    import multiprocessing as mp
    world, n = 2, 10
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_set_constraints_worker, args=(r, world, "/fembrain_test_%d_setfix_%d" % (os.getpid(), later), n, q, bool(later)))
             for later in (0, 1) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in procs:
            r = q.get(timeout=120)
            assert r[3] is not None, r
            res[(r[0], r[1])] = r
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for rank in range(world):
        _, _, its_c, dofs_c, q_c, _ = res[(rank, False)]
        _, _, its_s, dofs_s, q_s, refusals = res[(rank, True)]
        assert "out of range" in refusals[0] and "strictly ascending" in refusals[1], refusals
        assert its_s == its_c and its_c[0] > 0, (its_s, its_c)
        assert np.array_equal(dofs_s, dofs_c) and np.abs(q_c).max() > 0
        assert np.array_equal(q_s, q_c), (rank, np.abs(q_s - q_c).max())


def test_renumbered_shards_refuse_ranks_that_hold_different_meshes(gpu):
    """the internal order is derived per rank; ranks that were not given the same whole mesh derive different orders, and creation
    fails on every rank alike instead of solving a scrambled system"""
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = "/fembrain_test_%d_renum_bad" % os.getpid()
    procs = [ctx.Process(target=_renumbered_worker, args=(r, 2, name, 10, 0, q, True)) for r in range(2)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(2):
            res.append(q.get(timeout=240))
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    assert all(isinstance(r[1], str) and "refused" in r[1] and "different node orders" in r[1] for r in res), res


@pytest.mark.parametrize("world,variant,p2p", [(2, 0, 0), (3, 0, 2), (2, 0, 3), (3, 0, 4), (2, 1, 4)])
def test_sharded_ranks_with_the_row_kernel(gpu, world, variant, p2p):
    """small shards take the split SpMV by themselves (the tests above); the row kernel of large shards is forced here"""
    from fembrain_amd import lib as fl
    _run_sharded(world, variant, p2p, 12, spmv=fl.FB_SPMV_ROWS)


@pytest.mark.parametrize("world,p2p", [(2, 0), (3, 2), (3, 4), (4, 4)])
def test_sharded_unstructured_mesh_all_to_all_halos(gpu, world, p2p):
    """Delaunay mesh in random node order cut into equal index ranges, the caller's numbering KEPT (FB_RENUMBER_OFF): every rank is
    every other rank's neighbour."""
    from fembrain_amd import lib as fl
    info = _run_sharded(world, 0, p2p, -900, renumber=fl.FB_RENUMBER_OFF)
    assert all(not on and nbr == world - 1 for on, halo, nbr in info), info


@pytest.mark.parametrize("world,p2p", [(4, 0), (4, 4), (5, 2)])
def test_auto_node_order_on_shards_gives_slabs_without_being_asked(gpu, world, p2p):
    """VERDICT r4 item 1 / SURVEY 8e: FB_RENUMBER_AUTO (the default) on a sharded handle.  A 12^3 cube whose node ids are a random
    permutation: equal ranges of the caller's ids would give every rank world - 1 neighbours and half the mesh as halo, so the ranks vote
    for the internal slab order before they build (no FB_RENUMBER_ON, no environment variable) and each ends up with at most two neighbour
    ranks and a halo of a plane or two; the steps gathered through fb_fem_owned_nodes equal the unsharded handle's."""
    info = _run_sharded(world, 0, p2p, 1012)
    assert all(on and nbr <= 2 and halo <= 2 * (144 + 13) for on, halo, nbr in info), info


def test_sharded_mesh_with_hull_slices_wider_than_the_element_major_kernel_takes(gpu, monkeypatch):
    """Round 5: the Delaunay mesh of 4,000 random points on 2 ranks.  Hull nodes have 40 and more neighbours, so some slices of a shard
    are wider than the 31 slots the element-major assembly kernel takes: those go to k_assemble_wide (a workgroup per slice) beside it, on
    a shard as on an unsharded handle -- the two steps equal the unsharded handle's (checked by _run_sharded), the element-major kernel
    is the one in use and at least one rank has such slices."""
    monkeypatch.setenv("FEMBRAIN_TEST_REPORT_WIDE", "1")
    info = _run_sharded(2, 0, 0, -4000)
    assert all(kern in (1, 2) for *_, kern, wide in info) and any(wide > 0 for *_, kern, wide in info), info


def test_auto_node_order_on_an_unstructured_mesh(gpu):
    """the Delaunay mesh of 900 random points in random order on 4 ranks: the vote switches the internal order on and the halos shrink
    (hull slivers still join far slabs, so a rank may keep a third neighbour -- with a handful of nodes)"""
    from fembrain_amd import lib as fl
    off = _run_sharded(4, 0, 0, -900, renumber=fl.FB_RENUMBER_OFF)
    auto = _run_sharded(4, 0, 0, -900)
    assert all(on for on, halo, nbr in auto) and not any(on for on, halo, nbr in off)
    assert sum(h for _, h, _ in auto) < 0.6 * sum(h for _, h, _ in off), (auto, off)


def test_auto_node_order_leaves_plane_slabs_alone(gpu):
    """a cube numbered plane by plane and cut at planes: two neighbours at most under the caller's numbering, nothing to vote for"""
    info = _run_sharded(4, 0, 4, 12)
    assert all(not on and nbr <= 2 for on, halo, nbr in info), info


def _run_sharded(world, variant, p2p, n, spmv=0, renumber=0):
    """p2p != 0: the direct inbox transport (HIP IPC mapped inboxes, kernels that store into the peer's inbox and spin --
    bounded -- on their own flags) between processes that share the GPU, in its three forms: an own kernel per exchange
    (2), sums inside the PCG kernels (3), sums and halo values inside the PCG kernels (4)."""
    import multiprocessing as mp
    from fembrain_amd.fem import FemIntegrator
    steps = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = "/fembrain_test_%d_%d_%d_%d" % (os.getpid(), world, variant, int(p2p))
    procs = [ctx.Process(target=_worker, args=(r, world, name, n, variant, steps, q, p2p, False, spmv, renumber)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(world):
            res.append(q.get(timeout=240))
            assert res[-1][2] is not None, res[-1]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    v, t, fixed, _ = _mesh(n, world)
    g = FemIntegrator(v, t, fixed, pcg_variant=variant)
    f = np.zeros(g.r)
    f[1::3] = -10000.0 if n > 0 else -200.0
    f[0::3] = (300.0 if n > 0 else 20.0) * np.sin(np.arange(len(v)))
    its = []
    for _ in range(steps):
        g.set_external_forces(f)
        its.append(g.do_timestep())
    qs, vs, _ = g.get_q_state()
    qg, vg = np.zeros_like(qs), np.zeros_like(vs)
    seen = np.zeros(len(qs), int)
    for rank, rits, qq, vv, dofs, info in res:
        assert rits == res[0][1]                                  # every rank stopped at the same iteration
        assert all(abs(a - b) <= max(2, 0.01 * b) for a, b in zip(rits, its))
        qg[dofs], vg[dofs] = qq, vv
        seen[dofs] += 1
    assert (seen == 1).all()                                      # the ranks' owned nodes partition the mesh
    # rank-ordered partial sums instead of one block-ordered sum: same iterates up to rounding
    assert np.abs(qg - qs).max() <= 1e-6 * np.abs(qs).max()
    assert np.abs(vg - vs).max() <= 1e-5 * np.abs(vs).max()
    return [r[5] for r in sorted(res, key=lambda r: r[0])]


def _bench_worker(rank, world, shm_name, n, q):
    """one rank of bench.py's sharded 8M-tet leg: i-plane slabs, rebuild + uniform load + one step from rest"""
    try:
        from fembrain_amd import lib as fl
        from fembrain_amd.fem import FemIntegrator
        L = fl.lib()
        comm = C.c_void_p()
        fl.check(L.fb_comm_create_local(C.byref(comm), rank, world, shm_name.encode(), 16 << 20, 0))
        v, t, fixed, splits = _mesh(n, world)
        g = FemIntegrator(v, t, fixed, shard=(world, rank, splits, comm))
        g.rebuild_elements()
        g.set_uniform_force(1, -10000.0)
        its = g.do_timestep()
        qq = g.get_q_state()[0]
        lo, hi = 3 * int(splits[rank]), 3 * int(splits[rank + 1])
        # 2-byte column words on a shard of 4M tets (the halo form: halo columns count from the slice's first halo column)
        n_own = int(splits[rank + 1] - splits[rank])
        index_bytes = (g.spmv_bytes() - (n_own + 1) * 4 - 24 * n_own - 96 * n_own) / g.num_blocks() - 36
        assert index_bytes == 2.0, index_bytes
        q.put((rank, its, qq[lo:hi].copy(), None, lo, hi))
        g.close()
        L.fb_comm_destroy(comm)
    except Exception as e:
        q.put((rank, repr(e), None, None, 0, 0))
        q.close()
        q.join_thread()
        os._exit(1)


def test_config5_8M_tets_in_two_processes_match_the_unsharded_handle(gpu):
    """BASELINE config 5 at size: the 111^3-node cube (7,986,000 tets) as two i-plane slabs in two processes (host-staged
    communicator: the box has one GPU) against the unsharded handle -- the check bench.py's sharded runs do on themselves
    before timing: first step from rest, iterations within max(3, 2 %), displacements within 2e-4 of max|q|."""
    import multiprocessing as mp
    from fembrain_amd.fem import FemIntegrator
    world, n = 2, 111
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = "/fembrain_test_%d_cfg5" % os.getpid()
    procs = [ctx.Process(target=_bench_worker, args=(r, world, name, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(world):
            res.append(q.get(timeout=500))
            assert res[-1][2] is not None, res[-1]
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    v, t, fixed, _ = _mesh(n, world)
    g = FemIntegrator(v, t, fixed)
    g.rebuild_elements()
    g.set_uniform_force(1, -10000.0)
    it1 = g.do_timestep()
    q1 = g.get_q_state()[0]
    g.close()
    qs = np.zeros_like(q1)
    for rank, its, qq, _, lo, hi in res:
        assert its == res[0][1]
        assert abs(its - it1) <= max(3, 0.02 * it1), (its, it1)
        qs[lo:hi] = qq
    assert np.abs(qs - q1).max() <= 2e-4 * np.abs(q1).max()


def test_p2p_wait_is_bounded_when_a_peer_leaves(gpu):
    """One rank exits after the collective set-up.  The survivor's exchange kernels give up at the wall-clock bound, poison
    the inbox, drain the queue, and the step returns FB_ECOMM -- no hang."""
    import multiprocessing as mp
    import time
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = "/fembrain_test_%d_leave" % os.getpid()
    procs = [ctx.Process(target=_worker, args=(r, 2, name, 8, 0, 1, q, 4, True)) for r in range(2)]
    t0 = time.time()
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(2):
            r = q.get(timeout=120)
            res[r[0]] = r
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    assert res[1][1] == "left"
    assert res[0][2] is None and "timed out" in res[0][1], res[0]
    assert time.time() - t0 < 100


def _field_worker(rank, world, port, q):
    """one rank of the sharded field path: its z-slab through sweep / classify / tetrahedralize, vertex base from a real
    all-gather (torch.distributed, gloo)"""
    try:
        import torch.distributed as dist
        from fembrain_amd.blobtree import sphere_blob
        from fembrain_amd.poly import GpuPoly
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)

        def allgather(x):
            out = [None] * world
            dist.all_gather_object(out, int(x))
            return out
        blob = sphere_blob()
        g = GpuPoly(blob)
        xyz, tets = g.run_tetrahedralizer_slab(blob.bbox[0], 0.043, (26, 26, 26), rank, world, allgather)
        q.put((rank, xyz, tets))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:
        q.put((rank, repr(e), None))
        q.close()
        q.join_thread()
        os._exit(1)


def test_field_slabs_in_processes_concatenate_to_the_whole_mesh(gpu):
    import multiprocessing as mp
    from fembrain_amd.blobtree import sphere_blob
    from fembrain_amd.poly import GpuPoly
    world, port = 3, 29700 + os.getpid() % 200
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_field_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(world):
            r = q.get(timeout=240)
            assert r[2] is not None, r
            res[r[0]] = r
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    blob = sphere_blob()
    g = GpuPoly(blob)
    g.sweep_grid(blob.bbox[0], 0.043, (26, 26, 26))
    g.classify()
    g.tetrahedralize()
    xyz, tets = g.read_tetmesh()
    assert np.array_equal(np.concatenate([res[r][1] for r in range(world)]), xyz)
    assert np.array_equal(np.concatenate([res[r][2] for r in range(world)]), tets) and len(tets) > 10000


def _plan_worker(rank, world, shm_name, n, q):
    """one rank: its share of the plan built on the device (sharded handles since round 2) against the host builder, array by
    array; then a collective re-sync on the same handle against a fresh one"""
    try:
        import time
        from fembrain_amd import lib as fl
        from fembrain_amd.fem import FemIntegrator
        L = fl.lib()
        comm = C.c_void_p()
        fl.check(L.fb_comm_create_local(C.byref(comm), rank, world, shm_name.encode(), 8 << 20, 0))
        v, t, fixed, splits = _mesh(n, world)
        # (the plan in the CALLER's numbering is what is compared: the vote of FB_RENUMBER_AUTO would give the unstructured meshes an internal order)
        g = FemIntegrator(v, t, fixed, shard=(world, rank, splits, comm), renumber=fl.FB_RENUMBER_OFF)
        assert L.fb_fem_plan_on_device(g.h) == 1
        hp = C.c_void_p()
        tt, fd = np.ascontiguousarray(t, np.int32).reshape(-1), np.ascontiguousarray(fixed, np.int32)
        fl.check(L.fb_plan_create(C.byref(hp), len(v), len(t), fl.iptr(tt), len(fd), fl.iptr(fd), world, rank, fl.iptr(splits)))
        bad = []
        for name in ("bptr", "bcol", "blk_slot", "slice_off", "colidx", "slot_coff", "slot_ccnt", "contrib"):
            cnt = L.fb_plan_get(hp, name.encode(), None, 0)
            want = np.zeros(cnt, np.int32)
            assert L.fb_plan_get(hp, name.encode(), fl.iptr(want), cnt) == cnt
            dcnt = L.fb_fem_device_plan_get(g.h, name.encode(), None, 0)
            got = np.zeros(max(dcnt, 1), np.int32)
            L.fb_fem_device_plan_get(g.h, name.encode(), fl.iptr(got), dcnt)
            if dcnt != cnt or not np.array_equal(got[:dcnt], want):
                bad.append(name)
        L.fb_plan_destroy(hp)
        # collective re-sync to a different mesh size and back, then a step that must equal a fresh sharded handle's
        v2, t2, fixed2, splits2 = _mesh(n + 2 if n > 0 else n, world)
        g.resync(v2, t2, fixed2, node_splits=splits2)
        assert (g.node_lo, g.node_hi) == (int(splits2[rank]), int(splits2[rank + 1]))
        t0 = time.perf_counter()
        g.resync(v, t, fixed, node_splits=splits)
        resync_ms = (time.perf_counter() - t0) * 1e3
        fresh = FemIntegrator(v, t, fixed, shard=(world, rank, splits, comm), renumber=fl.FB_RENUMBER_OFF)
        # per-rank ingest: only the elements with an owned node (ascending global order), positions of other ranks' nodes poisoned
        own = ((t >= splits[rank]) & (t < splits[rank + 1])).any(axis=1)
        vown = np.full_like(v, np.nan)
        used = np.unique(t[own])
        vown[used] = v[used]
        mine = FemIntegrator(vown, t[own], fixed, shard=(world, rank, splits, comm))
        its = []
        for h in (g, fresh, mine):
            h.set_uniform_force(1, -3000.0)
            its.append(h.do_timestep())
        qf = fresh.get_q_state()[0]
        same = its[0] == its[1] == its[2] and np.array_equal(g.get_q_state()[0], qf) and np.array_equal(mine.get_q_state()[0], qf)
        # a re-sync without node ranges to a mesh of another size falls to the equal split (fb_fem_resync's rule), and steps
        g.resync(v2, t2, fixed2)
        eq = [len(v2) * i // world for i in range(world + 1)]
        same = same and (g.node_lo, g.node_hi) == (eq[rank], eq[rank + 1])
        g.set_uniform_force(1, -100.0)
        same = same and g.do_timestep() > 0 and bool(np.isfinite(g.get_q_state()[0]).all())
        q.put((rank, bad, same, resync_ms, its))
        g.close(); fresh.close(); mine.close()
        L.fb_comm_destroy(comm)
    except Exception as e:
        import traceback
        q.put((rank, repr(e) + traceback.format_exc(), False, 0.0, []))
        q.close()
        q.join_thread()
        os._exit(1)


@pytest.mark.parametrize("world,n", [(2, 12), (3, 14), (3, -900), (5, 10), (4, -1300)])
def test_sharded_device_plan_equals_host_plan_and_resyncs(gpu, world, n):
    """every rank's rows of the plan built by plan_device.hip (sort by local row and GLOBAL column) are bit for bit the host
    builder's (fem_plan.cpp) -- cubes cut into slabs and a Delaunay mesh in random node order where every rank neighbours every
    other; fb_fem_resync_sharded (collective) gives the handle a fresh one would be, and a handle created from the rank's own
    elements only (per-rank ingest) steps bit for bit like one created from the whole mesh"""
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = "/fembrain_test_%d_plan_%d_%d" % (os.getpid(), world, abs(n))
    procs = [ctx.Process(target=_plan_worker, args=(r, world, name, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(world):
            res.append(q.get(timeout=240))
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for rank, bad, same, ms, its in res:
        assert bad == [], (rank, bad)
        assert same, (rank, its)


def _bad_resync_worker(rank, world, shm_name, q):
    try:
        from fembrain_amd import lib as fl
        from fembrain_amd.fem import FemIntegrator
        L = fl.lib()
        comm = C.c_void_p()
        fl.check(L.fb_comm_create_local(C.byref(comm), rank, world, shm_name.encode(), 8 << 20, 0))
        v, t, fixed, splits = _mesh(10, world)
        g = FemIntegrator(v, t, fixed, shard=(world, rank, splits, comm))
        g.set_uniform_force(1, -3000.0)
        it0 = g.do_timestep()
        # the re-sync mesh of the LAST rank has a flat element among its own (every rank passes its own elements: per-rank ingest)
        own = ((t >= splits[rank]) & (t < splits[rank + 1])).any(axis=1)
        t_mine = t[own].copy()
        v_mine = v.copy()
        if rank == world - 1:
            e = t_mine[len(t_mine) // 2]
            v_mine[e[3]] = v_mine[e[0]]
        msg = None
        try:
            g.resync(v_mine, t_mine, fixed, node_splits=splits)
        except fl.FbError as e:
            msg = str(e)
        poisoned = None
        try:
            g.do_timestep()
        except fl.FbError as e:
            poisoned = str(e)
        # a good collective re-sync heals every rank, and the step is the step of a fresh handle
        g.resync(v, t, fixed, node_splits=splits)
        g.set_uniform_force(1, -3000.0)
        it1 = g.do_timestep()
        q.put((rank, msg, poisoned, it0, it1))
        g.close()
        L.fb_comm_destroy(comm)
    except Exception as e:
        import traceback
        q.put((rank, "EXC " + repr(e) + traceback.format_exc(), None, 0, 0))
        q.close()
        q.join_thread()
        os._exit(1)


def test_a_failed_collective_resync_fails_on_every_rank_instead_of_hanging(gpu):
    """fb_fem_resync_sharded is collective, its plan build is not: one rank's mesh has a flat element after a 'cut'.  The ranks
    agree on the outcome before the collective attach of the peer inboxes: the bad rank reports its element, the
    healthy rank reports that rank -- within the call, not after a communicator time-out --, both handles are unusable until a
    re-sync that succeeds everywhere, and that one restores the step of a fresh handle."""
    import multiprocessing as mp
    import time
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = "/fembrain_test_%d_badresync" % os.getpid()
    procs = [ctx.Process(target=_bad_resync_worker, args=(r, world, name, q)) for r in range(world)]
    t0 = time.time()
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(world):
            r = q.get(timeout=120)
            res[r[0]] = r
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    assert time.time() - t0 < 100
    for rank in range(world):
        _, msg, poisoned, it0, it1 = res[rank]
        assert msg is not None and not msg.startswith("EXC"), res[rank]
        assert ("rest volume" in msg) if rank == world - 1 else ("failed on rank %d" % (world - 1) in msg), (rank, msg)
        assert poisoned is not None and "unusable after a failed" in poisoned, (rank, poisoned)
        assert it0 > 0 and it1 == it0, (rank, it0, it1)


def _bad_create_worker(rank, world, shm_name, q):
    try:
        from fembrain_amd import lib as fl
        from fembrain_amd.fem import FemIntegrator
        L = fl.lib()
        comm = C.c_void_p()
        fl.check(L.fb_comm_create_local(C.byref(comm), rank, world, shm_name.encode(), 8 << 20, 0))
        v, t, fixed, splits = _mesh(10, world)

        def step_of_a_new_handle():
            g = FemIntegrator(v, t, fixed, shard=(world, rank, splits, comm))
            g.set_uniform_force(1, -3000.0)
            it = g.do_timestep()
            g.close()
            return it
        it0 = step_of_a_new_handle()   # (before anything has failed on this communicator)
        # the mesh of the LAST rank has a flat element among its own (every rank passes its own elements: per-rank ingest)
        own = ((t >= splits[rank]) & (t < splits[rank + 1])).any(axis=1)
        t_mine = t[own].copy()
        v_mine = v.copy()
        if rank == world - 1:
            e = t_mine[len(t_mine) // 2]
            v_mine[e[3]] = v_mine[e[0]]
        msg = None
        try:
            FemIntegrator(v_mine, t_mine, fixed, shard=(world, rank, splits, comm)).close()
        except fl.FbError as e:
            msg = str(e)
        it1 = step_of_a_new_handle()
        q.put((rank, msg, it0, it1))
        L.fb_comm_destroy(comm)
    except Exception as e:
        import traceback
        q.put((rank, "EXC " + repr(e) + traceback.format_exc(), 0, 0))
        q.close()
        q.join_thread()
        os._exit(1)


def test_a_failed_collective_creation_fails_on_every_rank_instead_of_hanging(gpu):
    """fb_fem_create_sharded is collective, its plan build is not: one rank's mesh has a flat element.  The ranks agree on the outcome
    before the collective attach of the peer inboxes: the bad rank reports its element, the healthy rank reports that rank --
    within the call, not after a communicator time-out --, no handle is made, and a good creation on the same communicator afterwards
    steps like the one before the failure."""
    import multiprocessing as mp
    import time
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = "/fembrain_test_%d_badcreate" % os.getpid()
    procs = [ctx.Process(target=_bad_create_worker, args=(r, world, name, q)) for r in range(world)]
    t0 = time.time()
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(world):
            r = q.get(timeout=120)
            res[r[0]] = r
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    assert time.time() - t0 < 100
    for rank in range(world):
        _, msg, it0, it1 = res[rank]
        assert msg is not None and not msg.startswith("EXC"), res[rank]
        assert ("rest volume" in msg) if rank == world - 1 else ("failed on rank %d" % (world - 1) in msg), (rank, msg)
        assert it0 > 0 and it1 == it0, (rank, it0, it1)


def _sp_force(n, v):
    """Load of the sharded persistent tests.  The 56^3 cube gets a quarter of the smaller cubes' load: under the full one its third step
    sits on a discontinuity of the corotational model (an element's rotation flips), where runs that agree to 1e-7 after two steps
    and whose solves all meet the tolerance on the same system (measured: true residuals 1.30e-6 .. 1.31e-6, x within 3e-7) end
    2.7e-4 or 5.4e-4 apart depending on the rounding of their sums -- not a property of any solver."""
    f = np.zeros(3 * len(v))
    scale = 0.25 if n >= 50 else 1.0
    f[1::3] = (-10000.0 if n > 0 else -200.0) * scale
    f[0::3] = (300.0 if n > 0 else 20.0) * scale * np.sin(np.arange(len(v)))
    return f


def _shard_persist_worker(rank, world, shm_name, n, steps, q, cut=None, timeout_ms="2000", newmark=False, resync=False, planes=None):
    try:
        os.environ["FEMBRAIN_CU_MASK"] = "%d:%d" % (rank * (256 // world // 32 * 32), 256 // world // 32 * 32)   # each rank on its own share of the CUs: whole XCDs (mask bits 32 k .. 32 k + 31 are one XCD; a share that cuts an XCD leaves workgroups without a CU)
        os.environ["FEMBRAIN_SHARDED_PERSIST"] = "1"
        os.environ["FEMBRAIN_PERSIST_TIMEOUT_MS"] = timeout_ms
        if cut:
            os.environ["FEMBRAIN_PERSIST_MAX_RUN"] = str(cut)
        from fembrain_amd import lib as fl
        from fembrain_amd.fem import FemIntegrator
        L = fl.lib()
        comm = C.c_void_p()
        fl.check(L.fb_comm_create_local(C.byref(comm), rank, world, shm_name.encode(), 8 << 20, 0))
        v, t, fixed, splits = _mesh(n, world)
        if planes is not None:   # (uneven slabs)
            splits = np.array([p * n * n for p in planes], np.int32)
        g = FemIntegrator(v, t, fixed, shard=(world, rank, splits, comm), cg_eps=1e-6 if n > 0 else 1e-8,
                          integrator=fl.FB_INTEGRATOR_NEWMARK if newmark else fl.FB_INTEGRATOR_VOLUME_CONSERVING)
        f = _sp_force(n, v)
        its, paths = [], []
        for k in range(steps):
            if resync and k == steps - 1:
                # Deformable::syncForceModel after a cut, collective: the last tets of the mesh go (the slab boundaries move with them),
                # the box, the send lists, the proxies and the relief deal are all made again
                t = np.ascontiguousarray(t[:len(t) - len(t) // 50])
                g.resync(v, t, fixed, node_splits=splits)
            g.set_external_forces(f)
            its.append(g.do_timestep())
            paths.append(int(g.last.pcg_path))
        qq = g.get_q_state()[0]
        lo, hi = _own_dofs(g), None     # (the rank's own nodes: a range of the caller's ids unless the ranks voted for the internal order)
        q.put((rank, its, qq[lo].copy(), g.pcg_path(), paths, g.persist_info(), lo, hi))
        g.close()
        L.fb_comm_destroy(comm)
    except Exception as e:
        import traceback
        q.put((rank, repr(e) + traceback.format_exc(), None, None, None, None, 0, 0))
        q.close()
        q.join_thread()
        os._exit(1)


@pytest.mark.parametrize("world,n,kernel", [(2, 40, "k_pcg_pipe_shard<8,8>"), (2, -30000, "k_pcg_pipe_shard<8,8>"), (3, 40, "k_pcg_pipe_shard<8,8>"), (4, 40, "k_pcg_pipe_shard<8,8>"),
                                            (2, 56, "k_pcg_pipe_shard<12,6>"), (2, 70, "k_pcg_pipe2_shard")])
def test_sharded_persistent_solver_on_disjoint_cus_matches_the_unsharded_handle(gpu, world, n, kernel):
    """The sharded persistent pipelined solver (pcg_shard_box.hip.h; opt-in FEMBRAIN_SHARDED_PERSIST=1; UNMEASURED on multi-GPU
    hardware): one persistent launch per solve ON EVERY RANK, the halo rows written by their owners straight into the neighbour rank's
    box (HIP IPC), copied into the planes by a proxy wavefront, the rank sums posted into every rank's box -- no collective on the
    path.  Here the ranks are processes on the one GPU of the box, each confined to its own share of the CUs (FEMBRAIN_CU_MASK), so
    their persistent grids are resident together.  Three steps against the unsharded handle: the same iteration counts to max(2, 1 %),
    the gathered displacements to 1e-6; every rank reports the sharded kernel, the persistent path and no fallback; a solve cut into
    launches of 7 iterations gives the same bits.  Cube slabs (two neighbours at most), a Delaunay mesh in random node order (every
    rank neighbours every other, every workgroup polls all flags), four ranks, the 12-wavefront instantiation, and the two-rows-per-lane
    kernel (2M tets, 21 slices per CU on half a GPU)."""
    import multiprocessing as mp
    from fembrain_amd.fem import FemIntegrator
    from fembrain_amd import lib as fl
    steps = 3
    ctx = mp.get_context("spawn")
    runs = []
    for cut in (None, 7):
        q = ctx.Queue()
        name = "/fembrain_test_%d_sp_%d_%d_%s" % (os.getpid(), world, abs(n), cut)
        procs = [ctx.Process(target=_shard_persist_worker, args=(r, world, name, n, steps, q, cut)) for r in range(world)]
        for p in procs:
            p.start()
        res = []
        try:
            for _ in range(world):
                res.append(q.get(timeout=300))
                assert res[-1][2] is not None, res[-1]
        finally:
            for p in procs:
                p.join(timeout=30)
                if p.is_alive():
                    p.kill()
        runs.append(sorted(res, key=lambda r: r[0]))
        if n < 0 or world > 2:
            break      # (the cut run for the slab cubes only)
    v, t, fixed, _ = _mesh(n, world)
    g = FemIntegrator(v, t, fixed, cg_eps=1e-6 if n > 0 else 1e-8)   # (the ill-conditioned Delaunay systems: two solvers agree to the tolerance they stop at)
    f = _sp_force(n, v)
    its = []
    for _ in range(steps):
        g.set_external_forces(f)
        its.append(g.do_timestep())
    qs = g.get_q_state()[0]
    qg = np.zeros_like(qs)
    for rank, rits, qq, path, paths, info, lo, hi in runs[0]:
        assert rits == runs[0][0][1]
        assert all(abs(a - b) <= max(2, 0.01 * b) for a, b in zip(rits, its)), (rits, its)
        assert path["kernel"] == kernel and path["fallbacks"] == 0 and all(p == fl.FB_PCG_PATH_PERSISTENT for p in paths), (rank, path, paths)
        assert info[0] and info[2] == 256 // world // 32 * 32, info
        _put(qg, qq, lo, hi)
    # the Delaunay mesh has sliver tets: fp32 matrix entries summed in another order move its solution by 3e-5 (the two-launch sharded
    # path sits 3.0e-5 from the unsharded handle at eps 1e-8, this one 3.2e-5, the two sharded paths 1e-5 from each other)
    assert np.abs(qg - qs).max() <= (1e-6 if n > 0 else 1e-4) * np.abs(qs).max()
    if len(runs) > 1:
        for a, b in zip(runs[0], runs[1]):
            assert a[1] == b[1] and np.array_equal(a[2], b[2]), "a cut solve differs from the uncut one"


def test_sharded_persistent_solver_that_times_out_falls_back_on_every_rank(gpu):
    """A wait bound no launch can meet (0.1 us): every rank's first launch gives up, the ranks agree on it (the error words are
    gathered), and all of them repeat the solve with the two-launch sharded iteration and stay with it -- same result as the unsharded
    handle, the path reported as fallback, one fallback counted per rank."""
    import multiprocessing as mp
    from fembrain_amd.fem import FemIntegrator
    from fembrain_amd import lib as fl
    world, n, steps = 2, 40, 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_shard_persist_worker, args=(r, world, "/fembrain_test_%d_spto" % os.getpid(), n, steps, q, None, "0.0001")) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(world):
            res.append(q.get(timeout=300))
            assert res[-1][2] is not None, res[-1]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    v, t, fixed, _ = _mesh(n, world)
    g = FemIntegrator(v, t, fixed)
    f = _sp_force(n, v)
    its = []
    for _ in range(steps):
        g.set_external_forces(f)
        its.append(g.do_timestep())
    qs = g.get_q_state()[0]
    qg = np.zeros_like(qs)
    for rank, rits, qq, path, paths, info, lo, hi in res:
        assert all(abs(a - b) <= max(2, 0.01 * b) for a, b in zip(rits, its)), (rits, its)
        assert path["fallbacks"] == 1 and paths == [fl.FB_PCG_PATH_FALLBACK, fl.FB_PCG_PATH_TWO_LAUNCH], (rank, path, paths)
        _put(qg, qq, lo, hi)
    assert np.abs(qg - qs).max() <= 1e-6 * np.abs(qs).max()


def test_sharded_persistent_solver_under_the_newmark_integrator_keeps_the_warm_start(gpu):
    """ImplicitNewmarkSparse does not clear its solution buffer between solves (implicitNewmarkSparse.cpp:317-320): every solve after
    the first starts from the previous x, which in the persistent kernels is a launch that begins with r = b - A x (the halo rows of x
    cross the ranks like any other published vector).  Three Newmark steps on two ranks against the unsharded handle."""
    import multiprocessing as mp
    from fembrain_amd.fem import FemIntegrator
    from fembrain_amd import lib as fl
    world, n, steps = 2, 40, 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_shard_persist_worker, args=(r, world, "/fembrain_test_%d_spnm" % os.getpid(), n, steps, q, None, "2000", True)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(world):
            res.append(q.get(timeout=300))
            assert res[-1][2] is not None, res[-1]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    v, t, fixed, _ = _mesh(n, world)
    g = FemIntegrator(v, t, fixed, integrator=fl.FB_INTEGRATOR_NEWMARK)
    f = _sp_force(n, v)
    its = []
    for _ in range(steps):
        g.set_external_forces(f)
        its.append(g.do_timestep())
    qs = g.get_q_state()[0]
    qg = np.zeros_like(qs)
    for rank, rits, qq, path, paths, info, lo, hi in res:
        assert all(abs(a - b) <= max(2, 0.01 * b) for a, b in zip(rits, its)), (rits, its)
        assert path["kernel"] == "k_pcg_pipe_shard<8,8>" and path["fallbacks"] == 0 and all(p == fl.FB_PCG_PATH_PERSISTENT for p in paths), (rank, path, paths)
        _put(qg, qq, lo, hi)
    assert np.abs(qg - qs).max() <= 1e-6 * np.abs(qs).max()


def test_sharded_persistent_solver_survives_a_collective_resync(gpu):
    """fb_fem_resync_sharded on handles that run the sharded persistent solver: every rank drops 2 % of the elements between the second
    and the third step (state reset, as Deformable::syncForceModel does) -- boxes, mappings, send lists, proxies are rebuilt -- and the
    third step still runs in persistent launches and matches the unsharded handle put through the same re-sync."""
    import multiprocessing as mp
    from fembrain_amd.fem import FemIntegrator
    from fembrain_amd import lib as fl
    world, n, steps = 2, 40, 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_shard_persist_worker, args=(r, world, "/fembrain_test_%d_sprs" % os.getpid(), n, steps, q, None, "2000", False, True)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(world):
            res.append(q.get(timeout=300))
            assert res[-1][2] is not None, res[-1]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    v, t, fixed, _ = _mesh(n, world)
    g = FemIntegrator(v, t, fixed)
    f = _sp_force(n, v)
    its = []
    for k in range(steps):
        if k == steps - 1:
            t = np.ascontiguousarray(t[:len(t) - len(t) // 50])
            g.resync(v, t, fixed)
        g.set_external_forces(f)
        its.append(g.do_timestep())
    qs = g.get_q_state()[0]
    qg = np.zeros_like(qs)
    for rank, rits, qq, path, paths, info, lo, hi in res:
        assert all(abs(a - b) <= max(2, 0.01 * b) for a, b in zip(rits, its)), (rits, its)
        assert path["kernel"] == "k_pcg_pipe_shard<8,8>" and path["fallbacks"] == 0 and all(p == fl.FB_PCG_PATH_PERSISTENT for p in paths), (rank, path, paths)
        _put(qg, qq, lo, hi)
    assert np.abs(qg - qs).max() <= 1e-6 * np.abs(qs).max()


def _sp_eligibility_worker(rank, world, shm_name, sizes, q):
    try:
        os.environ["FEMBRAIN_CU_MASK"] = "%d:%d" % (rank * (256 // world // 32 * 32), 256 // world // 32 * 32)
        os.environ["FEMBRAIN_SHARDED_PERSIST"] = "1"
        os.environ["FEMBRAIN_PERSIST_TIMEOUT_MS"] = "2000"
        from fembrain_amd import lib as fl
        from fembrain_amd.fem import FemIntegrator
        L = fl.lib()
        comm = C.c_void_p()
        fl.check(L.fb_comm_create_local(C.byref(comm), rank, world, shm_name.encode(), 8 << 20, 0))
        g = None
        out = []
        for n in sizes:
            v, t, fixed, splits = _mesh(n, world)
            if g is None:
                g = FemIntegrator(v, t, fixed, shard=(world, rank, splits, comm))
            else:
                g.resync(v, t, fixed, node_splits=splits)
            g.set_external_forces(_sp_force(n, v))
            it = g.do_timestep()
            qq = g.get_q_state()[0]
            lo, hi = 3 * int(splits[rank]), 3 * int(splits[rank + 1])
            out.append((n, it, bool(g.sharded_persist()), int(g.last.pcg_path), g.pcg_path()["kernel"], g.pcg_path()["fallbacks"], qq[lo:hi].copy(), lo, hi))
        q.put((rank, out))
        g.close()
        L.fb_comm_destroy(comm)
    except Exception as e:
        import traceback
        q.put((rank, repr(e) + traceback.format_exc()))
        q.close()
        q.join_thread()
        os._exit(1)


def test_sharded_persistent_solver_across_resyncs_that_cross_its_limits(gpu):
    """a collective re-sync may take a handle out of the sharded persistent solver's range and back -- 40^3 (4 slices per
    CU on two half-GPUs: the persistent kernel), 12^3 (less than one per CU: the two-launch iteration), 40^3 again, 72^3 (23 per CU:
    one more than the two-row kernel takes), 40^3 again.  Nothing of an old plan's send lists, workgroup deal or box may survive into
    the next: fb_fem_sharded_persist() says what runs, and every step matches an unsharded handle led through the same meshes."""
    import multiprocessing as mp
    from fembrain_amd.fem import FemIntegrator
    from fembrain_amd import lib as fl
    world, sizes = 2, [40, 12, 40, 72, 40]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sp_eligibility_worker, args=(r, world, "/fembrain_test_%d_spel" % os.getpid(), sizes, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(world):
            r = q.get(timeout=600)
            assert not isinstance(r[1], str), r
            res[r[0]] = r[1]
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    g = None
    for k, n in enumerate(sizes):
        v, t, fixed, _ = _mesh(n, world)
        if g is None:
            g = FemIntegrator(v, t, fixed)
        else:
            g.resync(v, t, fixed)
        g.set_external_forces(_sp_force(n, v))
        it = g.do_timestep()
        qs = g.get_q_state()[0]
        qg = np.zeros_like(qs)
        for rank in range(world):
            rn, rit, on, path, kernel, fallbacks, qq, lo, hi = res[rank][k]
            assert rn == n and abs(rit - it) <= max(2, 0.01 * it) and fallbacks == 0, (rank, k, rit, it, fallbacks)
            assert on == (n == 40) and (path == fl.FB_PCG_PATH_PERSISTENT) == (n == 40), (rank, n, on, path)
            assert kernel == ("k_pcg_pipe_shard<8,8>" if n == 40 else ""), (rank, n, kernel)
            _put(qg, qq, lo, hi)
        assert np.abs(qg - qs).max() <= 2e-6 * np.abs(qs).max(), (n, np.abs(qg - qs).max() / np.abs(qs).max())
    g.close()


def test_sharded_persistent_ranks_with_different_kernels_interoperate(gpu):
    """Uneven slabs of the 58^3 cube on two half-GPUs: 26 planes (11 slices per CU: the one-row kernel) and 32 planes (14 per CU: the
    two-row kernel).  Box, counters, proxies and sums are the same protocol in both, so the ranks need not run the same kernel; three
    steps against the unsharded handle."""
    import multiprocessing as mp
    from fembrain_amd.fem import FemIntegrator
    from fembrain_amd import lib as fl
    world, n, steps, planes = 2, 58, 3, (0, 26, 58)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_shard_persist_worker, args=(r, world, "/fembrain_test_%d_spmx" % os.getpid(), n, steps, q, None, "2000", False, False, planes)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(world):
            res.append(q.get(timeout=300))
            assert res[-1][2] is not None, res[-1]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    v, t, fixed, _ = _mesh(n, world)
    g = FemIntegrator(v, t, fixed)
    f = _sp_force(n, v)
    its = []
    for _ in range(steps):
        g.set_external_forces(f)
        its.append(g.do_timestep())
    qs = g.get_q_state()[0]
    qg = np.zeros_like(qs)
    kernels = {}
    for rank, rits, qq, path, paths, info, lo, hi in res:
        assert all(abs(a - b) <= max(2, 0.01 * b) for a, b in zip(rits, its)), (rits, its)
        assert path["fallbacks"] == 0 and all(p == fl.FB_PCG_PATH_PERSISTENT for p in paths), (rank, path, paths)
        kernels[rank] = path["kernel"]
        _put(qg, qq, lo, hi)
    assert kernels == {0: "k_pcg_pipe_shard<12,6>", 1: "k_pcg_pipe2_shard"}, kernels
    assert np.abs(qg - qs).max() <= 1e-6 * np.abs(qs).max()
