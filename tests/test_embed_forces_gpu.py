"""The way back from an embedding to the tets on the device: fb_fem_embed_add_forces (the transpose of the binding, an ordered scatter),
fb_fem_get_external_forces, fb_fem_embed_pick_ray / pick_point and fb_fem_embed_stress, against numpy.

Forces are compared by bytes with the host loop of the header over the binding fb_fem_read_embedding returns (np.add.at applies its
additions in index order: point ascending, corner ascending -- one multiply and one add each).  The picks are compared with fp64 numpy
on the positions the binding gives at the state read back; the ray fixtures are generic by assertion (nearest hit more than 1e-6 in t
from the next, more than 1e-6 inside its triangle), so the triangle must be the same and t, the barycentrics and the hit agree to
1e-9: coordinates are O(1) and no ray grazes, which leaves a few thousand ulps."""
import os

import numpy as np
import pytest

import cut_inputs as ci
import cutref as cr
import embedref as er
from fembrain_amd import lib as fl
from fembrain_amd.fem import Deformable, FemIntegrator
from fembrain_amd.meshgen import delaunay_jittered, fixed_vertices_to_dofs, synthetic_cut, truth_cube

pytestmark = pytest.mark.gpu

OFF, ON = fl.FB_RENUMBER_OFF, fl.FB_RENUMBER_ON


def _fixed_of(v):
    return fixed_vertices_to_dofs(np.nonzero(v[:, 0] <= v[:, 0].min() + 1e-12)[0].astype(np.int32))


def _shuffled(v, t, seed=3):
    perm = np.random.default_rng(seed).permutation(len(v))  # new id of old node
    v2 = np.empty_like(v)
    v2[perm] = v
    return v2, np.ascontiguousarray(perm[t].astype(np.int32))


def _cube(n):
    v, t = truth_cube(n, n, n, 0.1)
    return np.array(v, np.float64).reshape(-1, 3), np.array(t, np.int32).reshape(-1, 4)


def host_add(base, binding, forces, ids=None):
    """the loop of the header: for s (p = ids[s] ascending), k, c: f[3 v + c] = f[3 v + c] + w[4 p + k] * forces[3 s + c]"""
    f = np.array(base, np.float64).reshape(-1, 3).copy()
    ids = np.arange(len(binding["elements"])) if ids is None else np.asarray(ids, np.int64)
    forces = np.asarray(forces, np.float64).reshape(-1, 3)
    assert len(forces) == len(ids)
    prod = binding["weights"][ids][:, :, None] * forces[:, None, :]  # (m, 4, 3): every product rounded on its own
    np.add.at(f, binding["vertices"][ids].ravel(), prod.reshape(-1, 3))  # unbuffered, in index order
    return f.reshape(-1)


def _set_base(g, seed):
    g.set_external_forces(np.random.default_rng(seed).standard_normal(g.r) * 100.0)
    return g.external_forces()


def _einval(call):
    with pytest.raises(fl.FbError) as e:
        call()
    return e.value.code == fl.FB_EINVAL


# ---- 1. the scatter equals the loop ----
def _mesh(name):
    if name == "cube3":
        return _cube(3)  # 27 nodes, 48 tets: runs of hundreds of corners per node
    v, t, _ = delaunay_jittered(7)
    return v, t


@pytest.mark.parametrize("renumber", [OFF, ON])
@pytest.mark.parametrize("zero_threshold", [0.0, 0.06])
@pytest.mark.parametrize("name", ["cube3", "delaunay"])
def test_scatter_equals_the_host_loop_bit_for_bit(gpu, name, zero_threshold, renumber):
    v, t = _mesh(name)
    assert (len(v), len(t)) == (27, 48) if name == "cube3" else 200 < len(v) < 1000
    if renumber == ON:
        v, t = _shuffled(v, t)
    g = FemIntegrator(v, t, _fixed_of(v), renumber=renumber)
    assert g.renumbering()[0] == (renumber == ON)
    pts = er.generic_points(v, 3000, 11, grow=0.1)
    eid, info = g.embed(pts, zero_threshold=zero_threshold, info=True)
    assert info["n_external"] > 0 and (info["n_zeroed"] > 0) == (zero_threshold > 0)
    b = g.embedding(eid)
    assert (b["weights"] < 0).any(), "external points take part with the weights they have"
    base = _set_base(g, 5)
    f1 = np.random.default_rng(6).standard_normal((len(pts), 3))
    g.embed_add_forces(eid, f1)
    want = host_add(base, b, f1)
    got = g.external_forces()
    assert got.tobytes() == want.tobytes(), "max difference %g" % np.abs(got - want).max()
    assert got.tobytes() != base.tobytes()
    # a second call on top of the first: the sum goes on from what is there
    f2 = np.random.default_rng(7).standard_normal((len(pts), 3)) * 1e-3
    g.embed_add_forces(eid, f2)
    assert g.external_forces().tobytes() == host_add(want, b, f2).tobytes()
    counts = np.bincount(b["vertices"].ravel(), minlength=len(v))
    fi = g.embed_forces_info(eid)
    assert fi == dict(n_table_builds=1, longest_run=int(counts.max()), n_nodes_touched=int((counts > 0).sum())), (fi, counts.max())
    assert fi["longest_run"] > 256 or name != "cube3", "runs that span several passes of a wavefront and cross workgroups in the table"
    g.close()


# ---- 2. lists ----
def test_lists(gpu):
    v, t = _cube(4)
    g = FemIntegrator(v, t, _fixed_of(v))
    pts = er.generic_points(v, 700, 12, grow=0.1)
    eid = g.embed(pts)
    b = g.embedding(eid)
    rng = np.random.default_rng(8)
    cur = _set_base(g, 9)
    for ids in ([0], [699], [5, 300, 698], np.arange(0, 700, 2), np.arange(1, 700, 2), np.arange(350), np.arange(700)):
        ids = np.asarray(ids, np.int32)
        f = rng.standard_normal((len(ids), 3))
        g.embed_add_forces(eid, f, ids)
        cur = host_add(cur, b, f, ids)
        assert g.external_forces().tobytes() == cur.tobytes(), ids[:4]
    # arange(n_points) is bitwise the form without a list
    f = rng.standard_normal((700, 3))
    base = _set_base(g, 10)
    g.embed_add_forces(eid, f, np.arange(700))
    with_list = g.external_forces()
    g.set_external_forces(base)
    g.embed_add_forces(eid, f)
    assert g.external_forces().tobytes() == with_list.tobytes() == host_add(base, b, f).tobytes()
    # n == 0 changes nothing, with either form of the list
    g.embed_add_forces(eid, np.zeros((0, 3)), np.zeros(0, np.int32))
    assert g._L.fb_fem_embed_add_forces(g.h, eid, 0, None, None) == fl.FB_OK
    assert g.external_forces().tobytes() == with_list.tobytes()
    # an embedding of a few points on a mesh of many nodes: most nodes have no run
    e2 = g.embed(pts[:3])
    b2 = g.embedding(e2)
    f = rng.standard_normal((3, 3))
    g.embed_add_forces(e2, f)
    assert g.external_forces().tobytes() == host_add(with_list, b2, f).tobytes()
    assert g.embed_forces_info(e2)["n_nodes_touched"] == len(np.unique(b2["vertices"])) < len(v)
    assert g.embed_forces_info(eid)["n_table_builds"] == 1
    g.close()


# ---- 3. errors ----
def test_refused_calls_change_nothing(gpu):
    v, t = _cube(4)
    g = FemIntegrator(v, t, _fixed_of(v))
    pts = er.generic_points(v, 50, 13, grow=0.1)
    eid = g.embed(pts)
    base = _set_base(g, 14)
    f3 = np.ones((3, 3))
    nan = f3.copy()
    nan[1, 2] = np.nan
    inf = f3.copy()
    inf[0, 0] = np.inf
    all_nan = np.ones((50, 3))
    all_nan[49, 1] = np.nan
    assert _einval(lambda: g.embed_add_forces(eid, f3, [7, 5, 9]))     # descending
    assert _einval(lambda: g.embed_add_forces(eid, f3, [5, 5, 9]))     # a duplicate
    assert _einval(lambda: g.embed_add_forces(eid, f3, [5, 9, 50]))    # out of range
    assert _einval(lambda: g.embed_add_forces(eid, f3, [-1, 5, 9]))
    assert _einval(lambda: g.embed_add_forces(eid, nan, [5, 9, 11]))
    assert _einval(lambda: g.embed_add_forces(eid, inf, [5, 9, 11]))
    assert _einval(lambda: g.embed_add_forces(eid, all_nan))
    L = g._L
    ids = np.array([5, 9, 11], np.int32)
    assert L.fb_fem_embed_add_forces(g.h, eid, 3, fl.iptr(ids), None) == fl.FB_EINVAL            # null forces
    assert L.fb_fem_embed_add_forces(g.h, eid, 3, None, fl.dptr(f3.reshape(-1))) == fl.FB_EINVAL  # no list: n must be n_points
    for dead in (-1, 1, 7, 8, 100):
        assert L.fb_fem_embed_add_forces(g.h, dead, 3, fl.iptr(ids), fl.dptr(f3.reshape(-1))) == fl.FB_EINVAL
        assert L.fb_fem_embed_forces_info(g.h, dead, None, None, None) == fl.FB_EINVAL
        assert L.fb_fem_embed_pick_point(g.h, dead, fl.dptr(np.zeros(3)), None, None, None) == fl.FB_EINVAL
        assert L.fb_fem_embed_pick_ray(g.h, dead, fl.dptr(np.zeros(3)), fl.dptr(np.ones(3)), 1.0, None, None, None, None) == fl.FB_EINVAL
        assert L.fb_fem_embed_stress(g.h, dead, None) == fl.FB_EINVAL
    assert g.external_forces().tobytes() == base.tobytes()
    assert g.embed_forces_info(eid) == dict(n_table_builds=0, longest_run=0, n_nodes_touched=0), "a refused call builds nothing"
    g.embed_release(eid)
    assert _einval(lambda: g.embed_add_forces(eid, f3, [5, 9, 11]))  # a released one
    assert g.external_forces().tobytes() == base.tobytes()
    g.close()


def _shard_child(rank, world, shm_name, q):
    import ctypes as C
    try:
        from test_sharded_gpu import _mesh as sharded_mesh
        L = fl.lib()
        comm = C.c_void_p()
        fl.check(L.fb_comm_create_local(C.byref(comm), rank, world, shm_name.encode(), 8 << 20, 0))
        v, t, fixed, splits = sharded_mesh(6, world)
        g = FemIntegrator(v, t, fixed, shard=(world, rank, splits, comm))
        f, ids, z3, o3 = np.ones(3), np.zeros(1, np.int32), np.zeros(3), np.ones(3)
        codes = [L.fb_fem_embed_add_forces(g.h, 0, 1, fl.iptr(ids), fl.dptr(f)), L.fb_fem_embed_forces_info(g.h, 0, None, None, None),
                 L.fb_fem_embed_pick_ray(g.h, 0, fl.dptr(z3), fl.dptr(o3), 1.0, None, None, None, None),
                 L.fb_fem_embed_pick_point(g.h, 0, fl.dptr(z3), None, None, None), L.fb_fem_embed_stress(g.h, 0, None)]
        g.close()
        L.fb_comm_destroy(comm)
        q.put((rank, codes))
    except Exception as e:
        q.put((rank, repr(e)))
        q.close()
        q.join_thread()
        os._exit(1)


def test_sharded_handle_is_refused(gpu):
    from test_fem_surface_gpu import _run_children
    name = "fbtouch%d" % os.getpid()
    got = _run_children(_shard_child, [(r, 2, name) for r in range(2)])
    assert sorted(got) == [(0, [fl.FB_EINVAL] * 5), (1, [fl.FB_EINVAL] * 5)], got


# ---- 4. through a step ----
@pytest.mark.parametrize("renumber", [OFF, ON])
def test_a_step_reads_what_the_scatter_left(gpu, renumber):
    v, t = _cube(5)
    a, b = FemIntegrator(v, t, _fixed_of(v), renumber=renumber), FemIntegrator(v, t, _fixed_of(v), renumber=renumber)
    pts = er.generic_points(v, 400, 15, grow=0.05)
    eid = a.embed(pts)
    bind = a.embedding(eid)
    f = np.random.default_rng(16).standard_normal((400, 3)) * 20.0
    a.set_uniform_force(1, -300.0)
    base = a.external_forces()
    assert np.array_equal(base.reshape(-1, 3), np.tile([0.0, -300.0, 0.0], (len(v), 1)))
    a.embed_add_forces(eid, f)
    host = host_add(base, bind, f)
    assert a.external_forces().tobytes() == host.tobytes()
    b.set_external_forces(host)
    assert b.external_forces().tobytes() == host.tobytes()
    a.do_timestep()
    b.do_timestep()
    qa, qb = a.get_q_state(), b.get_q_state()
    assert np.abs(qa[0]).max() > 0
    assert qa[0].tobytes() == qb[0].tobytes() and qa[1].tobytes() == qb[1].tobytes()
    a.close(); b.close()


# ---- 5. the table is lazy and follows the mesh ----
def _add_and_check(g, eid, seed, n_nodes=None):
    """one dense add on a fresh base: equal to the loop over the binding read AFTER it (the add itself searches what waits for a search)"""
    base = _set_base(g, seed)
    n = g._embed_n[eid]
    f = np.random.default_rng(seed + 1).standard_normal((n, 3))
    g.embed_add_forces(eid, f)
    got = g.external_forces()
    b = g.embedding(eid)
    assert got.tobytes() == host_add(base, b, f).tobytes()
    counts = np.bincount(b["vertices"].ravel(), minlength=g.r // 3)
    fi = g.embed_forces_info(eid)
    assert (fi["longest_run"], fi["n_nodes_touched"]) == (int(counts.max()), int((counts > 0).sum()))
    return fi["n_table_builds"]


def test_ten_adds_build_one_table(gpu):
    v, t = _cube(4)
    g = FemIntegrator(v, t, _fixed_of(v))
    eid = g.embed(er.generic_points(v, 300, 17))
    assert g.embed_forces_info(eid)["n_table_builds"] == 0
    for k in range(10):
        g.embed_add_forces(eid, np.full((300, 3), 1.0 + k))
        g.embed_update(eid)  # (reads change nothing of the binding)
        g.embedding(eid)
    assert g.embed_forces_info(eid)["n_table_builds"] == 1
    # a slot that is released and used again starts at zero
    g.embed_release(eid)
    assert g.embed(er.generic_points(v, 20, 18)) == eid and g.embed_forces_info(eid) == dict(n_table_builds=0, longest_run=0, n_nodes_touched=0)
    g.close()


@pytest.mark.parametrize("renumber", [OFF, ON])
@pytest.mark.parametrize("mode", ["bake", "carry"])
def test_the_table_follows_a_cut(gpu, mode, renumber):
    v, t = _cube(6)
    strip = cr.plane_strip(0.5 * (v.min(0) + v.max(0)) + [0.0013, 0.0007, 0.0003], (1.0, 0.013, 0.007))
    g = FemIntegrator(v, t, _fixed_of(v), renumber=renumber, expect_cuts=True, cg_max_iter=50000)
    g.set_q_state(ci.smooth_displacement(v).reshape(-1), np.zeros(v.size))
    eid = g.embed(er.generic_points(v, 1200, 91, grow=0.05))
    assert _add_and_check(g, eid, 20) == 1
    before = g.embedding(eid)
    info, _ = g.cut(strip, mode=mode)
    assert info["status"] == fl.FB_CUT_DONE, info
    assert not g.external_forces().any() and g.r == 3 * (len(v) + info["n_new_nodes"])
    assert _add_and_check(g, eid, 22) == 2
    assert (g.embedding(eid)["vertices"] != before["vertices"]).any(), "points were bound again to the pieces"
    assert _add_and_check(g, eid, 24) == 2
    g.close()


def test_the_table_follows_resync_delta_and_detach(gpu):
    v, t = er.jittered_cube()
    g = FemIntegrator(v, t, _fixed_of(v))
    eid = g.embed(er.generic_points(v, 800, 51))
    assert _add_and_check(g, eid, 30) == 1
    # another mesh: every point is searched again by the add itself
    v2, t2, _ = delaunay_jittered(4, cellsize=0.1)
    i0 = g.embed_update(eid)[2]["n_locates"]
    g.resync(v2, t2, _fixed_of(v2))
    assert _add_and_check(g, eid, 32) == 2
    assert g.embed_update(eid)[2]["n_locates"] == i0 + 1
    g.close()
    # a change in place that leaves orphans, under both numberings
    v, t = _cube(6)
    fixed = _fixed_of(v)
    for renumber in (OFF, ON):
        g = FemIntegrator(v, t, fixed, renumber=renumber, expect_cuts=True)
        eid = g.embed(er.generic_points(v, 800, 94, grow=0.0))
        assert _add_and_check(g, eid, 34) == 1
        _, _, delta = synthetic_cut(v, t)
        i0 = g.embed_update(eid)[2]["n_locates"]
        g.resync_delta(delta, fixed)
        assert _add_and_check(g, eid, 36) == 2
        assert g.embed_update(eid)[2]["n_locates"] == i0 + 1, "the orphans were searched, once"
        g.close()
    # a part taken out of the parent
    g = FemIntegrator(v, t, fixed, expect_cuts=True)
    eid = g.embed(er.generic_points(v, 800, 94, grow=0.0))
    c = 0.5 * (v.min(0) + v.max(0)) + [0.0013, 0.0007, 0.0003]
    assert g.cut(cr.plane_strip(c, (1.0, 0.013, 0.007)), mode="carry")[0]["status"] == fl.FB_CUT_DONE
    assert _add_and_check(g, eid, 38) == 1
    piece, _, _ = g.detach_part(1, remove=True)
    assert _add_and_check(g, eid, 40) == 2
    piece.close(); g.close()


# ---- 6. the ray ----
def _sheet(lo, hi, k=12):
    """k x k points of a curved height field inside the box and the 2 (k - 1)^2 triangles over them"""
    s, u = np.meshgrid(np.linspace(0.08, 0.92, k), np.linspace(0.1, 0.9, k), indexing="ij")
    p = np.stack([s, u, 0.5 + 0.18 * np.sin(3.1 * s + 0.4) * np.cos(2.3 * u - 0.2) + 0.1 * s * u], axis=-1).reshape(-1, 3)
    idx = np.arange(k * k).reshape(k, k)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    return lo + p * (hi - lo), np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]).astype(np.int32)


def _uv_sphere(centre, radius, n_lat=12, n_lon=22):
    """a closed sphere: two poles, n_lat - 1 rings of n_lon points, 2 n_lon (n_lat - 1) triangles"""
    th = np.pi * np.arange(1, n_lat) / n_lat
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.cos(th), np.ones(n_lon)), np.outer(np.sin(th), np.sin(ph))], axis=-1).reshape(-1, 3)
    p = np.vstack([[0.0, 1.0, 0.0], ring, [0.0, -1.0, 0.0]])
    rid = 1 + np.arange((n_lat - 1) * n_lon).reshape(n_lat - 1, n_lon)
    nxt = np.roll(rid, -1, axis=1)
    tri = [np.stack([np.zeros(n_lon, int), nxt[0], rid[0]], 1), np.stack([np.full(n_lon, len(p) - 1), rid[-1], nxt[-1]], 1)]
    for r in range(n_lat - 2):
        tri += [np.stack([rid[r], nxt[r], rid[r + 1]], 1), np.stack([nxt[r], nxt[r + 1], rid[r + 1]], 1)]
    return centre + radius * p, np.concatenate(tri).astype(np.int32)


def ray_hits(P, tri, o, d, t_max=np.inf):
    """Moeller-Trumbore in fp64 over every triangle: (hit mask, t, u, v)"""
    a, b, c = P[tri[:, 0]], P[tri[:, 1]], P[tri[:, 2]]
    e1, e2 = b - a, c - a
    pv = np.cross(d[None, :], e2)
    det = (e1 * pv).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        tv = o[None, :] - a
        u = (tv * pv).sum(axis=1) * inv
        qv = np.cross(tv, e1)
        v = (qv * d[None, :]).sum(axis=1) * inv
        tt = (e2 * qv).sum(axis=1) * inv
        hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (tt >= 0) & (tt <= t_max)
    return hit, tt, u, v


def nearest_generic_hit(P, tri, o, d):
    """the nearest hit of a ray that must be generic: (triangle, t, u, v)"""
    hit, tt, u, v = ray_hits(P, tri, o, d)
    ids = np.nonzero(hit)[0]
    assert len(ids) >= 1, "the ray was aimed at a triangle"
    order = ids[np.argsort(tt[ids], kind="stable")]
    k = order[0]
    assert len(order) == 1 or tt[order[1]] - tt[k] > 1e-6, "two hits within 1e-6 in t: choose another seed"
    assert min(u[k], v[k], 1.0 - u[k] - v[k]) > 1e-6, "the nearest hit is within 1e-6 of an edge: choose another seed"
    return int(k), tt[k], u[k], v[k]


@pytest.fixture(scope="module")
def ray_scene(gpu):
    """a truth_cube(5) after two steps under load with the two surfaces embedded; the fp64 positions the bindings give at that state"""
    v, t = _cube(5)
    g = FemIntegrator(v, t, _fixed_of(v))
    lo, hi = v.min(0), v.max(0)
    surf = {"sheet": _sheet(lo, hi), "sphere": _uv_sphere(0.5 * (lo + hi), 0.4 * (hi - lo).min())}
    assert len(surf["sheet"][1]) == 242 and 450 <= len(surf["sphere"][1]) <= 550
    out = {}
    for name, (p, tri) in surf.items():
        out[name] = dict(eid=g.embed(p, tri), tri=tri)
    for _ in range(2):
        g.set_uniform_force(1, -300.0)
        g.do_timestep()
    x0, _ = g.read_mesh()
    q = g.get_q_state()[0]
    assert np.abs(q).max() > 1e-5
    for name in out:
        b = g.embedding(out[name]["eid"])
        out[name]["P"] = er.positions(x0, q, b["vertices"], b["weights"])
        out[name]["binding"] = b
    out["g"] = g
    yield out
    g.close()


def _rays(P, tri, n, seed, kind):
    """n rays from outside towards an interior point of a random triangle each"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(tri), n)
    uv = rng.random((n, 2))
    flip = uv.sum(axis=1) > 1
    uv[flip] = 1.0 - uv[flip]
    uv = 1.0 / 3 + 0.8 * (uv - 1.0 / 3)  # (well inside the triangle)
    a, b, c = P[tri[k, 0]], P[tri[k, 1]], P[tri[k, 2]]
    target = a + uv[:, :1] * (b - a) + uv[:, 1:] * (c - a)
    centre = 0.5 * (P.min(0) + P.max(0))
    if kind == "sphere":  # from outside, roughly along the radius through the target
        away = target - centre
        away = away / np.linalg.norm(away, axis=1)[:, None] + 0.3 * rng.standard_normal((n, 3))
    else:                 # from either side of the sheet, steeply
        away = np.stack([0.4 * rng.standard_normal(n), 0.4 * rng.standard_normal(n), rng.choice([-1.0, 1.0], n)], axis=1)
    origin = target + 2.0 * away / np.linalg.norm(away, axis=1)[:, None]
    return origin, 1.3 * (target - origin)  # (the aimed-at point lies at t = 1 / 1.3)


@pytest.mark.parametrize("name", ["sheet", "sphere"])
def test_ray_pick_equals_numpy(ray_scene, name):
    g, S = ray_scene["g"], ray_scene[name]
    P, tri = S["P"], S["tri"]
    lo, hi = P.min(0), P.max(0)
    origin, direction = _rays(P, tri, 200, 41 if name == "sheet" else 42, name)
    assert ((origin < lo - 0.5) | (origin > hi + 0.5)).any(axis=1).all(), "every origin lies outside"
    worst = np.zeros(3)
    n_other = 0
    for o, d in zip(origin, direction):
        k, t_ref, u_ref, v_ref = nearest_generic_hit(P, tri, o, d)
        hit = g.embed_pick_ray(S["eid"], o, d)
        assert hit["triangle"] == k, (hit, k, t_ref)
        err = np.array([abs(hit["t"] - t_ref) / (1 + abs(t_ref)), np.abs(hit["bary"] - [u_ref, v_ref]).max(), np.abs(hit["xyz"] - (o + t_ref * d)).max()])
        worst = np.maximum(worst, err)
        n_other += abs(t_ref - 1 / 1.3) > 1e-6
    print("%s: worst errors t %.3g, barycentrics %.3g, xyz %.3g; %d rays hit another triangle first" % (name, worst[0], worst[1], worst[2], n_other))
    assert (worst <= 1e-9).all(), worst


def test_ray_pick_edge_cases(ray_scene):
    g, S = ray_scene["g"], ray_scene["sheet"]
    P, tri, eid = S["P"], S["tri"], S["eid"]
    centroid = P[tri[37]].mean(axis=0)
    o, d = centroid + [0.0, 0.0, 1.0], np.array([0.0, 0.0, -1.0])
    k, t_ref, _, _ = nearest_generic_hit(P, tri, o, d)
    assert k == 37 and g.embed_pick_ray(eid, o, d)["triangle"] == 37
    # pointing away; ending short of the hit; reaching it exactly when t_max allows
    miss = g.embed_pick_ray(eid, o, -d)
    assert miss["triangle"] == -1 and miss["t"] == 0 and not miss["bary"].any()
    assert g.embed_pick_ray(eid, o, d, t_max=0.5 * t_ref)["triangle"] == -1
    assert g.embed_pick_ray(eid, o, d, t_max=2.0 * t_ref)["triangle"] == 37
    assert g.embed_pick_ray(eid, o, d, t_max=-1.0)["triangle"] == -1
    # the sheet has two sides
    back = g.embed_pick_ray(eid, centroid - [0.0, 0.0, 1.0], -d)
    assert back["triangle"] == 37
    # a direction that is no unit vector scales t
    long = g.embed_pick_ray(eid, o, 4.0 * d)
    assert long["triangle"] == 37 and abs(long["t"] - t_ref / 4.0) <= 1e-9
    # one triangle listed twice, 300 triangles apart (other workgroups): an exact tie, the lower id
    rest = S["binding"]["rest_xyz"]
    tri2 = np.vstack([tri[37:38], tri, tri, tri[37:38]]).astype(np.int32)
    e2 = g.embed(rest, tri2)
    hits, tt, _, _ = ray_hits(P, tri2, o, d)
    ids = np.nonzero(hits)[0]
    assert list(ids) == [0, 38, 242 + 38, 485] and len(set(tt[ids].tolist())) == 1
    assert g.embed_pick_ray(e2, o, d)["triangle"] == 0
    g.embed_release(e2)
    # no triangles
    e3 = g.embed(rest)
    assert g.embed_pick_ray(e3, o, d)["triangle"] == -1
    g.embed_release(e3)
    # refused directions
    for bad in ([0.0, 0.0, 0.0], [0.0, np.nan, 1.0], [np.inf, 0.0, 0.0]):
        assert _einval(lambda: g.embed_pick_ray(eid, o, bad))
    assert _einval(lambda: g.embed_pick_ray(eid, [np.nan, 0, 0], d))


# ---- 7. the closest point ----
def test_point_pick_equals_numpy(ray_scene):
    g, S = ray_scene["g"], ray_scene["sphere"]
    P, eid = S["P"], S["eid"]
    rng = np.random.default_rng(43)
    lo, hi = P.min(0), P.max(0)
    for w in np.vstack([lo - 0.2 + rng.random((40, 3)) * (hi - lo + 0.4), P[17] + [1e-6, -2e-6, 3e-6], P[0] + 1e-9]):
        d = P - w
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        k = int(np.argmin(d2))
        two = np.sort(d2)[:2]
        assert two[1] - two[0] > 1e-12 * max(two[1], 1e-30), "two points at the same distance up to rounding: choose another seed"
        idx, xyz, dist2 = g.embed_pick_point(eid, w)
        assert idx == k and abs(dist2 - d2[k]) <= 1e-12 * d2[k] and np.abs(xyz - P[k]).max() <= 1e-12
    # two coincident points 600 apart (other workgroups): the lower id
    v = np.asarray(g.verts, np.float64).reshape(-1, 3)
    pts = er.generic_points(v, 600, 44, grow=0.0)
    pts = np.vstack([pts, pts[10:11], pts[599:600]])
    e2 = g.embed(pts)
    b = g.embedding(e2)
    x0, _ = g.read_mesh()
    P2 = er.positions(x0, g.get_q_state()[0], b["vertices"], b["weights"])
    assert P2[600].tobytes() == P2[10].tobytes() and P2[601].tobytes() == P2[599].tobytes()
    assert g.embed_pick_point(e2, P2[10] + [1e-7, 0, 0])[0] == 10
    idx, xyz, dist2 = g.embed_pick_point(e2, P2[599] - [0, 1e-7, 0])
    assert idx == 599 and abs(dist2 - 1e-14) <= 1e-18 and np.abs(xyz - P2[599]).max() <= 1e-12
    g.embed_release(e2)


# ---- 8. stress ----
def test_embed_stress(gpu):
    v, t = _cube(6)
    for renumber in (OFF, ON):
        g = FemIntegrator(v, t, _fixed_of(v), renumber=renumber, expect_cuts=True)
        eid = g.embed(er.generic_points(v, 900, 45, grow=0.05))
        assert _einval(lambda: g.embed_stress(eid)), "no stress() yet"
        with pytest.raises(fl.FbError) as e1:
            g.embed_stress(eid)
        with pytest.raises(fl.FbError) as e2:
            g.surface_stress()
        assert str(e1.value).replace("fb_fem_embed_stress", "X") == str(e2.value).replace("fb_fem_read_stress", "X").replace("fb_fem_surface_stress", "X")
        for _ in range(2):
            g.set_uniform_force(1, -300.0)
            g.do_timestep()
        g.stress()
        vm = g.element_stress()["von_mises"]
        got = g.embed_stress(eid)
        assert got.dtype == np.float32 and got.tobytes() == vm[g.embedding(eid)["elements"]].astype(np.float32).tobytes() and got.max() > 0
        # a cut makes the stress stale until stress() has run again
        c = 0.5 * (v.min(0) + v.max(0)) + [0.0013, 0.0007, 0.0003]
        assert g.cut(cr.plane_strip(c, (1.0, 0.013, 0.007)), mode="carry")[0]["status"] == fl.FB_CUT_DONE
        assert _einval(lambda: g.embed_stress(eid))
        g.stress()
        vm = g.element_stress()["von_mises"]
        assert g.embed_stress(eid).tobytes() == vm[g.embedding(eid)["elements"]].astype(np.float32).tobytes()
        g.close()


# ---- 9. Deformable ----
def test_touch_embedded_adds_what_embed_add_forces_adds(gpu):
    v, t = _cube(5)
    fixed = np.nonzero(v[:, 0] == v[:, 0].min())[0]
    d, twin = Deformable(v, t, fixed), Deformable(v, t, fixed)
    pts, tri = _sheet(v.min(0), v.max(0))
    eid, e2 = d.embed(pts, tri), twin.embed(pts, tri)
    for body in (d, twin):
        body.timestep()
        body.integrator.set_uniform_force(1, body.GRAVITY_FORCE)
    base = d.external_forces()
    assert base.tobytes() == twin.external_forces().tobytes()
    centroid = d.embedded_mesh(eid)[0][tri[100]].astype(np.float64).mean(axis=0)
    o, direction, force = centroid + [0.002, -0.003, 1.0], np.array([0.0, 0.0, -1.0]), np.array([3.0, -40.0, 7.5])
    want = twin.embed_pick_ray(e2, o, direction)
    hit = d.touch_embedded(eid, o, direction, force)
    assert hit["triangle"] == want["triangle"] >= 0 and hit["t"] == want["t"] and np.array_equal(hit["bary"], want["bary"])
    u, w = want["bary"]
    ids = tri[want["triangle"]]
    order = np.argsort(ids)
    f3 = (np.array([1.0 - u - w, u, w])[:, None] * force[None, :])[order]
    assert np.array_equal(hit["point_ids"], ids[order]) and (np.diff(hit["point_ids"]) > 0).all() and np.array_equal(hit["forces"], f3)
    twin.embed_add_forces(e2, f3, ids[order])
    got = d.external_forces()
    assert got.tobytes() == twin.external_forces().tobytes() == host_add(base, d.integrator.embedding(eid), f3, ids[order]).tobytes()
    assert got.tobytes() != base.tobytes()
    assert abs((got - base).reshape(-1, 3).sum(axis=0) - force).max() < 1e-9 * np.abs(force).max(), "the weights of a point sum to one: the force arrives whole"
    # a miss adds nothing
    miss = d.touch_embedded(eid, o, -direction, force)
    assert miss["triangle"] == -1 and d.external_forces().tobytes() == got.tobytes()


def test_a_handle_that_uses_none_of_this_steps_the_same(gpu):
    v, t = _cube(5)
    a, b = FemIntegrator(v, t, _fixed_of(v)), FemIntegrator(v, t, _fixed_of(v))
    for _ in range(3):
        for g in (a, b):
            g.set_uniform_force(1, -300.0)
        assert np.array_equal(b.external_forces()[1::3], np.full(len(v), -300.0))
        a.do_timestep()
        b.do_timestep()
    for x, y in zip(a.get_q_state(), b.get_q_state()):
        assert x.tobytes() == y.tobytes()
    a.close(); b.close()
