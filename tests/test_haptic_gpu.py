"""The haptic probe on the device (fb_fem_add_haptic_forces / fb_fem_pick_vertex / fb_fem_pick_box / fb_fem_volume) against its host
restatements: ``fembrain_amd.fem.spread_haptic_forces`` on the handle's own pattern, and tests/hapticref.py.

The handle has no entry point that reads the external force vector back, so the spread is compared through the state after one step: a
second handle of the same mesh is fed the host-spread vector through ``set_external_forces``, and q and qvel of the two must be equal
bit for bit (the step is deterministic, and one differing bit of the load moves the solution)."""
import math

import numpy as np
import pytest

import cut_inputs as ci
import hapticref as hr
from fembrain_amd import lib as fl
from fembrain_amd.fem import Deformable, FemIntegrator, spread_haptic_forces
from fembrain_amd.meshgen import cube_fixed_plane_i0, delaunay_jittered, fixed_vertices_to_dofs, truth_cube

pytestmark = pytest.mark.gpu

OFF, ON = fl.FB_RENUMBER_OFF, fl.FB_RENUMBER_ON
BATCH = 32          # kHapticBatch of fembrain_amd/csrc/haptic.h
GRAVITY = -10000.0
FORCE = np.array([137.3, 2503.1, -419.7])   # (no power of two: every fall-off product rounds)


def _cube(nx, ny, nz):
    v, t = truth_cube(nx, ny, nz, 0.1)
    return v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(ny, nz))


def _delaunay():
    v, t, fv = delaunay_jittered(6)
    return v, t, fixed_vertices_to_dofs(fv)


MESHES = {"cube4": (lambda: _cube(4, 4, 4), {}), "cube5": (lambda: _cube(5, 5, 5), {}), "cube976": (lambda: _cube(9, 7, 6), {}),
          "delaunay_on": (_delaunay, dict(renumber=ON)), "delaunay_off": (_delaunay, dict(renumber=OFF))}


class Pair:
    """two handles of one mesh: `dev` gets its probe forces on the device, `host` the host-spread vector"""

    def __init__(self, v, t, fixed, **kw):
        self.dev, self.host = FemIntegrator(v, t, fixed, **kw), FemIntegrator(v, t, fixed, **kw)
        self.pattern = None
        self.fixed_node = int(np.asarray(fixed)[0]) // 3

    def both(self):
        return (self.dev, self.host)

    def close(self):
        for g in self.both():
            g.close()

    def spread_pattern(self):
        if self.pattern is None:
            self.pattern = self.host.pattern()
        return self.pattern

    def host_vector(self, ids, forces, size, gravity):
        f = np.zeros(self.host.r)
        if gravity:
            f[1::3] = GRAVITY
        bptr, bcol = self.spread_pattern()
        return spread_haptic_forces(bptr, bcol, [int(i) for i in ids], [tuple(x) for x in np.asarray(forces, np.float64).reshape(-1, 3)], size, f)

    def step_both(self, f_host):
        self.host.set_external_forces(f_host)
        self.dev.do_timestep()
        self.host.do_timestep()
        (qa, va, _), (qb, vb, _) = self.dev.get_q_state(), self.host.get_q_state()
        return np.array_equal(qa, qb) and np.array_equal(va, vb) and bool(np.abs(qa).max() > 0)

    def check(self, ids, forces, size, gravity=True):
        for g in self.both():
            g.reset_to_rest()
        if gravity:
            self.dev.set_uniform_force(1, GRAVITY)
        else:
            self.dev.set_external_forces_to_zero()
        self.dev.add_haptic_forces(ids, forces, size)
        f = self.host_vector(ids, forces, size, gravity)
        assert self.step_both(f), (list(ids), size, gravity)
        return f


@pytest.fixture(scope="module")
def pairs(gpu):
    made = {}

    def get(name):
        if name not in made:
            build, kw = MESHES[name]
            made[name] = Pair(*build(), **kw)
        return made[name]
    yield get
    for p in made.values():
        p.close()


def _centre_node(v):
    return int(np.argmin(((v - v.mean(0)) ** 2).sum(1)))


def _forces(n, seed=3):
    rng = np.random.default_rng(seed)
    return FORCE[None, :] * rng.uniform(0.3, 1.7, size=(n, 1)) * np.where(rng.uniform(size=(n, 3)) < 0.3, -1.0, 1.0)


def _source_sets(p):
    g = p.host
    v, n = g.verts, g.n_nodes
    c = _centre_node(v)
    near = int(np.argsort(((v - v[c]) ** 2).sum(1))[1])                       # the node closest to the centre one: the balls overlap
    many = np.random.default_rng(11).permutation(n)[:BATCH + 1]
    return {"one": [c], "two_overlapping": [c, near], "same_id_twice": [c, c], "clamped": [p.fixed_node, c], "batch_plus_one": [int(i) for i in many],
            "batch_plus_one_with_repeats": [int(i) for i in many[:BATCH]] + [int(many[3])], "none": []}


@pytest.mark.parametrize("name", list(MESHES))
def test_spread_is_the_host_spread_bit_for_bit(pairs, name):
    p = pairs(name)
    kw = MESHES[name][1]
    if "renumber" in kw:
        assert p.dev.renumbering()[0] == (kw["renumber"] == ON)
    sets = _source_sets(p)
    for size in (1, 2, 5):
        for label, ids in sets.items():
            f = p.check(ids, _forces(len(ids)), size)
            if label == "one" and size == 5:
                assert np.count_nonzero(f[0::3]) > 5          # (the load does spread: x components come from the probe only)
    # a vector that is not gravity to start from, and no gravity at all
    p.check(sets["two_overlapping"], _forces(2, 5), 5, gravity=False)


def test_rings_that_exhaust_the_mesh_add_nothing(pairs):
    p = pairs("cube5")
    c = _centre_node(p.host.verts)
    f12 = p.check([c, 0], _forces(2), 12)
    assert np.count_nonzero(f12[0::3]) == p.host.n_nodes    # every node was reached ...
    f = np.zeros(p.host.r)
    spread_haptic_forces(*p.spread_pattern(), [c], [tuple(FORCE)], 12, f)
    ring = np.rint((1.0 - f[0::3] / FORCE[0]) * 12).astype(int)
    assert ring.min() == 0 and ring.max() < 11               # ... before the 11 passes are over: the last ones find no frontier


def test_refusals_leave_the_force_vector_alone(pairs):
    p = pairs("cube4")
    n = p.dev.n_nodes
    for g in p.both():
        g.reset_to_rest()
    p.dev.set_uniform_force(1, GRAVITY)
    too_many = [i % n for i in range(fl.FB_HAPTIC_MAX_SOURCES + 1)]
    for ids, size in (([-1], 5), ([n], 5), ([3, n], 5), ([3, -1, 4], 5), ([3], 0), ([3], 256), ([3], -2), (too_many, 2)):
        with pytest.raises(fl.FbError) as e:
            p.dev.add_haptic_forces(ids, _forces(len(ids)), size)
        assert e.value.code == fl.FB_EINVAL, (ids, size)
    assert p.step_both(p.host_vector([], [], 5, True))


def test_spread_after_a_cut(gpu):
    v, t, fixed = _cube(6, 6, 6)
    _, _, strip = ci.random_planes(7, 1, centre=v.mean(0), spread=0.03, half=10.0)[0]
    p = Pair(v, t, fixed, expect_cuts=True)
    try:
        n_before = p.dev.n_nodes
        p.check([_centre_node(v)], _forces(1), 5)             # (a level array of the old size exists before the cut)
        deltas = []
        for g in p.both():
            g.reset_to_rest()
            info, delta = g.cut(strip)
            assert info["status"] == fl.FB_CUT_DONE and info["n_new_nodes"] > 0
            deltas.append(delta)
        p.pattern = None
        assert p.dev.n_nodes == p.host.n_nodes > n_before
        src = int(deltas[0]["edge_nodes"][0, 0])             # an old node on a cut edge: beside the cut
        f = p.check([src], _forces(1), 3, gravity=False)
        # the post-cut pattern, not the old one: the blade went through the whole cube, so the walk stays on the source's side.  (These
        # properties are read off the HOST vector: no entry point reads fext back, so they hold for the device through the bitwise step
        # comparison inside p.check only -- which does not see a force on a clamped DOF.)
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import connected_components
        bptr, bcol = p.spread_pattern()
        n = p.host.n_nodes
        ncomp, comp = connected_components(csr_matrix((np.ones(len(bcol)), bcol, bptr), shape=(n, n)), directed=False)
        assert ncomp == 2
        got = np.abs(f.reshape(-1, 3)).sum(1) > 0
        assert not got[comp != comp[src]].any()              # nothing across the cut
        assert got[n_before:][comp[n_before:] == comp[src]].any()   # new nodes on the source's side are reached
        other = int(deltas[0]["edge_nodes"][0, 1])            # the far end of that edge was a neighbour before the cut
        assert comp[other] != comp[src] and not got[other]
        # volume after the cut (the mesh the device holds: read_mesh's order)
        _check_volume(p.dev)
    finally:
        p.close()


def test_spread_after_resync_to_other_meshes(gpu):
    v, t, fixed = _cube(9, 7, 6)
    p = Pair(v, t, fixed)
    try:
        p.check([_centre_node(v), 0], _forces(2), 5)
        for build in (lambda: _cube(4, 4, 4), _delaunay):      # smaller, then larger and unstructured: stale sizes, a stale level array
            v2, t2, fixed2 = build()
            for g in p.both():
                g.resync(v2, t2, fixed2)
            p.pattern = None
            ids = [_centre_node(v2), 1, int(len(v2) - 1)]
            p.check(ids, _forces(3), 5)
            _check_pick(p.dev, (10.0, 0.2, 10.0))
            _check_volume(p.dev)
    finally:
        p.close()


def test_host_built_plan(gpu, monkeypatch):
    monkeypatch.setenv("FEMBRAIN_PLAN_DEVICE", "0")
    v, t, fixed = _cube(5, 5, 5)
    p = Pair(v, t, fixed)
    try:
        assert p.dev._L.fb_fem_plan_on_device(p.dev.h) == 0
        c = _centre_node(v)
        p.check([c, c + 1, 0], _forces(3), 5)
        _check_pick(p.dev, (10.0, 0.2, 10.0))
        _check_box(p.dev, (-1.0, -1.0, -1.0), (0.0, 1.0, 1.0))
        _check_volume(p.dev)
    finally:
        p.close()


# ---- pick ----

def _current(g):
    """x0 + q of the handle, and its mesh, as the host sees them"""
    return hr.positions(g.verts, g.get_q_state()[0])


def _check_pick(g, wpos):
    i, xyz, d = hr.pick_vertex(_current(g), wpos)
    gi, gxyz, gd = g.pick_vertex(wpos)
    assert gi == i and np.array_equal(gxyz, xyz) and gd == d, (wpos, gi, i, gd, d)
    return i


def _load_steps(g, steps=3):
    f = np.zeros(g.r)
    f[1::3] = GRAVITY
    f[0::3] = 3000.0 * np.sin(np.arange(g.n_nodes))
    for _ in range(steps):
        g.set_external_forces(f)
        g.do_timestep()
    assert np.abs(g.get_q_state()[0]).max() > 1e-4


def test_pick_far_point_and_after_loaded_steps(pairs):
    g = pairs("cube5").dev
    g.reset_to_rest()
    n = 5
    assert _check_pick(g, (10.0, 0.2, 10.0)) in [(n - 1) * n * n + j * n + (n - 1) for j in range(n)]
    _check_pick(g, (-3.0, 7.0, 0.013))
    _load_steps(g)
    _check_pick(g, (10.0, 0.2, 10.0))
    _check_pick(g, (0.01, 0.17, -0.02))
    g.reset_to_rest()


def _snapped_delaunay():
    """meshgen.delaunay_jittered(6) with its coordinates rounded to multiples of 2^-12 (a move of at most 1.3e-4 where the cells are 0.1
    wide): sums, halves and squared differences of such coordinates are exact in fp64, so a point can lie EXACTLY midway between two
    nodes.  Elements the rounding flattened are dropped as the generator drops its slivers."""
    v, t, fv = delaunay_jittered(6)
    v = np.rint(v * 4096.0) / 4096.0
    vol = np.einsum("ij,ij->i", v[t[:, 1]] - v[t[:, 0]], np.cross(v[t[:, 2]] - v[t[:, 0]], v[t[:, 3]] - v[t[:, 0]])) / 6
    t = np.ascontiguousarray(t[vol > 1e-9])
    assert len(np.unique(t)) == len(v)
    return v, t, fixed_vertices_to_dofs(fv)


def test_pick_tie_takes_the_lowest_caller_id(gpu):
    v, t, fixed = _snapped_delaunay()
    g = FemIntegrator(v, t, fixed, renumber=ON)
    try:
        assert g.renumbering()[0]
        new_of_old = np.empty(len(v), np.int64)
        new_of_old[g.owned_nodes()] = np.arange(len(v))
        assert not np.array_equal(new_of_old, np.arange(len(v)))
        d2 = ((v[:, None, :] - v[None, :, :]) ** 2).sum(2)
        iu = np.triu_indices(len(v), 1)
        tried = 0
        for k in np.argsort(d2[iu])[:400]:
            a, b = int(iu[0][k]), int(iu[1][k])                      # a < b
            if new_of_old[a] < new_of_old[b]:
                continue                                             # (the internal order would give the same answer)
            w = (v[a] + v[b]) / 2.0
            dx = v - w
            d = (dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1]) + dx[:, 2] * dx[:, 2]
            if d[a] != d[b] or np.count_nonzero(d <= d[a]) != 2:
                continue
            assert _check_pick(g, w) == a
            tried += 1
            if tried == 4:
                break
        assert tried == 4
    finally:
        g.close()


# ---- box ----

def _check_box(g, lo, hi):
    ids, xyz = hr.pick_box(_current(g), lo, hi)
    n, gids, gxyz = g.pick_box(lo, hi)
    assert n == len(ids) and np.array_equal(gids, ids) and np.array_equal(gxyz, xyz), (lo, hi, n, len(ids))
    assert g.pick_box(lo, hi, capacity=0) == (len(ids), None, None)
    return ids


def test_box(pairs):
    g = pairs("cube5").dev
    g.reset_to_rest()
    v = g.verts
    # bounds exactly on lattice coordinates: the planes of the bounds belong to the box
    ids = _check_box(g, v[31], v[93])                 # (1,1,1) .. (3,3,3)
    assert len(ids) == 27 and ids[0] == 31 and ids[-1] == 93
    assert len(_check_box(g, v[62], v[62])) == 1      # a box that is one node
    assert len(_check_box(g, (5.0, 5.0, 5.0), (6.0, 6.0, 6.0))) == 0
    assert len(_check_box(g, (0.3, 0.0, 0.0), (0.2, 1.0, 1.0))) == 0      # lo > hi
    assert len(_check_box(g, v.min(0), v.max(0))) == 125
    # capacity below the count: the full count, the first entries, nothing beyond them
    want, wxyz = hr.pick_box(v, v[31], v[93])
    ids_buf, xyz_buf = np.full(40, -7, np.int32), np.full((40, 3), -7.0)
    n, gids, gxyz = g.pick_box(v[31], v[93], capacity=10, ids=ids_buf, xyz=xyz_buf)
    assert n == 27 and np.array_equal(gids, want[:10]) and np.array_equal(gxyz, wxyz[:10]) and (np.diff(gids) > 0).all()
    assert (ids_buf[10:] == -7).all() and (xyz_buf[10:] == -7.0).all()
    # capacity above the count: nothing beyond the count is touched either
    ids_buf[:], xyz_buf[:] = -7, -7.0
    n, gids, _ = g.pick_box(v[31], v[93], capacity=40, ids=ids_buf, xyz=xyz_buf)
    assert n == 27 and np.array_equal(gids, want) and (ids_buf[27:] == -7).all() and (xyz_buf[27:] == -7.0).all()
    # on the displaced mesh, and on a renumbered unstructured one
    _load_steps(g)
    _check_box(g, v[31], v[93])
    _check_box(g, (-1.0, -1.0, -1.0), (-0.24, 1.0, 1.0))
    g.reset_to_rest()
    d = pairs("delaunay_on").dev
    d.reset_to_rest()
    assert 0 < len(_check_box(d, (0.1, 0.1, 0.1), (0.35, 0.4, 0.3))) < d.n_nodes


# ---- volume ----

def _check_volume(g):
    """per element bitwise, the total within the worst case of any summation order, and the same bits twice"""
    x0, tets = g.read_mesh()
    want = hr.element_volumes(hr.positions(x0, g.get_q_state()[0]), tets)
    total, per = g.volume(per_element=True)
    assert np.array_equal(per, want)
    assert abs(total - math.fsum(per)) <= len(per) * 2.0 ** -53 * float(np.sum(per))
    assert g.volume() == total and g.volume(per_element=True)[0] == total
    return total


@pytest.mark.parametrize("name", ["cube4", "cube976", "delaunay_on"])
def test_volume_at_rest_and_after_loaded_steps(pairs, name):
    g = pairs(name).dev
    g.reset_to_rest()
    rest = _check_volume(g)
    if name == "cube976":
        assert abs(rest - 0.8 * 0.6 * 0.5) < 1e-13
    _load_steps(g)
    assert _check_volume(g) != rest
    g.reset_to_rest()


def test_volume_total_does_not_depend_on_the_numbering(pairs):
    a, b = pairs("delaunay_on").dev, pairs("delaunay_off").dev
    for g in (a, b):
        g.reset_to_rest()
    assert a.renumbering()[0] and not b.renumbering()[0]
    ta, pa = a.volume(per_element=True)
    tb, pb = b.volume(per_element=True)
    assert np.array_equal(pa, pb) and ta == tb


# ---- the driver ----

def _drive(on_device, cut_strip=None):
    v, t, _ = _cube(6, 6, 6)
    d = Deformable(v, t, fixed_vertices=cube_fixed_plane_i0(6, 6), haptic_on_device=on_device, expect_cuts=True)
    try:
        assert not d.haptic_start_at((-10.0, 0.33, 10.0))     # a clamped node cannot be pulled
        assert d.haptic_start_at((10.0, 0.33, 10.0))
        pulled = d.pick_vertex((10.0, 0.33, 10.0))[0]
        d.haptic_set_current_forces([pulled, pulled - 1], [(0.0, 2500.0, 300.0), (-200.0, 900.0, 0.0)])
        for step in range(3):
            d.timestep()
            if cut_strip is not None and step == 0:
                info, _ = d.cut(cut_strip)
                assert info["status"] == fl.FB_CUT_DONE
        q, qv, _ = d.integrator.get_q_state()
        vol = d.compute_volume()
        at = d.pick_vertex((10.0, 0.33, 10.0))[1]
        box = d.pick_vertices(at - 0.25, at + 0.25)[1]       # around where the free end's corner has got to
        assert len(box) > 1
        return pulled, q, qv, vol, box, len(d.integrator.tets)
    finally:
        d.integrator.close()


@pytest.mark.parametrize("with_cut", [False, True])
def test_driver_device_route_is_the_host_route(gpu, with_cut):
    strip = None
    if with_cut:
        v, _, _ = _cube(6, 6, 6)
        strip = ci.random_planes(7, 1, centre=v.mean(0), spread=0.03, half=10.0)[0][2]
    pa, qa, va, vola, boxa, n_tets = _drive(True, strip)
    pb, qb, vb, volb, boxb, _ = _drive(False, strip)
    assert pa == pb and np.array_equal(qa, qb) and np.array_equal(va, vb) and np.abs(qa).max() > 0
    assert np.array_equal(boxa, boxb)
    assert abs(vola - volb) <= 2 * n_tets * 2.0 ** -53 * volb      # (two summation orders of the same element volumes)


def test_example_runs(gpu):
    """examples/haptic_probe.py is documentation that must not rot"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "haptic_probe.py"), "6", "2"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "picked node" in out.stdout and "volume drift:" in out.stdout


def test_pick_box_volume_on_more_than_256_workgroups(gpu):
    """67,200 nodes and 383,214 elements: the single-workgroup folds of the per-workgroup partials take their strided paths (more than 256
    partials), at a state set directly (no step is needed for a displaced mesh)"""
    v, t, fixed = _cube(42, 40, 40)
    g = FemIntegrator(v, t, fixed, renumber=ON)
    try:
        assert g.n_nodes > 256 * 256 and len(t) > 256 * 256
        g.set_q_state(ci.smooth_displacement(v, scale=0.03).reshape(-1))
        p = _current(g)
        # the vectorised form of hapticref.pick_vertex (argmin takes the first of equal minima)
        for w in ((10.0, 0.2, 10.0), tuple(p[40000] + 1e-3), tuple((p[123] + p[124]) / 2.0)):
            dx = p - np.asarray(w)
            d = (dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1]) + dx[:, 2] * dx[:, 2]
            i = int(np.argmin(d))
            gi, gxyz, gd = g.pick_vertex(w)
            assert gi == i and gd == d[i] and np.array_equal(gxyz, p[i])
        assert len(_check_box(g, p.min(0), p.max(0))) == g.n_nodes              # every workgroup full, the scan over 263 counts
        assert 1000 < len(_check_box(g, (-1.0, 0.5, -0.7), (0.3, 2.0, 0.9))) < g.n_nodes
        _check_volume(g)
    finally:
        g.close()
