"""The probe's box contact on the device (fb_fem_contact_move / _info_get / _reset / fb_fem_read_contact / fb_fem_contact_apply) against
its host restatements: ``fembrain_amd.fem.ProbeContact`` on the positions read back, ``spread_haptic_forces`` on the handle's own
pattern, and the record count of tests/contactref.py.  Everything is compared with ``np.array_equal``."""
import numpy as np
import pytest

import contactref as cr
import cutref
from fembrain_amd import lib as fl
from fembrain_amd.fem import Deformable, FemIntegrator, ProbeContact
from fembrain_amd.meshgen import cube_fixed_plane_i0, delaunay_jittered, fixed_vertices_to_dofs, truth_cube

pytestmark = pytest.mark.gpu

OFF, ON = fl.FB_RENUMBER_OFF, fl.FB_RENUMBER_ON
MISS, EMPTY, SET = fl.FB_CONTACT_MISS, fl.FB_CONTACT_EMPTY, fl.FB_CONTACT_SET
BOTTOM, LEFT = 2, 0


def _cube(nx, ny, nz, cell=0.1):
    v, t = truth_cube(nx, ny, nz, cell)
    return v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(ny, nz))


def _delaunay():
    v, t, fv = delaunay_jittered(6)
    return v, t, fixed_vertices_to_dofs(fv)


MESHES = {"cube5": (lambda: _cube(5, 5, 5), {}), "cube12x8x12": (lambda: _cube(12, 8, 12), {}),
          "delaunay_on": (_delaunay, dict(renumber=ON)), "delaunay_off": (_delaunay, dict(renumber=OFF))}


# 1. session parity
@pytest.mark.parametrize("name", list(MESHES))
def test_session_parity(gpu, name):
    build, kw = MESHES[name]
    g = FemIntegrator(*build(), **kw)
    try:
        fresh = g.contact_info()
        assert (fresh["status"], fresh["n_touched"], fresh["face"], fresh["closest_node"], fresh["list_size"], fresh["n_clears"]) == (0, 0, -1, -1, 0, 0)
        infos = cr.walk_sequence(g, ProbeContact())
        assert infos[0]["status"] == MISS and infos[2]["status"] == SET and infos[2]["n_touched"] > 0
        assert [i["face"] for i in infos[1:]] == [BOTTOM, BOTTOM, BOTTOM, BOTTOM, LEFT]
        assert np.abs(g.get_q_state()[0]).max() > 0
        if name == "cube12x8x12":
            assert infos[2]["n_touched"] > fl.FB_HAPTIC_MAX_SOURCES
    finally:
        g.close()


@pytest.fixture(scope="module")
def pressed12(gpu):
    """cube12x8x12 after a step, the tool over its top two node layers: more sources than fb_fem_add_haptic_forces takes"""
    g = FemIntegrator(*_cube(12, 8, 12))
    g.set_uniform_force(1, cr.GRAVITY)
    g.do_timestep()
    probe = ProbeContact()
    op = cr.press_sequence(g.verts, 0.1)[2]
    dev, host = g.contact_move(op[1], op[2], cr.COEFF), probe.move(cr.positions(g), op[1], op[2], cr.COEFF)
    cr.assert_same_info(dev, host)
    assert dev["list_size"] == 288 > fl.FB_HAPTIC_MAX_SOURCES and dev["n_pushing"] == 288
    yield g, probe, g.pattern()[:2]
    g.close()


# 2. more than 256 sources
@pytest.mark.parametrize("size", [1, 2, 3, 5])
def test_more_than_256_sources(pressed12, size):
    g, probe, pattern = pressed12
    info = cr.assert_apply(g, probe, pattern, size, path=cr.RECORDS)
    want = cr.spread_by_records(pattern[0], pattern[1], probe.ids, probe.forces, size, np.zeros(g.r))
    assert want["path"] == cr.RECORDS
    assert info["n_records"] == want["n_records"] and info["n_targets"] == want["n_targets"], (info, want)


# 3. the strict miss rule, ties
def test_strict_miss_and_ties(gpu):
    v, t, fixed = _cube(4, 4, 4, 0.25)
    assert np.array_equal(v, np.float32(v)) and np.array_equal(v * 8, np.round(v * 8)), "binary-exact coordinates"
    g, probe = FemIntegrator(v, t, fixed), ProbeContact()
    try:
        pattern = g.pattern()[:2]
        lo, hi, top = v.min(0) - 1.0, v.max(0) + 1.0, v[:, 1].max()
        first = ([lo[0], top - 0.125, lo[2]], [hi[0], top + 1.0, hi[2]])
        cr.assert_same_info(g.contact_move(*first, cr.COEFF), probe.move(v, *first, cr.COEFF))
        assert probe.info()["n_touched"] == 16
        # the tool's bottom ON the tissue's top: a miss although the inclusive node test would find nodes; nothing changes
        on_top = ([lo[0], top, lo[2]], [hi[0], top + 1.0, hi[2]])
        assert g.pick_box(*on_top, capacity=0)[0] == 16
        dev = g.contact_move(*on_top, cr.COEFF)
        assert dev["status"] == MISS
        cr.assert_same_info(dev, probe.move(v, *on_top, cr.COEFF))
        cr.assert_same_list(g, probe)
        assert cr.assert_apply(g, probe, pattern, 3)["n_pushing"] == 16   # (the previous list is still added)
        # two faces (LEFT and BOTTOM, both 0.125 away) and four nodes tie exactly: the lowest node, then the lowest face
        g.contact_reset(keep_face=False)
        probe.reset(keep_face=False)
        tie = ([0.125, top - 0.125, lo[2]], [hi[0], hi[1], hi[2]])
        dev, host = g.contact_move(*tie, cr.COEFF), probe.move(v, *tie, cr.COEFF)
        cr.assert_same_info(dev, host)
        tied = np.nonzero((v[:, 0] == 0.25) & (v[:, 1] == top))[0]
        assert dev["n_touched"] == len(tied) == 4 and dev["closest_node"] == tied.min() and dev["face"] == LEFT and dev["contact_dist"] == 0.125
        cr.assert_same_list(g, probe)
    finally:
        g.close()


# 4. the fallback
def test_fallback_by_record_budget(pressed12, monkeypatch):
    g, probe, pattern = pressed12
    need = cr.assert_apply(g, probe, pattern, 3, path=cr.RECORDS)["n_records"]
    monkeypatch.setenv("FEMBRAIN_CONTACT_MAX_RECORDS", str(need - 1))
    info = cr.assert_apply(g, probe, pattern, 3, path=cr.LEVELS)
    assert info["n_records"] == need and info["n_targets"] == -1
    monkeypatch.setenv("FEMBRAIN_CONTACT_MAX_RECORDS", str(need))
    cr.assert_apply(g, probe, pattern, 3, path=cr.RECORDS)


def test_fallback_by_table_overflow(gpu):
    """eleven rings around a node in the middle of the top of cube12x8x12 hold more nodes than the walk's table: the level arrays"""
    v, t, fixed = _cube(12, 8, 12)
    g, probe = FemIntegrator(v, t, fixed), ProbeContact()
    try:
        top = v[:, 1].max()
        box = ([-0.12, top - 0.05, -0.12], [0.02, top + 1.0, 0.02])
        cr.assert_same_info(g.contact_move(*box, cr.COEFF), probe.move(v, *box, cr.COEFF))
        assert probe.info()["n_touched"] == 4
        pattern = g.pattern()[:2]
        want = cr.spread_by_records(pattern[0], pattern[1], probe.ids, probe.forces, 12, np.zeros(g.r))
        assert want["path"] == cr.LEVELS and max(len(cr.ball(pattern[0], pattern[1], i, 12)) for i in probe.ids) >= cr.BALL_MAX
        info = cr.assert_apply(g, probe, pattern, 12, path=cr.LEVELS)
        assert info["n_records"] == -1 and info["n_targets"] == -1
        cr.assert_apply(g, probe, pattern, 5, path=cr.RECORDS)   # (the next apply walks again)
    finally:
        g.close()


def test_rings_exhaust_the_mesh(gpu):
    g, probe = FemIntegrator(*_cube(5, 5, 5)), ProbeContact()
    try:
        op = cr.press_sequence(g.verts, 0.1)[2]
        cr.assert_same_info(g.contact_move(op[1], op[2], cr.COEFF), probe.move(g.verts, op[1], op[2], cr.COEFF))
        pattern = g.pattern()[:2]
        info = cr.assert_apply(g, probe, pattern, 12)
        assert info["path"] in (cr.RECORDS, cr.LEVELS)
        if info["path"] == cr.RECORDS:   # (every ball is the whole mesh but for the nodes more than eleven edges away)
            want = cr.spread_by_records(pattern[0], pattern[1], probe.ids, probe.forces, 12, np.zeros(g.r))
            assert info["n_records"] == want["n_records"] > 45 * g.n_nodes and info["n_targets"] == want["n_targets"] == g.n_nodes
    finally:
        g.close()


# 5. mesh changes
def test_cut_keeps_and_resync_clears(gpu):
    v, t, fixed = _cube(8, 5, 5)
    g, probe = FemIntegrator(v, t, fixed, expect_cuts=True), ProbeContact()
    try:
        g.set_uniform_force(1, cr.GRAVITY)
        g.do_timestep()
        seq = cr.press_sequence(v, 0.1)
        cr.assert_same_info(g.contact_move(seq[1][1], seq[1][2], cr.COEFF), probe.move(cr.positions(g), seq[1][1], seq[1][2], cr.COEFF))
        before, n_old = g.contact_info(), g.n_nodes
        c = v.min(0) + (v.max(0) - v.min(0)) * np.array([0.52, 0.5, 0.5]) + [0.0013, 0.0007, 0.0003]
        info, _ = g.cut(cutref.plane_strip(c, (1.0, 0.013, 0.007)), mode="carry")
        assert info["status"] == fl.FB_CUT_DONE and g.n_nodes > n_old
        cr.assert_same_info(g.contact_info(), before, "after the cut")
        cr.assert_same_list(g, probe, "after the cut")
        pattern = g.pattern()[:2]
        assert len(pattern[0]) == g.n_nodes + 1
        for size in (2, 5):
            cr.assert_apply(g, probe, pattern, size, "after the cut", path=cr.RECORDS)
        g.do_timestep()
        dev, host = g.contact_move(seq[2][1], seq[2][2], cr.COEFF), probe.move(cr.positions(g), seq[2][1], seq[2][2], cr.COEFF)
        cr.assert_same_info(dev, host, "move after the cut")
        ids = g.read_contact()[0]
        assert dev["n_new"] > 0 and (ids >= n_old).any(), "the cut's new nodes are found by a move"
        cr.assert_same_list(g, probe, "move after the cut")
        cr.assert_apply(g, probe, pattern, 3, "move after the cut")
        # a full re-sync: a new mesh, the session is gone
        g.resync(v, t, fixed)
        probe.clear()
        now = g.contact_info()
        cr.assert_same_info(now, probe.info(), "after the re-sync")
        assert now["n_clears"] == 1 and now["list_size"] == 0 and now["face"] == -1
        f0 = g.external_forces()
        assert g.contact_apply(3)["n_sources"] == 0 and np.array_equal(g.external_forces(), f0)
        cr.assert_same_info(g.contact_move(seq[1][1], seq[1][2], cr.COEFF), probe.move(cr.positions(g), seq[1][1], seq[1][2], cr.COEFF), "after the re-sync")
        cr.assert_same_list(g, probe, "after the re-sync")
    finally:
        g.close()


# 6. a host-built plan
def test_host_built_plan(gpu, monkeypatch):
    monkeypatch.setenv("FEMBRAIN_PLAN_DEVICE", "0")
    g = FemIntegrator(*_cube(5, 5, 5))
    try:
        assert g._L.fb_fem_plan_on_device(g.h) == 0
        infos = cr.walk_sequence(g, ProbeContact())
        assert [i["face"] for i in infos[1:]] == [BOTTOM, BOTTOM, BOTTOM, BOTTOM, LEFT]
        assert g.contact_apply(3)["path"] == cr.RECORDS   # (the pattern is uploaded)
    finally:
        g.close()


# 7. refusals
def test_refusals_change_nothing(gpu):
    g, probe = FemIntegrator(*_cube(5, 5, 5)), ProbeContact()
    try:
        op = cr.press_sequence(g.verts, 0.1)[1]
        g.contact_move(op[1], op[2], cr.COEFF)
        g.set_uniform_force(1, cr.GRAVITY)
        g.contact_apply(3)
        f0, info0, list0 = g.external_forces(), g.contact_info(), g.read_contact()
        nan, inf = float("nan"), float("inf")
        bad_moves = [([0.0, 1.0, 0.0], [1.0, 0.5, 1.0], 1.0), ([nan, 0.0, 0.0], [1.0, 1.0, 1.0], 1.0), ([0.0, 0.0, 0.0], [1.0, inf, 1.0], 1.0),
                     ([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], inf), ([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], nan)]
        for lo, hi, coeff in bad_moves:
            with pytest.raises(fl.FbError) as e:
                g.contact_move(lo, hi, coeff)
            assert e.value.code == fl.FB_EINVAL, (lo, hi, coeff)
        box = np.array([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
        assert g._L.fb_fem_contact_move(g.h, None, fl.dptr(box[3:]), 1.0, None) == fl.FB_EINVAL
        assert g._L.fb_fem_contact_move(g.h, fl.dptr(box[:3]), None, 1.0, None) == fl.FB_EINVAL
        for size in (0, 256, -3):
            with pytest.raises(fl.FbError) as e:
                g.contact_apply(size)
            assert e.value.code == fl.FB_EINVAL, size
        assert np.array_equal(g.external_forces(), f0)
        cr.assert_same_info(g.contact_info(), info0)
        for a, b in zip(g.read_contact(), list0):
            assert np.array_equal(a, b)
    finally:
        g.close()


# 8. more than 256 workgroups
def test_more_than_256_workgroups(gpu):
    v, t, fixed = _cube(41, 41, 41)
    assert len(v) == 68921 > 256 * 256
    g, probe = FemIntegrator(v, t, fixed), ProbeContact()
    try:
        op = cr.press_sequence(v, 0.1)[1]
        dev, host = g.contact_move(op[1], op[2], cr.COEFF), probe.move(v, op[1], op[2], cr.COEFF)
        cr.assert_same_info(dev, host)
        assert dev["n_touched"] == 41 * 41
        cr.assert_same_list(g, probe)
        cr.assert_apply(g, probe, g.pattern()[:2], 3, path=cr.RECORDS)
    finally:
        g.close()


# 9. the drivers
@pytest.mark.parametrize("with_cut", [False, True])
def test_driver_routes_agree(gpu, with_cut):
    v, t, _ = _cube(8, 5, 5)
    fixed = cube_fixed_plane_i0(5, 5)
    dev, host = Deformable(v, t, fixed, haptic_on_device=True, expect_cuts=True), Deformable(v, t, fixed, haptic_on_device=False, expect_cuts=True)
    try:
        lo, hi, top = v.min(0) - 1.0, v.max(0) + 1.0, v[:, 1].max()
        c = v.min(0) + (v.max(0) - v.min(0)) * np.array([0.52, 0.5, 0.5]) + [0.0013, 0.0007, 0.0003]
        for d in (dev, host):
            d.set_haptic_force_radius(3)
            d.probe_start()
        for k, depth in enumerate((0.02, 0.06, 0.12, 0.17, 0.12)):
            box = ([lo[0], top - depth, lo[2]], [hi[0], top + 1.0, hi[2]])
            a, b = dev.probe_move(*box, cr.COEFF), host.probe_move(*box, cr.COEFF)
            cr.assert_same_info(a, b, "move %d" % k)
            for d in (dev, host):
                d.timestep()
            if with_cut and k == 2:
                for d in (dev, host):
                    assert d.cut(cutref.plane_strip(c, (1.0, 0.013, 0.007)), mode="carry")[0]["status"] == fl.FB_CUT_DONE
            (qa, va, _), (qb, vb, _) = dev.integrator.get_q_state(), host.integrator.get_q_state()
            assert np.array_equal(qa, qb) and np.array_equal(va, vb) and np.abs(qa).max() > 0, "step %d" % k
        assert a["n_touched"] > 0 and a["status"] == SET
        for d in (dev, host):
            d.probe_end()
            d.timestep()
        assert dev.integrator.contact_info()["list_size"] == 0 and dev.integrator.contact_info()["face"] == BOTTOM
        assert np.array_equal(dev.integrator.get_q_state()[0], host.integrator.get_q_state()[0])
    finally:
        dev.integrator.close()
        host.integrator.close()
