"""fembrain_amd.erosion.erode_host on a handle: the selected elements go, everything else is as it was."""
import numpy as np
import pytest

from fembrain_amd import erosion as er
from fembrain_amd import lib as fl
from fembrain_amd.fem import FemIntegrator
from test_detach_gpu import MATS, _beam, _same_snapshot, _snapshot

pytestmark = pytest.mark.gpu

CENTRE = (-0.1 + 0.013, 0.2 + 0.007, -0.05 - 0.004)
SPHERE = ("sphere", CENTRE, 0.2)


def _parent(**kw):
    """test_detach_gpu's parent without the cut: both ends clamped, two materials alternating by element, loaded and stepped twice, a
    random external force vector, stepped once"""
    v, t, fixed = _beam()
    g = FemIntegrator(v, t, fixed, **kw)
    g.set_materials(*MATS, element_ids=np.arange(len(t)) % 2)
    for _ in range(2):
        g.set_uniform_force(1, -3000.0)
        g.do_timestep()
    fext = np.random.default_rng(5).normal(size=g.r) * 40.0
    g.set_external_forces(fext)
    g.do_timestep()
    assert g.last.converged == 1
    return g, fixed, fext


@pytest.mark.parametrize("integrator", [fl.FB_INTEGRATOR_VOLUME_CONSERVING, fl.FB_INTEGRATOR_NEWMARK])
def test_the_elements_go_and_the_rest_is_carried(gpu, integrator):
    g, fixed, fext = _parent(integrator=integrator)
    before, mats = _snapshot(g), g.element_materials()
    volume_before = g.part_table()["volume"].sum()
    info = er.erode_host(g, [SPHERE], frame="rest")
    ids, freed = info["element_ids"], info["freed_nodes"]
    assert (info["status"], info["n_selected"], info["n_removed"], info["n_nodes_freed"]) == ("done", 213, 213, 11)   # tests/test_erode_ref.py's counts
    assert info["n_elements_left"] == g.num_tets() == 1440 - 213 and info["resync_path"] == g.resync_path() == fl.FB_RESYNC_DELTA_MERGED
    x, t = g.read_mesh()
    assert np.array_equal(x, before["x"]) and np.array_equal(t, np.delete(before["t"], ids, axis=0)) and np.array_equal(g.tets, t)
    for u, w in zip(g.get_q_state(), before["state"]):
        assert np.array_equal(u, w)
    assert np.abs(before["state"][0]).max() > 0 and (integrator != fl.FB_INTEGRATOR_NEWMARK or np.abs(before["state"][2]).max() > 0)
    assert np.array_equal(g.external_forces(), fext) and np.array_equal(g.constrained_dofs(), fixed)
    assert np.array_equal(g.element_materials(), np.delete(mats, ids))
    assert g.parts()["n_unused_nodes"] == 11 and not np.isin(freed, t).any()
    volume_after = g.part_table()["volume"].sum()
    print("rest volume %.17g - %.17g, reported %.17g; mass %.17g" % (volume_before, volume_after, info["volume"], info["mass"]))
    assert abs((volume_before - volume_after) - info["volume"]) <= 1e-12 * volume_before
    rho = np.array(MATS[2])[mats[ids]]
    assert abs(info["mass"] - (rho * er.rest_volumes(before["x"], before["t"])[ids]).sum()) <= 1e-12 * info["mass"]
    for _ in range(3):
        g.do_timestep()
        assert g.last.converged == 1
    again = er.erode_host(g, [SPHERE], frame="rest")      # the same place: nothing left there
    assert (again["status"], again["n_selected"]) == ("none", 0)
    g.close()


def test_filters(gpu):
    g, _, _ = _parent()
    info = er.erode_host(g, [SPHERE], frame="rest", material=1, dry_run=True)
    assert info["status"] == "dry" and len(info["element_ids"]) > 0 and (info["element_ids"] % 2 == 1).all()
    g.stress()
    vm = g.element_stress()["von_mises"]
    limit = float(np.median(vm))
    info = er.erode_host(g, [], min_von_mises=limit, dry_run=True)
    assert np.array_equal(info["element_ids"], np.nonzero(vm >= limit)[0]) and info["n_selected"] == 720
    x, t = g.read_mesh()
    world = er.select(x, t, g.get_q_state()[0], [SPHERE])
    info = er.erode_host(g, [SPHERE], min_von_mises=limit, dry_run=True)
    assert np.array_equal(info["element_ids"], np.intersect1d(world, np.nonzero(vm >= limit)[0])) and len(world) > 0
    info = er.erode_host(g, [], material=1)
    assert info["status"] == "done" and np.array_equal(info["element_ids"], np.arange(1, 1440, 2)) and (g.element_materials() == 0).all()
    g.do_timestep()
    assert g.last.converged == 1
    g.close()


def test_refusals_change_nothing(gpu):
    g, _, _ = _parent()
    builds = (g.surface()["n_builds"], g.parts()["n_builds"])
    before = _snapshot(g)
    n = len(before["t"])
    want = er.select(before["x"], before["t"], None, [SPHERE], frame="rest")
    for status, shapes, kw in (("none", [("sphere", (5.0, 5.0, 5.0), 0.2)], {}), ("all", [("box", (0.0, 0.2, 0.0), (2.0, 2.0, 2.0), None)], {}),
                               ("over_cap", [SPHERE], dict(max_elements=len(want) - 1)), ("dry", [SPHERE], dict(dry_run=True, max_elements=len(want)))):
        info = er.erode_host(g, shapes, frame="rest", **kw)
        assert (info["status"], info["n_removed"], info["n_elements_left"]) == (status, 0, n), status
        assert info["n_selected"] == {"none": 0, "all": n}.get(status, len(want))
        assert _same_snapshot(before, _snapshot(g)) and (g.surface()["n_builds"], g.parts()["n_builds"]) == builds
    assert np.array_equal(info["element_ids"], want) and np.array_equal(info["freed_nodes"], er.freed_nodes(before["t"], want))
    g.close()
