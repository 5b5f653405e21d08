"""The LDS window of the persistent one-row kernel (fembrain_amd/csrc/pcg_pipe_mirror.h): layers of a slice whose blocks have a lower row of
the same workgroup as column are read from LDS as the transposes of those rows' resident blocks.  The sum of a row runs over the same
slots in the same order with the same values as without the window, so every case here compares a handle with FEMBRAIN_PIPE_MIRROR=0
against the default one BIT FOR BIT: the solution of a PCG solve, its iteration count, launches cut into 1 / 7 / 30 iterations, three
reference-load steps, and the same after a delta re-sync and after a full re-sync (the table is planned again for the new plan)."""
import numpy as np
import pytest

from fembrain_amd import lib as fl
from fembrain_amd.fem import FemIntegrator
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, synthetic_cut, truth_cube

pytestmark = pytest.mark.gpu


def _cube(n):
    v, t = truth_cube(n, n, n, 0.1)
    return v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n))


def _pair(monkeypatch, v, t, fixed, c16=True, **kw):
    """(handle without the window, default handle)"""
    if not c16:
        monkeypatch.setenv("FEMBRAIN_SPMV_C16", "0")
    monkeypatch.setenv("FEMBRAIN_PIPE_MIRROR", "0")
    g0 = FemIntegrator(v, t, fixed, **kw)
    monkeypatch.delenv("FEMBRAIN_PIPE_MIRROR")
    g1 = FemIntegrator(v, t, fixed, **kw)
    monkeypatch.delenv("FEMBRAIN_SPMV_C16", raising=False)
    assert g0.persist_mirror() == (False, 0, 0, 0)
    assert g0.pcg_path()["kernel"] == g1.pcg_path()["kernel"] and g0.persist_info() == g1.persist_info()
    return g0, g1


def _same_solves(monkeypatch, g0, g1, runs=("1", "7", "30")):
    for g in (g0, g1):
        g.set_uniform_force(1, -10000.0)
    _, rhs = g0.system()
    _, rhs1 = g1.system()
    assert np.array_equal(rhs, rhs1)
    it0, x0 = g0.pcg(rhs, eps=1e-6, max_iter=20000)
    it1, x1 = g1.pcg(rhs, eps=1e-6, max_iter=20000)
    assert g1.pcg_path()["path"] == fl.FB_PCG_PATH_PERSISTENT and g1.pcg_path()["fallbacks"] == 0
    assert it0 > 100 and it1 == it0 and np.array_equal(x1, x0)
    for run in runs:
        monkeypatch.setenv("FEMBRAIN_PERSIST_MAX_RUN", run)
        itc, xc = g1.pcg(rhs, eps=1e-6, max_iter=20000)
        assert itc == it0 and np.array_equal(xc, x0), run
    monkeypatch.delenv("FEMBRAIN_PERSIST_MAX_RUN", raising=False)
    return it0


def _same_steps(g0, g1, k=3):
    for _ in range(k):
        assert g0.do_timestep() == g1.do_timestep()
        for a, b in zip(g0.get_q_state(), g1.get_q_state()):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("n,c16,kernel,waves", [(56, True, "k_pcg_pipe<float,c16,12,6>", 11), (56, False, "k_pcg_pipe<float,c32,12,6>", 11),
                                                (58, True, "k_pcg_pipe<float,c16,12,6>", 12), (52, True, "k_pcg_pipe<float,c16,12,7>", 9)])
def test_mirror_layers_give_the_iterates_of_the_plain_window(gpu, monkeypatch, n, c16, kernel, waves):
    v, t, fixed = _cube(n)
    g0, g1 = _pair(monkeypatch, v, t, fixed, c16=c16)
    on, waves_, wgs, share = g1.persist_info()
    assert on and waves_ == waves and wgs == 256 and g1.pcg_path()["kernel"] == kernel
    mon, layers, pool, plain = g1.persist_mirror()
    n_slices = -(-n ** 3 // 64)
    assert mon and plain >= share, (layers / n_slices, pool, plain, share)
    if waves >= 11:
        assert layers >= (2.5 if c16 else 2.0) * n_slices, (layers / n_slices, pool, plain, share)
    _same_solves(monkeypatch, g0, g1, runs=("1", "7", "30") if n == 56 and c16 else ("7",))
    if n == 56 and c16:
        _same_steps(g0, g1)
    g0.close(); g1.close()


def test_mirror_table_is_planned_again_after_a_delta_and_a_full_resync(gpu, monkeypatch):
    v, t, fixed = _cube(56)
    g0, g1 = _pair(monkeypatch, v, t, fixed)
    before = g1.persist_mirror()
    v2, t2, d = synthetic_cut(v, t, axis=1, where=0.45, stride=3)
    for g in (g0, g1):
        g.resync_delta(d, fixed)
    assert g0.persist_mirror()[1] == 0
    after = g1.persist_mirror()
    assert g0.pcg_path()["kernel"] == g1.pcg_path()["kernel"]
    if g1.pcg_path()["kernel"].startswith("k_pcg_pipe<float,c16,12,"):
        assert after[0] and after != before
    _same_solves(monkeypatch, g0, g1, runs=("7",))
    for g in (g0, g1):
        g.resync(v, t, fixed)
    assert g1.persist_mirror() == before and g0.persist_mirror()[1] == 0
    _same_solves(monkeypatch, g0, g1, runs=())
    _same_steps(g0, g1, 1)
    g0.close(); g1.close()


def test_no_mirror_layers_with_helper_wavefronts(gpu, monkeypatch):
    """A cut cube dealt by slots with helper wavefronts runs the table-driven instantiation: no window there, nothing changes."""
    v, t, fixed = _cube(40)
    monkeypatch.setenv("FEMBRAIN_PIPE_HELPERS", "1")
    g0, g1 = _pair(monkeypatch, v, t, fixed)
    monkeypatch.delenv("FEMBRAIN_PIPE_HELPERS")
    assert g1.persist_mirror() == (False, 0, 0, 0)
    _same_solves(monkeypatch, g0, g1, runs=())
    g0.close(); g1.close()
