"""Plan arithmetic of the persistent solver's register slots (fembrain_amd/csrc/pcg_pipe_mirror.h mir_reg_slots / mir_reg_split, which
k_pipe_mirror_plan and k_pcg_pipe_regs apply; fb_plan_regs_model runs them over the host model of the LDS window): for every slice the slots
streamed in front, the register slots in front, the mirror layers, the plain layers, the register slots behind and the slots streamed behind
partition the slice in slot order, and the slice holds r = min(REGS, streamed slots) register slots, behind the window first."""
import ctypes as C

import numpy as np
import pytest

from fembrain_amd import lib as fl
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube


@pytest.fixture(scope="module")
def plans():
    L = fl.lib()
    made = {}

    def make(n):
        if n not in made:
            v, t = truth_cube(n, n, n, 0.1)
            fixed = np.ascontiguousarray(fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n)), np.int32)
            tt = np.ascontiguousarray(t, np.int32).reshape(-1)
            h = C.c_void_p()
            fl.check(L.fb_plan_create(C.byref(h), len(v), len(t), fl.iptr(tt), len(fixed), fl.iptr(fixed), 1, 0, None))
            cnt = L.fb_plan_get(h, b"slice_off", None, 0)
            so = np.zeros(cnt, np.int32)
            assert L.fb_plan_get(h, b"slice_off", fl.iptr(so), cnt) == cnt
            made[n] = (h, so)
        return made[n]
    yield L, make
    for h, _ in made.values():
        L.fb_plan_destroy(h)


def _parts(L, h, n_slices, nb, c16, klt, regs):
    out = np.full(6 * n_slices, -1, np.int32)
    fl.check(L.fb_plan_regs_model(h, nb, c16, klt, regs, fl.iptr(out)))
    return out.reshape(n_slices, 6).astype(np.int64)


# (nodes per edge, workgroups, unroll bound): the headline cube on the whole device, and the small cubes of the GPU cases on one XCD --
# (12, 6) with 10 and 11 slices per workgroup, (12, 7) with 9, and 12 per workgroup with slices of width 8
@pytest.mark.parametrize("n,nb,klt", [(56, 256, 6), (28, 32, 6), (26, 32, 7), (29, 32, 6)])
@pytest.mark.parametrize("c16", [1, 0])
def test_register_slots_partition_every_slice(plans, n, nb, klt, c16):
    L, make = plans
    h, so = make(n)
    n_slices = len(so) - 1
    width = np.diff(so).astype(np.int64)
    base = _parts(L, h, n_slices, nb, c16, klt, 0)
    assert (base >= 0).all() and (base[:, 1] == 0).all() and (base[:, 4] == 0).all()
    assert (base.sum(1) == width).all()
    front, behind = base[:, 0], base[:, 5]
    streamed = front + behind
    for regs in (1, 2, 3):
        p = _parts(L, h, n_slices, nb, c16, klt, regs)
        assert (p >= 0).all()
        assert (p.sum(1) == width).all()                                  # in slot order, the six parts are the slice
        assert (p[:, 2] == base[:, 2]).all() and (p[:, 3] == base[:, 3]).all()  # the window itself does not move
        r = p[:, 1] + p[:, 4]
        assert (r == np.minimum(regs, streamed)).all()                    # r = min(REGS, streamed slots of the slice)
        assert (p[:, 4] == np.minimum(regs, behind)).all()                # behind the window first ...
        assert (p[:, 1] == np.minimum(regs - p[:, 4], front)).all()       # ... the others in front of it
        assert (p[:, 0] == front - p[:, 1]).all() and (p[:, 5] == behind - p[:, 4]).all()
    if n == 56 and c16:
        # the headline: 6.3 of a slice's 14.9 slots are streamed, and nearly every slice holds three of them
        assert 6.0 < streamed.mean() < 6.6 and np.minimum(3, streamed).mean() > 2.9, (streamed.mean(), np.minimum(3, streamed).mean())


def test_regs_model_refuses_bad_arguments(plans):
    L, make = plans
    h, so = make(26)
    out = np.zeros(6 * (len(so) - 1), np.int32)
    assert L.fb_plan_regs_model(h, 32, 1, 7, 4, fl.iptr(out)) != 0
    assert L.fb_plan_regs_model(h, 32, 1, 5, 3, fl.iptr(out)) != 0
    assert L.fb_plan_regs_model(h, 12, 1, 6, 3, fl.iptr(out)) != 0
