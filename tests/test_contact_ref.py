"""The host side of the probe's box contact, without a GPU: ``fembrain_amd.fem.ProbeContact`` (the transcription of
AvatarProbe::onTranslate) on the press sequence of tests/contactref.py, and the record formulation of the ring spread
(contactref.spread_by_records, what fembrain_amd/csrc/contact.hip runs) against ``spread_haptic_forces``."""
import numpy as np
import pytest

import contactref as cr
from fembrain_amd import lib as fl
from fembrain_amd.fem import ProbeContact, spread_haptic_forces
from fembrain_amd.meshgen import truth_cube

MISS, EMPTY, SET = fl.FB_CONTACT_MISS, fl.FB_CONTACT_EMPTY, fl.FB_CONTACT_SET
BOTTOM, LEFT = 2, 0


def _press(v):
    """the sequence at rest: the infos of the moves"""
    probe, infos = ProbeContact(), []
    for op in cr.press_sequence(v, 0.1):
        if op[0] == "reset":
            probe.reset(keep_face=op[1])
        else:
            infos.append(probe.move(v, op[1], op[2], cr.COEFF))
    return probe, infos


@pytest.mark.parametrize("shape,layer", [((5, 5, 5), 25), ((12, 8, 12), 144)])
def test_probe_contact_sequence(shape, layer):
    v, _ = truth_cube(*shape, 0.1)
    probe, infos = _press(v)
    assert [i["status"] for i in infos] == [MISS, SET, SET, SET, SET, SET]
    assert [i["n_touched"] for i in infos[:4]] == [0, layer, 2 * layer, 2 * layer]
    assert [i["n_new"] for i in infos[:4]] == [0, layer, layer, 0]
    assert [i["face"] for i in infos] == [-1, BOTTOM, BOTTOM, BOTTOM, BOTTOM, LEFT]   # (kept across reset(keep_face=1), chosen again after reset(0))
    top = v[:, 1].max()
    # touch: the tool's bottom is half a cell below the top layer, every touched node pushed down by coeff * 0.05
    assert infos[1]["contact_dist"] == (top - (top - 0.05)) * 1.0 and infos[1]["n_pushing"] == layer
    # retreat: first-touch positions stay, so the second layer (0.1 below the top, the tool's bottom 0.05 below) is no longer pushed
    assert infos[3]["n_pushing"] == layer and infos[3]["list_size"] == 2 * layer
    ids, first, forces = probe.read()
    assert (np.diff(ids) > 0).all() and np.array_equal(first, v[ids])
    assert (forces[:, 0] < 0).all() and not forces[:, 1:].any()   # LEFT: along -x


def test_probe_contact_strict_miss_and_empty():
    v, _ = truth_cube(4, 4, 4, 0.25)
    assert np.array_equal(v, np.float32(v)), "binary-exact coordinates"
    top = v[:, 1].max()
    probe = ProbeContact()
    lo, hi = v.min(0) - 1.0, v.max(0) + 1.0
    # the tool's bottom ON the tissue's top: the inclusive node test would find the top layer, the strict box test says miss
    assert probe.move(v, [lo[0], top, lo[2]], [hi[0], top + 1.0, hi[2]], 1.0)["status"] == MISS and not probe.hash
    # the boxes intersect between two node layers: nothing touched
    assert probe.move(v, [lo[0], top - 0.2, lo[2]], [hi[0], top - 0.1, hi[2]], 1.0)["status"] == EMPTY
    with pytest.raises(ValueError):
        probe.move(v, [0, 1, 0], [1, 0, 1], 1.0)
    with pytest.raises(ValueError):
        probe.move(v, [0, 0, 0], [1, 1, 1], np.inf)


def _list_on_cube12():
    v, t = truth_cube(12, 8, 12, 0.1)
    probe, _ = _press(v)
    probe.reset(keep_face=False)
    seq = cr.press_sequence(v, 0.1)
    probe.move(v, seq[2][1], seq[2][2], cr.COEFF)   # "deeper": 288 nodes, all pushed
    return cr.pattern_of(t, len(v)), probe, len(v)


@pytest.fixture(scope="module")
def cube12():
    pattern, probe, n = _list_on_cube12()
    want = {size: cr.host_vector(pattern, probe.ids, probe.forces, size, 3 * n) for size in (1, 2, 3, 5)}
    return pattern, probe, n, want


@pytest.mark.parametrize("size", [1, 2, 3, 5])
def test_records_equal_host_walk(cube12, size):
    pattern, probe, n, want = cube12
    assert len(probe.ids) == 288 > fl.FB_HAPTIC_MAX_SOURCES
    f = np.zeros(3 * n)
    f[1::3] = cr.GRAVITY
    info = cr.spread_by_records(pattern[0], pattern[1], probe.ids, probe.forces, size, f)
    assert info["path"] == cr.RECORDS and (info["n_records"] > 0) == (size > 1)
    assert np.array_equal(f, want[size])


@pytest.mark.parametrize("size,kw", [(3, dict(ball_max=8)), (5, dict(ball_max=40)), (3, dict(max_records=100))])
def test_fallback_equals_host_walk(cube12, size, kw):
    pattern, probe, n, want = cube12
    f = np.zeros(3 * n)
    f[1::3] = cr.GRAVITY
    info = cr.spread_by_records(pattern[0], pattern[1], probe.ids, probe.forces, size, f, **kw)
    assert info["path"] == cr.LEVELS
    assert np.array_equal(f, want[size])


def test_pattern_of_is_the_handle_pattern_shape():
    v, t = truth_cube(3, 3, 3, 0.1)
    bptr, bcol = cr.pattern_of(t, len(v))
    for a in range(len(v)):
        row = bcol[bptr[a]:bptr[a + 1]]
        assert a in row and (np.diff(row) > 0).all()
        assert set(row) == {int(x) for e in t if a in e for x in e}
