"""fb_fem_body_contact on the device against tests/bodycontactref.py, the rule in numpy by brute force.

Contact sets and every integer output (node, element, face) of the points whose decision lies outside rounding are compared exactly; a
test may leave out at most 2 % of the reference's candidates, and none in the structured shapes.  The doubles (closest point, weights,
depth, the two force vectors, the sums) are compared BIT FOR BIT: the device functions and the reference are the same sequence of fp64
operations without contraction, and the device's division and square root round as numpy's do.  (Had they differed in the last place,
the bound would have been 8 x the largest relative difference between the float64 reference and the same reference in np.longdouble
over the shapes below (the three structured ones, deformed, permuted, before and after the cut, parent and piece), relative to
stiffness * max_depth: measured 1.43e-14 at its largest -- "many_onto_one", where a node sums 100 contributions; 2.4e-15 or less elsewhere
-- so 1.1e-13.  It is not needed.)"""
import os

import numpy as np
import pytest

import bodycontactref as R
from fembrain_amd import lib as fl
from fembrain_amd.fem import FemIntegrator
from fembrain_amd.meshgen import truth_cube

pytestmark = pytest.mark.gpu

K = 1000.0
KW = dict(E=1e6, timestep=0.01)


class _Env:
    """environment knobs for the duration of a block (the library reads them at every call)"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, str(v))

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _pair(name, **kw):
    va, ta, vb, tb = R.two_cubes(*R.SHAPES[name])
    return FemIntegrator(va, ta, **dict(KW, **kw)), FemIntegrator(vb, tb, **dict(KW, **kw))


def _current(g):
    x, t = g.read_mesh()
    return x, t, x + g.get_q_state()[0].reshape(-1, 3)


def _reference(ga, gb, stiffness, depth_cap=0.0, directions=3, fa0=None, fb0=None):
    xa, ta, ca = _current(ga)
    xb, tb, cb = _current(gb)
    ref = R.body_contact(xa, ta, ca, xb, tb, cb, stiffness, depth_cap, directions, fa0, fb0)
    ref["extent"] = (float((cb.max(axis=0) - cb.min(axis=0)).max()), float((ca.max(axis=0) - ca.min(axis=0)).max()))  # of the body searched, per direction
    return ref


def _call(ga, gb, stiffness, depth_cap=0.0, directions="both", fa0=None, fb0=None):
    """sets the two force vectors (zero where none is given), calls, returns everything that comes back"""
    for g, f in ((ga, fa0), (gb, fb0)):
        g.set_external_forces_to_zero() if f is None else g.set_external_forces(f)
    info = ga.body_contact(gb, stiffness, depth_cap, directions)
    return dict(info=info, dirs=(ga.read_body_contact("a_into_b"), ga.read_body_contact("b_into_a")), fa=ga.external_forces().reshape(-1, 3),
                fb=gb.external_forces().reshape(-1, 3))


def _compare(out, ref, max_left_out=0.0, label=""):
    """the device's call against the reference's; returns the number of candidates left out"""
    info, left, total = out["info"], 0, 0
    all_generic = True
    for k, (dev, r) in enumerate(zip(out["dirs"], ref["dirs"])):
        if r is None:
            assert info["n_contacts"][k] == 0 and info["n_candidates"][k] == 0
            continue
        cand_ok, contact_ok = R.generic(r, ref["extent"][k])
        left += int((~cand_ok).sum()) + int((~contact_ok & cand_ok[r["in_contact"]]).sum())
        total += len(cand_ok)
        print("%s direction %d: %d candidates, %d contacts (device %d, %d), degenerate %d, margins %.3g / %.3g, left out %d" % (
            label, k, len(cand_ok), len(r["node"]), info["n_candidates"][k], info["n_contacts"][k], info["n_degenerate"][k],
            r["contain_margin"].min() if len(cand_ok) else np.inf, r["gap"].min() if len(r["node"]) else np.inf, int((~cand_ok).sum()) + int((~contact_ok).sum())))
        assert info["n_candidates"][k] == len(r["candidates"])
        # the contact set of the generic candidates
        sure = set(r["candidates"][cand_ok].tolist())
        assert set(n for n in dev["node"].tolist() if n in sure) == set(n for n in r["node"].tolist() if n in sure)
        assert np.all(np.diff(dev["node"]) > 0)
        where = {int(n): i for i, n in enumerate(dev["node"])}
        keep = np.nonzero(contact_ok)[0]
        rows = np.array([where[int(r["node"][i])] for i in keep], np.int64)
        assert np.array_equal(dev["element"][rows], r["element"][keep]) and np.array_equal(dev["face"][rows], r["face"][keep])
        for key in ("closest", "bary", "depth"):
            assert np.array_equal(dev[key][rows], r[key][keep]), (label, k, key, np.abs(dev[key][rows] - r[key][keep]).max())
        all_generic &= bool(cand_ok.all() and contact_ok.all())
        if all_generic:
            assert info["n_contacts"][k] == len(r["node"]) and info["n_degenerate"][k] == int(r["degenerate"].sum())
    assert left <= max_left_out * total, (left, total)
    if all_generic:  # every contribution is pinned down: the vectors and the sums bit for bit
        for key in ("fa", "fb"):
            assert np.array_equal(out[key], ref[key]), (label, key, np.abs(out[key] - ref[key]).max())
        assert np.array_equal(info["force_on_a"], ref["force_on_a"]) and np.array_equal(info["force_on_b"], ref["force_on_b"])
        assert info["max_depth"] == ref["max_depth"]
    return left


def _same_bits(x, y):
    assert x["info"].keys() == y["info"].keys()
    for key, v in x["info"].items():
        if key not in ("path", "faces_tested", "n_face_grid_builds"):
            assert np.array_equal(v, y["info"][key]), key
    for dx, dy in zip(x["dirs"], y["dirs"]):
        for key in dx:
            assert np.array_equal(dx[key], dy[key]), key
    assert np.array_equal(x["fa"], y["fa"]) and np.array_equal(x["fb"], y["fb"])


WANT = {"two_way": (16, 9), "many_onto_one": (392, 4), "deep": (26, 0)}


@pytest.mark.parametrize("name", ["two_way", "many_onto_one", "deep"])
def test_shapes_against_the_reference(name):
    ga, gb = _pair(name)
    out = _call(ga, gb, K)
    assert out["info"]["n_contacts"] == WANT[name]
    assert _compare(out, _reference(ga, gb, K), 0.0, name) == 0
    if name == "many_onto_one":  # a node of b collects more records than a wavefront has lanes
        faces = gb.surface()["faces"]
        per_node = np.bincount(faces[out["dirs"][0]["face"]].reshape(-1))
        assert per_node.max() > 64
    if name == "deep":  # the closest face is cells away from the point; and the cap
        assert out["info"]["n_candidates"][1] == 0 and 0.36 < out["dirs"][0]["depth"].min() and out["dirs"][0]["depth"].max() < 0.44
        capped = _call(ga, gb, K, depth_cap=0.1)
        assert capped["info"]["max_depth"] == 0.1
        _compare(capped, _reference(ga, gb, K, depth_cap=0.1), 0.0, name + " capped")
    ga.close(); gb.close()


def test_both_bodies_deformed():
    va, ta, vb, tb = R.two_cubes(*R.SHAPES["two_way"])
    clamp = np.nonzero(vb[:, 0] == vb[:, 0].min())[0]
    fixed = np.sort((3 * clamp[:, None] + np.arange(3)).reshape(-1)).astype(np.int32)
    ga, gb = FemIntegrator(va, ta, **KW), FemIntegrator(vb, tb, fixed, **KW)
    for _ in range(3):
        ga.set_uniform_force(0, 3.0)
        gb.set_uniform_force(1, -40.0)
        ga.do_timestep(); gb.do_timestep()
    assert np.abs(ga.get_q_state()[0]).max() > 1e-4 and np.abs(gb.get_q_state()[0]).max() > 1e-4
    out = _call(ga, gb, K)
    assert sum(out["info"]["n_contacts"]) > 10
    _compare(out, _reference(ga, gb, K), 0.02, "deformed")
    ga.close(); gb.close()


def test_permuted_ids_and_forced_renumbering():
    va, ta, vb, tb = R.two_cubes(*R.SHAPES["many_onto_one"])
    meshes = []
    for v, t, seed in ((va, ta, 3), (vb, tb, 4)):
        p = np.random.default_rng(seed).permutation(len(v))   # new id of old node i
        v2 = np.empty_like(v)
        v2[p] = v
        meshes.append((v2, p[t].astype(np.int32)))
    ga, gb = (FemIntegrator(v, t, renumber=fl.FB_RENUMBER_ON, **KW) for v, t in meshes)
    assert ga.renumbering()[0] and gb.renumbering()[0]
    out = _call(ga, gb, K)
    assert out["info"]["n_contacts"] == WANT["many_onto_one"]
    assert _compare(out, _reference(ga, gb, K), 0.0, "permuted") == 0
    # the caller's numbering: every contact node is a surface vertex of its own body, element and face index the other body's arrays
    assert set(out["dirs"][0]["node"]) <= set(ga.surface()["vertex_ids"]) and out["dirs"][0]["face"].max() < len(gb.surface()["faces"])
    ga.close(); gb.close()


def _beam_and_block():
    from test_detach_gpu import _beam, _blade
    v, t, fixed = _beam()
    beam = FemIntegrator(v, t, fixed, **KW)
    vc, tc = truth_cube(3, 3, 3, 0.1)
    vc = vc + (np.array([v[:, 0].min() + 0.713, v[:, 1].max() - 0.0637, v[:, 2].min() + 0.1291]) - vc.min(axis=0))[None, :]  # across the blade, sunk into the top
    return beam, FemIntegrator(vc, tc, **KW), v, _blade(v)


def test_after_cut_and_detach():
    beam, block, v, blade = _beam_and_block()
    before = _call(block, beam, K)
    assert before["info"]["n_contacts"][0] > 0 and beam.surface()["n_builds"] == 1
    _compare(before, _reference(block, beam, K), 0.02, "before the cut")
    info, _ = beam.cut(blade, mode="carry", track=False)
    assert info["status"] == fl.FB_CUT_DONE
    beam.r = 3 * int(beam._L.fb_fem_num_nodes(beam.h))
    after = _call(block, beam, K)   # the same pair: the call sees the new surface
    assert beam.surface()["n_builds"] == 2 and len(beam.surface()["faces"]) > 2 * (15 * 4 * 4 + 2 * 4 * 4) + 30
    _compare(after, _reference(block, beam, K), 0.02, "after the cut")
    # the detached half, moved back into the parent by about 0.3 of a cell (and off the parent's sides, so that few points sit on a boundary)
    assert beam.parts()["n_parts"] == 2
    piece, _, _ = beam.detach_part(1, remove=True, track=True)
    q = piece.get_q_state()[0].reshape(-1, 3)
    x = piece.read_mesh()[0]
    toward = -1.0 if x[:, 0].mean() > v[:, 0].mean() else 1.0
    piece.set_q_state((q + np.array([toward * 0.031, 0.0137, -0.0171])[None, :]).reshape(-1))
    out = _call(beam, piece, K)
    assert min(out["info"]["n_contacts"]) > 0
    _compare(out, _reference(beam, piece, K), 0.02, "parent and piece")
    for g in (beam, piece, block):
        g.set_uniform_force(1, -10.0)
        g.do_timestep()
        g.close()


def test_disjoint_boxes():
    va, ta, vb, tb = R.two_cubes((3, 3, 3, 0.1), (4, 3, 3, 0.1), (0.45, 0.0, 0.0))
    ga, gb = FemIntegrator(va, ta, **KW), FemIntegrator(vb, tb, **KW)
    rng = np.random.default_rng(1)
    fa0, fb0 = rng.normal(size=3 * len(va)), rng.normal(size=3 * len(vb))
    out = _call(ga, gb, K, fa0=fa0, fb0=fb0)
    info = out["info"]
    assert info["n_contacts"] == (0, 0) and info["n_candidates"] == (0, 0) and info["n_tet_grid_builds"] == 0 and info["n_face_grid_builds"] == 0
    assert info["path"] == fl.FB_BODY_CONTACT_NONE and info["faces_tested"] == 0
    assert np.array_equal(out["fa"].reshape(-1), fa0) and np.array_equal(out["fb"].reshape(-1), fb0)
    ga.close(); gb.close()


def test_overlapping_boxes_nothing_inside():
    """b is a cube without the element at one corner (of the corner cell's six the one that holds the corner node: x + y + z >= 2 in
    the cell's coordinates); a, a fifth of a cell wide, sits in the notch.  The boxes of the cell's other five elements cover the notch."""
    vb, tb = truth_cube(5, 5, 5, 0.1)
    hi = vb.max(axis=0)
    assert (vb[tb[-1]] >= hi - 0.1 - 1e-12).all() and (vb[tb[-1]] == hi).all(axis=1).any()
    tb = tb[:-1]
    va, ta = truth_cube(2, 2, 2, 0.02)
    va = va + (hi - 0.03 - va.min(axis=0))[None, :]   # 0.7 .. 0.9 of the cell on every axis
    ga, gb = FemIntegrator(va, ta, **KW), FemIntegrator(vb, tb, **KW)
    rng = np.random.default_rng(2)
    fa0, fb0 = rng.normal(size=3 * len(va)), rng.normal(size=3 * len(vb))
    out = _call(ga, gb, K, fa0=fa0, fb0=fb0)
    info = out["info"]
    assert info["n_candidates"][0] == 8 and info["n_contacts"] == (0, 0) and info["n_tet_grid_builds"] == 1 and info["n_face_grid_builds"] == 0
    assert np.array_equal(out["fa"].reshape(-1), fa0) and np.array_equal(out["fb"].reshape(-1), fb0)
    ref = _reference(ga, gb, K)
    assert len(ref["dirs"][0]["candidates"]) == 8 and len(ref["dirs"][0]["node"]) == 0 and ref["dirs"][0]["contain_margin"].min() > 0.01
    ga.close(); gb.close()


@pytest.mark.parametrize("name", ["two_way", "many_onto_one", "deep"])
def test_scan_and_ring_give_the_same_bits(name):
    ga, gb = _pair(name)
    n_faces = (len(gb.surface()["faces"]), len(ga.surface()["faces"]))
    with _Env(FEMBRAIN_BODY_CONTACT="ring", FEMBRAIN_BODY_CONTACT_BUDGET=None):
        ring, again = _call(ga, gb, K), _call(ga, gb, K)
    with _Env(FEMBRAIN_BODY_CONTACT="scan", FEMBRAIN_BODY_CONTACT_BUDGET=None):
        scan = _call(ga, gb, K)
    with _Env(FEMBRAIN_BODY_CONTACT="ring", FEMBRAIN_BODY_CONTACT_BUDGET=1):
        starved = _call(ga, gb, K)
    with _Env(FEMBRAIN_BODY_CONTACT=None, FEMBRAIN_BODY_CONTACT_BUDGET=None):
        default = _call(ga, gb, K)
    assert ring["info"]["path"] == fl.FB_BODY_CONTACT_RING and scan["info"]["path"] == fl.FB_BODY_CONTACT_SCAN and default["info"]["path"] == fl.FB_BODY_CONTACT_RING
    every = sum(n * f for n, f in zip(scan["info"]["n_contacts"], n_faces))
    assert scan["info"]["faces_tested"] == every and scan["info"]["n_face_grid_builds"] == 0
    assert ring["info"]["n_face_grid_builds"] == sum(1 for n in ring["info"]["n_contacts"] if n)
    assert 0 < ring["info"]["faces_tested"] and starved["info"]["faces_tested"] > every   # every point gave up and was scanned
    print(name, "faces tested: ring", ring["info"]["faces_tested"], "scan", every)
    _same_bits(ring, again)
    assert ring["info"]["faces_tested"] == again["info"]["faces_tested"]
    for other in (scan, starved, default):
        _same_bits(ring, other)
    ga.close(); gb.close()


def test_additivity_and_direction_masks():
    ga, gb = _pair("two_way")
    rng = np.random.default_rng(7)
    fa0, fb0 = rng.normal(size=3 * ga.n_nodes) * 5.0, rng.normal(size=3 * gb.n_nodes) * 5.0
    both = _call(ga, gb, K, fa0=fa0, fb0=fb0)
    _compare(both, _reference(ga, gb, K, fa0=fa0, fb0=fb0), 0.0, "onto a prior vector")
    touched = np.concatenate([both["dirs"][0]["node"], ga.surface()["faces"][both["dirs"][1]["face"]].reshape(-1)])
    untouched = ~np.isin(np.arange(ga.n_nodes), touched)
    assert untouched.any() and np.array_equal(both["fa"][untouched], fa0.reshape(-1, 3)[untouched])
    # one direction after the other on the same vectors is the call with both: the order of the sums is a into b first
    for g, f in ((ga, fa0), (gb, fb0)):
        g.set_external_forces(f)
    i1 = ga.body_contact(gb, K, directions="a_into_b")
    d1 = ga.read_body_contact("a_into_b")
    assert i1["n_contacts"][1] == 0 and len(ga.read_body_contact("b_into_a")["node"]) == 0
    i2 = ga.body_contact(gb, K, directions=fl.FB_BODY_B_INTO_A)
    d2 = ga.read_body_contact("b_into_a")
    assert i2["n_contacts"][0] == 0 and (i1["n_contacts"][0], i2["n_contacts"][1]) == both["info"]["n_contacts"]
    for key in d1:
        assert np.array_equal(d1[key], both["dirs"][0][key]) and np.array_equal(d2[key], both["dirs"][1][key])
    assert np.array_equal(ga.external_forces().reshape(-1, 3), both["fa"]) and np.array_equal(gb.external_forces().reshape(-1, 3), both["fb"])
    # the timing entry point runs the same stages, adds no force and leaves the last call's contacts as they are
    seconds = ga.time_body_contact(gb, K, reps=2)
    assert seconds.shape == (5,) and np.isfinite(seconds).all() and (seconds >= 0).all() and seconds.sum() > 0
    assert np.array_equal(ga.external_forces().reshape(-1, 3), both["fa"]) and np.array_equal(gb.external_forces().reshape(-1, 3), both["fb"])
    assert np.array_equal(ga.read_body_contact("b_into_a")["closest"], d2["closest"])
    ga.close(); gb.close()


def test_invalid_arguments():
    ga, gb = _pair("two_way")
    cases = [(ga, dict(stiffness=K)), (gb, dict(stiffness=-1.0)), (gb, dict(stiffness=np.inf)), (gb, dict(stiffness=K, depth_cap=-0.1)),
             (gb, dict(stiffness=K, depth_cap=np.nan)), (gb, dict(stiffness=K, directions=0))]
    for other, kw in cases:
        with pytest.raises(fl.FbError) as e:
            ga.body_contact(other, **kw)
        assert e.value.code == fl.FB_EINVAL
        for g in (ga, gb):
            g.set_uniform_force(1, -5.0)
            g.do_timestep()
            assert g.last.converged == 1
    n_dev = fl.lib().fb_device_count()
    if n_dev > 1:   # handles on different devices
        va, ta = truth_cube(3, 3, 3, 0.1)
        far = FemIntegrator(va, ta, device=1, **KW)
        with pytest.raises(fl.FbError) as e:
            ga.body_contact(far, K)
        assert e.value.code == fl.FB_EINVAL
        far.close()
    ga.close(); gb.close()


def test_a_position_that_is_not_a_number_is_refused():
    """one NaN in q of either body: FB_EINVAL after the boxes, and neither force vector is written"""
    for which in (1, 0):  # the NaN in body b, then in body a
        ga, gb = _pair("two_way")
        rng = np.random.default_rng(11)
        fa0, fb0 = rng.normal(size=3 * ga.n_nodes), rng.normal(size=3 * gb.n_nodes)
        ga.set_external_forces(fa0)
        gb.set_external_forces(fb0)
        g = (ga, gb)[which]
        q = np.zeros(3 * g.n_nodes)
        q[3 * 17 + 1] = np.nan
        g.set_q_state(q)
        with pytest.raises(fl.FbError) as e:
            ga.body_contact(gb, K)
        assert e.value.code == fl.FB_EINVAL and "not finite" in str(e.value)
        assert np.array_equal(ga.external_forces(), fa0) and np.array_equal(gb.external_forces(), fb0)   # nothing was written
        ga.close(); gb.close()


def _sharded_worker(rank, world, shm_name, q):
    try:
        import ctypes as C
        L = fl.lib()
        comm = C.c_void_p()
        fl.check(L.fb_comm_create_local(C.byref(comm), rank, world, shm_name.encode(), 8 << 20, 0))
        v, t = truth_cube(6, 4, 4, 0.1)
        fixed = np.arange(3 * 16, dtype=np.int32)
        splits = np.array([0, 48, 96], np.int32)
        g = FemIntegrator(v, t, fixed, shard=(world, rank, splits, comm))
        plain = FemIntegrator(v + np.array([0.03, 0.05, 0.02])[None, :], t, fixed)
        codes = []
        for a, b in ((g, plain), (plain, g)):
            try:
                a.body_contact(b, K)
                codes.append(0)
            except fl.FbError as e:
                codes.append(e.code)
        for h in (g, plain):   # both still step
            h.set_uniform_force(1, -50.0)
            h.do_timestep()
            codes.append(h.last.converged)
        q.put((rank, codes))
        g.close(); plain.close()
        L.fb_comm_destroy(comm)
    except Exception as e:  # surface the failure instead of hanging the peer
        q.put((rank, repr(e)))
        q.close()
        q.join_thread()
        os._exit(1)


def test_a_sharded_handle_is_refused():
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, "/fembrain_test_bc_%d" % os.getpid(), q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=120) for _ in procs]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for rank, codes in res:
        assert codes == [fl.FB_EINVAL, fl.FB_EINVAL, 1, 1], (rank, codes)
