"""fb_fem_self_contact on the device against tests/selfcontactref.py, the rule in numpy by brute force.

As in test_body_contact_gpu.py: contact sets and every integer output (node, element, face) of the points whose decision lies outside
rounding (containment margin >= 1e-9, gap to a different closest point >= 1e-9 x extent) are compared exactly; a test may leave out at
most 2 % of the surface vertices, and none in the structured shapes.  The doubles (closest point, weights, depth, the force vector, the
two sums) are compared BIT FOR BIT wherever every point is generic: the device functions and the reference are the same sequence of
fp64 operations without contraction."""
import ctypes as C
import os

import numpy as np
import pytest

import bodycontactref as B
import selfcontactref as S
from fembrain_amd import lib as fl
from fembrain_amd.fem import FemIntegrator
from fembrain_amd.meshgen import truth_cube

pytestmark = pytest.mark.gpu

K = 1000.0
KW = dict(E=1e6, timestep=0.01)
MODES = {"any": S.ANY, "other_parts": S.OTHER_PARTS}


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


def _current(g):
    x, t = g.read_mesh()
    return x, t, x + g.get_q_state()[0].reshape(-1, 3)


_REFS = {}


def _reference(g, mode, stiffness=K, depth_cap=0.0, f0=None, key=None):
    """the reference at the handle's current state; key: computed once and shared by the tests that name it (never changed afterwards)"""
    if key is not None and key in _REFS:
        return _REFS[key]
    x, t, cur = _current(g)
    ref = S.self_contact(x, t, cur, stiffness, depth_cap, MODES[mode], f0)
    ref["extent"] = float((cur.max(axis=0) - cur.min(axis=0)).max())
    if key is not None:
        _REFS[key] = ref
    return ref


def _call(g, mode, stiffness=K, depth_cap=0.0, f0=None):
    """sets the force vector (zero where none is given), calls, returns everything that comes back"""
    g.set_external_forces_to_zero() if f0 is None else g.set_external_forces(f0)
    info = g.self_contact(stiffness, depth_cap, mode)
    return dict(info=info, contacts=g.read_self_contact(), f=g.external_forces().reshape(-1, 3))


def _compare(out, r, max_left_out=0.0, label=""):
    """the device's call against the reference's; returns the number of surface vertices left out"""
    info, dev = out["info"], out["contacts"]
    cand_ok, contact_ok = B.generic(r, r["extent"])
    left = int((~cand_ok).sum()) + int((~contact_ok & cand_ok[r["in_contact"]]).sum())
    print("%s: %d surface vertices, %d contacts (device %d), degenerate %d (device %d), margins %.3g / %.3g, left out %d, path %d, faces tested %d" % (
        label, len(cand_ok), len(r["node"]), info["n_contacts"], int(r["degenerate"].sum()), info["n_degenerate"], r["contain_margin"].min(),
        r["gap"].min() if len(r["node"]) else np.inf, left, info["path"], info["faces_tested"]))
    assert info["n_points"] == len(r["vids"]) and info["n_contacts"] == len(dev["node"])
    sure = set(r["candidates"][cand_ok].tolist())
    assert set(n for n in dev["node"].tolist() if n in sure) == set(n for n in r["node"].tolist() if n in sure)
    assert np.all(np.diff(dev["node"]) > 0)
    where = {int(n): i for i, n in enumerate(dev["node"])}
    keep = np.nonzero(contact_ok)[0]
    rows = np.array([where[int(r["node"][i])] for i in keep], np.int64)
    assert np.array_equal(dev["element"][rows], r["element"][keep]) and np.array_equal(dev["face"][rows], r["face"][keep])
    for key in ("closest", "bary", "depth"):
        assert np.array_equal(dev[key][rows], r[key][keep]), (label, key, np.abs(dev[key][rows] - r[key][keep]).max())
    assert left <= max_left_out * len(cand_ok), (left, len(cand_ok))
    if cand_ok.all() and contact_ok.all():  # every contribution is pinned down: the vector and the sums bit for bit
        assert info["n_contacts"] == len(r["node"]) and info["n_degenerate"] == int(r["degenerate"].sum())
        assert np.array_equal(out["f"], r["f"]), (label, np.abs(out["f"] - r["f"]).max())
        assert np.array_equal(info["force_on_points"], r["force_on_points"]) and np.array_equal(info["force_on_faces"], r["force_on_faces"])
        assert info["max_depth"] == r["max_depth"]
    return left


def _same_bits(x, y):
    assert x["info"].keys() == y["info"].keys()
    for key, v in x["info"].items():
        if key not in ("path", "faces_tested", "n_point_grid_builds", "n_face_grid_builds", "n_parts_builds"):
            assert np.array_equal(v, y["info"][key]), key
    for key in x["contacts"]:
        assert np.array_equal(x["contacts"][key], y["contacts"][key]), key
    assert np.array_equal(x["f"], y["f"])


def _union(name, **kw):
    v, t, _, _ = S.union(name)
    return FemIntegrator(v, t, **dict(KW, **kw))


# surface vertices and contacts of the reference, per shape: what tests/selfcontactref.py gives on the CPU (test_self_contact_ref.py asserts the
# same on the shapes that need no device); the cut beam has one candidate whose containment margin is below 1e-9, the others none
WANT = {"two_way": (148, 25), "many_onto_one": (760, 396), "deep": (514, 26), "rolled": (240, 12), "cut_pressed": (436, 129)}


@pytest.mark.parametrize("mode", ["any", "other_parts"])
def test_union_of_two_cubes_both_modes(mode):
    g = _union("two_way")
    out = _call(g, mode)
    ref = _reference(g, mode, key=("two_way", mode))
    assert (len(ref["vids"]), len(ref["node"])) == WANT["two_way"] and out["info"]["n_contacts"] == 25
    assert _compare(out, ref, 0.0, "two_way " + mode) == 0
    assert out["info"]["n_point_grid_builds"] == 1 and out["info"]["n_parts_builds"] == (1 if mode == "other_parts" else 0)
    # 24 of the 25 pushed nodes also push back as corners of a face
    assert len(np.intersect1d(out["contacts"]["node"], g.surface()["faces"][out["contacts"]["face"]].reshape(-1))) == 24
    g.close()


def test_many_onto_one_a_node_collects_more_records_than_a_wavefront_has_lanes():
    g = _union("many_onto_one")
    out = _call(g, "other_parts")
    ref = _reference(g, "other_parts", key=("many_onto_one", "other_parts"))
    assert (len(ref["vids"]), len(ref["node"])) == WANT["many_onto_one"] and ref["records_per_node"].max() == 177
    assert _compare(out, ref, 0.0, "many_onto_one") == 0
    c = out["contacts"]
    per_node = np.bincount(np.concatenate([c["node"], g.surface()["faces"][c["face"]].reshape(-1)]))
    assert per_node.max() > 64
    g.close()


def test_many_onto_one_under_any_every_bit():
    """The same union under ANY.  The small cube's cells are shallower than the penetration, so this is past the depth up to which ANY
    means what a caller wants (the header says so): faces of a vertex's own cube win, and 321 of the 396 contacts have a second closest
    point at the same distance to within 1e-9 -- the generic filter would leave them out.  The RULE is as well defined here as
    anywhere, a tie in d goes to the lowest face on both sides, and device and reference are the same fp64 operations in the same
    order: so nothing is left out and everything is compared exactly -- every integer, every double, the vector and the sums."""
    g = _union("many_onto_one")
    out = _call(g, "any")
    ref = _reference(g, "any")
    assert (len(ref["vids"]), len(ref["node"])) == WANT["many_onto_one"] and ref["n_dropped"] == 0 and ref["contain_margin"].min() > 1e-3
    info, dev = out["info"], out["contacts"]
    print("many_onto_one any: device %d contacts, faces that differ %d, max |f - ref| %.3g, faces tested %d" % (
        info["n_contacts"], int((dev["face"] != ref["face"]).sum()) if len(dev["face"]) == len(ref["face"]) else -1, np.abs(out["f"] - ref["f"]).max(), info["faces_tested"]))
    assert info["n_contacts"] == 396 and info["n_degenerate"] == 0
    for key in ("node", "element", "face", "closest", "bary", "depth"):
        assert np.array_equal(dev[key], ref[key]), key
    assert np.array_equal(out["f"], ref["f"]) and info["max_depth"] == ref["max_depth"]
    assert np.array_equal(info["force_on_points"], ref["force_on_points"]) and np.array_equal(info["force_on_faces"], ref["force_on_faces"])
    per_node = np.bincount(np.concatenate([dev["node"], g.surface()["faces"][dev["face"]].reshape(-1)]))
    assert per_node.max() == ref["records_per_node"].max() == 24
    g.close()


def test_deep_and_the_cap():
    g = _union("deep")
    out = _call(g, "other_parts")
    ref = _reference(g, "other_parts", key=("deep", "other_parts"))
    assert (len(ref["vids"]), len(ref["node"])) == WANT["deep"]
    assert _compare(out, ref, 0.0, "deep") == 0
    assert 0.36 < out["contacts"]["depth"].min() and out["contacts"]["depth"].max() < 0.44   # the closest face is cells away from the point
    capped = _call(g, "other_parts", depth_cap=0.1)
    assert capped["info"]["max_depth"] == 0.1
    assert _compare(capped, _reference(g, "other_parts", depth_cap=0.1), 0.0, "deep capped") == 0
    assert np.array_equal(capped["contacts"]["depth"], out["contacts"]["depth"])   # (read back before the cap)
    g.close()


def _rolled():
    v, t, cur = S.rolled_beam()
    g = FemIntegrator(v, t, **KW)
    g.set_q_state((cur - v).reshape(-1))
    return g


def test_rolled_beam_one_part_any():
    g = _rolled()
    out = _call(g, "any")
    ref = _reference(g, "any", key=("rolled", "any"))
    assert (len(ref["vids"]), len(ref["node"])) == WANT["rolled"]
    assert _compare(out, ref, 0.0, "rolled") == 0
    g.close()


def test_one_part_under_other_parts_builds_and_writes_nothing():
    g = _rolled()
    f0 = np.random.default_rng(5).normal(size=3 * g.n_nodes)
    out = _call(g, "other_parts", f0=f0)
    info = out["info"]
    assert info["n_contacts"] == 0 and info["n_point_grid_builds"] == 0 and info["n_face_grid_builds"] == 0 and info["path"] == fl.FB_BODY_CONTACT_NONE
    assert info["faces_tested"] == 0 and np.array_equal(out["f"].reshape(-1), f0) and len(out["contacts"]["node"]) == 0
    g.close()


def _cut_beam():
    from test_detach_gpu import _beam, _blade
    v, t, fixed = _beam()
    g = FemIntegrator(v, t, fixed, **KW)
    return g, v, _blade(v)


def _cut(g, blade):
    info, _ = g.cut(blade, mode="carry", track=False)
    assert info["status"] == fl.FB_CUT_DONE
    g.r = 3 * int(g._L.fb_fem_num_nodes(g.h))


def test_cut_beam_lips_coincide_then_pressed():
    g, v, blade = _cut_beam()
    _cut(g, blade)
    n = g.r // 3
    # right after the cut, both modes: every contact is at d == 0 and the force vector keeps its bits
    f0 = np.random.default_rng(9).normal(size=3 * n)
    for mode in ("any", "other_parts"):
        out = _call(g, mode, f0=f0)
        assert out["info"]["n_points"] == WANT["cut_pressed"][0]
        assert out["info"]["n_degenerate"] == out["info"]["n_contacts"] and (out["contacts"]["depth"] == 0).all()
        assert np.array_equal(out["f"].reshape(-1), f0)
    # the far part pushed 0.31 of a cell into the near one
    x, t = g.read_mesh()
    _, node_part, n_parts = S.parts_of(t, len(x))
    assert n_parts == 2 and x[node_part == 1, 0].mean() > x[node_part == 0, 0].mean()
    q = g.get_q_state()[0].reshape(-1, 3)
    g.set_q_state((q + np.where((node_part == 1)[:, None], np.array(S.PRESS)[None, :], 0.0)).reshape(-1))
    outs = {}
    for mode in ("any", "other_parts"):
        outs[mode] = _call(g, mode)
        ref = _reference(g, mode, key=("cut_pressed", mode))
        assert (len(ref["vids"]), len(ref["node"])) == WANT["cut_pressed"]
        assert _compare(outs[mode], ref, 0.02, "cut pressed " + mode) == 1   # (one candidate on a boundary of an element: margin 7e-15)
    both = np.intersect1d(outs["any"]["contacts"]["node"], outs["other_parts"]["contacts"]["node"])
    fa = outs["any"]["contacts"]["face"][np.isin(outs["any"]["contacts"]["node"], both)]
    fo = outs["other_parts"]["contacts"]["face"][np.isin(outs["other_parts"]["contacts"]["node"], both)]
    assert (fa != fo).any()      # this deep, ANY takes faces of the vertex's own side (the header says so)
    assert round(outs["any"]["info"]["max_depth"], 4) == 0.0275 and round(outs["other_parts"]["info"]["max_depth"], 4) == 0.0309
    g.set_uniform_force(1, -10.0)
    g.do_timestep()
    g.close()


def test_parts_are_built_once_and_again_after_a_cut():
    g, v, blade = _cut_beam()
    assert g.self_contact(K, mode="other_parts")["n_parts_builds"] == 1
    assert g.self_contact(K, mode="other_parts")["n_parts_builds"] == 0
    assert g.self_contact(K, mode="any")["n_parts_builds"] == 0
    _cut(g, blade)
    assert g.self_contact(K, mode="other_parts")["n_parts_builds"] == 1
    assert g.self_contact(K, mode="other_parts")["n_parts_builds"] == 0
    g.close()


def test_permuted_ids_and_forced_renumbering():
    v, t, _, _ = S.union("many_onto_one")
    p = np.random.default_rng(3).permutation(len(v))   # new id of old node i
    v2 = np.empty_like(v)
    v2[p] = v
    g = FemIntegrator(v2, p[t].astype(np.int32), renumber=fl.FB_RENUMBER_ON, **KW)
    assert g.renumbering()[0]
    out = _call(g, "other_parts")
    ref = _reference(g, "other_parts")
    assert len(ref["node"]) == WANT["many_onto_one"][1]
    assert _compare(out, ref, 0.0, "permuted") == 0
    assert set(out["contacts"]["node"]) <= set(g.surface()["vertex_ids"]) and out["contacts"]["face"].max() < len(g.surface()["faces"])
    g.close()


def test_additivity_same_bits_twice_and_timing_adds_nothing():
    g = _union("two_way")
    f0 = np.random.default_rng(7).normal(size=3 * g.n_nodes) * 5.0
    once = _call(g, "any", f0=f0)
    assert _compare(once, _reference(g, "any", f0=f0), 0.0, "onto a prior vector") == 0
    c = once["contacts"]
    touched = np.concatenate([c["node"], g.surface()["faces"][c["face"]].reshape(-1)])
    untouched = ~np.isin(np.arange(g.n_nodes), touched)
    assert untouched.any() and np.array_equal(once["f"][untouched], f0.reshape(-1, 3)[untouched])
    again = _call(g, "any", f0=f0)
    _same_bits(once, again)
    assert once["info"]["faces_tested"] == again["info"]["faces_tested"]
    seconds = g.time_self_contact(K, mode="any", reps=2)
    assert seconds.shape == (5,) and np.isfinite(seconds).all() and (seconds >= 0).all() and seconds.sum() > 0
    assert np.array_equal(g.external_forces().reshape(-1, 3), once["f"])
    assert np.array_equal(g.read_self_contact()["closest"], once["contacts"]["closest"])
    g.close()


@pytest.mark.parametrize("name,mode", [("two_way", "any"), ("many_onto_one", "other_parts"), ("deep", "other_parts")])
def test_scan_ring_and_a_starved_ring_give_the_same_bits(name, mode):
    g = _union(name)
    nf = len(g.surface()["faces"])
    with _Env(FEMBRAIN_SELF_CONTACT="ring", FEMBRAIN_SELF_CONTACT_BUDGET=None):
        ring = _call(g, mode)
    with _Env(FEMBRAIN_SELF_CONTACT="scan", FEMBRAIN_SELF_CONTACT_BUDGET=None):
        scan = _call(g, mode)
    with _Env(FEMBRAIN_SELF_CONTACT="ring", FEMBRAIN_SELF_CONTACT_BUDGET=3):
        starved = _call(g, mode)
    with _Env(FEMBRAIN_SELF_CONTACT=None, FEMBRAIN_SELF_CONTACT_BUDGET=None):
        default = _call(g, mode)
    assert ring["info"]["path"] == fl.FB_BODY_CONTACT_RING and scan["info"]["path"] == fl.FB_BODY_CONTACT_SCAN and default["info"]["path"] == fl.FB_BODY_CONTACT_RING
    every = scan["info"]["n_contacts"] * nf
    assert scan["info"]["faces_tested"] == every and scan["info"]["n_face_grid_builds"] == 0 and ring["info"]["n_face_grid_builds"] == 1
    assert 0 < ring["info"]["faces_tested"] and starved["info"]["faces_tested"] > every   # every point gave up and was scanned
    print(name, "faces tested: ring", ring["info"]["faces_tested"], "scan", every)
    for other in (scan, starved, default):
        _same_bits(ring, other)
    assert _compare(ring, _reference(g, mode, key=(name, mode)), 0.0, name + " ring") == 0
    g.close()


def test_elements_over_many_cells_take_the_overflow_list():
    """Node 572 of the "deep" union, an inner node of the large cube next to the small one, is pulled 20 body lengths out along the line
    from the opposite face of element 2183 through the node: that element only grows, so it keeps the points it held, and every element on
    the node now reaches across the whole grid of surface vertices (9 x 8 x 9 cells over the stretched box) -- hundreds of cells each
    against kEmbedWideCells = 64.  By the reference most of the 26 contacts then have such an element as their LOWEST containing one: a
    device that skipped the overflow list, or walked it wrongly, would report other elements or lose the contacts."""
    g = _union("deep")
    x, t = g.read_mesh()
    e, k, pull = 2183, 2, 20.0
    assert e in _reference(g, "other_parts", key=("deep", "other_parts"))["element"] and t[e, k] == 572
    d = x[t[e, k]] - x[t[e, [j for j in range(4) if j != k]]].mean(axis=0)
    q = np.zeros_like(x)
    q[t[e, k]] = d / np.linalg.norm(d) * pull
    g.set_q_state(q.reshape(-1))
    out = _call(g, "other_parts")
    ref = _reference(g, "other_parts")
    span = S.cells_spanned(x + q, t, len(ref["vids"]))
    in_wide = span[ref["element"]] > 64
    print("stretched: %d elements over more than 64 cells (the widest %d), %d of %d contacts lie in one" % ((span > 64).sum(), span.max(), in_wide.sum(), len(in_wide)))
    assert (span > 64).sum() == 24 and span[e] > 64 and span[span > 64].min() > 4 * 64      # (far from the threshold: the grid rule in numpy need not round as the library's)
    assert len(ref["node"]) == WANT["deep"][1] and in_wide.sum() == 17 and (~in_wide).sum() == 9    # both walks decide contacts of this call
    assert _compare(out, ref, 0.0, "stretched") == 0
    assert np.array_equal(out["contacts"]["element"], ref["element"])
    g.close()


def test_invalid_arguments():
    g = _union("two_way")
    L = fl.lib()
    info = fl.SelfContactInfo()
    assert L.fb_fem_self_contact(g.h, None, C.byref(info)) == fl.FB_EINVAL
    f0 = np.random.default_rng(2).normal(size=3 * g.n_nodes)
    g.set_external_forces(f0)
    for kw in (dict(stiffness=-1.0), dict(stiffness=np.nan), dict(stiffness=np.inf), dict(stiffness=K, depth_cap=-0.1), dict(stiffness=K, depth_cap=np.nan),
               dict(stiffness=K, mode=2), dict(stiffness=K, mode=-1)):
        with pytest.raises(fl.FbError) as e:
            g.self_contact(**kw)
        assert e.value.code == fl.FB_EINVAL
    q = np.zeros(3 * g.n_nodes)
    q[3 * 17 + 1] = np.nan
    g.set_q_state(q)
    for mode in ("any", "other_parts"):
        with pytest.raises(fl.FbError) as e:
            g.self_contact(K, mode=mode)
        assert e.value.code == fl.FB_EINVAL
    assert np.array_equal(g.external_forces(), f0)   # nothing was written
    g.set_q_state(np.zeros(3 * g.n_nodes))
    assert g.self_contact(K)["n_contacts"] == 25
    g.close()


def _sharded_worker(rank, world, shm_name, q):
    try:
        L = fl.lib()
        comm = C.c_void_p()
        fl.check(L.fb_comm_create_local(C.byref(comm), rank, world, shm_name.encode(), 8 << 20, 0))
        v, t = truth_cube(6, 4, 4, 0.1)
        fixed = np.arange(3 * 16, dtype=np.int32)
        splits = np.array([0, 48, 96], np.int32)
        g = FemIntegrator(v, t, fixed, shard=(world, rank, splits, comm))
        codes = []
        for mode in ("any", "other_parts"):
            try:
                g.self_contact(K, mode=mode)
                codes.append(0)
            except fl.FbError as e:
                codes.append(e.code)
        g.set_uniform_force(1, -50.0)   # it still steps
        g.do_timestep()
        codes.append(g.last.converged)
        q.put((rank, codes))
        g.close()
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
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, "/fembrain_test_sc_%d" % os.getpid(), q)) for r in range(2)]
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
        assert codes == [fl.FB_EINVAL, fl.FB_EINVAL, 1], (rank, codes)
