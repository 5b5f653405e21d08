"""Meshes built for their SELL slice shapes (tests/test_product_inputs.py; inputs of product-level device checks against tests/pcgref.py),
and the census of what a live handle's persistent plan makes of them.

The handles of these inputs are built with renumber=FB_RENUMBER_OFF: the numbering IS the input.  A slice is 64 consecutive nodes and
as wide as its longest block row, so a part's widths follow from its node degrees:

  rod(2, 2, N), rod(3, 3, N)   truth_cube rods along k: a slice lies on one or two of the rod's lines, widths 8 and 11 / 8, 11 and 15
  tet_path(n)                  single tets and pairs that share a face: widths 4 and 5 (a node of an element has three neighbours, so no
                               referenced node has a row shorter than 4 -- widths 2 and 3 do not exist on a tet mesh)
  isolated(n)                  nodes no element references: identity rows, whole slices of width 1 from 128 consecutive ones on
  cube(n)                      a truth_cube block, widths 8, 11 and 15
  delaunay_lattice(m)          jittered lattice (moved here from test_fem_gpu.py): hull hubs, widths above 24
  hub(k)                       a node joined to k points on a sphere around it: one slice of width k + 1 (k >= 61: wider than the
                               element-major assembly and the LDS of a CU take)

  hub_strip(ks)                one slice per k of hubs of degree k: any width from 5 to 64 where it is wanted

``join`` concatenates parts in the order given; an int among them pads the numbering to a multiple of it with isolated nodes."""
import ctypes as C

import numpy as np

from fembrain_amd import lib as fl
from fembrain_amd.meshgen import fixed_vertices_to_dofs, synthetic_cut, truth_cube


# ---- parts: (vertices, tets, fixed node ids) ---------------------------------------------------------------------------------------
def rod(nx, ny, n):
    v, t = truth_cube(nx, ny, n, 0.1)
    return v, t, np.arange(0, nx * ny * n, n, dtype=np.int32)[:2]     # (k = 0 of the first two lines)


def cube(n):
    v, t = truth_cube(n, n, n, 0.1)
    return v, t, np.arange(n * n, dtype=np.int32)


def tet_path(n_single, n_pair):
    """n_single tets of four nodes of their own (width 4), then n_pair bipyramids of five nodes: two tets that share a face (width 5)"""
    base = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1], [0.1, 0.1, 0.1]])
    vs, ts = [], []
    at = 0
    for i in range(n_single):
        vs.append(base[:4] + [0.2 * i, 0, 0])
        ts.append([at, at + 1, at + 2, at + 3])
        at += 4
    for i in range(n_pair):
        vs.append(base[[0, 1, 2, 3, 4]] + [0.2 * i, 0.3, 0])
        ts.append([at, at + 1, at + 2, at + 3])
        ts.append([at + 4, at + 2, at + 1, at + 3])
        at += 5
    return np.concatenate(vs), np.array(ts, np.int32), np.zeros(0, np.int32)


def isolated(n):
    return np.stack([0.1 * np.arange(n), np.full(n, -1.0), np.zeros(n)], 1), np.zeros((0, 4), np.int32), np.zeros(0, np.int32)


def _orient(pts, t):
    vol = np.einsum("ij,ij->i", pts[t[:, 1]] - pts[t[:, 0]], np.cross(pts[t[:, 2]] - pts[t[:, 0]], pts[t[:, 3]] - pts[t[:, 0]])) / 6
    keep = np.abs(vol) > 1e-9
    t, vol = t[keep], vol[keep]
    t[vol < 0] = t[vol < 0][:, [0, 2, 1, 3]]
    return np.ascontiguousarray(t)


def _delaunay_lattice(m, seed=2):
    """Delaunay tetrahedra of an m^3 lattice with jittered points: hull nodes with 40 and more neighbours next to interior nodes with 15"""
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(float)
    pts = (g + rng.uniform(-0.35, 0.35, size=g.shape)) * 0.1
    t = Delaunay(pts).simplices.astype(np.int32)
    vol = np.einsum("ij,ij->i", pts[t[:, 1]] - pts[t[:, 0]], np.cross(pts[t[:, 2]] - pts[t[:, 0]], pts[t[:, 3]] - pts[t[:, 0]])) / 6
    keep = np.abs(vol) > 1e-9
    t, vol = t[keep], vol[keep]
    t[vol < 0] = t[vol < 0][:, [0, 2, 1, 3]]
    return pts, np.ascontiguousarray(t), fixed_vertices_to_dofs(np.nonzero(g[:, 0] == 0)[0])


def delaunay_lattice(m, seed=2):
    v, t, fd = _delaunay_lattice(m, seed)
    return v, t, np.unique(fd // 3).astype(np.int32)


def hub(k, seed=5):
    """node 0 at the centre of k points on a sphere (their convex hull's triangles, each joined to the centre): degree k"""
    from scipy.spatial import ConvexHull
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(k, 3))
    p = 0.1 * p / np.linalg.norm(p, axis=1)[:, None]
    tri = ConvexHull(p).simplices.astype(np.int32)
    v = np.concatenate([np.zeros((1, 3)), p])
    t = np.concatenate([np.zeros((len(tri), 1), np.int32), tri + 1], axis=1)
    return v, _orient(v, t), np.array([1], np.int32)


def hub_block(k):
    """as many hub(k) as 64 nodes hold: placed on a slice boundary, a slice of width k + 1 exactly (k <= 63)"""
    parts = [hub(k, seed=100 * k + i) for i in range(64 // (k + 1))]
    return join(parts)[:2] + (np.array([1], np.int32),)


def hub_strip(ks):
    """one slice per k, in the order given: the widths k + 1 on purpose (to be placed on a slice boundary: `64` in front of it in join)"""
    v, t, _ = join([x for k in ks for x in (hub_block(k), 64)])
    return v, t, np.arange(1, len(v), 64, dtype=np.int32)


def fan(seed=9):
    """32 nodes `out`, then five slices of 64: `ia`, `ib`, `ic`, and the leaves `a`, `b`, each leaf the apex of one tet: a_i on two of
    `out` and ia_i, b_i on one of `out`, ib_i and ic_i.  Placed with `ia` on the first slice of a workgroup (`out` ends the workgroup
    before), a leaf's row is (out, out, ia, diagonal) / (out, ib, ic, diagonal): the LDS window of the (12, 6) / (12, 7) kernels takes one /
    two mirror layers and the diagonal -- on-chip runs of 2 and 3 layers, clipped by the slice's width, behind 2 / 1 streamed slots --
    and finds every transposed block among the resident slots of the rows of ia, ib, ic (four slots wide)."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0, 1, size=(32 + 5 * 64, 3))
    i = np.arange(64)
    out, ia, ib, ic, a, b = np.arange(32), 32 + i, 96 + i, 160 + i, 224 + i, 288 + i
    t = np.concatenate([np.stack([out[(2 * i) % 32], out[(2 * i + 1) % 32], ia, a], 1), np.stack([out[i % 32], ib, ic, b], 1)])
    t = _orient(v, t.astype(np.int32))
    assert len(t) == 128
    return v, t, out[:2].astype(np.int32)


def join(parts, n_nodes=None):
    """The parts one after the other; an int among them pads the numbering with isolated nodes to a multiple of it, ("at", n) up to node n.  n_nodes: isolated
    nodes appended up to that count.  Returns (vertices, tets, fixed DOFs)."""
    vs, ts, fx = [np.zeros((0, 3))], [np.zeros((0, 4), np.int32)], [np.zeros(0, np.int32)]
    at = 0
    for k, part in enumerate(parts):
        if isinstance(part, int):
            part = isolated((-at) % part)
        elif isinstance(part[0], str):
            assert part[1] >= at, (part, at)
            part = isolated(part[1] - at)
        v, t, f = part
        vs.append(np.asarray(v, float).reshape(-1, 3) + [0.0, 0.0, 10.0 * k])      # (apart in space; only the numbering couples anything)
        ts.append(np.asarray(t, np.int32).reshape(-1, 4) + at)
        fx.append(np.asarray(f, np.int32) + at)
        at += len(v)
    if n_nodes is not None:
        assert n_nodes >= at, (n_nodes, at)
        vs.append(isolated(n_nodes - at)[0] + [0.0, 0.0, 10.0 * len(parts)])
    return (np.ascontiguousarray(np.concatenate(vs)), np.ascontiguousarray(np.concatenate(ts).astype(np.int32)),
            fixed_vertices_to_dofs(np.concatenate(fx)))


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------
# The orders were chosen on the host plan (fb_plan_create: slice_off) so that every width class of the SpMV and persistent PCG kernels' tails
# occurs, and -- with the deal of pipe_slices / pipe_deal_by_slots restated below -- in workgroups of the wanted sizes.
FAN_SLICE = 36       # the first slice of a workgroup on 32 CUs with 288 slices (9 per workgroup) and with 370 (12, 12, 12, 11 of every 47)


def _regular_parts():
    return [rod(2, 2, 448), isolated(192), tet_path(64, 0), ("at", 64 * FAN_SLICE - 32), fan(), cube(15), 64, hub_strip(range(4, 30)), tet_path(96, 120),
            64, hub_strip(range(29, 3, -1)), rod(3, 3, 256), isolated(130), cube(15), 64, hub_strip(list(range(7, 25, 2)) + list(range(8, 25, 2))),
            rod(2, 3, 128), tet_path(40, 8)]


def regular(n_nodes=18369):
    """cube-like parts only: rods, tet paths, isolated runs, the fan, cube blocks and strips of hub blocks of every width from 5 to 30;
    18,369 nodes = 288 slices (9 per workgroup on 32 CUs), one row in the last"""
    return join(_regular_parts(), n_nodes=n_nodes)


def regular12(n_nodes=23617):
    """`regular` and more of the same: 23,617 nodes = 370 slices, 12, 11 and 10 per workgroup on 32 CUs"""
    return join(_regular_parts() + [64, hub_strip(range(30, 3, -2)), cube(15), rod(2, 2, 192), tet_path(30, 18)], n_nodes=n_nodes)


def irregular(n_nodes=20415):
    """the same kinds with two Delaunay lattices and a hub of 70 among them; 20,415 nodes = 319 slices, 63 rows in the last"""
    parts = [delaunay_lattice(12), 64, hub_strip(range(4, 30)), rod(2, 2, 320), hub(70), isolated(150), cube(14), tet_path(96, 64), delaunay_lattice(16, seed=3),
             64, hub_strip(range(29, 3, -1)), rod(3, 3, 256), cube(13), isolated(128), rod(2, 2, 192)]
    return join(parts, n_nodes=n_nodes)


def large(n_nodes=65601):
    """65,601 nodes = 1,026 slices (the split SpMV deals a slice to two wavefronts from 1,025 on), with odd widths"""
    parts = [cube(32), isolated(192), rod(3, 3, 1856), 64, delaunay_lattice(12), tet_path(200, 200), 64, hub_strip(range(4, 30)), rod(2, 2, 2500), isolated(256)]
    return join(parts, n_nodes=n_nodes)


def cut_delta(v, t):
    """synthetic_cut(stride=3) of a joined input as (cut vertices, cut tets, delta for resync_delta): the plane y = lowest + 0.45 of the
    extent crosses every part that has elements on both sides of it -- the cube blocks and the 3-wide rods --, every third crossed element
    is split in four on a new node appended to the numbering"""
    return synthetic_cut(v, t, axis=1, where=0.45, stride=3)


def regular_cut():
    """`regular` after cut_delta, as a fresh mesh (what a handle holds after resync_delta of the same delta)"""
    v, t, fixed = regular()
    v2, t2, _ = cut_delta(v, t)
    return v2, t2, fixed


INPUTS = {"regular": regular, "regular_cut": regular_cut, "regular12": regular12, "irregular": irregular, "large": large}
_cache = {}


def mesh(name):
    if name not in _cache:
        _cache[name] = INPUTS[name]()
    return _cache[name]


# ---- the host plan -------------------------------------------------------------------------------------------------------------------
def host_plan(v, t, fixed, names=("slice_off",)):
    L = fl.lib()
    h = C.c_void_p()
    tt = np.ascontiguousarray(t, np.int32)
    fd = fl.as_i32(fixed)
    fl.check(L.fb_plan_create(C.byref(h), len(v), len(tt), fl.iptr(tt), len(fd), fl.iptr(fd), 1, 0, None))
    out = {}
    try:
        for name in names:
            cnt = L.fb_plan_get(h, name.encode(), None, 0)
            a = np.zeros(max(cnt, 1), np.int32)
            assert L.fb_plan_get(h, name.encode(), fl.iptr(a), cnt) == cnt
            out[name] = a[:cnt]
    finally:
        L.fb_plan_destroy(h)
    return out


def widths(v, t, fixed):
    return np.diff(host_plan(v, t, fixed)["slice_off"])


def width_classes(wd):
    """the classes the two-launch cases name"""
    wd = np.asarray(wd)
    return dict(one=bool((wd == 1).any()), narrow=bool(((wd >= 2) & (wd <= 5)).any()), odd=bool(((wd > 5) & (wd % 2 == 1)).any()),
                even=bool(((wd > 5) & (wd % 2 == 0)).any()), wide=bool((wd >= 25).any()), hub=bool((wd > 61).any()))


# ---- what the live handle planned ----------------------------------------------------------------------------------------------------
def device_plan(g, name):
    """fb_fem_device_plan_get(name) or None where the handle's plan has no such array"""
    L = fl.lib()
    n = L.fb_fem_device_plan_get(g.h, name.encode(), None, 0)
    if n < 0:
        return None
    a = np.zeros(max(n, 1), np.int32)
    assert L.fb_fem_device_plan_get(g.h, name.encode(), fl.iptr(a), n) == n
    return a[:n]


def pipe_slices(n_slices, nb, b):
    """pcg_pipe.hip.h pipe_slices: the equal deal"""
    xcd, j, per = b & 7, b >> 3, nb >> 3
    chunk = (n_slices + 7) >> 3
    lo = xcd * chunk
    ln = min(max(n_slices - lo, 0), chunk)
    base = ln // per
    rem = ln - base * per
    return lo + j * base + min(j, rem), base + (1 if j < rem else 0)


def deal(wg_first, n_slices, nb):
    """[(first slice, count)] per workgroup: pipe_deal"""
    if wg_first is not None and len(wg_first):
        return [(int(wg_first[b]), int(wg_first[nb + 1 + b])) for b in range(nb)]
    return [pipe_slices(n_slices, nb, b) for b in range(nb)]


def equal_share(count, lds_slots, klt):
    """pipe_deal_lds' equal shares as the plain kernels compute them: resident slots dealt to wavefront 0 .. count-1"""
    lbase = min(klt, lds_slots // max(count, 1))
    lrem = min(count, lds_slots - lbase * count) if lbase < klt else 0
    return [lbase + (1 if w < lrem else 0) for w in range(count)]


KPIPE2_KLT, TASK_STRIDE = 4, 16


def _pipe2_lds_slots(count, c16):
    # pcg_pipe2.hip.h: 160 KB less the sync buffers (kPipeSyncDoubles doubles) and count + 1 vector areas, in wavefront-slots
    sync_doubles = 2 * 16 + 2 * 256 + 8
    slot = (9 * 256 + 128) if c16 else 10 * 256
    return max(0, (160 * 1024 - 8 * sync_doubles - (count + 1) * 24 * 64 * 4) // slot)


def census(g):
    """census_of what the live handle planned (fb_fem_device_plan_get, persist_info(), the kernel's name)"""
    on, waves, nb, _ = g.persist_info()
    assert on
    return census_of(g.pcg_path()["kernel"], waves, nb, device_plan(g, "slice_off"), device_plan(g, "pipe_tasks"), device_plan(g, "pipe_windows"),
                     device_plan(g, "pipe_wg_first"))


def census_of(kernel, waves, nb, so, tasks=None, windows=None, wg_first=None):
    """Per slice of a persistent plan what its product runs: dict of int arrays over the slices --
      wg, wave     the workgroup and wavefront that own it (pipe2: the lane's row set in `half`)
      front        slots streamed in front of the LDS window (0 without one)
      mirror, plain  the on-chip run: mirror layers, then plain resident slots (`dealt` of them, clipped by the slice's width)
      back         slots its owner streams behind the resident part (the whole stream where there is no window)
      helpers      list per slice of the lengths of the helper halves cut off its stream (task table)
    and `groups`: slices per workgroup, `no_mirror_wgs`: workgroups (with slices) none of whose slices has a mirror layer.
    kernel: the name fb_fem_pcg_path gives; waves: most slices of a workgroup; nb: workgroups; so: slice_off; the three pipe_* arrays."""
    wd = np.diff(so)
    ns = len(wd)
    c16 = ",c16" in kernel or "<c16" in kernel
    groups = deal(wg_first, ns, nb)
    out = {k: np.zeros(ns, np.int64) for k in ("wg", "wave", "half", "front", "mirror", "plain", "dealt", "back")}
    helpers = [[] for _ in range(ns)]
    pipe2 = kernel.startswith("k_pcg_pipe2")
    if not pipe2:
        wmax, klt = (int(x) for x in kernel[:-1].split(",")[2:4])
    lds = 65 if c16 else 62
    for b, (first, count) in enumerate(groups):
        if count <= 0:
            continue
        if pipe2:
            share = equal_share(count, _pipe2_lds_slots(count, c16), KPIPE2_KLT)
            n_waves = -(-waves // 2)
            n_waves += 1 if n_waves < 12 else 0        # (the service wavefront is launched where there is room, and owns row sets like the others)
        elif tasks is None:
            share = equal_share(count, lds, klt)
        for w in range(count):
            sl = first + w
            out["wg"][sl] = b
            out["wave"][sl] = w % n_waves if pipe2 else w
            out["half"][sl] = w // n_waves if pipe2 else 0
            a = m = 0
            own_end = wd[sl]
            if tasks is not None:
                tk = tasks.reshape(nb, TASK_STRIDE, 4)[b, w]
                p, own_end = int(tk[0]), int(tk[2])
            elif windows is not None:
                a, m, p = (int(x) for x in windows.reshape(ns, 3)[sl])
            else:
                p = share[w]
            kl = max(0, min(p, wd[sl] - a - m))
            out["front"][sl], out["mirror"][sl], out["plain"][sl], out["dealt"][sl] = a, m, kl, p
            out["back"][sl] = max(0, own_end - (a + m + p))
        if tasks is not None:
            for hw in range(count, TASK_STRIDE):
                tk = tasks.reshape(nb, TASK_STRIDE, 4)[b, hw]
                if tk[0] >= 0 and tk[2] > tk[1]:
                    helpers[first + int(tk[0])].append(int(tk[2] - tk[1]))
    out["helpers"] = helpers
    out["width"] = wd
    out["groups"] = [c for _, c in groups]
    out["no_mirror_wgs"] = [b for b, (f, c) in enumerate(groups) if c > 0 and windows is not None and not out["mirror"][f:f + c].any()]
    out["kernel"] = kernel
    return out


def count_classes(counts):
    """which of the slot-count classes {0, 1, 2, 3, even >= 4, odd >= 5} occur among `counts`"""
    c = np.asarray(list(counts), np.int64)
    return {"0": bool((c == 0).any()), "1": bool((c == 1).any()), "2": bool((c == 2).any()), "3": bool((c == 3).any()),
            "even": bool(((c >= 4) & (c % 2 == 0)).any()), "odd": bool(((c >= 5) & (c % 2 == 1)).any())}


# ---- host model of the LDS window's planner --------------------------------------------------------------------------------------------
def window_model(so, colidx, n_owned, nb, klt, c16, wg_first=None):
    """k_pipe_mirror_plan restated (fembrain_amd/csrc/pcg_pipe_mirror.h; plan_api.cpp fb_plan_mirror_model runs the C functions and reports
    totals: tests/test_product_inputs.py holds this against them).  Returns (windows [n_slices][a, m, p], pool entries, workgroups with
    mirrors): what "pipe_windows" of a live (12, klt) handle holds, computed from the host plan."""
    ns = len(so) - 1
    slotb, lds, tabb = (9 * 256 + 128, 65, 256) if c16 else (10 * 256, 62, 384)
    ci = np.asarray(colidx).reshape(-1, 64)
    res, pool_all, with_mirrors = np.zeros((ns, 3), np.int64), 0, 0
    lanes = np.arange(64)
    for first, count in deal(wg_first, ns, nb):
        count = min(count, 12)
        if count <= 0:
            continue
        lo, hi = first * 64, min((first + count) * 64, n_owned)
        mw = []
        for w in range(count):
            sl = first + w
            cols, rows = ci[so[sl]:so[sl + 1]], sl * 64 + lanes
            diag = np.where((cols == rows[None, :]).any(0) & (rows < n_owned), (cols == rows[None, :]).argmax(0), -1)
            hist = np.bincount(diag[(diag >= 0) & (diag < 256)], minlength=1)
            d = int(hist.argmax()) if hist.max() > 0 else -1                      # (the lowest slot among equals)
            m = 0
            while d >= 0 and m < 4 and d - 1 - m >= 0:
                c = cols[d - 1 - m]
                if int(((rows < hi) & (c >= lo) & (c < rows)).sum()) < 56:
                    break
                m += 1
            mw.append(dict(d=d, m=m, width=len(cols), a=0, p=0))

        def layout(pool, grow):
            total, share, used = lds * slotb, min(lds // count, klt, 6), 0
            for q in mw:
                q["a"] = q["d"] - q["m"] if q["m"] > 0 else 0
                q["p"] = share
                used += share * slotb + q["m"] * tabb
            pb = (pool + 63) // 64 * 9 * 256
            for q in reversed(mw):
                while q["m"] > 0 and used + pb > total:
                    q["m"] -= 1
                    q["a"] += 1
                    used -= tabb
            if used + pb > total:
                return False
            extra, grew = ((total - used - pb) // slotb if grow else 0), True
            while extra > 0 and grew:
                grew = False
                for q in mw:
                    if extra > 0 and q["p"] < klt:
                        q["p"] += 1
                        extra -= 1
                        grew = True
            return True

        def misses():
            e = 0
            for w, q in enumerate(mw):
                rows = (first + w) * 64 + lanes
                for k in range(q["m"]):
                    c = ci[so[first + w] + q["a"] + k]
                    for l in range(64):
                        row, cc = rows[l], c[l]
                        if not (row < hi and lo <= cc < row):
                            e += 1
                            continue
                        q2 = mw[(cc >> 6) - first]
                        k0 = q2["a"] + q2["m"]
                        s0 = so[cc >> 6] + k0
                        e += 0 if (ci[s0:s0 + max(0, min(q2["p"], q2["width"] - k0)), cc & 63] == row).any() else 1
            return e

        ok = layout(0, False)
        pool = misses() if ok else 0
        ok = ok and pool <= 1024 and layout(pool, True)
        if ok:
            pool = misses()
            plain = equal_share(count, lds, klt)
            before = sum(min(plain[w], q["width"]) for w, q in enumerate(mw))
            ok = sum(q["m"] + max(0, min(q["p"], q["width"] - q["a"] - q["m"])) for q in mw) > before
        if not ok:
            pool = 0
            for q, p in zip(mw, equal_share(count, lds, klt)):
                q.update(a=0, m=0, p=p)
        pool_all += pool
        with_mirrors += 1 if ok else 0
        for w, q in enumerate(mw):
            res[first + w] = (q["a"], q["m"], q["p"])
    return res, pool_all, with_mirrors
