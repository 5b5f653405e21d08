"""The way back from PS::FEM::EmbeddedMesh (include/fembrain/EmbeddedMesh.h: addForces, pickRay, pickPoint, touch, applyStress) from a C++
host program (tests/cpp/embed_forces_host.cpp): the headers compile with a plain C++11 compiler (no GPU) whichever comes first, and on the
GPU the values the program reports are the ones numpy makes of the mesh, state and binding it reports with them."""
import os
import subprocess

import numpy as np
import pytest

import embedref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "embed_forces_host")


def _build():
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "embed_forces_host.cpp"),
           "-o", EXE, "-L", os.path.join(ROOT, "fembrain_amd"), "-lfembrain_hip", "-Wl,-rpath," + os.path.join(ROOT, "fembrain_amd")]
    subprocess.check_call(cmd)


def test_embed_forces_host_compiles_with_any_header_first(tmp_path):
    _build()
    heads = ("Deformable.h", "SurfaceMesh.h", "EmbeddedMesh.h")
    body = ("int main() {\n  PS::FEM::EmbeddedMesh* m = 0;\n  PS::FEM::Deformable* d = 0;\n  PS::FEM::vec3d p;\n  std::vector<double> f;\n"
            "  if (m) { m->addForces(std::vector<PS::FEM::vec3d>()); m->applyStress(); d->externalForces(f);\n"
            "    return m->pickRay(p, p).triangle + m->pickPoint(p, p) + d->touchEmbedded(m, p, p, p) + (int)m->stressAt(0); }\n"
            "  return sizeof(PS::FEM::EmbeddedMesh::RayHit) && sizeof(PS::FEM::SurfaceMesh) ? 0 : 1;\n}\n")
    for k in range(3):
        src = tmp_path / "order.cpp"
        src.write_text("".join('#include "fembrain/%s"\n' % heads[(k + j) % 3] for j in range(3)) + body)
        subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def host_add(base, vertices, weights, forces, ids):
    f = np.array(base, np.float64).reshape(-1, 3).copy()
    prod = weights[ids][:, :, None] * forces[:, None, :]
    np.add.at(f, vertices[ids].ravel(), prod.reshape(-1, 3))  # in index order: point ascending, corner ascending
    return f.reshape(-1)


def nearest_hit(P, tri, o, d, t_max=np.inf):
    a, b, c = P[tri[:, 0]], P[tri[:, 1]], P[tri[:, 2]]
    e1, e2 = b - a, c - a
    pv = np.cross(d[None, :], e2)
    det = (e1 * pv).sum(axis=1)
    tv = o[None, :] - a
    u = (tv * pv).sum(axis=1) / det
    qv = np.cross(tv, e1)
    v = (qv * d[None, :]).sum(axis=1) / det
    t = (e2 * qv).sum(axis=1) / det
    ids = np.nonzero((u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t <= t_max))[0]
    if not len(ids):
        return -1, 0.0, 0.0, 0.0
    order = ids[np.argsort(t[ids], kind="stable")]
    k = order[0]
    assert len(order) == 1 or t[order[1]] - t[k] > 1e-6, "the fixture's ray is not generic"
    assert min(u[k], v[k], 1 - u[k] - v[k]) > 1e-6, "the fixture's ray is not generic"
    return int(k), t[k], u[k], v[k]


@pytest.mark.gpu
def test_embedded_mesh_forces_picks_and_stress(gpu):
    _build()
    out = subprocess.check_output([EXE], text=True, timeout=300)
    kv = dict(line.split(" =", 1) for line in out.strip().splitlines() if " =" in line)
    assert kv.get("embed_forces_host", "").strip() == "ok", out[-2000:]

    def arr(key, dtype, width=1):
        return np.array(kv[key].split(), dtype=dtype).reshape(-1, width)

    rest, q = arr("rest", np.float64, 3), arr("q", np.float64, 3)
    el, vt, w, tri = arr("elements", np.int64).reshape(-1), arr("vertices", np.int64, 4), arr("weights", np.float64, 4), arr("triangles", np.int64, 3)
    n = len(el)
    assert n == 84 and np.abs(q).max() > 0 and np.array_equal(vt, arr("tets", np.int64, 4)[el])
    # addForces: a list, then every point on top of it
    base = arr("f_base", np.float64).reshape(-1)
    assert np.array_equal(base.reshape(-1, 3), np.tile([0.0, -300.0, 0.0], (len(rest), 1)))
    ids, fl = arr("list_ids", np.int64).reshape(-1), arr("list_forces", np.float64, 3)
    want = host_add(base, vt, w, fl, ids)
    assert arr("f_list", np.float64).reshape(-1).tobytes() == want.tobytes() != base.tobytes()
    want = host_add(want, vt, w, arr("all_forces", np.float64, 3), np.arange(n))
    assert arr("f_all", np.float64).reshape(-1).tobytes() == want.tobytes()
    # pickRay / pickPoint on the positions the binding gives at the reported state
    P = er.positions(rest, q, vt, w)
    for key, t_max in (("ray1", np.inf), ("ray2", np.inf), ("ray_miss", np.inf), ("ray_short", 0.25)):
        r = arr(key, np.float64).reshape(-1)
        o, d, got_tri, got = r[0:3], r[3:6], int(r[6]), r[7:]
        k, t, u, v = nearest_hit(P, tri, o, d, t_max)
        assert got_tri == k and (k >= 0) == (key in ("ray1", "ray2")), key
        if k >= 0:
            assert abs(got[0] - t) <= 1e-9 * (1 + abs(t)) and abs(got[1] - u) <= 1e-9 and abs(got[2] - v) <= 1e-9 and np.abs(got[3:6] - (o + t * d)).max() <= 1e-9
    r = arr("point", np.float64).reshape(-1)
    dd = P - r[0:3]
    d2 = dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1] + dd[:, 2] * dd[:, 2]
    assert int(r[3]) == int(np.argmin(d2)) and np.sort(d2)[1] - np.sort(d2)[0] > 1e-9 and np.abs(r[4:7] - P[int(r[3])]).max() <= 1e-12
    # touch: a miss adds nothing; a hit adds (1-u-v, u, v) * force on the triangle's points, ascending
    assert arr("f_untouched", np.float64).reshape(-1).tobytes() == base.tobytes()
    tch = arr("touch", np.float64).reshape(-1)
    r1 = arr("ray1", np.float64).reshape(-1)
    assert int(tch[0]) == int(r1[6])
    u, v = r1[8], r1[9]
    pid = tri[int(tch[0])]
    order = np.argsort(pid)
    f3 = (np.array([1.0 - u - v, u, v])[:, None] * tch[1:4][None, :])[order]
    assert arr("f_touch", np.float64).reshape(-1).tobytes() == host_add(base, vt, w, f3, pid[order]).tobytes()
    # applyStress
    vm = arr("von_mises", np.float64).reshape(-1)
    assert arr("stress", np.float32).reshape(-1).tobytes() == vm[el].astype(np.float32).tobytes() and vm.max() > 0
