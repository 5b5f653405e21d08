"""PS::FEM::EmbeddedMesh (include/fembrain/EmbeddedMesh.h) over a Deformable, from a C++ host program (tests/cpp/embed_host.cpp): the header
compiles with a plain C++11 compiler (no GPU), and on the GPU its binding, vertexAt and normalAt after steps and after Deformable::cut are
the restatement's (tests/embedref.py) on the mesh and state the program reports."""
import os
import subprocess

import numpy as np
import pytest

import embedref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "embed_host")


def _build():
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "embed_host.cpp"),
           "-o", EXE, "-L", os.path.join(ROOT, "fembrain_amd"), "-lfembrain_hip", "-Wl,-rpath," + os.path.join(ROOT, "fembrain_amd")]
    subprocess.check_call(cmd)


def test_embed_host_compiles_with_any_header_first(tmp_path):
    _build()
    heads = ("Deformable.h", "SurfaceMesh.h", "EmbeddedMesh.h")
    for k in range(3):
        src = tmp_path / "order.cpp"
        src.write_text("".join('#include "fembrain/%s"\n' % heads[(k + j) % 3] for j in range(3)) +
                       "int main() { return sizeof(PS::FEM::EmbeddedMesh) && sizeof(PS::FEM::SurfaceMesh) && sizeof(PS::FEM::Deformable) ? 0 : 1; }\n")
        subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


@pytest.mark.gpu
def test_embedded_mesh_over_a_deformable(gpu):
    _build()
    out = subprocess.check_output([EXE], text=True, timeout=300)
    kv = dict(line.split(" =", 1) for line in out.strip().splitlines() if " =" in line)
    assert kv.get("embed_host", "").strip() == "ok", out[-2000:]
    mu, mv = 12, 7
    idx = np.arange(mu * mv).reshape(mu, mv)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    tri = np.stack([np.stack([a, b, c], 1), np.stack([b, d, c], 1)], axis=1).reshape(-1, 3)
    for tag in ("steps", "cut"):
        def arr(key, dtype, width):
            return np.array(kv["%s_%s" % (tag, key)].split(), dtype=dtype).reshape(-1, width)
        rest, q, tets = arr("rest", np.float64, 3), arr("q", np.float64, 3), arr("tets", np.int64, 4)
        el, vt, w, loc = arr("elements", np.int64, 1).reshape(-1), arr("vertices", np.int64, 4), arr("weights", np.float64, 4), arr("loc", np.float64, 3)
        assert np.abs(q).max() > 0
        # the binding names elements of the mesh the device holds, holds the point and reproduces its place in the rest shape
        assert np.array_equal(vt, tets[el]) and (w >= 0).all()
        # (each weight is off by at most the bound of its element; four of them times a coordinate, and the roundings of the sum)
        back = np.abs(er.positions(rest, np.zeros(rest.size), vt, w) - loc).max(axis=1)
        assert (back <= (4 * er.weight_bound(rest, tets, loc, el) + 8 * er.U) * np.abs(rest).max()).all()
        if tag == "steps":
            ref = er.bind(rest, tets, loc)
            assert er.margin(rest, tets, loc).min() >= 1e-9
            assert np.array_equal(el, ref["elements"]) and (np.abs(w - ref["weights"]).max(axis=1) <= ref["bound"]).all()
        want = er.positions(rest, q, vt, w)
        w32 = np.float32(want)
        xyz = arr("xyz", np.float32, 3)
        assert (np.abs(xyz.astype(np.float64) - w32.astype(np.float64)) <= np.spacing(np.abs(w32))).all()
        assert np.array_equal(arr("box", np.float32, 3), np.array([xyz.min(axis=0), xyz.max(axis=0)]))
        assert np.abs(arr("normals", np.float32, 3).astype(np.float64) - er.normals(want, tri)).max() <= 2e-7  # (the bound of tests/test_fem_surface_gpu.py)
        counts = [int(x) for x in kv["%s_counts" % tag].split()]
        assert counts[:3] == [mu * mv, len(tri), 0] and (counts[3] > 0) == (tag == "cut")
