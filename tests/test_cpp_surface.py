"""PS::FEM::SurfaceMesh (include/fembrain/SurfaceMesh.h) over a Deformable, from a C++ host program (tests/cpp/surface_host.cpp): the header
compiles with a plain C++11 compiler (no GPU), and on the GPU its counts, faceAt, vertexAt and normalAt after steps and after
Deformable::cut are the restatement's (tests/surfref.py) on the mesh and state the program reports."""
import os
import subprocess

import numpy as np
import pytest

import surfref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "surface_host")


def _build():
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "surface_host.cpp"),
           "-o", EXE, "-L", os.path.join(ROOT, "fembrain_amd"), "-lfembrain_hip", "-Wl,-rpath," + os.path.join(ROOT, "fembrain_amd")]
    subprocess.check_call(cmd)


def test_surface_host_compiles_with_either_header_first(tmp_path):
    _build()
    for first, second in (("Deformable.h", "SurfaceMesh.h"), ("SurfaceMesh.h", "Deformable.h")):
        src = tmp_path / "order.cpp"
        src.write_text('#include "fembrain/%s"\n#include "fembrain/%s"\nint main() { return sizeof(PS::FEM::SurfaceMesh) && sizeof(PS::FEM::Deformable) ? 0 : 1; }\n' % (first, second))
        subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


@pytest.mark.gpu
def test_surface_mesh_over_a_deformable(gpu):
    _build()
    out = subprocess.check_output([EXE], text=True, timeout=300)
    kv = dict(line.split(" =", 1) for line in out.strip().splitlines() if " =" in line)
    assert kv.get("surface_host", "").strip() == "ok", out[-2000:]
    counts = {}
    for tag in ("steps", "cut"):
        def arr(key, dtype, width):
            return np.array(kv["%s_%s" % (tag, key)].split(), dtype=dtype).reshape(-1, width)
        rest, q, tets = arr("rest", np.float64, 3), arr("q", np.float64, 3), arr("tets", np.int64, 4)
        faces, ft = sr.literal(rest, tets)
        ids = sr.vertex_ids(faces)
        assert np.array_equal(arr("faces", np.int64, 3), faces)
        assert np.array_equal(arr("ids", np.int64, 1).reshape(-1), ids)
        assert np.array_equal(ids[arr("compact", np.int64, 3)], faces)
        want = np.float32(rest + q)[ids]
        assert np.abs(q).max() > 0
        assert np.array_equal(arr("xyz", np.float32, 3), want)
        assert np.array_equal(arr("box", np.float32, 3), sr.aabb(want))
        ref, length = sr.normals(rest + q, faces, ids)
        assert length.min() >= 1e-3
        assert np.abs(arr("normals", np.float32, 3).astype(np.float64) - ref).max() <= 2e-7     # (the bound of tests/test_fem_surface_gpu.py)
        node, dist = kv["%s_closest" % tag].split()
        d = np.linalg.norm(want.astype(np.float64) - [10.0, 0.15, 0.15], axis=1)
        assert int(node) == ids[np.argmin(d)] and float(dist) == pytest.approx(d.min(), rel=1e-6)
        counts[tag] = (len(faces), len(ids))
    assert counts["cut"][0] > counts["steps"][0] and counts["cut"][1] > counts["steps"][1]
