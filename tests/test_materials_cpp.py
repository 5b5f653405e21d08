"""The per-element material surface of the C++ classes: PS::FEM::Deformable::setMaterials / setElementMaterials and the .veg reader with
materials through the C ABI on the GPU (tests/cpp/materials_host.cpp), and the VegaAdaptors constructor that takes every element's
material from the reference's own mesh object, syntax-checked against the reference's headers where that tree exists."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEGA = "/root/reference/src/3rdparty/vegafem"
VEG = os.path.join(ROOT, "tests", "golden", "cube3_materials.veg")


def _exe():
    exe = os.path.join(ROOT, "tests", "cpp", "materials_host")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "materials_host.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "fembrain_amd"), "-lfembrain_hip", "-Wl,-rpath," + os.path.join(ROOT, "fembrain_amd")])
    return exe


def test_materials_host_program_compiles_with_gxx():
    assert os.path.exists(_exe())


def test_vega_adaptor_per_element_constructor_against_the_reference_headers(tmp_path):
    """HipCorotationalForceModel(const Mesh*, int warp, int device) with the reference's TetMesh: syntax only, no reference binary."""
    if not os.path.isdir(VEGA):
        pytest.skip("the reference tree is not on this machine")
    src = tmp_path / "seam_materials.cpp"
    src.write_text('#include "tetMesh.h"\n#include "volumetricMeshENuMaterial.h"\n#include "fembrain/VegaAdaptors.h"\n'
                   "int check(const TetMesh* mesh) {\n"
                   "  PS::FEM::HipCorotationalForceModel a(mesh, 1, 0);\n"
                   "  PS::FEM::HipCorotationalForceModel b(mesh);\n"
                   "  PS::FEM::HipCorotationalForceModel c(mesh, 1e7, 0.46, 1000.0);\n"
                   "  ForceModel* fm = &a;\n"
                   "  return fm != 0 && a.ok() && b.ok() && c.ok();\n}\n")
    inc = [x for d in ("integrator", "forceModel", "sparseMatrix", "volumetricMesh", "minivector", "include") for x in ("-I", os.path.join(VEGA, d))]
    subprocess.check_call(["g++", "-std=gnu++98", "-fpermissive", "-w", "-fsyntax-only"] + inc + ["-I", os.path.join(ROOT, "include"), str(src)])


@pytest.mark.gpu
def test_deformable_with_the_materials_of_a_veg_file(gpu):
    import fem_params  # noqa: F401  (tests/ on the path)
    from fembrain_amd.meshgen import fixed_vertices_to_dofs, read_veg_materials
    from matref import MatRef
    out = subprocess.check_output([_exe(), "run", VEG], text=True)
    kv = dict(line.split("=", 1) for line in out.strip().splitlines())
    v, t, mats, ids = read_veg_materials(VEG)
    assert int(kv["MATERIALS"]) == len(mats) == int(kv["NUM_MATERIALS"]) and np.array_equal(np.array(kv["IDS"].split(","), int), ids)
    assert kv["IDS_BACK_SAME"] == "1" and kv["TABLE_BACK_SAME"] == "1" and kv["BAD_ID_REFUSED"] == "1" and int(kv["MAP_BYTES"]) >= len(t)
    # two steps of Deformable::timestep (gravity -10000 per y DOF, h 0.0333, c_K 0.01, CG 1e-6) against the restatement stepping with the
    # oracle's PCG at the same tolerance; bound: the fp32-matrix bound of the uniform three-step parity test (tests/test_fem_gpu.py), 2e-4
    fixed = fixed_vertices_to_dofs(np.nonzero(v[:, 0] < v[:, 0].min() + 1e-9)[0])
    ref = MatRef(v, t, mats, ids)
    q, qv = np.zeros(ref.r), np.zeros(ref.r)
    fext = np.zeros(ref.r)
    fext[1::3] = -10000.0
    for _ in range(2):
        q, qv, _, info = ref.step(q, qv, fext, fixed, 0.0333, 0.0, 0.01, pcg_eps=1e-6)
    qg = np.array(kv["Q"].split(","), float)
    assert np.abs(qg - q).max() <= 2e-4 * np.abs(q).max()
    assert abs(int(kv["ITERS"]) - abs(info)) <= max(3, 0.02 * abs(info))
    rho = np.array([m[2] for m in mats])[ids]
    assert abs(float(kv["TOTAL_MASS"]) - 3.0 * (rho * ref.volumes()).sum()) <= 1e-6 * 3.0 * (rho * ref.volumes()).sum()
