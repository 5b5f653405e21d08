"""The stress surface of the C++ classes: PS::FEM::Deformable::computeStress / readStress / surfaceStress, HipIntegrator::ReadStress and
the SurfaceMesh adaptor's vertex stress through the C ABI on the GPU (tests/cpp/stress_host.cpp), against tests/stressref.py."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEG = os.path.join(ROOT, "tests", "golden", "cube3_materials.veg")


def _exe():
    exe = os.path.join(ROOT, "tests", "cpp", "stress_host")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "stress_host.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "fembrain_amd"), "-lfembrain_hip", "-Wl,-rpath," + os.path.join(ROOT, "fembrain_amd")])
    return exe


def test_stress_host_program_compiles_with_gxx():
    assert os.path.exists(_exe())


@pytest.mark.gpu
def test_deformable_stress_of_a_veg_file_with_materials(gpu):
    import stressref as sr
    from fembrain_amd import lib as fl
    from fembrain_amd.meshgen import read_veg_materials
    from oracle.pyoracle import OrcFem
    out = subprocess.check_output([_exe(), VEG], text=True)
    kv = dict(line.split("=", 1) for line in out.strip().splitlines())
    arr = lambda k, dt=float: np.array(kv[k].split(","), dt) if kv[k] else np.zeros(0, dt)  # noqa: E731
    v, t, mats, ids = read_veg_materials(VEG)
    assert kv["STALE_REFUSED"] == "1" and kv["TENSORS_REFUSED"] == "1" and kv["ADAPTOR_SAME"] == "1" and kv["WORLD_SAME_SUMMARY"] == "1"
    assert int(kv["N_ELEMENTS"]) == len(t) and int(kv["FLAGS"]) == 0 and int(kv["WORLD_FLAGS"]) == (fl.FB_STRESS_WORLD | fl.FB_STRESS_TENSORS)
    q, vm, J, s6 = arr("Q"), arr("VM"), arr("J"), arr("STRESS6").reshape(-1, 6)
    assert np.abs(q).max() > 1e-4
    lam, mu = (np.array([sr.lame(m[0], m[1])[k] for m in mats])[ids] for k in (0, 1))
    ref = sr.stress(OrcFem(v, t), q, lam, mu, world=True)
    scale = 3 * lam + 2 * mu
    assert (np.abs(vm - ref["von_mises"]) <= 3 * scale * 1e-10).all() and (np.abs(s6 - ref["stress"]).max(axis=1) <= 3 * scale * 1e-10).all()
    assert (np.abs(J - ref["J"]) <= 1e-12 * np.abs(ref["J"])).all()
    assert float(kv["MAX_VM"]) == vm.max() and int(kv["MAX_ELEMENT"]) == int(np.argmax(vm))
    assert float(kv["MIN_J"]) == J.min() and int(kv["MIN_J_ELEMENT"]) == int(np.argmin(J)) and int(kv["N_INVERTED"]) == int((J < 0).sum())
    faces, vids, ft = arr("FACES", float).astype(int).reshape(-1, 3), arr("VERTEX_IDS", float).astype(int), arr("FACE_TETS", float).astype(int)
    want = sr.surface_mean(vm, faces, vids, ft)
    got = arr("SURFACE")
    assert len(got) == len(vids) > 0 and (np.abs(got - want) <= 2.0 ** -23 * np.abs(want)).all()
