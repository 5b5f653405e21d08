"""Deformable::detachPart / convertDisjointPartsToMeshes of include/fembrain/Deformable.h, compiled against the library and run
(tests/cpp/detach_deformable.cpp), as test_parts_gpu.py drives parts_deformable.cpp."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_deformable_detaches_and_converts_parts(gpu, tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "detach_deformable.cpp")
    exe = str(tmp_path / "detach_deformable")
    lib_dir = os.path.join(ROOT, "fembrain_amd")
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src,
           "-L", lib_dir, "-lfembrain_hip", "-Wl,-rpath," + lib_dir, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "detach_deformable ok" in r.stdout
