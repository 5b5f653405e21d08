"""Generates tests/golden/embed_ref.npz: what the reference's own VolumetricMesh::generateInterpolationWeights returns
(src/3rdparty/vegafem/volumetricMesh/volumetricMesh.cpp:1059-1134 with TetMesh::computeBarycentricWeights, tetMesh.cpp:242-305) for
two meshes and seeded points.

The driver below is ours: it reads a mesh and points from raw files, builds a TetMesh from the arrays, calls the reference's function
and writes elements (closestElementList), vertices, weights and the external count back.  It is compiled against the reference's VegaFEM
units where they lie, into a temporary directory; nothing built is kept.  Run once where the reference tree exists; the .npz is
committed and the tests need neither the tree nor a compiler.

  python tests/golden/make_embed_golden.py REFERENCE_ROOT            writes embed_ref.npz
  python tests/golden/make_embed_golden.py REFERENCE_ROOT --time N   writes nothing: seconds per point of the reference's linear scan,
                                                                     N points in the 56^3 cantilever (REFERENCE_ROOT may also come from
                                                                     the environment variable FEMBRAIN_REFERENCE)
"""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "tetMesh.h"
static void rd(const char* dir, const char* name, void* p, size_t bytes) {
  char path[4096]; snprintf(path, sizeof path, "%s/%s", dir, name);
  FILE* f = fopen(path, "rb"); if (!f || fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "read %s\n", path); exit(2); } fclose(f);
}
static void wr(const char* dir, const char* name, const void* p, size_t bytes) {
  char path[4096]; snprintf(path, sizeof path, "%s/%s", dir, name);
  FILE* f = fopen(path, "wb"); if (!f || fwrite(p, 1, bytes, f) != bytes) { fprintf(stderr, "write %s\n", path); exit(2); } fclose(f);
}
int main(int argc, char** argv) {
  const char* dir = argv[1];
  int n[3]; rd(dir, "sizes", n, sizeof n);  // nodes, tets, points
  std::vector<double> v(3 * (size_t)n[0]), p(3 * (size_t)n[2]);
  std::vector<int> t(4 * (size_t)n[1]);
  rd(dir, "verts", v.data(), v.size() * 8); rd(dir, "tets", t.data(), t.size() * 4); rd(dir, "points", p.data(), p.size() * 8);
  TetMesh mesh(n[0], v.data(), n[1], t.data());
  int* vertices = NULL; double* weights = NULL; std::vector<int> elements;
  int ext = mesh.generateInterpolationWeights(n[2], p.data(), &vertices, &weights, -1.0, &elements, 0);
  wr(dir, "elements", elements.data(), elements.size() * 4); wr(dir, "vertices", vertices, 16 * (size_t)n[2]);
  wr(dir, "weights", weights, 32 * (size_t)n[2]); wr(dir, "external", &ext, 4);
  return 0;
}
"""

UNITS = ("volumetricMesh/tetMesh.cpp", "volumetricMesh/volumetricMesh.cpp", "volumetricMesh/volumetricMeshParser.cpp",
         "volumetricMesh/volumetricMeshENuMaterial.cpp", "volumetricMesh/volumetricMeshMooneyRivlinMaterial.cpp",
         "minivector/vec3d.cpp", "minivector/mat3d.cpp", "minivector/eig3.cpp")


def build_driver(ref, tmp):
    vega = os.path.join(ref, "src", "3rdparty", "vegafem")
    src = os.path.join(tmp, "embed_driver.cpp")
    open(src, "w").write(DRIVER)
    exe = os.path.join(tmp, "embed_driver")
    inc = ["-I" + os.path.join(vega, d) for d in ("volumetricMesh", "minivector", "include")]
    subprocess.check_call(["g++", "-O2", "-std=gnu++98", "-fpermissive", "-w", "-ffp-contract=off", "-o", exe, src] + [os.path.join(vega, u) for u in UNITS] + inc)
    return exe


def run_reference(exe, tmp, verts, tets, points):
    verts, tets, points = np.ascontiguousarray(verts, np.float64), np.ascontiguousarray(tets, np.int32), np.ascontiguousarray(points, np.float64)
    np.array([len(verts), len(tets), len(points)], np.int32).tofile(os.path.join(tmp, "sizes"))
    verts.tofile(os.path.join(tmp, "verts")); tets.tofile(os.path.join(tmp, "tets")); points.tofile(os.path.join(tmp, "points"))
    t0 = time.perf_counter()
    subprocess.check_call([exe, tmp], stdout=subprocess.DEVNULL)
    seconds = time.perf_counter() - t0
    n = len(points)
    return dict(elements=np.fromfile(os.path.join(tmp, "elements"), np.int32), vertices=np.fromfile(os.path.join(tmp, "vertices"), np.int32).reshape(n, 4),
                weights=np.fromfile(os.path.join(tmp, "weights"), np.float64).reshape(n, 4),
                n_external=int(np.fromfile(os.path.join(tmp, "external"), np.int32)[0]), seconds=seconds)


N_GENERIC, SEEDS = 3000, {"cube": 11, "beam3": 12}


def meshes():
    import embedref
    cv, ct = embedref.jittered_cube()
    b = np.load(os.path.join(HERE, "fem_beam3.npz"))
    return {"cube": (cv, ct), "beam3": (np.array(b["verts"], np.float64), np.array(b["tets"], np.int32))}


def main():
    import embedref
    argv = sys.argv[1:]
    n_timed = int(argv[argv.index("--time") + 1]) if "--time" in argv else 0
    args = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--time")]
    ref = args[0] if args else os.environ.get("FEMBRAIN_REFERENCE")
    if not ref or not os.path.isdir(os.path.join(ref, "src", "3rdparty", "vegafem")):
        sys.exit("give the root of the reference tree (the directory that holds src/3rdparty/vegafem), or set FEMBRAIN_REFERENCE")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(ref, tmp)
        if n_timed:
            # the linear scan on one core, per point, for a mesh and a point count of the caller's choosing: tools/probe_embed.py extrapolates
            k = n_timed
            from fembrain_amd.meshgen import truth_cube
            v, t = truth_cube(56, 56, 56, 0.1)
            v, t = np.array(v, np.float64).reshape(-1, 3), np.array(t, np.int32).reshape(-1, 4)
            r = run_reference(exe, tmp, v, t, embedref.generic_points(v, k, 5, grow=0.0))
            print("linear scan, %d tets: %.4g s per point (%d points, process start and mesh set-up included)" % (len(t), r["seconds"] / k, k))
            return
        for name, (v, t) in meshes().items():
            gen, deg = embedref.generic_points(v, N_GENERIC, SEEDS[name]), embedref.degenerate_points(v, t)
            assert np.array_equal(np.float32(gen).astype(np.float64), gen)
            pts = np.vstack([gen, deg])  # (the order of every recorded array)
            r = run_reference(exe, tmp, v, t, pts)
            m = embedref.margin(v, t, pts[:N_GENERIC])
            print("%-6s %d nodes %d tets: %d points, %d external, smallest margin of the generic points %.3g, %.3g s" %
                  (name, len(v), len(t), len(pts), r["n_external"], m.min(), r["seconds"]))
            assert m.min() >= 1e-9, "choose another seed for %s" % name
            out.update({name + "_verts": v, name + "_tets": t, name + "_generic": np.float32(gen), name + "_degenerate": deg,
                        name + "_elements": r["elements"], name + "_vertices": r["vertices"], name + "_weights": r["weights"],
                        name + "_n_external": np.int32(r["n_external"])})
    np.savez_compressed(os.path.join(HERE, "embed_ref.npz"), **out)
    print("wrote embed_ref.npz, %d bytes" % os.path.getsize(os.path.join(HERE, "embed_ref.npz")))


if __name__ == "__main__":
    main()
