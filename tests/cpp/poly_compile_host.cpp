// Host-only: the polygonizer's tree compiler (fembrain_amd/csrc/poly_compile.cpp) on every model given, without the HIP runtime, so that
// it can run under the host sanitizers.  Reads each .blob with include/fembrain/BlobReader.h, makes fb_poly_create's matrix-node check,
// compiles the model under the three field semantics (a refusal with its message is a valid outcome), computes the support boxes, and
// builds the cube table.  Prints steps and slots per model and semantics.  Not a pytest test: build and run by hand,
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I include tests/cpp/poly_compile_host.cpp \
//       fembrain_amd/csrc/poly_compile.cpp fembrain_amd/csrc/fem_plan.cpp -pthread -o tests/cpp/poly_compile_host
//   tests/cpp/poly_compile_host tests/golden/blob/*.blob
#include <cstdio>
#include <string>

#include "../../fembrain_amd/csrc/poly_program.h"
#include "fembrain/BlobReader.h"

namespace fb {
std::string& last_error();  // fem_plan.cpp
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  static const char* const kSemName[3] = {"cpu", "cpu_box", "opencl"};
  for (int f = 1; f < argc; f++) {
    PS::SKETCH::LinearBlobTreeData d;
    std::string err;
    if (!PS::SKETCH::readBlobFile(argv[f], d, &err)) { std::printf("%s: ERROR %s\n", argv[f], err.c_str()); return 1; }
    const int n_ops = (int)(d.ops.size() / 16), n_prims = (int)(d.prims.size() / 20), n_mtx = (int)(d.mtx.size() / 12);
    std::printf("%s: %d operators, %d primitives, %d matrix nodes\n", argv[f], n_ops, n_prims, n_mtx);
    bool mtx_ok = n_prims >= 1 && n_mtx >= 1;
    for (int i = 0; i < n_prims && mtx_ok; i++) {  // (fb_poly_create refuses such a model before it compiles)
      const int im = (int)d.prims[20 * (size_t)i + 1];
      mtx_ok = im >= 0 && im < n_mtx;
    }
    if (!mtx_ok) { std::printf("  refused: a primitive references a matrix node that is not there\n"); continue; }
    for (int sem = 0; sem < 3; sem++) {
      const fb::TreeSource src = {d.ops.data(), d.prims.data(), d.mtx.data(), n_ops, n_prims, n_mtx, sem};
      fb::TreeProgram tp;
      if (fb::compile_tree(src, &tp) != FB_OK) {
        std::printf("  %-8s refused: %s\n", kSemName[sem], fb::last_error().c_str());
        continue;
      }
      fb::support_boxes(src, &tp);
      int bounded = 0;
      for (int i = 0; i < n_prims; i++) bounded += tp.pbox[6 * (size_t)i] > -1e30f && tp.pbox[6 * (size_t)i] <= tp.pbox[6 * (size_t)i + 3];
      std::printf("  %-8s %zu steps, %d slots, %d of %d support boxes bounded\n", kSemName[sem], tp.prog.size(), tp.depth, bounded, n_prims);
    }
  }
  const fb::CubeTable& ct = fb::cube_table();
  int indices = 0;
  for (int c = 0; c < 256; c++) indices += ct.nvert[c];
  std::printf("cube table: %d triangle indices over 256 configurations\n", indices);
  return 0;
}
