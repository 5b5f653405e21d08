// Host program over the per-element material surface of the C++ classes (tests/test_materials_cpp.py):
//   materials_host veg FILE    PS::FEM::readVegFile with materials: the table and the element ids it read (no device needed)
//   materials_host run FILE    the file's mesh in a PS::FEM::Deformable with its materials (Deformable::setMaterials /
//                              setElementMaterials), plane x = min clamped, two steps under the reference load; then the ids and
//                              the table read back through the C ABI, and a refused id
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "fembrain/BlobReader.h"
#include "fembrain/Deformable.h"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: materials_host veg|run FILE\n"); return 2; }
  std::vector<double> xyz;
  std::vector<int> tets;
  std::vector<PS::FEM::VegMaterial> mats;
  std::vector<unsigned char> ids;
  std::string err;
  if (!PS::FEM::readVegFile(argv[2], xyz, tets, mats, ids, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
  std::printf("NODES=%zu\nTETS=%zu\nMATERIALS=%zu\n", xyz.size() / 3, tets.size() / 4, mats.size());
  for (size_t m = 0; m < mats.size(); m++) std::printf("MATERIAL%zu=%s %.17g %.17g %.17g\n", m, mats[m].name.c_str(), mats[m].E, mats[m].nu, mats[m].rho);
  std::printf("IDS=");
  for (size_t e = 0; e < ids.size(); e++) std::printf("%s%d", e ? "," : "", (int)ids[e]);
  std::printf("\n");
  if (std::strcmp(argv[1], "run") != 0) return 0;

  const int nv = (int)(xyz.size() / 3), ne = (int)(tets.size() / 4);
  double xmin = xyz[0];
  for (int i = 0; i < nv; i++) xmin = std::min(xmin, xyz[3 * (size_t)i]);
  std::vector<int> fixed;
  for (int i = 0; i < nv; i++) if (xyz[3 * (size_t)i] < xmin + 1e-9) fixed.push_back(i);
  PS::FEM::Deformable d(nv, xyz.data(), ne, tets.data(), fixed);
  std::vector<double> E, nu, rho;
  for (size_t m = 0; m < mats.size(); m++) { E.push_back(mats[m].E); nu.push_back(mats[m].nu); rho.push_back(mats[m].rho); }
  d.setMaterials(E, nu, rho);
  d.setElementMaterials(ids);
  d.timestep();
  d.timestep();
  std::vector<double> q(3 * (size_t)nv);
  d.integrator()->GetqState(q.data());
  std::printf("Q=");
  for (size_t k = 0; k < q.size(); k++) std::printf("%s%.17g", k ? "," : "", q[k]);
  std::printf("\nITERS=%d\n", d.integrator()->GetLastIterations());
  const std::vector<unsigned char> back = d.getElementMaterials();
  std::printf("IDS_BACK_SAME=%d\n", back == ids ? 1 : 0);
  std::vector<double> e2(mats.size()), n2(mats.size()), r2(mats.size());
  d.integrator()->GetMaterials(e2.data(), n2.data(), r2.data());
  std::printf("TABLE_BACK_SAME=%d\nNUM_MATERIALS=%d\nMAP_BYTES=%lld\n", (e2 == E && n2 == nu && r2 == rho) ? 1 : 0, d.integrator()->GetNumMaterials(),
              fb_fem_element_map_bytes(d.integrator()->handle()));
  int refused = 0;
  try {
    d.setElementMaterials(std::vector<unsigned char>(1, (unsigned char)mats.size()));
  } catch (const std::exception&) { refused = 1; }
  std::printf("BAD_ID_REFUSED=%d\nTOTAL_MASS=%.17g\n", refused, d.integrator()->GetTotalMass());
  return 0;
}
