// Host program over the stress surface of the C++ classes (tests/test_stress_cpp.py):
//   stress_host FILE    the .veg file's mesh in a PS::FEM::Deformable with its materials, plane x = min clamped, two steps under the
//                       reference load; then Deformable::computeStress / readStress / surfaceStress and SurfaceMesh::applyStress, and
//                       the refusals before the first computeStress and of a tensor read that was not kept
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "fembrain/BlobReader.h"
#include "fembrain/Deformable.h"

template <typename T>
static void print_list(const char* name, const std::vector<T>& v) {
  std::printf("%s=", name);
  for (size_t k = 0; k < v.size(); k++) std::printf("%s%.17g", k ? "," : "", (double)v[k]);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: stress_host FILE\n"); return 2; }
  std::vector<double> xyz;
  std::vector<int> tets;
  std::vector<PS::FEM::VegMaterial> mats;
  std::vector<unsigned char> ids;
  std::string err;
  if (!PS::FEM::readVegFile(argv[1], xyz, tets, mats, ids, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
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
  std::vector<float> colour;
  int refused = 0;
  try {
    d.surfaceStress(colour);
  } catch (const std::exception&) { refused = 1; }
  std::printf("STALE_REFUSED=%d\n", refused);
  const fb_fem_stress_info info = d.computeStress();
  std::printf("N_ELEMENTS=%d\nFLAGS=%d\nMAX_VM=%.17g\nMAX_ELEMENT=%d\nMIN_J=%.17g\nMIN_J_ELEMENT=%d\nN_INVERTED=%d\nENERGY=%.17g\n", info.n_elements, info.flags,
              info.max_von_mises, info.max_element, info.min_J, info.min_J_element, info.n_inverted, info.energy);
  std::vector<double> vm, s6(6 * (size_t)ne);
  d.readStress(vm);
  print_list("VM", vm);
  refused = 0;
  try {
    d.integrator()->ReadStress(0, ne, nullptr, nullptr, nullptr, s6.data());
  } catch (const std::exception&) { refused = 1; }
  std::printf("TENSORS_REFUSED=%d\n", refused);
  const fb_fem_stress_info world = d.computeStress(true, true);
  std::vector<double> e6(6 * (size_t)ne), J((size_t)ne);
  d.integrator()->ReadStress(0, ne, nullptr, nullptr, J.data(), s6.data(), e6.data());
  std::printf("WORLD_FLAGS=%d\nWORLD_SAME_SUMMARY=%d\n", world.flags, (world.max_von_mises == info.max_von_mises && world.energy == info.energy && world.min_J == info.min_J) ? 1 : 0);
  print_list("STRESS6", s6);
  print_list("J", J);
  d.surfaceStress(colour);
  print_list("SURFACE", colour);
  PS::FEM::SurfaceMesh* sm = d.surfaceMesh();
  const std::vector<float>& again = sm->applyStress();
  std::printf("ADAPTOR_SAME=%d\n", (again == colour && sm->countVertices() == colour.size() && (colour.empty() || sm->vertexStressAt(0) == colour[0])) ? 1 : 0);
  print_list("FACES", sm->faces());
  print_list("VERTEX_IDS", sm->vertexIds());
  std::vector<int> ft;
  for (PS::FEM::U32 f = 0; f < sm->countFaceElements(); f++) ft.push_back((int)sm->faceElementAt(f));
  print_list("FACE_TETS", ft);
  std::vector<double> q(3 * (size_t)nv);
  d.integrator()->GetqState(q.data());
  print_list("Q", q);
  return 0;
}
