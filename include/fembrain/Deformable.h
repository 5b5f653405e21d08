// C++ adaptors with the reference's class surfaces over the C ABI (fembrain_hip.h).  Header-only; link with
// -lfembrain_hip.  Scene-graph / GL members of the originals (SGMesh base, draw(), pickVertex, Bullet shapes) stay in
// the host application: these classes carry the simulation state and the per-step hot path only.
//
//   PS::FEM::HipIntegrator  <-> VolumeConservingIntegrator / ImplicitNewmarkSparse / IntegratorBaseSparse
//                               (reference src/deformable/PS_VolumeConservingIntegrator.h:15-37,
//                                vegafem/integrator/integratorBase.h:107-205, integratorBaseSparse.h:45-84)
//   PS::FEM::Deformable     <-> class Deformable (reference src/deformable/Deformable.h:63-235): same method names,
//                               argument meaning and callback type; timestep() follows Deformable.cpp:318-420.
//   PS::FEM::SurfaceMesh    <-> class SurfaceMesh (SurfaceMesh.h, included at the end of this file): what the host draws.
//   PS::FEM::EmbeddedMesh   (EmbeddedMesh.h, included at the end of this file): a finer drawn mesh bound to the tets, moved on the device.
#pragma once
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../fembrain_hip.h"

// CuttableMesh::cut return codes (src/deformable/CuttableMesh.h:24-28)
#ifndef CUT_ERR_INVALID_INPUT_ARG
#define CUT_ERR_INVALID_INPUT_ARG -1
#define CUT_ERR_NO_INTERSECTION -2
#define CUT_ERR_UNHANDLED_CUT_STATE -3
#define CUT_ERR_UNABLE_TO_CUT_EDGE -4
#define CUT_ERR_USER_CANCELLED_CUT -5
#endif

namespace PS {
namespace FEM {

typedef unsigned int U32;
// same signature as the reference's FOnApplyDeformations (Deformable.h:46): borrowed pointer, dof = 3 * nodes
typedef void (*FOnApplyDeformations)(U32 dof, double* displacements);

struct vec3d {
  double x, y, z;
  vec3d(double x_ = 0, double y_ = 0, double z_ = 0) : x(x_), y(y_), z(z_) {}
};

class HipIntegrator {
 public:
  // constrainedDOFs: 0-indexed, ascending, copied (implicitNewmarkSparse.h:78-80)
  HipIntegrator(int numVertices, const double* restPositions, int numElements, const int* elements, int numConstrainedDOFs,
                const int* constrainedDOFs, double timestep = 0.0333, double dampingMassCoef = 0.0, double dampingStiffnessCoef = 0.01,
                double E = 1e7, double nu = 0.46, double density = 1000.0, int device = 0, int warp = 1, bool expectCuts = false)
      : r_(3 * numVertices), h_(nullptr) {
    // warp: the argument of CorotationalLinearFEMForceModel (corotationalLinearFEMForceModel.h:42): 1 = corotational (default,
    // what FemBrain runs), 0 = linear elasticity; 2 (exact tangent) is not offered -- its Keff is not symmetric
    if (warp != 0 && warp != 1) throw std::invalid_argument("warp must be 0 or 1");
    fb_fem_default_params(&prm_);
    prm_.linear = warp == 0 ? 1 : 0;
    prm_.E = E; prm_.nu = nu; prm_.rho = density;
    prm_.timestep = timestep; prm_.damping_mass = dampingMassCoef; prm_.damping_stiffness = dampingStiffnessCoef;
    prm_.device = device;
    prm_.expect_cuts = expectCuts ? 1 : 0;  // (a cuttable body: slack, node order and re-sync workspace at creation, fembrain_hip.h)
    check(fb_fem_create(&h_, numVertices, restPositions, numElements, elements, numConstrainedDOFs, constrainedDOFs, &prm_));
    std::memset(&info_, 0, sizeof info_);
  }
  // the tet mesh a polygonizer handle (GPUPoly::handle()) holds on the device becomes the FEM mesh, no host copy
  // (fb_fem_create_from_poly; field grid -> tets -> K0 on the device)
  HipIntegrator(fb_poly_t poly, int numConstrainedDOFs, const int* constrainedDOFs, double timestep = 0.0333, double dampingMassCoef = 0.0,
                double dampingStiffnessCoef = 0.01, double E = 1e7, double nu = 0.46, double density = 1000.0, int device = 0)
      : r_(0), h_(nullptr) {
    fb_fem_default_params(&prm_);
    prm_.E = E; prm_.nu = nu; prm_.rho = density;
    prm_.timestep = timestep; prm_.damping_mass = dampingMassCoef; prm_.damping_stiffness = dampingStiffnessCoef;
    prm_.device = device;
    check(fb_fem_create_from_poly(&h_, poly, numConstrainedDOFs, constrainedDOFs, &prm_));
    r_ = 3 * fb_fem_num_nodes(h_);
    std::memset(&info_, 0, sizeof info_);
  }
  // a handle made by the library itself (fb_fem_detach_part) is adopted: this object owns it from here on.  params: the parameters the
  // handle was made with (the parent's, as its setters have left them), the host mirror GetTimestep and the damping setters work from
  HipIntegrator(fb_fem_t adopted, const fb_fem_params& params) : r_(0), h_(adopted), prm_(params) {
    if (!adopted) throw std::invalid_argument("null FEM handle");
    r_ = 3 * fb_fem_num_nodes(adopted);
    std::memset(&info_, 0, sizeof info_);
  }
  ~HipIntegrator() { fb_fem_destroy(h_); }
  HipIntegrator(const HipIntegrator&) = delete;
  HipIntegrator& operator=(const HipIntegrator&) = delete;

  int Getr() const { return r_; }
  // 0 = ok, 1 = solver failed (the reference prints and exit(-1)s, PS_VolumeConservingIntegrator.cpp:203-209)
  int DoTimestep() {
    const int rc = fb_fem_step(h_, &info_);
    if (rc == FB_ESOLVER) return 1;
    check(rc);
    return 0;
  }
  void SetExternalForces(double* f) { check(fb_fem_set_external_forces(h_, f)); }
  void AddExternalForces(double* f) { check(fb_fem_add_external_forces(h_, f)); }
  void SetExternalForcesToZero() { check(fb_fem_set_external_forces_zero(h_)); }
  void SetUniformForce(int axis, double value) { check(fb_fem_set_uniform_force(h_, axis, value)); }
  void SetqState(const double* q, const double* qvel = nullptr, const double* qaccel = nullptr) { check(fb_fem_set_state(h_, q, qvel, qaccel)); }
  void GetqState(double* q, double* qvel = nullptr, double* qaccel = nullptr) { check(fb_fem_get_state(h_, q, qvel, qaccel)); }
  int SetState(double* q, double* qvel = nullptr) { check(fb_fem_set_state(h_, q, qvel, nullptr)); return 0; }
  // Getq / Getqvel / Getqaccel (integratorBase.h:139-141) hand out the integrator's own arrays in the reference; the state
  // lives on the device here, so these return a host mirror refreshed by the call (borrowed, valid until the next call)
  double* Getq() { mirror(); return mq_.data(); }
  double* Getqvel() { mirror(); return mv_.data(); }
  double* Getqaccel() { mirror(); return ma_.data(); }
  void ResetToRest() { check(fb_fem_reset(h_)); }
  void SetTimestep(double t) { prm_.timestep = t; check(fb_fem_set_timestep(h_, t)); }
  double GetTimestep() const { return prm_.timestep; }
  void SetDampingMassCoef(double c) { prm_.damping_mass = c; check(fb_fem_set_damping(h_, prm_.damping_mass, prm_.damping_stiffness)); }
  void SetDampingStiffnessCoef(double c) { prm_.damping_stiffness = c; check(fb_fem_set_damping(h_, prm_.damping_mass, prm_.damping_stiffness)); }
  void SetInternalForceScalingFactor(double f) { check(fb_fem_set_internal_force_scaling(h_, f)); }
  // Per-element materials (fembrain_hip.h; the reference reads VolumetricMesh::getElementMaterial(el) of every element,
  // corotationalLinearFEM.cpp:55-66): a table of 1..256 ENU materials, entry 0 for every element without an id, and one id per element
  // in the caller's element order.  A re-sync from a whole mesh returns the ids to 0; a cut hands every piece its parent's id.
  void SetMaterials(int n, const double* E, const double* nu, const double* density) {
    check(fb_fem_set_materials(h_, n, E, nu, density));
    prm_.E = E[0]; prm_.nu = nu[0]; prm_.rho = density[0];
    mass_.clear();  // (GetTotalMass / GetKineticEnergy read the mass blocks again)
  }
  void SetElementMaterials(int first, int count, const unsigned char* ids) { check(fb_fem_set_element_materials(h_, first, count, ids)); mass_.clear(); }
  int GetNumMaterials() const { return fb_fem_num_materials(h_); }
  void GetMaterials(double* E, double* nu, double* density) { check(fb_fem_read_materials(h_, E, nu, density)); }
  void GetElementMaterials(int first, int count, unsigned char* ids) { check(fb_fem_read_element_materials(h_, first, count, ids)); }
  bool setConstrainedDOF(int num, int* arr) {
    if (num == 0 || arr == nullptr) return false;  // integratorBaseSparse.cpp:73-75
    check(fb_fem_set_constrained_dofs(h_, num, arr));
    return true;
  }
  // IntegratorBaseSparse::GetTotalMass / GetKineticEnergy (integratorBaseSparse.cpp:63-71): sum of the entries of the
  // inflated consistent mass matrix, and 1/2 qvel^T M qvel -- host arithmetic on the mass blocks (not on the step path)
  double GetTotalMass() {
    loadMass();
    double s = 0.0;
    for (size_t k = 0; k < mass_.size(); k++) s += mass_[k];
    return 3.0 * s;
  }
  double GetKineticEnergy() {
    loadMass();
    std::vector<double> v((size_t)r_);
    check(fb_fem_get_state(h_, nullptr, v.data(), nullptr));
    double e = 0.0;
    for (size_t a = 0; a + 1 < bptr_.size(); a++)
      for (int k = bptr_[a]; k < bptr_[a + 1]; k++) {
        const size_t b = (size_t)bcol_[k];
        e += mass_[k] * (v[3 * a] * v[3 * b] + v[3 * a + 1] * v[3 * b + 1] + v[3 * a + 2] * v[3 * b + 2]);
      }
    return 0.5 * e;
  }
  double GetForceAssemblyTime() const { return info_.assembly_seconds; }
  double GetSystemSolveTime() const { return info_.solve_seconds; }
  int GetLastIterations() const { return info_.cg_iterations; }
  int GetLastNewtonIterations() const { return info_.newton_iterations; }  // (Newmark: linear solves of the last step; 1 otherwise)
  int FloorCollision(double floorY, double restitution) {
    int n = 0;
    check(fb_fem_floor_collision(h_, floorY, restitution, &n));
    return n;
  }
  // The haptic probe on the device (fembrain_hip.h): ring-spread forces added into the current external forces, picking, volume.
  // Node ids are the caller's.  AddHapticForces takes at most FB_HAPTIC_MAX_SOURCES sources.
  void AddHapticForces(int n, const int* nodeIds, const double* forces3, int neighbourhoodSize) {
    check(fb_fem_add_haptic_forces(h_, n, nodeIds, forces3, neighbourhoodSize));
  }
  int PickVertex(const double wpos[3], double xyz[3], double* dist2 = nullptr) {
    int index = -1;
    check(fb_fem_pick_vertex(h_, wpos, &index, xyz, dist2));
    return index;
  }
  // ids / xyz: room for `capacity` entries (3 doubles each); returns the full count, of which min(count, capacity) were written
  int PickBox(const double lo[3], const double hi[3], int capacity, int* ids, double* xyz) {
    int found = 0;
    check(fb_fem_pick_box(h_, lo, hi, capacity, ids, xyz, &found));
    return found;
  }
  double Volume(double* perElement = nullptr) {
    double total = 0.0;
    check(fb_fem_volume(h_, &total, perElement));
    return total;
  }
  // The probe's box contact on the device (fembrain_hip.h): AvatarProbe::onTranslate as a session of the handle -- touched set, face,
  // penalty forces -- and the ring spread of its list, any number of sources.  Only the info structs come back.
  fb_fem_contact_info ContactMove(const double lo[3], const double hi[3], double forceCoeff) {
    fb_fem_contact_info info;
    check(fb_fem_contact_move(h_, lo, hi, forceCoeff, &info));
    return info;
  }
  fb_fem_contact_info ContactInfo() {
    fb_fem_contact_info info;
    check(fb_fem_contact_info_get(h_, &info));
    return info;
  }
  void ContactReset(bool keepFace) { check(fb_fem_contact_reset(h_, keepFace ? 1 : 0)); }
  // the stored list: ascending ids, first-touch positions and forces (3 doubles per entry), ContactInfo().list_size entries
  void ReadContact(std::vector<int>& ids, std::vector<double>& firstXyz, std::vector<double>& forces3) {
    const size_t n = (size_t)ContactInfo().list_size;
    ids.assign(n, 0); firstXyz.assign(3 * n, 0.0); forces3.assign(3 * n, 0.0);
    if (n) check(fb_fem_read_contact(h_, ids.data(), firstXyz.data(), forces3.data()));
  }
  fb_fem_contact_spread_info ContactApply(int neighbourhoodSize) {
    fb_fem_contact_spread_info info;
    check(fb_fem_contact_apply(h_, neighbourhoodSize, &info));
    return info;
  }
  // Contact with another body on the same device (fembrain_hip.h, "Contact between two bodies"): the surface vertices of each that lie
  // inside the other are pushed to the closest point of its boundary, the face there is pushed back; ADDED to both external force vectors.
  fb_fem_body_contact_info BodyContact(HipIntegrator& other, double stiffness, double depthCap = 0.0, int directions = FB_BODY_A_INTO_B | FB_BODY_B_INTO_A) {
    const fb_fem_body_contact_params p = {stiffness, depthCap, directions, 0};
    fb_fem_body_contact_info info;
    if (frictionless()) check(fb_fem_body_contact(h_, other.h_, &p, &info));
    else check(fb_fem_body_contact_friction(h_, other.h_, &p, &friction_, &info, &frictionInfo_));
    return info;
  }
  // Friction and damping of the contacts BodyContact and SelfContact of THIS integrator make from here on (fembrain_hip.h, "Friction and
  // damping of a contact"): regularised Coulomb friction, linear below slipSpeed and mu N at and above it, and a damper along the normal,
  // from the velocities of both sides.  Explicit: keep mu N / slipSpeed * dt and damping * dt below the mass a contact pushes
  // (LastContactFriction().max_stick_rate tells the first).  All zero, the default: the frictionless calls, as ever.
  void SetContactFriction(double mu, double slipSpeed, double damping) {
    friction_.mu = mu; friction_.slip_speed = slipSpeed; friction_.damping = damping; friction_.reserved = 0.0;
  }
  // classes, maxima and friction sums of the last BodyContact / SelfContact that ran with friction or damping
  const fb_fem_contact_friction_info& LastContactFriction() const { return frictionInfo_; }
  // per contact of that call, in ReadBodyContact's / ReadSelfContact's order: N, the tangential velocity t[3], the friction on the point -f[3]
  void ReadBodyContactFriction(int direction, int n, std::vector<double>& normalForce, std::vector<double>& slip3, std::vector<double>& friction3) {
    normalForce.assign((size_t)n, 0.0); slip3.assign(3 * (size_t)n, 0.0); friction3.assign(3 * (size_t)n, 0.0);
    check(fb_fem_read_body_contact_friction(h_, direction, normalForce.data(), slip3.data(), friction3.data()));
  }
  void ReadSelfContactFriction(int n, std::vector<double>& normalForce, std::vector<double>& slip3, std::vector<double>& friction3) {
    normalForce.assign((size_t)n, 0.0); slip3.assign(3 * (size_t)n, 0.0); friction3.assign(3 * (size_t)n, 0.0);
    check(fb_fem_read_self_contact_friction(h_, normalForce.data(), slip3.data(), friction3.data()));
  }
  // the contacts of one direction of the last BodyContact of this integrator, info.n_contacts[direction == FB_BODY_A_INTO_B ? 0 : 1] entries
  void ReadBodyContact(int direction, int n, std::vector<int>& node, std::vector<int>& element, std::vector<int>& face, std::vector<double>& closestXyz,
                       std::vector<double>& bary3, std::vector<double>& depth) {
    node.assign((size_t)n, 0); element.assign((size_t)n, 0); face.assign((size_t)n, 0);
    closestXyz.assign(3 * (size_t)n, 0.0); bary3.assign(3 * (size_t)n, 0.0); depth.assign((size_t)n, 0.0);
    check(fb_fem_read_body_contact(h_, direction, node.data(), element.data(), face.data(), closestXyz.data(), bary3.data(), depth.data()));
  }
  // Contact of the body with itself (fembrain_hip.h, "Contact of a body with itself"): every surface vertex inside an element it may meet
  // is pushed to the closest point of the boundary it may meet, the face there is pushed back; ADDED to the external force vector.
  // mode: FB_SELF_CONTACT_ANY (a fold of one part) or FB_SELF_CONTACT_OTHER_PARTS (the halves of a cut).
  fb_fem_self_contact_info SelfContact(double stiffness, double depthCap = 0.0, int mode = FB_SELF_CONTACT_ANY) {
    const fb_fem_self_contact_params p = {stiffness, depthCap, mode, 0};
    fb_fem_self_contact_info info;
    if (frictionless()) check(fb_fem_self_contact(h_, &p, &info));
    else check(fb_fem_self_contact_friction(h_, &p, &friction_, &info, &frictionInfo_));
    return info;
  }
  // the contacts of the last SelfContact of this integrator, info.n_contacts entries
  void ReadSelfContact(int n, std::vector<int>& node, std::vector<int>& element, std::vector<int>& face, std::vector<double>& closestXyz,
                       std::vector<double>& bary3, std::vector<double>& depth) {
    node.assign((size_t)n, 0); element.assign((size_t)n, 0); face.assign((size_t)n, 0);
    closestXyz.assign(3 * (size_t)n, 0.0); bary3.assign(3 * (size_t)n, 0.0); depth.assign((size_t)n, 0.0);
    check(fb_fem_read_self_contact(h_, node.data(), element.data(), face.data(), closestXyz.data(), bary3.data(), depth.data()));
  }
  // Contact with a rigid tool (fembrain_hip.h, "Contact with a rigid tool"): every point -- surface vertex, or node -- that a sphere,
  // capsule or oriented box of the tool holds is pushed out along that shape's normal; ADDED to the external force vector.  The info
  // holds what the tissue returns to the tool: force_on_tool, torque_on_tool about tool.origin.  SetContactFriction applies: the law
  // then takes the tool's velocity at the point from tool.velocity and tool.omega.
  fb_fem_tool_contact_info ToolContact(const fb_tool& tool, double stiffness, double depthCap = 0.0, int points = FB_TOOL_SURFACE_VERTICES) {
    const fb_fem_tool_contact_params p = {stiffness, depthCap, points, 0};
    fb_fem_tool_contact_info info;
    check(fb_fem_tool_contact(h_, &tool, &p, frictionless() ? nullptr : &friction_, &info));
    return info;
  }
  // the contacts of the last ToolContact of this integrator, n = info.n_contacts entries (a smaller or negative n reads them all): node,
  // winning shape, depth before the cap, normal, force
  void ReadToolContact(int n, std::vector<int>& node, std::vector<int>& shape, std::vector<double>& depth, std::vector<double>& normal3, std::vector<double>& force3) {
    n = std::max(n, fb_fem_num_tool_contacts(h_));
    node.assign((size_t)n, 0); shape.assign((size_t)n, 0); depth.assign((size_t)n, 0.0); normal3.assign(3 * (size_t)n, 0.0); force3.assign(3 * (size_t)n, 0.0);
    check(fb_fem_read_tool_contact(h_, node.data(), shape.data(), depth.data(), normal3.data(), force3.data(), nullptr, nullptr, nullptr));
  }
  // ... and what the friction law left per contact: N, the tangential velocity t[3], the friction on the node -f[3] (zero after a frictionless call)
  void ReadToolContactFriction(int n, std::vector<double>& normalForce, std::vector<double>& slip3, std::vector<double>& friction3) {
    n = std::max(n, fb_fem_num_tool_contacts(h_));
    normalForce.assign((size_t)n, 0.0); slip3.assign(3 * (size_t)n, 0.0); friction3.assign(3 * (size_t)n, 0.0);
    check(fb_fem_read_tool_contact(h_, nullptr, nullptr, nullptr, nullptr, nullptr, normalForce.data(), slip3.data(), friction3.data()));
  }
  // Constrained DOFs that follow targets, and the force they return (fembrain_hip.h, "Constrained motion"): dofs ascending, each a
  // constrained DOF of the handle; the next DoTimestep ends with q = displacements there, bit for bit.  n = 0 clears the set.
  void SetConstrainedMotion(int n, const int* dofs, const double* displacements) { check(fb_fem_set_constrained_motion(h_, n, dofs, displacements)); }
  void ReadConstrainedMotion(std::vector<int>& dofs, std::vector<double>& displacements) {
    const size_t n = (size_t)std::max(0, fb_fem_num_constrained_motion(h_));
    dofs.assign(n, 0); displacements.assign(n, 0.0);
    check(fb_fem_read_constrained_motion(h_, dofs.data(), displacements.data()));
  }
  // the reactions of the last DoTimestep in the set's order (null: not wanted) and their sum by axis
  void ReadReactions(std::vector<double>* forces, double sum3[3]) {
    if (forces) forces->assign((size_t)std::max(0, fb_fem_num_constrained_motion(h_)), 0.0);
    check(fb_fem_read_reactions(h_, forces ? forces->data() : nullptr, sum3));
  }
  fb_fem_motion_info MotionInfo() {
    fb_fem_motion_info info;
    check(fb_fem_motion_info_get(h_, &info));
    return info;
  }
  void TimeMotion(int reps, double seconds[4]) { check(fb_fem_time_motion(h_, reps, seconds)); }
  // the grasp on top: nodes ascending; targets = R (p_grab - pivot) + pivot + t - x0 set on the device; Release frees what Grasp constrained
  fb_fem_motion_info Grasp(int n, const int* nodes) {
    fb_fem_motion_info info;
    check(fb_fem_grasp(h_, n, nodes, &info));
    return info;
  }
  void GraspMove(const double R[9], const double t[3], const double pivot[3]) { check(fb_fem_grasp_move(h_, R, t, pivot)); }
  void Release() { check(fb_fem_release(h_)); }
  // Element stress and strain on the device (fembrain_hip.h): von Mises stress, energy density and J of every element at the current
  // state stay on the device, `out` brings the summary.  flags: FB_STRESS_WORLD | FB_STRESS_TENSORS.
  void ComputeStress(int flags, fb_fem_stress_info* out) { check(fb_fem_stress(h_, flags, out)); }
  // the arrays of the last ComputeStress for elements first .. first + count - 1; any pointer may be null (stress6 / strain6: 6 per element)
  void ReadStress(int first, int count, double* vonMises, double* energyDensity, double* J, double* stress6 = nullptr, double* strain6 = nullptr) {
    check(fb_fem_read_stress(h_, first, count, vonMises, energyDensity, J, stress6, strain6));
  }
  // per surface vertex (fb_fem_read_surface's vertex order) the mean von Mises stress of the elements behind its faces
  void SurfaceStress(std::vector<float>& vonMises) {
    fb_fem_surface_info info;
    check(fb_fem_read_stress(h_, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr));  // (no stress of this mesh: throw before the surface is built)
    check(fb_fem_surface(h_, &info));
    vonMises.assign((size_t)info.n_vertices, 0.0f);
    check(fb_fem_surface_stress(h_, vonMises.data()));
  }
  // The way back from an embedding (fembrain_hip.h; EmbeddedMesh wraps these per mesh): forces on drawn points added to the nodes through
  // the binding (pointIds strictly ascending; null: every point, n = the embedding's points), picks on the drawn mesh at the current
  // state, and the von Mises stress of every point's element from the last ComputeStress.
  void EmbedAddForces(int id, int n, const int* pointIds, const double* forces3) { check(fb_fem_embed_add_forces(h_, id, n, pointIds, forces3)); }
  // returns the hit triangle, -1 for a miss; t, bary (u, v) and xyz may be null
  int EmbedPickRay(int id, const double origin[3], const double dir[3], double tMax, double* t, double bary[2], double xyz[3]) {
    int triangle = -1;
    check(fb_fem_embed_pick_ray(h_, id, origin, dir, tMax, &triangle, t, bary, xyz));
    return triangle;
  }
  int EmbedPickPoint(int id, const double wpos[3], double xyz[3], double* dist2 = nullptr) {
    int index = -1;
    check(fb_fem_embed_pick_point(h_, id, wpos, &index, xyz, dist2));
    return index;
  }
  void EmbedStress(int id, float* perPoint) { check(fb_fem_embed_stress(h_, id, perPoint)); }
  // the external forces the next step will read, Getr() doubles in the caller's node order
  void GetExternalForces(double* f) { check(fb_fem_get_external_forces(h_, f)); }
  void RebuildElements() { check(fb_fem_rebuild_elements(h_)); }
  void Resync(int numVertices, const double* rest, int numElements, const int* elements, int nFixed, const int* fixed) {
    mass_.clear(); bptr_.clear(); bcol_.clear();
    check(fb_fem_resync(h_, numVertices, rest, numElements, elements, nFixed, fixed));
    r_ = 3 * numVertices;
  }
  // the same from a description of the change (fb_fem_resync_delta): the mesh stays on the device
  void ResyncDelta(int nRemoved, const int* removed, int nChanged, const int* changedIds, const int* changedNodes, int nAdded, const int* added, int nNewVertices,
                   const double* newRest, int nFixed, const int* fixed) {
    mass_.clear(); bptr_.clear(); bcol_.clear();
    check(fb_fem_resync_delta(h_, nRemoved, removed, nChanged, changedIds, changedNodes, nAdded, added, nNewVertices, newRest, nFixed, fixed));
    r_ = 3 * fb_fem_num_nodes(h_);
  }
  // fb_fem_cut: the blade's swept quad strip (nPoints xyz) cuts the mesh on the device and the handle re-syncs; `out` says what happened
  void Cut(int nPoints, const double* strip, int mode, bool modify, fb_cut_result* out) {
    check(fb_fem_cut(h_, nPoints, strip, mode, modify ? 1 : 0, out));
    if (out->status == FB_CUT_DONE) { mass_.clear(); bptr_.clear(); bcol_.clear(); }
    r_ = 3 * fb_fem_num_nodes(h_);
  }
  // the device-resident mesh in the caller's numbering
  void ReadMesh(std::vector<double>& rest, std::vector<int>& elements) {
    rest.resize(3 * (size_t)fb_fem_num_nodes(h_));
    elements.resize(4 * (size_t)fb_fem_num_tets(h_));
    check(fb_fem_read_mesh(h_, rest.data(), elements.data()));
  }
  // fb_fem_parts / fb_fem_split_parts: the disjoint parts of the device's mesh, and the parts on either side of a quad pushed apart
  void Parts(fb_fem_parts_info* out) { check(fb_fem_parts(h_, out)); }
  void SplitParts(const double quad[12], double dist, fb_fem_split_info* out) { check(fb_fem_split_parts(h_, quad, dist, out)); }
  // fb_fem_detach_part: part `part` as an integrator of its own, made on the device with the parameters of this one and the state, forces,
  // materials and constraints of its nodes and elements; FB_DETACH_REMOVE erases its elements here.  The caller deletes the returned integrator.
  HipIntegrator* DetachPart(int part, int flags, fb_fem_detach_info* out = nullptr) {
    fb_fem_t piece = nullptr;
    check(fb_fem_detach_part(h_, part, flags, &piece, nullptr, nullptr, out));
    if (flags == FB_DETACH_REMOVE) { mass_.clear(); bptr_.clear(); bcol_.clear(); }
    try { return new HipIntegrator(piece, prm_); } catch (...) { fb_fem_destroy(piece); throw; }
  }
  // the constrained DOFs as the handle holds them (caller ids, ascending)
  void ReadConstrainedDofs(std::vector<int>& dofs) {
    dofs.assign((size_t)std::max(0, fb_fem_num_constrained_dofs(h_)), 0);
    check(fb_fem_read_constrained_dofs(h_, dofs.data()));
  }
  fb_fem_t handle() const { return h_; }
  static void check(int rc) {
    if (rc != FB_OK) throw std::runtime_error(std::string("fembrain_hip: ") + fb_last_error());
  }

 private:
  void loadMass() {
    if (!mass_.empty()) return;
    bptr_.resize((size_t)fb_fem_num_nodes(h_) + 1);
    bcol_.resize((size_t)fb_fem_num_blocks(h_));
    mass_.resize(bcol_.size());
    check(fb_fem_pattern(h_, bptr_.data(), bcol_.data()));
    check(fb_fem_mass(h_, mass_.data()));
  }
  std::vector<int> bptr_, bcol_;
  std::vector<double> mass_;
  int r_;
  void mirror() {
    mq_.resize((size_t)r_); mv_.resize((size_t)r_); ma_.resize((size_t)r_);
    check(fb_fem_get_state(h_, mq_.data(), mv_.data(), ma_.data()));
  }
  std::vector<double> mq_, mv_, ma_;
  fb_fem_t h_;
  fb_fem_params prm_;
  fb_step_info info_;
  bool frictionless() const { return friction_.mu == 0.0 && friction_.slip_speed == 0.0 && friction_.damping == 0.0; }
  fb_fem_contact_friction_params friction_ = {0.0, 0.0, 0.0, 0.0};  // SetContactFriction
  fb_fem_contact_friction_info frictionInfo_ = {};
};

// ---- the narrower VegaFEM seams, for hosts that keep their own integrator -------------------------
// ForceModel (vegafem/forceModel/forceModel.h:42-67) over a HipIntegrator's handle: internal force and tangent stiffness
// at a displacement u.  The matrix comes as 3x3 blocks on the node-level pattern (bptr / bcol, ascending columns per row
// = the block rows of the reference's SparseMatrix, sparseMatrix.cpp:238-262), 9 row-major values per block.
class HipForceModel {
 public:
  explicit HipForceModel(HipIntegrator* integrator) : in_(integrator) {}
  int Getr() const { return in_->Getr(); }
  void GetInternalForce(double* u, double* internalForces) { HipIntegrator::check(fb_fem_assemble(in_->handle(), u, internalForces, nullptr)); }
  // GetTangentStiffnessMatrixTopology: callee-allocated in the reference; here the caller's vectors are filled
  void GetTangentStiffnessMatrixTopology(std::vector<int>& bptr, std::vector<int>& bcol) {
    bptr.resize((size_t)fb_fem_num_nodes(in_->handle()) + 1);
    bcol.resize((size_t)fb_fem_num_blocks(in_->handle()));
    HipIntegrator::check(fb_fem_pattern(in_->handle(), bptr.data(), bcol.data()));
  }
  void GetTangentStiffnessMatrix(double* u, std::vector<double>& blocks) {
    blocks.resize(9 * (size_t)fb_fem_num_blocks(in_->handle()));
    HipIntegrator::check(fb_fem_assemble(in_->handle(), u, nullptr, blocks.data()));
  }
  void GetForceAndMatrix(double* u, double* internalForces, std::vector<double>& blocks) {
    blocks.resize(9 * (size_t)fb_fem_num_blocks(in_->handle()));
    HipIntegrator::check(fb_fem_assemble(in_->handle(), u, internalForces, blocks.data()));
  }

 private:
  HipIntegrator* in_;
};

// LinearSolver (vegafem/sparseSolver/linearSolver.h:44-53) + CGSolver's Jacobi-PCG entry (CGSolver.cpp:129-190) on the
// system the handle assembled last (Keff of the current state): returns the reference's code, > 0 iterations when
// converged, < 0 when not.
class HipCGSolver {
 public:
  explicit HipCGSolver(HipIntegrator* integrator) : in_(integrator) {}
  int SolveLinearSystemWithJacobiPreconditioner(double* x, const double* b, double eps, int maxIterations) {
    int it = 0;
    HipIntegrator::check(fb_fem_pcg(in_->handle(), b, x, eps, maxIterations, &it));
    return it;
  }
  int SolveLinearSystem(double* x, const double* rhs) { return SolveLinearSystemWithJacobiPreconditioner(x, rhs, 1e-6, 10000) > 0 ? 0 : 1; }
  // CGSolver's C hook `typedef void (*blackBoxProductType)(const void* data, const double* x, double* Ax)` (CGSolver.h:65-66):
  // pass HipCGSolver::BlackBoxProduct with data = the HipIntegrator to run the reference's own CG on the device SpMV
  static void BlackBoxProduct(const void* data, const double* x, double* Ax) {
    HipIntegrator::check(fb_fem_spmv(static_cast<const HipIntegrator*>(data)->handle(), x, Ax));
  }

 private:
  HipIntegrator* in_;
};

class SurfaceMesh;
class EmbeddedMesh;

class Deformable {
 public:
  Deformable(int numVertices, const double* restPositions, int numElements, const int* elements,
             const std::vector<int>& vFixedVertices = std::vector<int>(), int device = 0)
      : m_rest(restPositions, restPositions + 3 * (size_t)numVertices), m_elements(elements, elements + 4 * (size_t)numElements),
        m_vFixedVertices(vFixedVertices), m_device(device) {
    init();
    syncForceModel();
  }
  ~Deformable();  // (SurfaceMesh.h)
  // What the host draws (the reference's Deformable IS an SGMesh; its surface is getSurfMesh()): the boundary triangles of the mesh the
  // device holds, built and kept current there (SurfaceMesh.h).  Owned by the Deformable, created at the first call.
  SurfaceMesh* surfaceMesh();
  // The mesh the host draws instead (the marching-cubes surface, an organ mesh), bound to the tets and moved with them on the device:
  // what replaces the receiver of setDeformCallback (EmbeddedMesh.h).  xyz: 3 doubles per point in the rest frame; triangles: 3 point
  // indices each, may be empty.  Owned by the Deformable; the binding follows cut, syncForceModel(Delta) and detached parts by itself.
  EmbeddedMesh* embed(const std::vector<double>& xyz, const std::vector<int>& triangles = std::vector<int>(), double zeroThreshold = 0.0);
  // A click on an embedded mesh that pulls (EmbeddedMesh::touch): the nearest hit of the ray on its triangles at the current state, and
  // `force` shared among the hit triangle's three points by the hit's barycentrics, added to the external forces on the device.  Returns
  // the hit triangle, -1 for a miss (nothing is added).  The forces act in the next DoTimestep of the integrator; timestep() itself
  // sets the external forces anew (gravity, the probe) before it steps.
  int touchEmbedded(EmbeddedMesh* mesh, const vec3d& origin, const vec3d& dir, const vec3d& force);
  // the external forces the next integrator step will read, 3 doubles per node
  void externalForces(std::vector<double>& f) {
    f.assign((size_t)m_lpIntegrator->Getr(), 0.0);
    m_lpIntegrator->GetExternalForces(f.data());
  }

  // Deformable::timestep (Deformable.cpp:318-420)
  void timestep() {
    if (m_lpIntegrator == nullptr) return;
    const bool applyGravity = m_bApplyGravity && (m_ctCollided == 0);
    if (m_bHapticInProgress && m_bContactList) {
      // the probe's contact list, kept on the device by probeMove: any number of sources (fb_fem_contact_apply)
      if (applyGravity) m_lpIntegrator->SetUniformForce(1, -10000.0);
      else m_lpIntegrator->SetExternalForcesToZero();
      m_lpIntegrator->ContactApply(m_hapticForceNeighorhoodSize);
    } else if (m_bHapticInProgress && !m_vHapticIndices.empty() && m_vHapticIndices.size() <= (size_t)FB_HAPTIC_MAX_SOURCES &&
        m_vHapticForces.size() >= m_vHapticIndices.size()) {
      // the probe on the device: gravity or zero generated there, then the ring-spread forces added (fb_fem_add_haptic_forces)
      if (applyGravity) m_lpIntegrator->SetUniformForce(1, -10000.0);
      else m_lpIntegrator->SetExternalForcesToZero();
      m_hapticStage.resize(3 * m_vHapticIndices.size());
      for (size_t i = 0; i < m_vHapticIndices.size(); i++) {
        m_hapticStage[3 * i] = m_vHapticForces[i].x; m_hapticStage[3 * i + 1] = m_vHapticForces[i].y; m_hapticStage[3 * i + 2] = m_vHapticForces[i].z;
      }
      m_lpIntegrator->AddHapticForces((int)m_vHapticIndices.size(), m_vHapticIndices.data(), m_hapticStage.data(), m_hapticForceNeighorhoodSize);
    } else if (m_bHapticInProgress && !m_vHapticIndices.empty()) {  // more sources than the device call takes: the host walk
      std::fill(m_arrExtForces.begin(), m_arrExtForces.end(), 0.0);
      if (applyGravity)
        for (U32 i = 1; i < m_dof; i += 3) m_arrExtForces[i] += -10000.0;
      applyHapticForces();
      m_lpIntegrator->SetExternalForces(m_arrExtForces.data());
    } else if (applyGravity) {
      m_lpIntegrator->SetUniformForce(1, -10000.0);
    } else {
      m_lpIntegrator->SetExternalForcesToZero();
    }
    if (m_lpCollisionBody != nullptr) collideWith(*m_lpCollisionBody, m_collisionStiffness);  // (behind gravity and the probe)
    if (m_selfCollision) selfCollide(m_selfStiffness, m_selfDepthCap, m_selfMode);
    if (m_hasTool) collideTool(m_tool, m_toolStiffness, m_toolDepthCap, m_toolPoints);
    m_lpIntegrator->DoTimestep();
    if (m_hasFloor) m_ctCollided = (U32)m_lpIntegrator->FloorCollision(m_floorY, 0.4);
    if (m_fOnDeform) {
      m_lpIntegrator->GetqState(m_q.data(), m_qVel.data(), nullptr);
      m_fOnDeform(m_dof, m_q.data());
    }
    m_ctTimeStep++;
  }

  // rebuild after a topology change (Deformable.cpp:127-220)
  bool syncForceModel() {
    const int n = (int)(m_rest.size() / 3), m = (int)(m_elements.size() / 4);
    m_dof = 3 * n;
    FixedVerticesToFixedDOF(m_vFixedVertices, m_vFixedDofs);
    if (m_lpIntegrator) m_lpIntegrator->Resync(n, m_rest.data(), m, m_elements.data(), (int)m_vFixedDofs.size(), m_vFixedDofs.data());
    else m_lpIntegrator = new HipIntegrator(n, m_rest.data(), m, m_elements.data(), (int)m_vFixedDofs.size(), m_vFixedDofs.data(),
                                            m_timeStep, m_dampingMassCoeff, m_dampingStiffnessCoeff, 1e7, 0.46, 1000.0, m_device, 1,
                                            /* a Deformable is what FemBrain's scalpel cuts (CuttableMesh): */ true);
    m_q.assign(m_dof, 0.0); m_qVel.assign(m_dof, 0.0); m_arrExtForces.assign(m_dof, 0.0);
    m_bptr.clear(); m_bcol.clear();
    m_restVolume = -1.0;
    surfaceChanged();
    return true;
  }
  // The same after a cut that the host can describe (CuttableMesh::cut erases the cut cells -- VolMesh.cpp:630 -- appends their pieces
  // and the new nodes -- :1083-1088 -- and re-points cells in place -- :1630-1650): `removed` ascending ids of the current element list,
  // `changedIds` ascending with their new nodes, `added` and `newRest` appended.  The host copy of the mesh follows.
  bool syncForceModelDelta(const std::vector<int>& removed, const std::vector<int>& changedIds, const std::vector<int>& changedNodes, const std::vector<int>& added,
                           const std::vector<double>& newRest) {
    if (!m_lpIntegrator) return syncForceModel();
    // The DEVICE first: ResyncDelta refuses bad input before anything changes and throws; the host copy of the mesh is edited
    // only after it has returned, so host and device never disagree.  Ids are range-checked here too: they index the host arrays below.
    const size_t n_el = m_elements.size() / 4;
    for (size_t k = 0; k < changedIds.size(); k++)
      if (changedIds[k] < 0 || (size_t)changedIds[k] >= n_el) throw std::runtime_error("syncForceModelDelta: changed element id out of range");
    for (size_t k = 0; k < removed.size(); k++)
      if (removed[k] < 0 || (size_t)removed[k] >= n_el || (k && removed[k] <= removed[k - 1])) throw std::runtime_error("syncForceModelDelta: removed ids must ascend inside the element list");
    if (changedNodes.size() != 4 * changedIds.size() || added.size() % 4 != 0 || newRest.size() % 3 != 0) throw std::runtime_error("syncForceModelDelta: array sizes do not match");
    std::vector<int> fixedDofs;
    FixedVerticesToFixedDOF(m_vFixedVertices, fixedDofs);
    m_lpIntegrator->ResyncDelta((int)removed.size(), removed.data(), (int)changedIds.size(), changedIds.data(), changedNodes.data(), (int)(added.size() / 4), added.data(),
                                (int)(newRest.size() / 3), newRest.data(), (int)fixedDofs.size(), fixedDofs.data());
    for (size_t k = 0; k < changedIds.size(); k++)
      for (int c = 0; c < 4; c++) m_elements[4 * (size_t)changedIds[k] + c] = changedNodes[4 * k + c];
    if (!removed.empty()) {
      std::vector<int> kept;
      kept.reserve(m_elements.size());
      size_t r = 0;
      for (size_t e = 0; e < n_el; e++) {
        if (r < removed.size() && (size_t)removed[r] == e) { r++; continue; }
        kept.insert(kept.end(), m_elements.begin() + 4 * e, m_elements.begin() + 4 * e + 4);
      }
      m_elements.swap(kept);
    }
    m_elements.insert(m_elements.end(), added.begin(), added.end());
    m_rest.insert(m_rest.end(), newRest.begin(), newRest.end());
    m_dof = (U32)m_rest.size();
    m_vFixedDofs.swap(fixedDofs);
    m_q.assign(m_dof, 0.0); m_qVel.assign(m_dof, 0.0); m_arrExtForces.assign(m_dof, 0.0);
    m_bptr.clear(); m_bcol.clear();
    m_restVolume = -1.0;
    surfaceChanged();
    return true;
  }
  // CuttableMesh::cut(segments, quadstrips, modifyMesh) (CuttableMesh.cpp:283-505) + cutCompleted's syncForceModel (main.cpp:614-617) in
  // one device call (fb_fem_cut, FB_CUT_BAKE: the deformed shape becomes the rest shape).  Returns the number of subdivided cells, 0 when
  // nothing was cut, or CUT_ERR_INVALID_INPUT_ARG / CUT_ERR_UNHANDLED_CUT_STATE / CUT_ERR_USER_CANCELLED_CUT as the reference does.
  // segments: the blade's path, used by the reference's cut-node detection only, which FemBrain leaves off -- accepted and ignored.
  // The host copy of the mesh is read back after the device call has returned (the rule syncForceModelDelta keeps).
  int cut(const std::vector<vec3d>& segments, const std::vector<vec3d>& quadstrips, bool modifyMesh) {
    if (segments.size() < 2) return CUT_ERR_INVALID_INPUT_ARG;
    if (quadstrips.size() < 4 || quadstrips.size() % 2 != 0) return CUT_ERR_INVALID_INPUT_ARG;
    if (!m_lpIntegrator) syncForceModel();
    std::vector<double> strip;
    strip.reserve(3 * quadstrips.size());
    for (size_t i = 0; i < quadstrips.size(); i++) { strip.push_back(quadstrips[i].x); strip.push_back(quadstrips[i].y); strip.push_back(quadstrips[i].z); }
    fb_cut_result r;
    m_lpIntegrator->Cut((int)quadstrips.size(), strip.data(), FB_CUT_BAKE, modifyMesh, &r);
    if (r.status == FB_CUT_NOTHING) return 0;
    if (r.status == FB_CUT_UNHANDLED) return CUT_ERR_UNHANDLED_CUT_STATE;
    if (r.status == FB_CUT_DRY) return CUT_ERR_USER_CANCELLED_CUT;
    m_lpIntegrator->ReadMesh(m_rest, m_elements);
    m_dof = (U32)m_rest.size();
    m_q.assign(m_dof, 0.0); m_qVel.assign(m_dof, 0.0); m_arrExtForces.assign(m_dof, 0.0);
    m_bptr.clear(); m_bcol.clear();
    m_restVolume = -1.0;
    surfaceChanged();
    return r.n_removed;
  }
  // VolMesh::get_disjoint_parts (VolMesh.cpp:915-965), counted and labelled on the device (fb_fem_parts): the face-connected parts of
  // the mesh the handle holds, in ascending order of their smallest cell.
  int countDisjointParts() {
    if (!m_lpIntegrator) syncForceModel();
    fb_fem_parts_info info;
    m_lpIntegrator->Parts(&info);
    return info.n_parts;
  }
  // ... and the reference's signature and grouping: cells ascending inside a part.  Returns the number of parts.
  int getDisjointParts(std::vector<std::vector<U32> >& cellgroups) {
    const int n = countDisjointParts();
    std::vector<int> part((size_t)fb_fem_num_tets(m_lpIntegrator->handle()));
    HipIntegrator::check(fb_fem_read_parts(m_lpIntegrator->handle(), part.data(), nullptr, nullptr, nullptr, nullptr, nullptr));
    cellgroups.assign((size_t)n, std::vector<U32>());
    for (size_t e = 0; e < part.size(); e++) cellgroups[(size_t)part[e]].push_back((U32)e);
    return n;
  }
  // CuttableMesh::splitParts(sweptquad, dist) (CuttableMesh.cpp:553-626) on the rest shape (fb_fem_split_parts): the parts wholly in front
  // of the quad move by + normal * dist, those wholly behind by - normal * dist.  The host copy of the rest positions follows.
  bool splitParts(const vec3d sweptquad[4], double dist) {
    if (!m_lpIntegrator) syncForceModel();
    double quad[12];
    for (int i = 0; i < 4; i++) { quad[3 * i] = sweptquad[i].x; quad[3 * i + 1] = sweptquad[i].y; quad[3 * i + 2] = sweptquad[i].z; }
    fb_fem_split_info info;
    m_lpIntegrator->SplitParts(quad, dist, &info);
    m_lpIntegrator->ReadMesh(m_rest, m_elements);
    m_restVolume = -1.0;
    surfaceChanged();
    return true;
  }
  // One iteration of CuttableMesh::convertDisjointPartsToMeshes' loop (CuttableMesh.cpp:644-689; fb_fem_read_part): part `part` as the
  // flat node and cell arrays a CuttableMesh (or a second Deformable) is made of, nodes in order of first use.  Nothing is deleted here.
  void readPart(int part, std::vector<double>& xyz, std::vector<U32>& cells) {
    const int n = countDisjointParts();
    if (part < 0 || part >= n) throw std::runtime_error("fembrain_hip: readPart: no such part");
    std::vector<int> el((size_t)n), nd((size_t)n);
    fb_fem_t h = m_lpIntegrator->handle();
    HipIntegrator::check(fb_fem_read_parts(h, nullptr, nullptr, el.data(), nd.data(), nullptr, nullptr));
    xyz.resize(3 * (size_t)nd[(size_t)part]);
    std::vector<int> local(4 * (size_t)el[(size_t)part]);
    HipIntegrator::check(fb_fem_read_part(h, part, nullptr, nullptr, xyz.data(), local.data()));
    cells.assign(local.begin(), local.end());
  }
  // One part as a body of its own, made on the device (fb_fem_detach_part): the new Deformable owns a handle whose mesh is readPart's,
  // with the displacement, velocity, external forces, materials and fixed vertices the part had in this body; it takes over this body's
  // gravity, floor and haptic settings.  remove: the part's cells are erased from this body (its nodes stay, no cell uses them; state
  // and forces carried; the host copy of the mesh follows).  The caller deletes the returned body.
  Deformable* detachPart(int part, bool remove) {
    const int n = countDisjointParts();
    if (part < 0 || part >= n) throw std::runtime_error("fembrain_hip: detachPart: no such part");
    if (remove && n < 2) throw std::runtime_error("fembrain_hip: detachPart: the body has one part");
    HipIntegrator* in = m_lpIntegrator->DetachPart(part, remove ? FB_DETACH_REMOVE : FB_DETACH_KEEP);
    if (remove) {  // (first: the device has changed whatever happens to the piece below)
      try { m_lpIntegrator->ReadMesh(m_rest, m_elements); } catch (...) { delete in; throw; }
      m_bptr.clear(); m_bcol.clear();
      m_restVolume = -1.0;
      surfaceChanged();
    }
    try { return new Deformable(in, *this); } catch (...) { delete in; throw; }
  }
  // CuttableMesh::convertDisjointPartsToMeshes (CuttableMesh.cpp:628-698): every part becomes a body of its own and its cells are erased
  // from this one.  With fewer than two parts nothing happens and 0 is returned, as in the reference.  Otherwise parts n-1 ... 1 are
  // detached with removal (the labels are made again after each; the parts before the removed one keep their indices, which follow
  // their smallest cells), this body is left with part 0, `meshes` receives the n - 1 new bodies in ascending part order (the caller
  // deletes them), and n -- the number of bodies there are now -- is returned.  Should a detachPart throw on the way, the bodies made
  // so far are handed over all the same (their cells are gone from this body: they are the only copy) and the exception goes on.
  int convertDisjointPartsToMeshes(std::vector<Deformable*>& meshes) {
    const int n = countDisjointParts();
    if (n < 2) return 0;
    std::vector<Deformable*> made;
    try {
      for (int p = n - 1; p >= 1; p--) made.push_back(detachPart(p, true));
    } catch (...) {
      meshes.insert(meshes.end(), made.rbegin(), made.rend());
      throw;
    }
    meshes.insert(meshes.end(), made.rbegin(), made.rend());
    return n;
  }
  void setMesh(int numVertices, const double* rest, int numElements, const int* elements) {
    m_rest.assign(rest, rest + 3 * (size_t)numVertices);
    m_elements.assign(elements, elements + 4 * (size_t)numElements);
  }

  // Deformable::FixedVerticesToFixedDOF (Deformable.cpp:294-314)
  static int FixedVerticesToFixedDOF(std::vector<int>& arrInFixedVertices, std::vector<int>& arrOutFixedDOF) {
    arrOutFixedDOF.clear();
    if (arrInFixedVertices.empty()) return 0;
    std::sort(arrInFixedVertices.begin(), arrInFixedVertices.end());
    arrOutFixedDOF.resize(arrInFixedVertices.size() * 3);
    for (size_t i = 0; i < arrInFixedVertices.size(); i++)
      for (int k = 0; k < 3; k++) arrOutFixedDOF[3 * i + k] = arrInFixedVertices[i] * 3 + k;
    return (int)arrOutFixedDOF.size();
  }

  bool addFixedVertex(int index) {
    if (std::find(m_vFixedVertices.begin(), m_vFixedVertices.end(), index) != m_vFixedVertices.end()) return false;
    m_vFixedVertices.push_back(index);
    return updateFixedVertices();
  }
  bool removeFixedVertex(int index) {
    std::vector<int>::iterator it = std::find(m_vFixedVertices.begin(), m_vFixedVertices.end(), index);
    if (it == m_vFixedVertices.end()) return false;
    m_vFixedVertices.erase(it);
    return updateFixedVertices();
  }
  bool setFixedVertices(const std::vector<int>& v) { m_vFixedVertices = v; return updateFixedVertices(); }
  int getFixedVertices(std::vector<int>& v) { v = m_vFixedVertices; return (int)v.size(); }
  bool updateFixedVertices() {
    FixedVerticesToFixedDOF(m_vFixedVertices, m_vFixedDofs);
    return m_lpIntegrator->setConstrainedDOF((int)m_vFixedDofs.size(), m_vFixedDofs.data());
  }

  // Deformable::applyHapticForces (Deformable.cpp:634-706): each haptic force acts on its vertex and, with the linear
  // fall-off (size - j)/size, on the vertices first reached in ring j of a breadth-first walk over mesh edges.  Vertex
  // neighbours are the off-diagonal columns of the stiffness pattern (vertices sharing a tet edge).  The host walk: timestep() runs
  // it only for more than FB_HAPTIC_MAX_SOURCES sources (the pattern is fetched then, and only then).
  bool applyHapticForces() {
    if (m_vHapticIndices.empty() || !m_bHapticInProgress) return false;
    if (m_bptr.empty()) {
      m_bptr.resize(m_rest.size() / 3 + 1);
      m_bcol.resize(fb_fem_num_blocks(m_lpIntegrator->handle()));
      if (fb_fem_pattern(m_lpIntegrator->handle(), m_bptr.data(), m_bcol.data()) != FB_OK) return false;
    }
    for (size_t i = 0; i < m_vHapticIndices.size(); i++) {
      const int v = m_vHapticIndices[i];
      m_arrExtForces[3 * v + 0] += m_vHapticForces[i].x;
      m_arrExtForces[3 * v + 1] += m_vHapticForces[i].y;
      m_arrExtForces[3 * v + 2] += m_vHapticForces[i].z;
    }
    for (size_t iv = 0; iv < m_vHapticIndices.size(); iv++) {
      std::vector<char> affected(m_rest.size() / 3, 0);
      std::vector<int> last(1, m_vHapticIndices[iv]);
      affected[m_vHapticIndices[iv]] = 1;
      const vec3d f = m_vHapticForces[iv];
      for (int j = 1; j < m_hapticForceNeighorhoodSize; j++) {
        const double mag = 1.0 * (m_hapticForceNeighorhoodSize - j) / static_cast<double>(m_hapticForceNeighorhoodSize);
        std::vector<int> fresh;
        for (size_t a = 0; a < last.size(); a++)
          for (int p = m_bptr[last[a]]; p < m_bptr[last[a] + 1]; p++) {
            const int nb = m_bcol[p];
            if (!affected[nb]) { affected[nb] = 2; fresh.push_back(nb); }  // 2 = discovered in this ring
          }
        std::sort(fresh.begin(), fresh.end());
        for (size_t a = 0; a < fresh.size(); a++) {
          m_arrExtForces[3 * fresh[a] + 0] += mag * f.x;
          m_arrExtForces[3 * fresh[a] + 1] += mag * f.y;
          m_arrExtForces[3 * fresh[a] + 2] += mag * f.z;
          affected[fresh[a]] = 1;
        }
        last.swap(fresh);
      }
    }
    return true;
  }
  int getHapticForceRadius() const { return m_hapticForceNeighorhoodSize; }
  void setHapticForceRadius(int radius) { m_hapticForceNeighorhoodSize = radius; }
  void setPulledVertex(int index) { m_idxPulledVertex = index; }
  bool hapticStart(int index) { m_idxPulledVertex = index; m_bHapticInProgress = true; m_vHapticIndices.clear(); return true; }
  void hapticEnd() { m_bHapticInProgress = false; m_idxPulledVertex = -1; m_vHapticIndices.clear(); m_bContactList = false; }
  bool isHapticInProgress() const { return m_bHapticInProgress; }
  // (the list set last wins: this one, or a probeMove's)
  void hapticSetCurrentForces(const std::vector<int>& indices, const std::vector<vec3d>& forces) {
    m_vHapticIndices = indices; m_vHapticForces = forces; m_bContactList = false;
  }
  // The probe's box contact (AvatarProbe::onTranslate below its pick-mode branch) as a session on the device.  probeStart: the probe's
  // mouse-down without a picked node; probeMove: the tool box [lo, hi] against the tissue -- the session's list becomes the current haptic
  // forces, spread by every timestep(), and only the info comes back; probeEnd: mouse-up, the touched set is cleared and the face stays.
  bool probeStart() { return hapticStart(0); }
  fb_fem_contact_info probeMove(const vec3d& lo, const vec3d& hi, double forceCoeff) {
    const double l[3] = {lo.x, lo.y, lo.z}, h[3] = {hi.x, hi.y, hi.z};
    const fb_fem_contact_info info = m_lpIntegrator->ContactMove(l, h, forceCoeff);
    if (info.status == FB_CONTACT_SET) { m_vHapticIndices.clear(); m_vHapticForces.clear(); m_bContactList = true; }
    return info;
  }
  void probeEnd() {
    hapticEnd();
    m_lpIntegrator->ContactReset(true);
  }
  // the materials of the body's elements (HipIntegrator::SetMaterials / SetElementMaterials): E, nu, density equally long, 1..256 entries;
  // ids one per element of the current mesh from `first` on.  syncForceModel() from the whole mesh returns the ids to 0.
  void setMaterials(const std::vector<double>& E, const std::vector<double>& nu, const std::vector<double>& density) {
    if (E.empty() || E.size() != nu.size() || E.size() != density.size()) throw std::invalid_argument("E, nu and density must be equally long and not empty");
    m_lpIntegrator->SetMaterials((int)E.size(), E.data(), nu.data(), density.data());
  }
  void setElementMaterials(const std::vector<unsigned char>& ids, int first = 0) { m_lpIntegrator->SetElementMaterials(first, (int)ids.size(), ids.data()); }
  std::vector<unsigned char> getElementMaterials() {
    std::vector<unsigned char> ids((size_t)fb_fem_num_tets(m_lpIntegrator->handle()));
    m_lpIntegrator->GetElementMaterials(0, (int)ids.size(), ids.data());
    return ids;
  }
  void setDampingStiffnessCoeff(double s) { m_dampingStiffnessCoeff = s; m_lpIntegrator->SetDampingStiffnessCoef(s); }
  double getDampingStiffnessCoeff() const { return m_dampingStiffnessCoeff; }
  void setDampingMassCoeff(double m) { m_dampingMassCoeff = m; m_lpIntegrator->SetDampingMassCoef(m); }
  double getDampingMassCoeff() const { return m_dampingMassCoeff; }
  void setGravity(bool g) { m_bApplyGravity = g; }
  bool getGravity() const { return m_bApplyGravity; }
  void setFloor(double y) { m_hasFloor = true; m_floorY = y; }  // stands in for setCollisionObject(SGNode*): the floor plane height
  // What setCollisionObject / collisionDetect do through CollisionDetection (Bullet) in the reference, for another Deformable on the same
  // device: penalty contact at the current states of both, ADDED to the external forces of both on the device (fb_fem_body_contact).  The
  // forces act in the next DoTimestep of each integrator; timestep() itself sets the external forces anew before it steps, so a caller of
  // timestep() uses setCollisionBody instead.
  fb_fem_body_contact_info collideWith(Deformable& other, double stiffness, double depthCap = 0) {
    return m_lpIntegrator->BodyContact(*other.m_lpIntegrator, stiffness, depthCap);
  }
  // Opt-in: every timestep() of this body adds the contact forces with `other` behind gravity and the probe, just before it steps
  // (nullptr: off again).  The call adds to BOTH bodies, and `other` sets its forces anew in its own timestep(): two bodies that both
  // step set each other, and each then steps with exactly one set of contact forces.  Never set: timestep() does what it always did.
  // Not owned; the caller keeps `other` alive or clears the pointer.
  void setCollisionBody(Deformable* other, double stiffness) { m_lpCollisionBody = other; m_collisionStiffness = stiffness; }
  // Friction and damping for collideWith, selfCollide and the two timestep() opt-ins of THIS body (HipIntegrator::SetContactFriction):
  // a piece rests on a stump whose cut is not level, and lands without ringing.  All zero, the default: the frictionless contact.
  void setContactFriction(double mu, double slipSpeed, double damping) { m_lpIntegrator->SetContactFriction(mu, slipSpeed, damping); }
  const fb_fem_contact_friction_info& lastContactFriction() const { return m_lpIntegrator->LastContactFriction(); }
  Deformable* getCollisionBody() const { return m_lpCollisionBody; }
  // The body against itself -- the lips of a cut in one handle, a fold: penalty contact at the current state, ADDED to the external forces
  // on the device (fb_fem_self_contact; the reference has no counterpart).  As with collideWith, a caller of timestep() opts in instead:
  fb_fem_self_contact_info selfCollide(double stiffness, double depthCap = 0, int mode = FB_SELF_CONTACT_ANY) {
    return m_lpIntegrator->SelfContact(stiffness, depthCap, mode);
  }
  // every timestep() adds the self-contact forces behind gravity, the probe and the collision body, just before it steps (on = false: off)
  void setSelfCollision(bool on, double stiffness = 0.0, double depthCap = 0.0, int mode = FB_SELF_CONTACT_OTHER_PARTS) {
    m_selfCollision = on; m_selfStiffness = stiffness; m_selfDepthCap = depthCap; m_selfMode = mode;
  }
  bool getSelfCollision() const { return m_selfCollision; }
  // A rigid tool -- spheres, capsules, oriented boxes in the world frame -- against the tissue: penalty contact at the current state,
  // ADDED to the external forces on the device (fb_fem_tool_contact; the reference has only the probe's axis-aligned box).  toolForce()
  // and toolTorque() are what the tissue returned to the tool in the last such call, the torque about tool.origin: what a haptic device
  // renders.  setContactFriction applies, with the tool's velocity and angular velocity as the other side's.
  fb_fem_tool_contact_info collideTool(const fb_tool& tool, double stiffness, double depthCap = 0, int points = FB_TOOL_SURFACE_VERTICES) {
    m_toolInfo = m_lpIntegrator->ToolContact(tool, stiffness, depthCap, points);
    return m_toolInfo;
  }
  // every timestep() applies the tool behind gravity, the probe, the collision body and the self contact, just before it steps; the
  // caller sets the tool again whenever it has moved.  clearTool: off again.  Never set: timestep() does what it always did.
  void setTool(const fb_tool& tool, double stiffness, double depthCap = 0, int points = FB_TOOL_SURFACE_VERTICES) {
    m_tool = tool; m_hasTool = true; m_toolStiffness = stiffness; m_toolDepthCap = depthCap; m_toolPoints = points;
  }
  void clearTool() { m_hasTool = false; }
  bool hasTool() const { return m_hasTool; }
  const fb_fem_tool_contact_info& lastToolContact() const { return m_toolInfo; }
  vec3d toolForce() const { return vec3d(m_toolInfo.force_on_tool[0], m_toolInfo.force_on_tool[1], m_toolInfo.force_on_tool[2]); }
  vec3d toolTorque() const { return vec3d(m_toolInfo.torque_on_tool[0], m_toolInfo.torque_on_tool[1], m_toolInfo.torque_on_tool[2]); }
  // Held and moved -- what the reference only flags (IAvatar::grip() sets m_isGripped, src/deformable/IScalpel.cpp:42-44, read at
  // AvatarRing.cpp:177; its integrator nails constrained DOFs to rest).  grip: the tool closes on `nodes` (ascending ids, e.g. pickVertices'),
  // which are held where they are.  moveGrip: they follow the tool, rotated by R (row-major) about pivot and shifted by t from where they
  // were gripped; the next timestep() takes them there in ONE step, so move a little per step.  releaseGrip: the tool opens, the nodes
  // are free again with the state they have.  gripForce: what the tissue returned to the tool during the last step, minus the sum of
  // the reactions -- what a displacement-driven haptic device is fed (fembrain_hip.h, "Constrained motion").  The held DOFs are constrained
  // in the handle, not in the fixed-vertex list of this class: setFixedVertices / syncForceModel while gripping let the tool go.
  fb_fem_motion_info grip(int n, const int* nodes) { return m_lpIntegrator->Grasp(n, nodes); }
  void moveGrip(const double R[9], const double t[3], const double pivot[3]) { m_lpIntegrator->GraspMove(R, t, pivot); }
  void releaseGrip() { m_lpIntegrator->Release(); }
  void gripForce(double force[3]) {
    m_lpIntegrator->ReadReactions(nullptr, force);
    for (int k = 0; k < 3; k++) force[k] = -force[k];
  }
  // Deformable::collisionDetect (Deformable.cpp:541-600) against the floor plane set with setFloor: vertices at or below it are
  // put back on it and their velocity reflected (the device pass timestep() also runs); true if any vertex was touched
  bool collisionDetect() {
    if (!m_hasFloor) return false;
    m_ctCollided = (U32)m_lpIntegrator->FloorCollision(m_floorY, 0.4);
    return m_ctCollided > 0;
  }
  // Deformable::statFillRecord (Deformable.cpp:225-258) without the sqlite logger: the same fields in a plain record
  struct StatRecord {
    U32 ctElements, ctVertices;
    double restVolume, totalVolume, youngModulo, poissonRatio;
    const char *xpElementType, *xpForceModel, *xpIntegrator;
    std::string xpModelName;
  };
  void statFillRecord(StatRecord& rec) {
    rec.ctElements = countCells(); rec.ctVertices = countNodes();
    (void)isVolumeChanged();  // fills the rest volume on first use
    rec.restVolume = m_restVolume; rec.totalVolume = computeVolume();
    rec.youngModulo = 0.0; rec.poissonRatio = 0.0;  // as the reference leaves them
    rec.xpElementType = "TET"; rec.xpForceModel = "COROTATIONAL LINEAR FEM"; rec.xpIntegrator = "JACOBI PRECONDITIONED CG";
    rec.xpModelName = m_strModelName;
  }
  // Stress of every element at the current state, on the device (HipIntegrator::ComputeStress): returns the summary -- the largest
  // von Mises stress and its element, the smallest J and its element, the inverted elements, the strain energy.  The per-element arrays
  // stay on the device for readStress / surfaceStress until the mesh changes (cut, syncForceModel).
  fb_fem_stress_info computeStress(bool worldFrame = false, bool keepTensors = false) {
    fb_fem_stress_info info;
    m_lpIntegrator->ComputeStress((worldFrame ? FB_STRESS_WORLD : 0) | (keepTensors ? FB_STRESS_TENSORS : 0), &info);
    return info;
  }
  // von Mises stress of every element of the last computeStress, in countCells() order
  void readStress(std::vector<double>& vonMises) {
    vonMises.assign((size_t)fb_fem_num_tets(m_lpIntegrator->handle()), 0.0);
    m_lpIntegrator->ReadStress(0, (int)vonMises.size(), vonMises.data(), nullptr, nullptr);
  }
  // the colour of the drawn surface: one float per vertex of surfaceMesh(), the mean von Mises stress behind its faces
  void surfaceStress(std::vector<float>& vonMises) { m_lpIntegrator->SurfaceStress(vonMises); }
  void resetDeformations() { m_lpIntegrator->ResetToRest(); m_vHapticForces.clear(); }
  void setDeformCallback(FOnApplyDeformations fOnDeform) { m_fOnDeform = fOnDeform; }
  double getSolverTime() const { return m_lpIntegrator->GetSystemSolveTime(); }
  // Deformable::pickVertex (Deformable.cpp:422-428): closest vertex of the displaced mesh to a world position
  // (VolMesh::findClosestVertex: d = dx dx + dy dy + dz dz on rest + q, the first of equal minima), on the device: 40 bytes come back
  int pickVertex(const vec3d& wpos, vec3d& vertex) {
    const double w[3] = {wpos.x, wpos.y, wpos.z};
    double p[3] = {0.0, 0.0, 0.0};
    const int best = m_lpIntegrator->PickVertex(w, p);
    if (best >= 0) { vertex.x = p[0]; vertex.y = p[1]; vertex.z = p[2]; }
    return best;
  }
  // Deformable::pickVertices (Deformable.cpp:430-448)
  int pickVertices(const vec3d& boxLo, const vec3d& boxHi, std::vector<vec3d>& arrFoundCoords, std::vector<int>& arrFoundIndices) {
    // on the device, ascending index order: one call with the capacity remembered from earlier picks (a probe's box holds a few dozen
    // nodes), a second one only when the box holds more than that
    const double lo[3] = {boxLo.x, boxLo.y, boxLo.z}, hi[3] = {boxHi.x, boxHi.y, boxHi.z};
    arrFoundCoords.clear();
    arrFoundIndices.resize((size_t)m_boxCapacity);
    m_boxStage.resize(3 * (size_t)m_boxCapacity);
    int n = m_lpIntegrator->PickBox(lo, hi, m_boxCapacity, arrFoundIndices.data(), m_boxStage.data());
    if (n > m_boxCapacity) {
      while (m_boxCapacity < n) m_boxCapacity *= 2;
      arrFoundIndices.resize((size_t)m_boxCapacity);
      m_boxStage.resize(3 * (size_t)m_boxCapacity);
      n = std::min(m_boxCapacity, m_lpIntegrator->PickBox(lo, hi, m_boxCapacity, arrFoundIndices.data(), m_boxStage.data()));  // (the state does not change in between)
    }
    const int got = std::max(n, 0);
    arrFoundIndices.resize((size_t)got);
    for (int i = 0; i < got; i++) arrFoundCoords.push_back(vec3d(m_boxStage[3 * (size_t)i], m_boxStage[3 * (size_t)i + 1], m_boxStage[3 * (size_t)i + 2]));
    return got;
  }
  // Deformable::hapticStart(const vec3d&) (Deformable.cpp:519-532): refuses a clamped vertex
  bool hapticStart(const vec3d& wpos) {
    vec3d vertex;
    const int idx = pickVertex(wpos, vertex);
    for (size_t i = 0; i < m_vFixedVertices.size(); i++)
      if (m_vFixedVertices[i] == idx) { m_idxPulledVertex = idx; return false; }
    return hapticStart(idx);
  }
  // Deformable::isVolumeChanged (Deformable.h:128); the rest volume is taken at the first call after a (re)build
  bool isVolumeChanged() {
    if (m_restVolume < 0.0) m_restVolume = volumeOf(std::vector<double>(m_rest.size(), 0.0));  // (the rest shape: the host's copy of it, no transfer)
    return std::abs(computeVolume() - m_restVolume) > 0.0001;
  }
  std::string getModelName() const { return m_strModelName; }
  void setModelName(const std::string& name) { m_strModelName = name; }
  U32 getDof() const { return m_dof; }
  U32 getCollidedCount() const { return m_ctCollided; }
  HipIntegrator* integrator() { return m_lpIntegrator; }
  // what getVolMesh()->countNodes() / countCells() / const_nodeAt(i).pos / const_cellAt(e).nodes give the cutting tool
  // (Cutting.cpp:96-147): the current (displaced) node positions and the element list
  U32 countNodes() const { return (U32)(m_rest.size() / 3); }
  U32 countCells() const { return (U32)(m_elements.size() / 4); }
  const std::vector<int>& cells() const { return m_elements; }
  HipIntegrator* getIntegrator() const { return m_lpIntegrator; }
  std::vector<double> currentPositions() {
    if (m_lpIntegrator) m_lpIntegrator->GetqState(m_q.data(), nullptr, nullptr);
    std::vector<double> p(m_rest);
    for (size_t i = 0; i < p.size() && i < m_q.size(); i++) p[i] += m_q[i];
    return p;
  }
  // Deformable::computeVolume (Deformable.cpp:260-279) on the current displaced positions, on the device (fb_fem_volume): 8 bytes come
  // back, or with arrStore the volume of every element too.  count must then be the DEVICE's element count (= countCells() of this class,
  // which follows every cut): anything else throws instead of leaving the array unwritten or overrunning it
  double computeVolume(double* arrStore = nullptr, U32 count = 0) {
    if (arrStore != nullptr && (int)count != fb_fem_num_tets(m_lpIntegrator->handle()))
      throw std::invalid_argument("computeVolume: arrStore holds another number of elements than the mesh has");
    return m_lpIntegrator->Volume(arrStore);
  }

 private:
  // the body of a detached part (detachPart): the integrator is adopted, mesh and fixed vertices are read from it, the settings are `from`'s
  Deformable(HipIntegrator* adopted, const Deformable& from) : m_device(from.m_device) {
    init();
    m_bApplyGravity = from.m_bApplyGravity; m_hasFloor = from.m_hasFloor; m_floorY = from.m_floorY;
    m_hapticForceNeighorhoodSize = from.m_hapticForceNeighorhoodSize; m_boxCapacity = from.m_boxCapacity;
    m_dampingMassCoeff = from.m_dampingMassCoeff; m_dampingStiffnessCoeff = from.m_dampingStiffnessCoeff; m_timeStep = from.m_timeStep;
    adopted->ReadMesh(m_rest, m_elements);
    adopted->ReadConstrainedDofs(m_vFixedDofs);
    for (size_t i = 0; i < m_vFixedDofs.size(); i++)
      if (m_vFixedVertices.empty() || m_vFixedVertices.back() != m_vFixedDofs[i] / 3) m_vFixedVertices.push_back(m_vFixedDofs[i] / 3);
    m_dof = (U32)m_rest.size();
    m_q.assign(m_dof, 0.0); m_qVel.assign(m_dof, 0.0); m_arrExtForces.assign(m_dof, 0.0);
    adopted->GetqState(m_q.data(), m_qVel.data(), nullptr);
    m_lpIntegrator = adopted;  // (last: nothing above may leave a half-made body that owns it)
  }
  void surfaceChanged();  // the surface mesh, if there is one, re-reads its topology at the next access (SurfaceMesh.h)
  void releaseEmbedded();  // deletes the embedded meshes, before the integrator they live on (EmbeddedMesh.h)
  double volumeOf(const std::vector<double>& q, double* arrStore = nullptr, U32 count = 0) const {
    const U32 m = (U32)(m_elements.size() / 4);
    const bool store = arrStore != nullptr && count == m;
    double vol = 0.0;
    for (U32 e = 0; e < m; e++) {
      double p[4][3];
      for (int k = 0; k < 4; k++)
        for (int d = 0; d < 3; d++) p[k][d] = m_rest[3 * (size_t)m_elements[4 * e + k] + d] + q[3 * (size_t)m_elements[4 * e + k] + d];
      const double u[3] = {p[0][0] - p[3][0], p[0][1] - p[3][1], p[0][2] - p[3][2]}, v[3] = {p[1][0] - p[3][0], p[1][1] - p[3][1], p[1][2] - p[3][2]},
                   w[3] = {p[2][0] - p[3][0], p[2][1] - p[3][1], p[2][2] - p[3][2]};
      const double cur = std::abs(u[0] * (v[1] * w[2] - v[2] * w[1]) + u[1] * (v[2] * w[0] - v[0] * w[2]) + u[2] * (v[0] * w[1] - v[1] * w[0])) / 6.0;
      if (store) arrStore[e] = cur;
      vol += cur;
    }
    return vol;
  }
  void init() {  // Deformable::init (Deformable.cpp:85-124)
    m_ctCollided = 0; m_fOnDeform = nullptr; m_idxPulledVertex = -1; m_bHapticInProgress = false; m_bContactList = false;
    m_dampingMassCoeff = 0.0; m_dampingStiffnessCoeff = 0.01; m_timeStep = 0.0333; m_ctTimeStep = 0;
    m_hapticForceNeighorhoodSize = 5;  // DEFAULT_FORCE_NEIGHBORHOOD_SIZE, Deformable.h:41
    m_bApplyGravity = true;  // left uninitialised by the reference's init(); true is what its .sim files set
    m_boxCapacity = 64; m_lpIntegrator = nullptr; m_lpSurface = nullptr; m_hasFloor = false; m_floorY = 0.0; m_dof = 0; m_restVolume = -1.0;
    m_lpCollisionBody = nullptr; m_collisionStiffness = 0.0;
    m_selfCollision = false; m_selfStiffness = m_selfDepthCap = 0.0; m_selfMode = FB_SELF_CONTACT_OTHER_PARTS;
    m_hasTool = false; m_toolStiffness = m_toolDepthCap = 0.0; m_toolPoints = FB_TOOL_SURFACE_VERTICES;
    memset(&m_tool, 0, sizeof(m_tool)); memset(&m_toolInfo, 0, sizeof(m_toolInfo));
  }
  std::vector<double> m_rest;
  std::vector<int> m_elements;
  std::vector<int> m_vFixedVertices, m_vFixedDofs, m_vHapticIndices, m_bptr, m_bcol;
  std::vector<vec3d> m_vHapticForces;
  std::vector<double> m_q, m_qVel, m_arrExtForces, m_hapticStage, m_boxStage;
  HipIntegrator* m_lpIntegrator;
  SurfaceMesh* m_lpSurface;
  Deformable* m_lpCollisionBody;  // setCollisionBody: not owned
  bool m_selfCollision;           // setSelfCollision
  double m_selfStiffness, m_selfDepthCap;
  int m_selfMode;
  bool m_hasTool;                 // setTool
  fb_tool m_tool;
  double m_toolStiffness, m_toolDepthCap;
  int m_toolPoints;
  fb_fem_tool_contact_info m_toolInfo;  // the last collideTool
  std::vector<EmbeddedMesh*> m_vEmbedded;
  FOnApplyDeformations m_fOnDeform;
  U32 m_dof, m_ctCollided, m_ctTimeStep;
  int m_idxPulledVertex, m_device, m_hapticForceNeighorhoodSize, m_boxCapacity;
  bool m_bHapticInProgress, m_bApplyGravity, m_hasFloor;
  bool m_bContactList;  // the list set last is the device session's (probeMove), not m_vHapticIndices
  double m_dampingMassCoeff, m_dampingStiffnessCoeff, m_timeStep, m_floorY, m_restVolume, m_collisionStiffness;
  std::string m_strModelName;
};

}  // namespace FEM
}  // namespace PS

#include "EmbeddedMesh.h"  // class EmbeddedMesh and the members of Deformable that need it (before SurfaceMesh.h: ~Deformable deletes both)
#include "SurfaceMesh.h"  // class SurfaceMesh and the members of Deformable that need it
