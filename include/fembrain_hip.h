/* fembrain_hip.h -- C ABI of libfembrain_hip.so: the MI355X (gfx950) implementation of FemBrain's per-step
 * deformable hot path (element stiffness, sparse assembly, Keff/rhs algebra, Jacobi-PCG) and of the BlobTree
 * field sweep / cell classification / tetrahedral polygonizer.
 *
 * Conventions: plain pointers and sizes, caller-owned host buffers (copied during the call), device memory
 * owned by the handle, one caller thread per handle, no exceptions across the boundary.  Every function
 * returns FB_OK (0) or a negative FB_E* code; fb_last_error() gives the text of the last failure on the
 * calling thread.  Paths cited below are relative to the reference tree's src/ directory.
 */
#ifndef FEMBRAIN_HIP_H
#define FEMBRAIN_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define FB_OK 0
#define FB_EINVAL (-1)   /* bad argument (size, index range, unsorted constrained DOFs, ...) */
#define FB_EDEVICE (-2)  /* HIP runtime error / no gfx950 device */
#define FB_ENOMEM (-3)
#define FB_ESOLVER (-4)  /* PCG did not converge (reference: printf + exit(-1), PS_VolumeConservingIntegrator.cpp:203-209) */
#define FB_ECOMM (-5)    /* RCCL not available / communicator error */

/* matrix storage precision (vectors, dot products and all per-element geometry are always fp64) */
#define FB_MATRIX_F32 0 /* north-star fp32 stiffness storage (every product, sum and vector stays fp64) */
#define FB_MATRIX_F64 1 /* reference-width storage, used by the tight parity tests */
/* default (fb_fem_default_params): by size.  fp32 where it buys speed -- from 2 SELL slices per CU on (> 16,384 nodes on 256 CUs: the
 * persistent solver's range, where a third of the matrix stays in LDS; a shard decides by the whole mesh) -- and fp64 below: a system that
 * small is solved from L2 by the two-launch iteration either way, and fp32 storage only costs it accuracy (the 204-DOF disc.1.veg, condition
 * ~1e5: 1e-2 of max|q| after three steps with fp32 values, 2e-5 with fp64).  Decided again at every re-sync.
 * FB_PCG_PERSISTENT asked for explicitly means fp32. */
#define FB_MATRIX_AUTO 2

/* PCG formulation.  Both run the Jacobi-PCG of CGSolver.cpp:129-190 with the exact-residual refresh every 30th
 * iteration.  REFERENCE performs its two reductions per iteration literally (d.q, then sum r^2/diag).  MERGED obtains
 * rho_new = rho - 2 alpha S1 + alpha^2 S2 from sums taken in the SpMV launch, so an iteration is two kernels and one
 * reduction (one RCCL all-reduce when sharded); iterates agree to rounding, checked by the parity tests. */
#define FB_PCG_MERGED 0
#define FB_PCG_REFERENCE 1
/* (value 2, an experimental one-launch-per-iteration form that measured 1.8x slower, was removed in round 3: FB_EINVAL) */
/* PERSISTENT: the whole solve inside ONE launch (fembrain_amd/csrc/pcg_pipe.hip.h): one workgroup per CU, one wavefront per SELL
 * slice, every lane keeps its row's x, r, w, z, s, p, 1/diag in registers.  The iteration is the PIPELINED form of the same
 * Jacobi-PCG (Ghysels & Vanroose 2014: the same iterates in exact arithmetic): its two sums are posted before the product and
 * read after it, so the only wait of an iteration is for the neighbouring workgroups' part of the product's input vector.
 * Every 30th iteration takes the exact residual as CGSolver.cpp:159-166 does.  Unsharded handles (sharded ones: opt-in, see
 * fb_fem_set_sharded_persist), FB_MATRIX_F32 storage, up to
 * 24 slices per CU (~2.2M tets on 256 CUs: one row per lane up to 12 slices per CU, two rows per lane with x, p, z in LDS from 13
 * on); chosen BY DEFAULT from 2 slices per CU on (FB_PCG_MERGED + FEMBRAIN_PCG_PERSIST unset).  Iteration
 * counts equal those of the literal solver within max(3, 2 %) (tests), iterates agree to rounding and are bitwise
 * reproducible however the solve is cut into launches.  If a wait inside the launch times out (FEMBRAIN_PERSIST_TIMEOUT_MS,
 * default 50, 2000 on a sharded handle; the workgroups must all be resident) the solve is repeated with the two-launch iteration and the handle stays
 * with it: fb_step_info.pcg_path = FB_PCG_PATH_FALLBACK, fb_step_info.persist_fallbacks counts (FEMBRAIN_PERSIST_STRICT=1:
 * FB_EDEVICE instead).  ACCURACY LIMIT: the pipelined recurrences stall at a relative residual of ~1e-11 on these systems (the
 * literal ones go on below 1e-12), so solves with a tolerance below 1e-8 (the reference uses 1e-6) run the two-launch solver, and
 * a persistent solve that ends at the iteration cap is checked with ONE exact residual: if the true r . r / diag of its iterate is within a
 * factor of four of what the recurrences carried, the iterate stands (-max_iter iterations, as CGSolver.cpp:189 returns); otherwise the
 * two-launch solver repeats the solve (FB_PCG_PATH_RESOLVED; FEMBRAIN_PERSIST_CAP_CHECK=0: always). */
#define FB_PCG_PERSISTENT 3
/* BLOCK_JACOBI (opt-in; NOT the reference's solver, excluded from parity): PCG with the inverse of every row's 3x3 diagonal block
 * as preconditioner instead of the inverse diagonal.  Same convergence test (on r . B^-1 r).  Unsharded handles.  Where the
 * handle is eligible for the one-row persistent kernel (fp32 matrix, 2..12 slices per CU) the solve runs inside it
 * (k_pcg_pipe<.., BJ>: the pipelined recurrences); otherwise, and below a tolerance of 1e-8, the literal two-launch sequence.
 * Measured on the 1M-tet cube, first step from rest: 1,459 instead of 1,713 iterations at the same time each. */
#define FB_PCG_BLOCK_JACOBI 4

const char* fb_last_error(void);
int fb_device_count(void);
/* name/arch of device `dev` into caller buffers (may be NULL) */
int fb_device_info(int dev, char* name, int name_len, char* arch, int arch_len, int* n_cu);
/* Page-locks caller memory (hipHostRegister) so that the state copies of a step (fb_fem_set_state / fb_fem_get_state /
 * fb_fem_set_external_forces: the q, qvel, qaccel, externalForces arrays IntegratorBase allocates, integratorBase.cpp:36-60) run
 * at PCIe speed instead of through a staging copy.  Optional; unregister before the memory is freed. */
int fb_host_register(void* p, unsigned long long bytes);
int fb_host_unregister(void* p);

/* ------------------------------------------------------------------------------------------------------
 * FEM handle.  One handle = what Deformable::syncForceModel builds (deformable/Deformable.cpp:127-220):
 * TetMesh + CorotationalLinearFEM (3rdparty/vegafem/corotationalLinearFEM/corotationalLinearFEM.cpp:40-146)
 * + consistent mass (volumetricMesh/generateMassMatrix.cpp:33-76) + the integrator state of
 * ImplicitNewmarkSparse / VolumeConservingIntegrator (integrator/implicitNewmarkSparse.cpp:39-83,
 * deformable/PS_VolumeConservingIntegrator.cpp:17-28).
 * ---------------------------------------------------------------------------------------------------- */
typedef struct fb_fem_s* fb_fem_t;

typedef struct fb_fem_params {
  double E, nu, rho;            /* Deformable.cpp:178 uses 1e7, 0.46, 1000 */
  double timestep;              /* Deformable.cpp:113: 0.0333 */
  double damping_mass;          /* Rayleigh c_M, Deformable.cpp:107: 0 */
  double damping_stiffness;     /* Rayleigh c_K, Deformable.cpp:110: 0.01 */
  double cg_eps;                /* PS_VolumeConservingIntegrator.cpp:196: 1e-6 */
  int cg_max_iter;              /* PS_VolumeConservingIntegrator.cpp:197: 10000 */
  int matrix_precision;         /* FB_MATRIX_AUTO (default) / FB_MATRIX_F32 / FB_MATRIX_F64 */
  int device;                   /* HIP device ordinal */
  int pcg_variant;              /* FB_PCG_MERGED (default) / FB_PCG_REFERENCE */
  int spmv_kernel;              /* 0 = choose by size, FB_SPMV_ROWS, FB_SPMV_SPLIT (small meshes: one slice per block) */
  int linear;                   /* non-zero: warp = 0 of CorotationalLinearFEMForceModel (corotationalLinearFEM.cpp:429-453): no rotation
                                 * extraction, K = K0 and f = K0 u.  0 = the corotational model FemBrain uses (warp = 1, its default) */
  int exact_tangent;            /* non-zero: warp = 2 (corotationalLinearFEM.cpp:296-428): the derivative of the element rotation is added
                                 * to the tangent stiffness (f_int is that of warp = 1); costs 144 stored values per element.  0 = FemBrain's */
  int integrator;               /* FB_INTEGRATOR_VOLUME_CONSERVING (0, FemBrain's VolumeConservingIntegrator::DoTimestep) or
                                 * FB_INTEGRATOR_NEWMARK (ImplicitNewmarkSparse::DoTimestep, implicitNewmarkSparse.cpp:183-379) */
  int renumber;                 /* FB_RENUMBER_AUTO (0) / FB_RENUMBER_ON / FB_RENUMBER_OFF: locality renumbering of the nodes inside the handle,
                                 * see below.  FEMBRAIN_RENUMBER=0/1 in the environment overrides */
  int expect_cuts;              /* non-zero: the caller will cut this mesh (CuttableMesh::cut, deformable/CuttableMesh.cpp:283-470: cells erased,
                                 * pieces and nodes appended) and re-sync with fb_fem_resync_delta.  The handle then (1) keeps a quarter of slack
                                 * in every buffer that grows with the mesh (an eighth otherwise) -- or room for reserve_nodes / reserve_elements --
                                 * so that a growing mesh re-allocates every few cuts, not every second one; (2) chooses its internal node order
                                 * at creation under FB_RENUMBER_AUTO (appended nodes make any caller order wide at the first cut: the full
                                 * builder would run then); (3) allocates the re-sync's workspace at creation.  The first fb_fem_resync_delta is
                                 * then as cheap as the fifth.  Unsharded handles. */
  int reserve_nodes;            /* expect_cuts: node / element counts the mesh is expected to reach (0: a quarter more than it has) */
  int reserve_elements;
} fb_fem_params;
/* Node numbering.  FemBrain appends every node a cut creates at the end of the node list (deformable/VolMesh.cpp:1086-1091,
 * 1639-1642) and its shipped tet meshes are TetGen outputs (surface vertices first): numberings in which a node's neighbours lie
 * anywhere in the list.  The handle then works in an INTERNAL slab order of its own (nodes sorted by their rest position quantised
 * to cells, longest axis of the bounding box first; fembrain_amd/csrc/renumber.h) and maps node ids on the way in and out: xyz,
 * tets, constrained DOFs, forces, state and fb_fem_pattern / the block arrays in its order all stay in the CALLER's numbering
 * (columns ascending in the caller's ids); elements keep their order.  Only the rounding of a row's sum in the SpMV changes with
 * the order of its columns.  AUTO renumbers meshes of >= 8,192 nodes whose widest element (largest id difference inside a tet)
 * exceeds min(32,767, nodes / 8) and keeps the caller's order when the slab order is not at least a quarter narrower.  On a sharded
 * handle (fb_fem_create_sharded) the renumbering needs the whole mesh on every rank, and the rank then owns a contiguous range of the
 * INTERNAL order: fb_fem_owned_range reports that range, fb_fem_owned_nodes the caller ids in it, and the state / force arrays are
 * read and written at those nodes' positions.  AUTO on a sharded handle is a collective decision taken before the build (creation
 * and every re-sync): every rank counts the ranks its elements couple it to under the caller's ranges, and the ranks switch to the
 * internal order together when some rank would have more than two neighbour ranks (or, from 8,192 nodes, most of its elements
 * reaching into another rank's range) and every rank was handed the same whole mesh (sizes and a checksum of the element list are
 * compared); ranks that were handed their own elements only keep the caller's numbering.  ON / OFF must be the same on every rank. */
#define FB_RENUMBER_AUTO 0
#define FB_RENUMBER_ON 1
#define FB_RENUMBER_OFF (-1)
#define FB_INTEGRATOR_VOLUME_CONSERVING 0
#define FB_INTEGRATOR_NEWMARK 1
#define FB_SPMV_ROWS 1
#define FB_SPMV_SPLIT 2

/* fills the reference's defaults listed above */
void fb_fem_default_params(fb_fem_params* p);

/* xyz: n_nodes*3 rest positions (fp64); tets: n_tets*4 node ids (0-based);
 * fixed_dofs: ascending, 0-based constrained DOFs (implicitNewmarkSparse.h:78-80), copied. */
int fb_fem_create(fb_fem_t* out, int n_nodes, const double* xyz, int n_tets, const int* tets,
                  int n_fixed_dofs, const int* fixed_dofs, const fb_fem_params* params);

/* Domain-decomposed variant: rank `rank` of `n_ranks` owns the contiguous node range
 * [node_splits[rank], node_splits[rank+1]) of one global mesh (node_splits has n_ranks+1 ascending entries covering
 * [0, n_nodes); NULL = equal split); it assembles every tet touching an owned node and keeps only owned rows, so no
 * force/stiffness reduction is needed.
 * Per-rank ingest: `tets` may be the whole element list (the rank filters it) or ONLY THE RANK'S OWN ELEMENTS -- every tet
 * with at least one owned node, global node ids, in ascending global element order (the order fixes the rounding of the
 * assembled sums).  Only the xyz rows of owned nodes and of nodes those elements reference are read, so a rank may back `xyz` with a sparse
 * mapping.  The plan (pattern, SELL-64, contribution lists) of the owned rows is built on the device.
 * Per PCG iteration: one halo exchange of the search direction and two fp64 scalar all-reduces over `comm`
 * (RCCL); `comm` may be NULL when n_ranks == 1. */
typedef struct fb_comm_s* fb_comm_t;
int fb_fem_create_sharded(fb_fem_t* out, int n_nodes, const double* xyz, int n_tets, const int* tets,
                          int n_fixed_dofs, const int* fixed_dofs, const fb_fem_params* params,
                          int n_ranks, int rank, const int* node_splits, fb_comm_t comm);
int fb_fem_destroy(fb_fem_t h);
/* How a sharded handle runs the two exchanges of a PCG iteration (halo refresh of the search direction, 3-scalar sum):
 *   FB_XCH_COLLECTIVE  RCCL all-reduce + send/recv (or the host-staged test communicator)
 *   FB_XCH_P2P         direct peer-to-peer inboxes over xGMI (HIP IPC), one small kernel per exchange
 *   FB_XCH_P2P_SUMS    as above, but the sums are posted by the last SpMV block and awaited by the vector pass
 *   FB_XCH_P2P_FUSED   both exchanges ride inside the two kernels of the iteration (default when every rank could map
 *                      every peer; FEMBRAIN_P2P=0 keeps the collective library, FEMBRAIN_XCH_MODE=n picks a mode)
 * All modes give bitwise identical iterates (fixed rank-order sums).  fb_fem_transport: 0 for an unsharded handle, else
 * the mode in use.  fb_fem_set_exchange_mode is COLLECTIVE: every rank switches between two solves. */
#define FB_XCH_COLLECTIVE 1
#define FB_XCH_P2P 2
#define FB_XCH_P2P_SUMS 3
#define FB_XCH_P2P_FUSED 4
int fb_fem_transport(fb_fem_t h);
int fb_fem_set_exchange_mode(fb_fem_t h, int mode);
/* The sharded persistent pipelined solver (pcg_shard_box.hip.h): one launch per solve on every rank, halo rows and rank sums crossing
 * the GPUs inside the launches, no exchange kernels or collectives on the path.  OPT-IN (FEMBRAIN_SHARDED_PERSIST=1 when the handle
 * is created; <= 22 slices per CU -- two rows per lane from 12 on -- and <= 16 ranks) and UNMEASURED on multi-GPU hardware.  fb_fem_sharded_persist: 1 when the handle's
 * solves run in it.  fb_fem_set_sharded_persist is COLLECTIVE like fb_fem_set_exchange_mode (0: the two-launch iteration with the
 * exchange mode above); FB_EINVAL when it was never attached, FB_EDEVICE after a launch has timed out (every rank fell back). */
int fb_fem_sharded_persist(fb_fem_t h);
int fb_fem_set_sharded_persist(fb_fem_t h, int on);

/* Rebuild after a topology change (Deformable::syncForceModel after CuttableMesh::cut, main.cpp:614-617):
 * same semantics as destroy + create but keeps the device, parameters and constraints. State is reset. */
int fb_fem_resync(fb_fem_t h, int n_nodes, const double* xyz, int n_tets, const int* tets,
                  int n_fixed_dofs, const int* fixed_dofs);
/* The same on a sharded handle, COLLECTIVE (every rank calls it at the same point, with the arguments fb_fem_create_sharded
 * takes: the whole mesh or the rank's own elements).  node_splits: the new node ranges; NULL keeps the handle's ranges when
 * the node count is unchanged and falls to the equal split otherwise (fb_fem_resync on a sharded handle does exactly that).
 * The exchange mode in use stays; peer-to-peer inboxes are re-attached for the new halo. */
int fb_fem_resync_sharded(fb_fem_t h, int n_nodes, const double* xyz, int n_tets, const int* tets,
                          int n_fixed_dofs, const int* fixed_dofs, const int* node_splits);

/* The same re-sync from a DESCRIPTION of the change (fembrain_amd/csrc/delta.h).  CuttableMesh::cut (CuttableMesh.cpp:283-470) erases
 * the cells its blade crosses keeping the order of the rest (VolMesh.cpp:630, m_vCells.erase), appends their pieces and the new nodes
 * (push_back, VolMesh.cpp:1083-1088) and re-points cells on a split edge in place (:1630-1650); the host passes just that:
 *   removed[n_removed]        ids (in the handle's CURRENT element list) of the elements to erase, ascending
 *   changed_ids[n_changed]    ids of elements that stay in place with new nodes, ascending, none of them removed;
 *   changed_nodes[4 n_changed]  their four node ids
 *   added_tets[4 n_added]     elements appended behind the last one
 *   new_xyz[3 n_new_nodes]    rest positions of nodes appended behind the last one (ids n_nodes, n_nodes + 1, ...)
 *   fixed_dofs                the whole constrained-DOF list of the new mesh, as fb_fem_resync takes it
 * The element list and the rest positions stay on the device; the result is the state fb_fem_resync would leave with the whole new
 * mesh (state reset).  The plan is updated from the plan (block pattern with the pairs of every block, contribution table:
 * fembrain_amd/csrc/delta.hip) instead of built and sorted again: for a handle in the caller's node order the plan is bit for bit the full rebuild's; a renumbered handle
 * (fb_fem_renumbering) puts the new nodes into its slab order under the cell size the order was made with, where a full rebuild
 * would derive a new cell size -- same pattern and values in the caller's ids, roundings of sums aside.  Otherwise (and with
 * FEMBRAIN_RESYNC_DELTA=rebuild) the full builder runs from the device copy of the new mesh.  fb_fem_resync_path: what the last
 * re-sync of the handle did.  Unsharded handles with a device-built plan only (FB_EINVAL otherwise); a bad id is refused before
 * anything changes; after a failure further in the handle is unusable until a full fb_fem_resync succeeds. */
#define FB_RESYNC_FULL 0           /* fb_fem_create / fb_fem_resync: whole mesh from the host */
#define FB_RESYNC_DELTA_MERGED 1   /* fb_fem_resync_delta: the plan updated from the plan */
#define FB_RESYNC_DELTA_REBUILT 2  /* fb_fem_resync_delta: full builder from the device copy of the mesh */
int fb_fem_resync_delta(fb_fem_t h, int n_removed, const int* removed, int n_changed, const int* changed_ids, const int* changed_nodes,
                        int n_added, const int* added_tets, int n_new_nodes, const double* new_xyz, int n_fixed_dofs, const int* fixed_dofs);
int fb_fem_resync_path(fb_fem_t h);

/* The cut itself: CuttableMesh::cut(segments, quadstrips, modifyMesh) (CuttableMesh.cpp:283-505) + cutCompleted's
 * Deformable::syncForceModel (main.cpp:614-617) in one call, on the device (fembrain_amd/csrc/subdivide.h).  strip_xyz: the blade's
 * swept quad strip, n_strip_points >= 4 and even, quad i = points 2i .. 2i+3 (degenerate quads skipped, CuttableMesh.cpp:154-164).
 * Every mesh edge an odd number of quads cross (fp64 IntersectSegmentTriangle against the current positions rest + q) is split in two
 * coincident nodes; every element on a cut edge is subdivided (case A: 4 pieces, case B: 6).  Any other cut pattern refuses the whole
 * cut and changes nothing (FB_CUT_UNHANDLED, CUT_ERR_UNHANDLED_CUT_STATE), as does modify == 0 (FB_CUT_DRY, CUT_ERR_USER_CANCELLED_CUT)
 * and a strip that cuts nothing (FB_CUT_NOTHING).  Otherwise the change -- cut elements removed keeping the order of the rest, pieces
 * and new nodes appended: fb_fem_resync_delta's contract, fed from device memory -- is applied (FB_CUT_DONE).  Where this differs from
 * the reference (edge orientation lo -> hi, node ids, prism diagonals): DESIGN.md section 7.
 *   FB_CUT_BAKE   (FemBrain: syncForceModel rebuilds from the deformed positions) the rest shape becomes x0 + q, new nodes at the split
 *                 point, state reset
 *   FB_CUT_CARRY  the rest shape is kept, a new node's rest position is at the edge fraction f = t / |current edge| of its rest edge; q,
 *                 qvel, qaccel of old nodes carried over, new nodes interpolated at f
 * State and forces after FB_CUT_DONE, on the merged and on the rebuilt re-sync path alike: BAKE leaves q, qvel and qaccel zero on every
 * node; CARRY leaves them as described; in either mode the external forces are ZERO afterwards (the vector is made anew for the new node
 * count) -- call fb_fem_set_external_forces / fb_fem_set_uniform_force again before the next step.
 * Refused with FB_EINVAL before anything changes (modify != 0; a dry run still reports the cut and its min_volume_ratio):
 *   - a piece without volume (min_volume_ratio <= 0: a split point on a node);
 *   - a piece whose volume, as a float, is below FLT_MIN (1.18e-38).  Every handle keeps the rest volumes as floats and fp32 matrix
 *     storage keeps the element records so; below FLT_MIN a float loses bits, below 1.4e-45 it is zero, and a node that lies in such
 *     pieces only would get an empty row.  (k_tet_rest works in fp64 and would accept the piece.)  The limit is on the volume the records
 *     hold, not on the ratio: a piece 1e-15 of a parent of volume 1/6 is cut.
 * A cut that is made gives the handle of the cut mesh -- what a handle created from fb_fem_read_mesh's arrays is, slivers included: thin
 * pieces cost PCG iterations (FB_ESOLVER at cg_max_iter, state unchanged), they do not harm the handle.
 * Constrained DOFs stay the handle's own (new nodes are free).  Unsharded handles with a device-built plan only (FB_EINVAL otherwise);
 * a failure after the change began leaves the handle unusable until a full fb_fem_resync, as fb_fem_resync_delta does. */
#define FB_CUT_BAKE 0
#define FB_CUT_CARRY 1
#define FB_CUT_NOTHING 0    /* no edge cut: nothing changed */
#define FB_CUT_DONE 1       /* the mesh was cut and the handle re-synced */
#define FB_CUT_UNHANDLED 2  /* a cut element is neither case A nor case B: nothing changed */
#define FB_CUT_DRY 3        /* modify == 0: the cut was worked out (fb_fem_read_cut) but nothing changed */
typedef struct fb_cut_result {
  int status;             /* FB_CUT_* */
  int n_quads;            /* usable quads of the strip */
  int n_cut_edges;        /* unique cut edges (0 unless status is DONE or DRY) */
  int n_case_a, n_case_b; /* cut elements of case A / B */
  int n_unhandled;        /* cut elements of neither case */
  int n_removed, n_added, n_new_nodes;  /* the delta (0 unless DONE or DRY) */
  double min_volume_ratio;  /* smallest piece volume / parent volume in the new rest shape (0 unless DONE or DRY) */
} fb_cut_result;
int fb_fem_cut(fb_fem_t h, int n_strip_points, const double* strip_xyz, int mode, int modify, fb_cut_result* out);
/* The last fb_fem_cut's change in fb_fem_resync_delta's form (also after a dry run): removed[n_removed], added_tets[4 n_added],
 * new_xyz[3 n_new_nodes] (rest positions); per new node the cut edge it lies on (edge_nodes[2 n_new_nodes]: lo, hi caller ids) and
 * its fraction from lo (edge_frac[n_new_nodes]); the first min(n_unhandled, 64) unhandled element ids (ascending) and their 6-bit edge
 * codes (bit e: local edge (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)).  Any pointer may be NULL.  FB_EINVAL when no cut has run. */
int fb_fem_read_cut(fb_fem_t h, int* removed, int* added_tets, double* new_xyz, int* edge_nodes, double* edge_frac, int* unhandled_ids, int* unhandled_codes);
/* The device-resident mesh in the caller's numbering: rest_xyz[3 fb_fem_num_nodes], tets[4 fb_fem_num_tets] (either may be NULL).
 * Unsharded handles only. */
int fb_fem_read_mesh(fb_fem_t h, double* rest_xyz, int* tets);

/* ---- The surface of the simulated (and cut) mesh, on the device ----
 * What a host draws a deformable through in the reference: the boundary triangles of the tet mesh
 * (SurfaceMesh::setupFromTetMesh, src/deformable/SurfaceMesh.cpp:141-213), their current positions and box
 * (applyDisplacements + updateAABB, :338-373) and a normal per node (VolMeshRender::sync, src/deformable/VolMeshRender.cpp:74-112).
 * Unsharded handles only (where fb_fem_read_mesh works), device- or host-built plan alike.  A handle that never asks allocates and
 * launches nothing.
 *
 * Faces (SurfaceMesh.cpp:155-207): for every element in element order det = (v1-v0).((v2-v0)x(v3-v0)) on the fp64 rest positions;
 * det >= 0 gives the local faces (1,2,3) (2,0,3) (3,0,1) (1,0,2), otherwise (3,2,1) (3,0,2) (1,0,3) (2,0,1) (:180-190).  A face whose
 * sorted vertex triple occurs an odd number of times survives with the vertex order of its LAST occurrence (what insert / erase /
 * insert on the reference's std::set leaves, :168-178), and the faces are listed in ascending order of the sorted triple (:200-207).
 * Node ids are the CALLER's, also on a renumbered handle.  face_tets (not in the reference): the element of that last occurrence.
 * vertex_ids: the ascending caller ids of the nodes some face uses -- the reference keeps every tet vertex in the surface mesh
 * (:147-148); faces index node ids as its m_faces do, and vertex_ids is the compact list a vertex buffer is filled from.
 *
 * The handle counts mesh generations: creation, fb_fem_resync, fb_fem_resync_delta and a fb_fem_cut that returns FB_CUT_DONE make the
 * topology stale; a step, a state change and a cut that changes nothing do not.  fb_fem_surface builds only when stale (n_builds counts
 * the builds of this handle) and fills the box from the rest positions; fb_fem_surface_update builds first if it must. */
typedef struct fb_fem_surface_info {
  int n_faces, n_vertices, n_builds;
  float aabb_lo[3], aabb_hi[3];
} fb_fem_surface_info;
int fb_fem_surface(fb_fem_t h, fb_fem_surface_info* out);
/* faces[3 n_faces], vertex_ids[n_vertices], face_tets[n_faces] of the current topology (built first if stale); any pointer may be NULL */
int fb_fem_read_surface(fb_fem_t h, int* faces, int* vertex_ids, int* face_tets);
/* The current state of the surface vertices, in vertex_ids' order: xyz[3 n_vertices] = (float)(x0 + q) (fp64 add, one rounding;
 * SurfaceMesh.cpp:338-352), normals[3 n_vertices] = (float) of the normalised fp64 sum, in ascending face order, of the fp64 unit
 * normals (p1-p0)x(p2-p0)/|..| of the node's faces at the current positions (VolMeshRender.cpp:74-112; a sum of length 0 gives
 * (0,0,0), a face without area adds nothing).  The reference's flip towards the camera (VolMeshRender.cpp:83-91) is not reproduced:
 * the faces are wound outward already.  out->aabb_lo/hi: min / max of xyz (SurfaceMesh.cpp:354-373).  Pointers may be NULL.  One copy
 * of 24 n_vertices + 24 bytes leaves the device. */
int fb_fem_surface_update(fb_fem_t h, float* xyz, float* normals, fb_fem_surface_info* out);
/* Device time of `reps` forced builds and of `reps` updates (HIP events on the handle's stream around each; the medians).  Either
 * pointer may be NULL.  The build's figure includes its two host waits. */
int fb_fem_time_surface(fb_fem_t h, int reps, double* seconds_build, double* seconds_update);

/* ---- Embedded point sets: what is drawn instead of the boundary triangles ----
 * The reference draws a finer mesh than the tets (the marching-cubes surface, an organ mesh) and moves it with them through
 * Deformable::setDeformCallback; the binding is VolumetricMesh::generateInterpolationWeights with TetMesh::computeBarycentricWeights
 * (src/3rdparty/vegafem/volumetricMesh/volumetricMesh.cpp:971-1134, tetMesh.cpp:233-305), a linear scan of all elements per point.  Here
 * a set of points, optionally with triangles, is bound on the device through a uniform grid over the rest box, and its current
 * positions, normals and box come out of x0 + q there.  Unsharded handles only (FB_EINVAL otherwise).  A handle that never embeds
 * allocates and launches nothing.
 *
 * Binding, in fp64 on the handle's rest positions: w_i = D_i / D_0, D_0 = TetMesh::getTetDeterminant of the element's four vertices, D_i
 * the same with vertex i replaced by the point.  An element contains the point when all four w_i >= 0; the point binds to the
 * lowest-numbered containing element.  A point no element contains is EXTERNAL: it binds to the element whose centre (the mean of the
 * four vertices) is closest, distance sqrt(dx^2 + dy^2 + dz^2) compared with < in ascending element order; its weights are still
 * D_i / D_0, some negative.  zero_threshold > 0: a point farther than that from every vertex of its element gets four zero weights
 * (counted in n_zeroed; its vertices are still the element's -- the reference leaves them uninitialised).  Elements are numbered as
 * in fb_fem_read_mesh, node ids are the CALLER's, also on a renumbered handle.  A point on a face, an edge or a node shared by several
 * elements is in each of them up to rounding: which of those the device picks may differ from a CPU evaluation of the same rule.
 *
 * Up to 8 embeddings live on a handle; id is a slot number and a released slot is reused.  FB_EINVAL before anything is uploaded:
 * n_points <= 0, a coordinate that is not finite, a triangle index outside [0, n_points), an id without an embedding, a ninth embedding.
 *
 * Mesh changes.  Each point keeps its location in the handle's CURRENT rest shape (fb_fem_read_embedding's rest_xyz: the point as given,
 * later sum w_i x0_i); that is what any later search looks for.
 *  - A change of the mesh in place -- a fb_fem_cut that returns FB_CUT_DONE, fb_fem_resync_delta, fb_fem_detach_part with
 *    FB_DETACH_REMOVE -- is applied to every embedding in the same call.  A point in a kept element gets the element's new number and
 *    keeps its weights bit for bit.  A point in an element a cut subdivided is bound again among that parent's pieces: its location is
 *    sum w_i x0_i over the parent's nodes in the rest shape after the cut, the lowest-numbered piece that contains it wins, else the piece
 *    with the closest centre, and the weights are that piece's, new nodes included (a point whose weights were zeroed keeps four zeros and
 *    its location).  A point in any other removed or changed element becomes an ORPHAN.  FB_CUT_BAKE moves the rest shape under every
 *    point, so rest_xyz is refreshed for all (zeroed points excepted).  A point outside the body stays with the element it has.
 *  - fb_fem_resync (a new mesh) orphans every point; rest_xyz stands as it was.
 *  - Orphans are searched again by the rule above, in the mesh the handle then holds, when the embedding is next read or updated.  The
 *    grid is built once per mesh generation and only if somebody needs it.  n_locates counts the searches; n_rebound the points that cuts
 *    re-bound, orphans that were searched, and points a search after fb_fem_resync moved to an element with another number.
 *  - fb_fem_split_parts keeps elements and weights (rest_xyz of the moved points is not refreshed).
 *  - An orphan has no binding to refresh rest_xyz through: if a FB_CUT_BAKE cut or fb_fem_split_parts moves the rest shape before the
 *    orphan has been searched (no read or update in between), it is searched where it stood in the OLD rest shape.  Read or update the
 *    embedding between such changes.
 * fb_fem_detach_part does not copy embeddings to the new handle.
 *
 * Points outside.  A surface drawn AROUND the body (a skin over coarser tets, a cage) has half or all of its points external.  Their
 * closest centre is found by one of two passes that give the same binding bit for bit: SCAN tests every centre of the mesh for every
 * such point; RING looks, one wavefront per point, only at the cells of a grid of the centres that could hold a closer one (built once
 * per mesh generation, on the first search that takes this path), and hands a point that has tested more than a budget of centres -- one
 * that sees much of the mesh at about its closest distance -- to the scan.  A search chooses by itself: RING when the centre grid of this
 * mesh generation exists already or the search has at least 8,192 external points, else SCAN.  FEMBRAIN_EMBED_CLOSEST=scan|ring forces a
 * path and FEMBRAIN_EMBED_RING_BUDGET=n sets the budget (default max(64, n_tets / 32)); both are read at every search. */
#define FB_EMBED_CLOSEST_NONE 0 /* the last search had no external point */
#define FB_EMBED_CLOSEST_SCAN 1
#define FB_EMBED_CLOSEST_RING 2
typedef struct fb_fem_embed_search_info {
  int path;                  /* FB_EMBED_CLOSEST_*: the external pass of the last search of this embedding */
  int n_outside;             /* points that search sent to the external pass */
  int n_far;                 /* ... of them, those the scan finished (SCAN: all of them) */
  int centre_grid_builds;    /* centre grids built since the handle was made */
  int max_centres_one_point; /* the most centres one point tested in that search (SCAN: n_tets; RING: in the ring pass, where a far
                                point's count ends past the budget) */
  long long centres_tested;  /* all centres tested in that search: SCAN n_outside * n_tets; RING the ring pass plus n_far * n_tets */
} fb_fem_embed_search_info;
typedef struct fb_fem_embed_params { double zero_threshold; /* <= 0: off */ } fb_fem_embed_params;
typedef struct fb_fem_embed_info {
  int id, n_points, n_triangles;
  int n_external, n_zeroed;
  int n_locates;      /* full searches run for this embedding */
  int n_rebound;      /* points that changed element through mesh changes since creation */
  int grid[3], n_wide;/* the search grid; elements kept in the overflow list (their box covers more than 64 cells) */
  float aabb_lo[3], aabb_hi[3];
} fb_fem_embed_info;
/* xyz[3 n_points] in the handle's rest frame; triangles[3 n_triangles] index the points (n_triangles may be 0); p may be NULL.  out (may
 * be NULL): the counts, and the box of the bound points in the rest shape. */
int fb_fem_embed(fb_fem_t h, int n_points, const double* xyz, int n_triangles, const int* triangles, const fb_fem_embed_params* p, int* id, fb_fem_embed_info* out);
/* (fb_fem_embed_from_poly, the same from a polygonizer's surface on the device, stands beside fb_fem_create_from_poly below) */
/* elements[n], vertices4[4 n] (caller ids), weights4[4 n], rest_xyz[3 n]; any pointer may be NULL */
int fb_fem_read_embedding(fb_fem_t h, int id, int* elements, int* vertices4, double* weights4, double* rest_xyz);
/* The current state of the points: xyz[3 n] = (float) of the fp64 sum ((w0 p0 + w1 p1) + w2 p2) + w3 p3 with p_i = x0_i + q_i;
 * normals[3 n] by fb_fem_surface_update's rule over the embedding's own triangles at those fp64 positions (zero where a point has no
 * triangle); out->aabb_lo/hi: min / max of xyz.  Pointers may be NULL.  One copy of 24 n + 24 bytes leaves the device. */
int fb_fem_embed_update(fb_fem_t h, int id, float* xyz, float* normals, fb_fem_embed_info* out);
int fb_fem_embed_release(fb_fem_t h, int id);
/* Medians of `reps` HIP-event timings of a full search (grid build, every point, the external pass; host waits included) and of an
 * update with its copy.  Either pointer may be NULL.  The search runs on a scratch copy of the points' rest_xyz: the binding, its counts
 * and n_locates are left as they are. */
int fb_fem_time_embed(fb_fem_t h, int id, int reps, double* seconds_locate, double* seconds_update);
/* ... the search by phase: seconds3[0] the grid build (with its two host waits), [1] the search of every point through the grid and the
 * overflow list with the compaction of the points without an element (and the host wait for their number), [2] the external pass
 * (closest centre), the weights and the counts.  Each the median of `reps`; fb_fem_time_embed's seconds_locate is their sum. */
int fb_fem_time_embed_search(fb_fem_t h, int id, int reps, double seconds3[3]);
/* What the external pass of embedding id's last search did (points that wait for a search are searched first).  FB_EINVAL for an id
 * without an embedding. */
int fb_fem_embed_search_info_get(fb_fem_t h, int id, fb_fem_embed_search_info* out);
/* Medians of `reps` HIP-event timings of the external pass alone, for this embedding's external points, with path FB_EMBED_CLOSEST_SCAN or
 * _RING: seconds2[0] the centre grid's build (0 for SCAN), seconds2[1] the pass (RING: with its host wait and the scan of its far points).
 * On a scratch copy, like fb_fem_time_embed_search: the binding, its counts, n_locates, the search info and whether the handle has a
 * centre grid are left as they are.  In fb_fem_time_embed_search a centre grid's build, when the search makes one, belongs to [2]. */
int fb_fem_time_embed_closest(fb_fem_t h, int id, int reps, int path, double seconds2[2]);

/* ---- The way back: touching, picking and colouring what an embedding draws ----
 * fb_fem_embed sends data outward, from the tets to the drawn points.  These calls go the other way, on the device, so that a host which
 * draws an embedding can push on it, click on it and colour it without reading the binding back (52 bytes per point), scattering on the
 * host and uploading a 3*n_nodes force vector per touch.  The reference has neither: its probe talks to nodes, and its drawn surface only
 * receives Deformable::setDeformCallback.  Unsharded handles only (FB_EINVAL otherwise); ids are the caller's, also on a renumbered
 * handle; points that wait for a search (after fb_fem_resync, orphans of a change in place) are searched first, as fb_fem_embed_update
 * does.  A handle that never calls these allocates and launches nothing extra.
 *
 * fb_fem_embed_add_forces is the transpose of the embedding, ADDED into the current external force vector (set gravity or zero first).
 * With the binding fb_fem_read_embedding returns, the result is bit for bit this loop:
 *     for s = 0 .. n-1 (p = point_ids[s], strictly ascending), k = 0 .. 3 (v = vertices4[4 p + k]), c = 0 .. 2:
 *         fext[3 v + c] = fext[3 v + c] + weights4[4 p + k] * forces3[3 s + c]
 * one fp64 multiply and one fp64 add per addition, the value fext holds being the start of each node's sequential sum.  point_ids NULL:
 * every point (n must be n_points, forces3 is [3 n_points]).  External points and points with zeroed weights take part with the weights
 * they have.  n == 0 is a no-op.  FB_EINVAL before anything is launched or changed: an id outside [0, n_points), a list that is not
 * strictly ascending, NULL forces3 with n > 0, a force that is not finite, an id without a live embedding.  Mechanism: the 4 n_points
 * corners are sorted once, stably, by node (the transposed table); a wavefront per node that has corners forms the products of 64 corners
 * at a time and adds them in order.  No floating-point atomics, one path for short and long lists: the same bits from call to call.  The
 * table is built by the first call and kept until the binding changes (a search, a change of the mesh in place, a release); the time of
 * a dense add is bounded below by the node with the most corners (longest_run sequential additions). */
int fb_fem_embed_add_forces(fb_fem_t h, int id, int n, const int* point_ids, const double* forces3);
/* Of embedding id: transposed tables built since its creation; of the last of them the most corners of one node and the nodes that have
 * a corner (zeros before the first fb_fem_embed_add_forces).  Any pointer may be NULL. */
int fb_fem_embed_forces_info(fb_fem_t h, int id, int* n_table_builds, int* longest_run, int* n_nodes_touched);
/* The nearest hit of the ray origin + t dir, 0 <= t <= t_max (dir need not be a unit vector; t_max may be INFINITY), on the embedding's
 * triangles at the current state: the fp64 positions fb_fem_embed_update forms, recomputed here.  Per triangle (a, b, c) Moeller-Trumbore
 * in fp64 with e1 = b - a, e2 = c - a: P = dir x e2, det = e1 . P (a triangle with det == 0 is skipped; both sides are hit), T = origin - a,
 * u = (T . P) / det, Q = T x e1, v = (dir . Q) / det, t = (e2 . Q) / det; a hit when u >= 0, v >= 0, u + v <= 1 and 0 <= t <= t_max.  Of all hits
 * the smallest t, of equal t the lowest triangle.  *triangle = -1 (and FB_OK) for a miss or an embedding without triangles; bary = (u, v),
 * the hit is (1-u-v) a + u b + v c; xyz = origin + t dir.  Output pointers may be NULL.  FB_EINVAL: a zero or non-finite dir, a
 * non-finite origin, t_max not a number.  One copy of 56 bytes leaves the device. */
int fb_fem_embed_pick_ray(fb_fem_t h, int id, const double origin[3], const double dir[3], double t_max, int* triangle, double* t, double bary[2], double xyz[3]);
/* fb_fem_pick_vertex over the embedded points at the current state: the point with the smallest d = dx*dx + dy*dy + dz*dz, of equal d
 * the lowest id; xyz its fp64 position.  Output pointers may be NULL.  One copy of 56 bytes leaves the device. */
int fb_fem_embed_pick_point(fb_fem_t h, int id, const double wpos[3], int* index, double xyz[3], double* dist2);
/* per_point[n_points]: (float) of the von Mises stress of the element each point is bound to, from the last fb_fem_stress.  FB_EINVAL
 * when there is no stress of the current mesh, by fb_fem_surface_stress's rule.  One copy of 4 n_points bytes leaves the device. */
int fb_fem_embed_stress(fb_fem_t h, int id, float* per_point);

/* ---- Disjoint parts of the (cut) mesh, on the device ----
 * What the reference does after every completed cut: VolMesh::get_disjoint_parts (src/deformable/VolMesh.cpp:915-965) counts the parts,
 * CuttableMesh::splitParts (src/deformable/CuttableMesh.cpp:553-626) pushes the parts on either side of the swept quad apart, and
 * convertDisjointPartsToMeshes (:628-698) makes a mesh of each.  Unsharded handles only (FB_EINVAL otherwise), device- or host-built plan
 * alike.  A handle that never asks allocates and launches nothing.
 *
 * Two elements are adjacent exactly when they share a face (an equal sorted triple of node ids); an edge or a node in common does not
 * connect, and a face that three or more elements carry connects all of them.  Parts are numbered in ascending order of their smallest
 * element id (the order get_disjoint_parts produces).  Elements are in fb_fem_read_mesh's order, node ids are the CALLER's, also on a
 * renumbered handle.
 * Staleness as for the surface: creation, fb_fem_resync, fb_fem_resync_delta and a fb_fem_cut that returns FB_CUT_DONE make the labels
 * stale; a step, a state change, a cut that changes nothing and fb_fem_split_parts do not.  Every call below labels first when stale
 * (n_builds counts the labellings of this handle). */
typedef struct fb_fem_parts_info {
  int n_parts;          /* face-connected components of the element list */
  int n_builds;         /* labellings this handle has run */
  int largest_part;     /* index of the part with the most elements (lowest index of equals) */
  int n_shared_nodes;   /* nodes used by elements of more than one part (parts touching at a node or an edge only) */
  int n_unused_nodes;   /* nodes no element uses */
} fb_fem_parts_info;
int fb_fem_parts(fb_fem_t h, fb_fem_parts_info* out);
/* element_part[fb_fem_num_tets]; node_part[fb_fem_num_nodes]: the lowest part whose elements use the node, -1 for a node no element
 * uses; per part: part_elements[n_parts], part_nodes[n_parts] (nodes the part uses: a shared node counts in each of its parts),
 * part_first_element[n_parts] (its smallest element id), part_volume[n_parts] (the sum of the rest volumes |det| / 6 of its elements in
 * fp64, in a fixed order that depends on the element counts alone: the same bits from call to call; within part_elements[k] 2^-52
 * relative of any other order of summation).  Any pointer may be NULL. */
int fb_fem_read_parts(fb_fem_t h, int* element_part, int* node_part, int* part_elements, int* part_nodes, int* part_first_element, double* part_volume);
/* CuttableMesh::splitParts(sweptquad, dist) on the REST positions.  n = normalised (q1 - q0) x (q2 - q0), c = the mean of the four
 * points; an element is in front when dot(centroid(x0 + q) - c, n) > 0 (the centroid: a quarter of the sum of its four current
 * positions, fp64).  A part whose elements are all in front is a front part, one with none in front a back part, every other part
 * straddles and is left alone.  Every node a front part uses gets + shift, every node a back part uses - shift (shift = n * dist, computed
 * once and returned), a node of both gets both and stays: one fp64 add per coordinate.  The reference moves `pos`, which its
 * syncForceModel bakes into the rest shape; after a FB_CUT_BAKE cut q is zero and the two coincide.
 * q, qvel, qaccel and the external forces are untouched; the element rest data are made again as by fb_fem_rebuild_elements; surface and
 * stress become stale; the labels stay valid (part_volume is summed again).  Later re-syncs and cuts start from the moved positions.
 * A handle that works in an internal node order (fb_fem_renumbering) derived that order from the old positions: it is built again from its
 * own mesh on the device, in the order a handle created from fb_fem_read_mesh's arrays would get, with q, qvel, qaccel and the external
 * forces carried across -- the cost of a full fb_fem_resync_delta rebuild, once per split; fb_fem_resync_path then reports
 * FB_RESYNC_DELTA_REBUILT.  (Such a handle always has a device-built plan: a host-built plan keeps the caller's order.)  Should that
 * rebuild fail, the positions have moved already and the handle is unusable until a full fb_fem_resync, as after any failed re-sync.
 * FB_EINVAL with nothing changed: a quad whose first three points span no plane, a coordinate or a dist that is not finite. */
typedef struct fb_fem_split_info {
  int n_front_parts, n_back_parts, n_straddling_parts;
  int n_nodes_moved;       /* nodes whose rest position changed */
  double shift[3];         /* the unit normal times dist: what was added to front nodes and subtracted from back nodes */
} fb_fem_split_info;
int fb_fem_split_parts(fb_fem_t h, const double quad_xyz[12], double dist, fb_fem_split_info* out);
/* One part as a mesh of its own (one iteration of convertDisjointPartsToMeshes' loop; nothing is deleted from the handle):
 * element_ids[part_elements[part]] ascending; node_ids[part_nodes[part]] the caller ids of its nodes in order of first use when those
 * elements are walked in ascending order, corners 0..3 (the order the reference's mapNodes assigns); rest_xyz[3 part_nodes] their rest
 * positions; tets_local[4 part_elements] the elements in that local numbering.  Pointers may be NULL.  Only the part's arrays leave the
 * device.  FB_EINVAL for a part outside [0, n_parts). */
int fb_fem_read_part(fb_fem_t h, int part, int* element_ids, int* node_ids, double* rest_xyz, int* tets_local);
/* Device time of `reps` forced labellings (host waits included) and of `reps` splits (HIP events on the handle's stream around each;
 * the medians).  The timed split runs a split's device work -- classification against the plane x = 0, node marks, the pass over the
 * nodes, the element rest data, the volumes -- with a zero shift and without its stores: nothing moves.  Either pointer may be NULL. */
int fb_fem_time_parts(fb_fem_t h, int reps, double* seconds_label, double* seconds_split);

/* ---- A part detached into a handle of its own, on the device ----
 * What convertDisjointPartsToMeshes (src/deformable/CuttableMesh.cpp:628-698) does with every part: the part becomes a body of its own,
 * and (FB_DETACH_REMOVE) its cells are erased from the original.  *out is a new handle on h's device, with a stream of its own, whose mesh
 * is exactly fb_fem_read_part(h, part, ...)'s arrays -- element order, nodes in order of first use, local ids, fp64 rest positions --
 * built by the device plan builder from the device copy; the piece decides its own node order and matrix width as any new handle does.
 * It inherits: h's current fb_fem_params (expect_cuts included: it can be cut again) with the timestep, damping, CG and Newmark settings
 * and the internal-force scaling set since creation; q, qvel, (qaccel on a Newmark handle) and the external forces of its nodes; the
 * material table, and -- where h has an element map -- the ids of its elements (a handle without a map gives a piece without one); every
 * constrained DOF of h on a node the part uses, ascending in the piece's ids (fb_fem_read_constrained_dofs).  A node that several parts
 * share is a node of each piece.  Only counts and the constrained-DOF list cross the bus.
 * element_ids / node_ids (either may be NULL): the arrays fb_fem_read_part returns.
 * FB_DETACH_REMOVE: afterwards the part's elements are erased from h as by fb_fem_resync_delta(removed = element_ids): the order of the
 * rest is kept, the node count does not change (the part's own nodes stay as nodes no element uses: identity rows), q, qvel, qaccel and the
 * external forces are carried, the element map follows; labels, surface and stress become stale.  fb_fem_resync_path(h) reports the path.
 * The piece is built first.  If anything fails before the removal begins the piece is destroyed, h is untouched and *out is NULL; a
 * failure inside the removal leaves h unusable like any failed delta re-sync, and the piece is destroyed as well.
 * FB_EINVAL before anything changes: a sharded handle, a host-built plan, a part outside [0, n_parts), out NULL, unknown flags,
 * FB_DETACH_REMOVE on a handle with one part (a handle cannot be left without elements). */
#define FB_DETACH_KEEP   0  /* the parent is left as it is */
#define FB_DETACH_REMOVE 1  /* the part's elements are erased from the parent */
typedef struct fb_fem_detach_info {
  int part, n_elements, n_nodes;   /* of the piece */
  int n_fixed_dofs;                /* constrained DOFs the piece inherited */
  int n_materials;                 /* entries of the material table it inherited (1: no map) */
  int parent_elements_left;        /* fb_fem_num_tets(parent) afterwards */
  int parent_resync_path;          /* FB_RESYNC_* of the parent's removal, -1 with KEEP */
} fb_fem_detach_info;
int fb_fem_detach_part(fb_fem_t h, int part, int flags, fb_fem_t* out, int* element_ids, int* node_ids, fb_fem_detach_info* info);
/* The constrained DOFs of an unsharded handle in the caller's ids, ascending: what fb_fem_create, the last re-sync or
 * fb_fem_set_constrained_dofs set, what a cut keeps, what a detached piece inherited -- "the whole constrained-DOF list" that
 * fb_fem_resync_delta takes.  FB_EINVAL for a sharded handle (-1 from the count). */
int fb_fem_num_constrained_dofs(fb_fem_t h);
int fb_fem_read_constrained_dofs(fb_fem_t h, int* dofs);


/* Per-element rest-state rebuild on the device (M^-1 rows / volume, corotationalLinearFEM.cpp:66-90 and
 * tetMesh.cpp:184-188) -- the per-step "K0 rebuild" of BASELINE config 4. */
int fb_fem_rebuild_elements(fb_fem_t h);

/* IntegratorBase::SetExternalForces / AddExternalForces / SetExternalForcesToZero (integratorBase.cpp:84-103);
 * f has 3*n_nodes entries (global numbering; a sharded handle reads its owned range). */
int fb_fem_set_external_forces(fb_fem_t h, const double* f);
int fb_fem_add_external_forces(fb_fem_t h, const double* f);
int fb_fem_set_external_forces_zero(fb_fem_t h);
/* The external force vector the next step will read -- whatever the calls above, fb_fem_set_uniform_force, fb_fem_add_haptic_forces and
 * fb_fem_embed_add_forces have left in it -- as 3*n_nodes doubles in the caller's node order (a sharded handle fills its owned range,
 * as fb_fem_get_state does). */
int fb_fem_get_external_forces(fb_fem_t h, double* f);
/* constant force on one axis of every node, generated on the device: axis 1, value -10000 is the gravity
 * load of Deformable::timestep (Deformable.cpp:331-338) */
int fb_fem_set_uniform_force(fb_fem_t h, int axis, double value);

typedef struct fb_step_info {
  int cg_iterations;      /* |return value| of CGSolver::SolveLinearSystemWithJacobiPreconditioner (CGSolver.cpp:189) */
  int converged;          /* 1 / 0 */
  double assembly_seconds;/* IntegratorBaseSparse::GetForceAssemblyTime (integratorBaseSparse.h:66), hipEvent-timed */
  double solve_seconds;   /* IntegratorBaseSparse::GetSystemSolveTime (integratorBaseSparse.h:67) */
  double rho0, rho;       /* initial / final sum r^2 / diag */
  int pcg_path;           /* FB_PCG_PATH_*: which solver form ran the (last) solve of this step */
  int persist_fallbacks;  /* solves of this handle so far that a timed-out persistent launch handed to the two-launch form */
  int newton_iterations;  /* FB_INTEGRATOR_NEWMARK: linear solves of this step (implicitNewmarkSparse.cpp:201-379, numIter); 1 otherwise */
} fb_step_info;
#define FB_PCG_PATH_TWO_LAUNCH 0  /* k_spmv + k_cg_fused per iteration (or the literal / block-Jacobi sequences) */
#define FB_PCG_PATH_PERSISTENT 1  /* the persistent launch (FB_PCG_PERSISTENT) */
#define FB_PCG_PATH_FALLBACK 2    /* a persistent launch timed out; the solve was repeated with the two-launch form */
#define FB_PCG_PATH_RESOLVED 3    /* the persistent solve reached the iteration cap; repeated by the two-launch solver, whose result stands */

/* VolumeConservingIntegrator::DoTimestep (PS_VolumeConservingIntegrator.cpp:46-260): assembly, Keff/rhs, PCG,
 * state update.  Returns FB_OK, or FB_ESOLVER when PCG hit cg_max_iter (state is then left unchanged). */
int fb_fem_step(fb_fem_t h, fb_step_info* info);

/* IntegratorBase::GetqState / SetqState / ResetToRest (integratorBase.cpp:105-131); any pointer may be NULL.
 * Arrays are 3*n_nodes long, global numbering; a sharded handle fills / reads only its owned range. */
int fb_fem_get_state(fb_fem_t h, double* q, double* qvel, double* qaccel);
int fb_fem_set_state(fb_fem_t h, const double* q, const double* qvel, const double* qaccel);
int fb_fem_reset(fb_fem_t h);
int fb_fem_set_timestep(fb_fem_t h, double timestep);
int fb_fem_set_damping(fb_fem_t h, double damping_mass, double damping_stiffness);
/* IntegratorBase::SetInternalForceScalingFactor (integratorBase.h; default 1): internal forces and tangent stiffness
 * are multiplied by `factor` from the next assembly on (both are linear in Young's modulus, which is what is scaled) */
int fb_fem_set_internal_force_scaling(fb_fem_t h, double factor);

/* ---- Per-element materials ----
 * The reference reads every element's own material (corotationalLinearFEM.cpp:55-66: getElementMaterial(el); tetMesh.cpp:171 and
 * generateMassMatrix.cpp: getElementDensity(el)).  A handle has a TABLE of 1..256 materials and, once one was set, a MAP of one id
 * byte per element, in the caller's element order (the node renumbering does not reorder elements).  Entry 0 is the material of
 * every element without an id; a fresh handle has the one-entry table of its fb_fem_params.  Unsharded handles only: a sharded
 * handle that is given more than one material, or a map, refuses.
 *
 * fb_fem_set_materials replaces the table.  Accepted is what VolumetricMesh's parser accepts (volumetricMesh.cpp:327): E > 0,
 * -1 < nu < 0.5, rho > 0, all finite; a table that would shrink to or below an id in use is refused (the handle keeps an upper bound
 * of the ids it was given, reset by fb_fem_resync).  With n_materials = 1 on a handle without a map it replaces the handle's E, nu,
 * rho and nothing else.  fb_fem_set_internal_force_scaling scales every material's E.
 * fb_fem_set_element_materials sets the ids of elements [first, first + count); an id >= fb_fem_num_materials or a bad range is refused.
 * The ids are checked on the host before they reach the device.  Every refusal is FB_EINVAL and leaves the handle as it was.
 * fb_fem_read_materials fills arrays of fb_fem_num_materials entries (any may be NULL); fb_fem_read_element_materials reads ids back
 * (zeros from a handle without a map).
 *
 * The map follows the mesh: fb_fem_resync returns every id to 0 and keeps the table; fb_fem_resync_delta drops the removed elements,
 * keeps the ids of kept and changed ones in order and gives appended ones 0 until the caller sets them; after fb_fem_cut (FB_CUT_DONE,
 * either mode) every piece has the id of the element it was cut from -- on the device, nothing crosses the bus.
 * A handle that never gets a non-zero id allocates no map and launches the kernels it always launched; fb_fem_element_map_bytes says
 * how many bytes the map holds (0: none).  A map whose ids all name a material equal to material 0 reproduces that handle bit for bit. */
int fb_fem_set_materials(fb_fem_t h, int n_materials, const double* E, const double* nu, const double* rho);
int fb_fem_num_materials(fb_fem_t h);
int fb_fem_read_materials(fb_fem_t h, double* E, double* nu, double* rho);
int fb_fem_set_element_materials(fb_fem_t h, int first, int count, const unsigned char* ids);
int fb_fem_read_element_materials(fb_fem_t h, int first, int count, unsigned char* ids);
long long fb_fem_element_map_bytes(fb_fem_t h);

int fb_fem_set_cg(fb_fem_t h, double eps, int max_iter);
/* Newmark parameters (implicitNewmarkSparse.h: NewmarkBeta 0.25, NewmarkGamma 0.5; IntegratorBase: maxIterations 1, epsilon
 * 1e-6): the Newton loop stops when |residual|^2 / |first residual|^2 < epsilon^2 or after max_newton_iterations.  Each Newton
 * iteration is one assembly + one PCG solve that -- as in the reference -- starts from the previous solution.  The residual is summed
 * over ALL DOFs, the reaction forces at the clamped ones included (implicitNewmarkSparse.cpp:258-262; rounds 2-4 summed the free DOFs
 * only).  Unsharded handles only for more than one iteration (the quotient is a global sum). */
int fb_fem_set_newmark(fb_fem_t h, double beta, double gamma, int max_newton_iterations, double epsilon);
/* IntegratorBaseSparse::setConstrainedDOF (integratorBaseSparse.cpp:73-87) -- takes effect at the next step
 * (the mask is applied when Keff is formed, so unlike the reference no stale systemMatrix can survive) */
int fb_fem_set_constrained_dofs(fb_fem_t h, int n_fixed_dofs, const int* fixed_dofs);

/* Floor-plane collision + velocity rewrite of Deformable::timestep (Deformable.cpp:350-402), on the device:
 * v <- v_t - restitution * v_n for every node (n = +y), q_y clamped so rest_y + q_y >= floor_y.
 * n_collided (may be NULL) counts nodes with rest_y + q_y <= floor_y before the clamp. */
int fb_fem_floor_collision(fb_fem_t h, double floor_y, double restitution, int* n_collided);

/* ---- The haptic probe, on the device ----
 * What FemBrain's AvatarProbe drives every frame while the user touches the tissue: Deformable::applyHapticForces
 * (src/deformable/Deformable.cpp:634-706), pickVertex / pickVertices (:422-448) and computeVolume (:260-279).  The probe's own
 * contact logic (its box faces, its vertex hash) is the next section's, fb_fem_contact_move.  Unsharded handles only (FB_EINVAL otherwise, as
 * fb_fem_read_mesh), device- or host-built plan alike; node ids are the CALLER's, also on a renumbered handle.  A handle that never
 * calls these allocates and launches nothing extra.
 *
 * fb_fem_add_haptic_forces ADDS into the current external force vector (set gravity or zero first, as Deformable::timestep does):
 * first forces3[3 s .. 3 s + 2] to node_ids[s] for s ascending (duplicate ids allowed); then for every source s ascending, to every node
 * first reached in ring j = 1 .. size-1 of a breadth-first walk from it, mag_j * forces3[s] with mag_j = 1.0 * (size - j) / (double)size.
 * Neighbours are the nodes sharing an element.  Each addition is one fp64 multiply and one fp64 add in that order per node: the
 * result is bit for bit the host walk's.  n == 0 is a no-op; neighbourhood_size outside [1, 255], a null pointer with n > 0,
 * n > FB_HAPTIC_MAX_SOURCES or an id outside [0, n_nodes) return FB_EINVAL before anything is launched or changed.  The walk is
 * (size - 1) passes over the element list per batch of 32 sources, so the cost grows with both: a caller with more sources than
 * FB_HAPTIC_MAX_SOURCES spreads on the host and uses fb_fem_set_external_forces. */
#define FB_HAPTIC_MAX_SOURCES 256
int fb_fem_add_haptic_forces(fb_fem_t h, int n, const int* node_ids, const double* forces3, int neighbourhood_size);
/* VolMesh::findClosestVertex: the node with the smallest d = dx*dx + dy*dy + dz*dz, (dx, dy, dz) = (x0 + q) - wpos in fp64; of equal d
 * the lowest id.  index, xyz (its current position) and dist2 may each be NULL.  One copy of 40 bytes leaves the device. */
int fb_fem_pick_vertex(fb_fem_t h, const double wpos[3], int* index, double xyz[3], double* dist2);
/* Deformable::pickVertices: the nodes with lo <= x0 + q <= hi on all three axes (inclusive), ascending ids in ids[] and their positions
 * in xyz[3 ..].  *n_found is the full count also when it exceeds capacity; only the first min(count, capacity) entries are written.
 * capacity == 0 (ids and xyz may then be NULL) returns the count only. */
int fb_fem_pick_box(fb_fem_t h, const double lo[3], const double hi[3], int capacity, int* ids, double* xyz, int* n_found);
/* Deformable::computeVolume: per element |u . (v x w)| / 6, u, v, w = p0 - p3, p1 - p3, p2 - p3 on x0 + q, evaluated as
 * u0 (v1 w2 - v2 w1) + u1 (v2 w0 - v0 w2) + u2 (v0 w1 - v1 w0).  per_element[fb_fem_num_tets] (may be NULL) is in fb_fem_read_mesh's
 * element order.  *total is their sum in a fixed tree that depends on the element count only (256 consecutive elements per leaf group):
 * the same bits from call to call, within n_tets * 2^-53 * total of any other order. */
int fb_fem_volume(fb_fem_t h, double* total, double* per_element);

/* ---- The probe's box contact, on the device ----
 * AvatarProbe::onTranslate (src/deformable/AvatarProbe.cpp:124-265) below its pick-mode branch -- the path FemBrain runs every frame while
 * the tool presses into tissue -- as a session kept on the device, and Deformable::applyHapticForces on the list it stores, for any
 * number of sources.  Unsharded handles only (FB_EINVAL otherwise), device- or host-built plan alike; node ids are the CALLER's, also
 * on a renumbered handle.  A handle that never calls these allocates and launches nothing extra.
 *
 * fb_fem_contact_move(lo, hi, coeff), every operation fp64 in the order written:
 *  1. Miss test.  The tissue box is the min / max over all nodes of (float)(x0 + q) (VolMesh::displace -> computeNodalAABB; the expand(1.0)
 *     of Deformable::syncForceModel is NOT reproduced: a tool within 1.0 of the tissue that the reference would let through is a miss
 *     here), the tool box (float)lo, (float)hi.  AABB::intersect is strict: a miss on any axis with t_lo >= hi or t_hi <= lo.  Status
 *     FB_CONTACT_MISS: the touched set, the face and the force list are unchanged.
 *  2. Touched set.  Every node with lo <= x0 + q <= hi on all three axes (fb_fem_pick_box's rule, in doubles) enters the set with its
 *     current position unless it is in it: a node keeps its first position, and never leaves on a move.  A set that is still empty:
 *     FB_CONTACT_EMPTY, nothing else changes.
 *  3. Face.  With s = {lo, hi, lo, hi, lo, hi} and n = {-x, +x, -y, +y, -z, +z} (LEFT RIGHT BOTTOM TOP NEAR FAR), d(k, j) = (s_j - p_k) . n_j
 *     on the first-touch positions p_k.  While face < 0: the face is the j of the smallest d over the nodes ascending, then the faces
 *     ascending (strict <: the first of equal minima wins); contact_dist is that d, closest_node / closest_point that node and its
 *     first-touch position.  Otherwise the face stays, and contact_dist / closest_* are the minimum over the nodes ascending for it alone.
 *  4. Force list.  One entry per touched node, ascending id: n_face * max(d(k, face) * force_coeff, 0); n_pushing counts the entries
 *     greater than zero.  The list replaces the stored one and stays on the device: FB_CONTACT_SET.  Only the info struct comes back.
 * After a MISS or EMPTY move the info keeps the last SET move's fields except status and n_new = 0.  A null lo or hi, lo[k] > hi[k], a
 * non-finite box or coefficient: FB_EINVAL before anything is launched or changed.
 *
 * fb_fem_contact_reset clears the touched set and the list; keep_face != 0 keeps the face (the reference's mouse-up, m_hashVertices.clear():
 * it never resets its face after the constructor), keep_face == 0 is a new probe.  fb_fem_read_contact: the touched set of the stored list,
 * ascending ids[list_size], their first-touch positions first_xyz[3 list_size] and forces3[3 list_size]; any pointer may be NULL.
 *
 * fb_fem_contact_apply ADDS the stored list into the current external force vector as fb_fem_add_haptic_forces adds a list (set gravity or
 * zero first): each force to its own node, then for the sources ascending mag_j * f_s to every node first reached in ring j = 1 .. size-1,
 * every node receiving its additions in ascending source order, one fp64 multiply and one fp64 add per component -- the values of the host
 * walk (the sign of a zero apart: zero forces are skipped).  No limit on the sources.  path says how: FB_CONTACT_SPREAD_RECORDS -- a
 * wavefront per source walks its ball over the node adjacency and emits (target, source, ring) records, sorted and added per target
 * (n_records of them, n_targets nodes) -- or, where a ball overflows its table or the records a budget, FB_CONTACT_SPREAD_LEVELS for the
 * whole apply: fb_fem_add_haptic_forces' passes in batches of 32 sources, slow, the same numbers (n_targets -1; n_records what the walk
 * counted, -1 if it did not finish).  n_sources is the list's length.  size outside [1, 255]: FB_EINVAL; an empty list: a no-op.
 *
 * The session is kept in the caller's numbering and survives steps, state changes, fb_fem_reset, fb_fem_cut and fb_fem_resync_delta (ids
 * stay valid; appended nodes are untouched until a move finds them; the spread uses the current mesh's adjacency).  A full fb_fem_resync
 * clears it (n_clears counts that); a detached part's handle starts without one. */
#define FB_CONTACT_MISS  0   /* the boxes do not intersect: nothing changed */
#define FB_CONTACT_EMPTY 1   /* they intersect, the touched set is (still) empty: nothing changed */
#define FB_CONTACT_SET   2   /* the force list was replaced */
typedef struct fb_fem_contact_info {
  int status, n_touched, n_new, face /* -1, or 0..5 = LEFT RIGHT BOTTOM TOP NEAR FAR */, closest_node /* caller id or -1 */, n_pushing, list_size, n_clears;
  double contact_dist, closest_point[3];
} fb_fem_contact_info;
int fb_fem_contact_move(fb_fem_t h, const double lo[3], const double hi[3], double force_coeff, fb_fem_contact_info* out);
int fb_fem_contact_info_get(fb_fem_t h, fb_fem_contact_info* out);   /* the state without a move (all zero / -1 on a fresh handle) */
int fb_fem_contact_reset(fb_fem_t h, int keep_face);
int fb_fem_read_contact(fb_fem_t h, int* ids, double* first_xyz, double* forces3);
#define FB_CONTACT_SPREAD_RECORDS 0
#define FB_CONTACT_SPREAD_LEVELS  1
typedef struct fb_fem_contact_spread_info { int n_sources, n_pushing, path, n_targets; long long n_records; } fb_fem_contact_spread_info;
int fb_fem_contact_apply(fb_fem_t h, int neighbourhood_size, fb_fem_contact_spread_info* out);

/* ---- Contact between two bodies, on the device ----
 * What Deformable::setCollisionObject / collisionDetect ask of CollisionDetection (Bullet) in the reference: two handles in one process
 * -- a parent and the piece fb_fem_detach_part made of it, or any two -- push each other apart.  Both unsharded and on the same device
 * (FB_EINVAL otherwise); node, element and face ids are the CALLER's (fb_fem_read_mesh, fb_fem_read_surface), also on renumbered handles.
 * The call uses the current states of both and ADDS penalty forces into both external force vectors, as fb_fem_add_haptic_forces and
 * fb_fem_contact_apply do (set gravity or zero first).  It is ordered by events after what both handles have queued, and what either
 * queues afterwards runs after it.  A handle that never calls it allocates and launches nothing extra.
 *
 * Direction "a into b" (FB_BODY_A_INTO_B; FB_BODY_B_INTO_A is the same with the roles swapped), every operation fp64, no contraction:
 *  1. Points: the surface vertices of a (fb_fem_surface's vertex_ids, ascending) at p = x0 + q.  A position of either body that is not
 *     finite, a NaN included, gives FB_EINVAL before anything is written.
 *  2. Candidates: the points in the closed box of b's current node positions.  Where the box of a's surface vertices and the box of b's
 *     nodes do not meet the direction ends: no grid is built, no force vector written.
 *  3. Containment: p is in contact if an element of b at b's current positions has four weights >= 0 (fb_fem_embed's weights D_i / D_0,
 *     no threshold); the lowest-numbered such element is recorded.
 *  4. Closest boundary point: over ALL boundary faces of b (fb_fem_read_surface's, at current positions) the closest point c of a face to
 *     p by the region-based closest point on a triangle (Ericson, Real-Time Collision Detection 5.1.5: vertex A, vertex B, edge AB,
 *     vertex C, edge AC, edge BC, interior, in that order, dot(u, v) = (u0 v0 + u1 v1) + u2 v2), d = sqrt(dx dx + dy dy + dz dz).  The
 *     least d wins, of bitwise equal d the lowest face.
 *  5. Force: d == 0 is counted as degenerate and pushes nothing.  Else n = (c - p) / d, depth = depth_cap > 0 ? min(d, depth_cap) : d,
 *     F = (stiffness * depth) * n.  +F goes to the node of p in a, (-F) * b_k to corner k of the face in b, with b1, b2 from the
 *     closest-point routine and b0 = (1 - b1) - b2.
 *  6. A node receives its contributions onto the value the force vector had, a into b before b into a, inside a direction by ascending
 *     surface vertex, inside a contact corners 0, 1, 2.  No floating-point atomics: two calls from one state give the same bits.
 *
 * path says how the closest faces of the last direction that had contacts were found: FB_BODY_CONTACT_RING -- through a grid of the
 * face centroids, a wavefront per contact, only the cells that can hold a closer face -- or FB_BODY_CONTACT_SCAN, every face for every
 * contact; the same bits.  FEMBRAIN_BODY_CONTACT=scan|ring chooses (read at every call; default: ring wherever its coverage proof holds,
 * see face_search.hip.h), FEMBRAIN_BODY_CONTACT_BUDGET the faces one point may test on the ring path before it goes to the scan (default:
 * the face count).  n_tet_grid_builds / n_face_grid_builds: grids built by this call; faces_tested: closest-point evaluations of the
 * searches; max_depth: the largest depth that entered a force (after the cap); force_on_a / force_on_b: the fp64 sums of all
 * contributions to each body, in the order of 6.  Indices [0] / [1] of the counts: a into b / b into a.
 *
 * fb_fem_read_body_contact(a, direction): the last call's contacts of ONE direction (n_contacts[..] entries each, any pointer may be NULL):
 * node of the point, containing element, closest face, closest point [3], weights b0 b1 b2 [3], and depth = d before the cap.
 * fb_fem_time_body_contact: seconds of the five stages (boxes | element grid and containment | face grid | closest faces | scatter),
 * means of `reps` runs, host waits included; it adds no force. */
#define FB_BODY_A_INTO_B 1
#define FB_BODY_B_INTO_A 2
#define FB_BODY_CONTACT_NONE 0
#define FB_BODY_CONTACT_SCAN 1
#define FB_BODY_CONTACT_RING 2
typedef struct fb_fem_body_contact_params { double stiffness, depth_cap; int directions /* FB_BODY_A_INTO_B | FB_BODY_B_INTO_A */; int reserved; } fb_fem_body_contact_params;
typedef struct fb_fem_body_contact_info {
  int n_candidates[2], n_contacts[2], n_degenerate[2]; int path; int n_tet_grid_builds, n_face_grid_builds;
  long long faces_tested; double max_depth; double force_on_a[3], force_on_b[3];
} fb_fem_body_contact_info;
int fb_fem_body_contact(fb_fem_t a, fb_fem_t b, const fb_fem_body_contact_params* p, fb_fem_body_contact_info* out);
int fb_fem_read_body_contact(fb_fem_t a, int direction, int* node, int* element, int* face, double* closest_xyz, double* bary3, double* depth);
int fb_fem_time_body_contact(fb_fem_t a, fb_fem_t b, const fb_fem_body_contact_params* p, int reps, double seconds[5]);

/* ---- Contact of a body with itself, on the device ----
 * fb_fem_cut leaves both halves of a cut in one handle and fb_fem_split_parts opens it: one mesh that can pass through itself.  So can a
 * body that was never cut, a beam folded onto itself.  fb_fem_body_contact needs two handles (and refuses a == b); this call is the
 * contact of ONE handle with itself.  The reference has no counterpart (its Deformable collides with one Bullet object and its floor):
 * the rule is this project's.  Unsharded handles only (FB_EINVAL otherwise); node, element and face ids are the CALLER's
 * (fb_fem_read_mesh, fb_fem_read_surface), also on renumbered handles.  The call uses the current state and ADDS penalty forces into
 * the external force vector (set gravity or zero first), on the handle's stream.  A handle that never calls it allocates and launches
 * nothing extra.  Every operation fp64, in the order written, no contraction:
 *  1. Points: the surface vertices of h (fb_fem_surface's vertex_ids, ascending) at p = x0 + q.  A position of the body that is not
 *     finite gives FB_EINVAL before anything is written.
 *  2. Exclusion, for the point on node n.  FB_SELF_CONTACT_ANY: every element that has n among its four nodes and every boundary face
 *     that has n among its three.  FB_SELF_CONTACT_OTHER_PARTS: every element whose part equals part(n) and every boundary face whose
 *     element (fb_fem_read_surface's face_tets) is in that part; part(n) is fb_fem_read_parts' node_part, the lowest part using the node
 *     (the labels are built first where they are stale: n_parts_builds).  A mesh of one part has no contacts under OTHER_PARTS: no grid is
 *     built, the force vector is not written.
 *  3. Containment: p is in contact if some element that is not excluded has, at the current positions, four weights >= 0 (fb_fem_embed's
 *     weights D_i / D_0, no threshold: the function fb_fem_body_contact evaluates); the lowest-numbered such element is recorded.
 *  4. Closest boundary point: over all boundary faces that are not excluded, at current positions, the closest point c of a face to p
 *     and d = |c - p| exactly as step 4 of "Contact between two bodies" forms them.  The least d wins, of bitwise equal d the lowest
 *     face.  A contact for which no face is left is dropped and not counted.
 *  5. Force: d == 0 is counted in n_degenerate and pushes nothing.  Else n = (c - p) / d, depth = depth_cap > 0 ? min(d, depth_cap) : d,
 *     F = (stiffness * depth) * n, b0 = (1 - b1) - b2.
 *  6. Scatter into the one external force vector.  Contact i, by ascending surface vertex, makes four records: 4i is +F on the point's
 *     node, 4i + 1..3 are (-F) * b_k on corner k of the face.  A node -- it may be a point of one contact and a corner of others --
 *     receives its records in ascending record index onto the value the vector had.  No floating-point atomics: two calls from one
 *     state give the same bits.  force_on_points / force_on_faces are the fp64 sums of the +F and of the corner records in record order.
 *
 * Right after a cut the twin nodes of the lips coincide bit for bit (FB_CUT_BAKE and FB_CUT_CARRY alike).  Whatever rounding decides
 * about their containment, their closest face is at d == 0: a body that has just been cut receives NO force from this call; only a lip
 * pressed into the other does.
 * FB_SELF_CONTACT_ANY is correct while the penetration is shallower than the distance from the vertex to the nearest face of its own
 * side that does not touch it -- about half a cell.  Beyond that a face of its own side can win.  (The cut beam of the tests, pressed in
 * by 0.31 of a cell: the largest depth is 0.0275 under ANY and 0.0309 under OTHER_PARTS, by the numpy restatement of the rule.)
 * OTHER_PARTS is the mode for the halves of a cut, ANY the mode for a fold of one part.
 *
 * path, faces_tested, max_depth as in fb_fem_body_contact_info (FB_BODY_CONTACT_NONE | _SCAN | _RING); FEMBRAIN_SELF_CONTACT=scan|ring
 * and FEMBRAIN_SELF_CONTACT_BUDGET=n are this call's knobs, read at every call (default: the ring wherever its coverage proof holds,
 * face_search.hip.h).  n_points: the surface vertices; n_point_grid_builds / n_face_grid_builds / n_parts_builds: built by this call.
 * fb_fem_read_self_contact: the last adding call's contacts (n_contacts entries each, any pointer may be NULL) in the layout of
 * fb_fem_read_body_contact; depth = d before the cap.  fb_fem_time_self_contact: seconds of the five stages (positions and box | point
 * grid and containment | face grid | closest faces | scatter), means of `reps` runs, host waits included; it adds no force. */
#define FB_SELF_CONTACT_ANY         0  /* exclusion by incidence */
#define FB_SELF_CONTACT_OTHER_PARTS 1  /* exclusion by part (fb_fem_parts' labels, built first if stale) */
typedef struct fb_fem_self_contact_params { double stiffness, depth_cap; int mode, reserved; } fb_fem_self_contact_params;
typedef struct fb_fem_self_contact_info {
  int n_points, n_contacts, n_degenerate, path /* FB_BODY_CONTACT_NONE | _SCAN | _RING */;
  int n_point_grid_builds, n_face_grid_builds, n_parts_builds;
  long long faces_tested; double max_depth; double force_on_points[3], force_on_faces[3];
} fb_fem_self_contact_info;
int fb_fem_self_contact(fb_fem_t h, const fb_fem_self_contact_params* p, fb_fem_self_contact_info* out);
int fb_fem_read_self_contact(fb_fem_t h, int* node, int* element, int* face, double* closest_xyz, double* bary3, double* depth);
int fb_fem_time_self_contact(fb_fem_t h, const fb_fem_self_contact_params* p, int reps, double seconds[5]);

/* ---- Friction and damping of a contact, on the device ----
 * fb_fem_body_contact and fb_fem_self_contact push along the normal with stiffness * depth and nothing else: a piece glides off a stump
 * whose cut is not level and rings on the penalty spring.  The two calls below are those calls with a force law that also uses the
 * velocity of the point relative to the face: regularised Coulomb friction and a damper along the normal.  The reference has no
 * counterpart; the rule is this project's (tests/frictionref.py restates it in numpy).  The frictionless calls, their
 * kernels and their bits are untouched, and a handle that never calls the new entry points allocates and launches nothing for them.
 *
 * Steps 1-4 of "Contact between two bodies" -- for the self call, steps 1-4 of "Contact of a body with itself", exclusions and dropped
 * contacts included -- are unchanged.  Step 5 is replaced.  The contact has the point on node i of body P at p and the closest point c
 * on face (j0, j1, j2) of body T with weights b0 = (1 - b1) - b2, b1, b2, and d = |c - p|.  d == 0 is degenerate as before: counted in
 * n_degenerate, nothing pushed.  Otherwise, with vP and vT the velocities (qvel) of the two handles as fb_fem_get_state would return them
 * at the moment of the call (one array for the self call), every operation fp64, in the order written, no contraction:
 *     n_k   = (c_k - p_k) / d
 *     depth = depth_cap > 0 ? min(d, depth_cap) : d
 *     sd    = stiffness * depth
 *     vf_k  = (b0 * vT[j0][k] + b1 * vT[j1][k]) + b2 * vT[j2][k]
 *     w_k   = vP[i][k] - vf_k
 *     vn    = (w_0 n_0 + w_1 n_1) + w_2 n_2
 *     N     = sd - damping * vn;   if !(N > 0) N = 0              (no adhesion)
 *     t_k   = w_k - vn * n_k
 *     s     = sqrt((t_0 t_0 + t_1 t_1) + t_2 t_2)
 *     g     = (mu * N) / max(s, slip_speed)                        (0 where max(s, slip_speed) == 0, which needs mu == 0)
 *     f_k   = g * t_k
 *     F_k   = N * n_k - f_k
 * Regularised Coulomb: the friction grows linearly with the slip below slip_speed and has |f| = mu N at and above it.  +F goes to node
 * i and (-F) * b_k to corner k through the scatter of the frictionless call (step 6 there: own-node addition and sorted corner records,
 * a into b before b into a; the four records 4i .. 4i + 3 of the self call).  With mu == 0 and damping == 0 the rule gives the bits of
 * the frictionless step 5.  A contact is classed by the first of these that holds: SEPARATING, N == 0 (it has d > 0, is still a contact,
 * still comes back from the read calls, and receives a zero force); STICKING, s < slip_speed; SLIDING, anything else.
 *
 * The law is EXPLICIT, like the penalty force: the step that follows sees forces formed from the velocities before it.  Below slip_speed
 * the friction is a damper of rate mu N / slip_speed on the tangential velocity, and `damping` is one on the normal velocity; an explicit
 * damper of rate r on a mass m reverses the velocity it acts on when r dt > m.  The caller keeps
 *     mu * N / slip_speed * dt   below the mass a contact pushes, and
 *     damping * dt               below the same mass.
 * (A 27 kg block resting under 384 N on its contacts with mu = 0.5 and dt = 0.01: slip_speed >= 0.5 * 384 * 0.01 / 27 = 0.071.)
 * max_stick_rate is the largest mu * N / slip_speed of the call (0 where slip_speed == 0), so the first bound can be checked without
 * reading anything back.
 *
 * `out` is filled exactly as the frictionless call fills it: force_on_* are the sums of the contributions actually added, so they hold
 * F with friction; max_depth as before.  fout: the classes per direction ([0] / [1]: a into b / b into a; the self call uses [0]); the
 * largest s, N and mu N / slip_speed over the contacts that are not degenerate; friction_on_points, per direction the fp64 sum of (-f)
 * over its contacts by ascending surface vertex.  They are formed on the host, in record order.
 * fb_fem_read_body_contact_friction / fb_fem_read_self_contact_friction: per contact of the last friction call, in the order of
 * fb_fem_read_body_contact / fb_fem_read_self_contact, N, t[3] and -f[3] (zero for a degenerate contact); any pointer may be NULL.
 * fb_fem_read_body_contact / fb_fem_read_self_contact serve the geometry of whichever call ran last, with or without friction.
 * FB_EINVAL before anything is launched or written: a null fr; mu, slip_speed or damping negative or not finite; mu > 0 with
 * slip_speed == 0; a non-zero reserved; everything the frictionless call refuses.  A velocity of either body that is not finite gives
 * FB_EINVAL before any force vector is written (a pass over qvel raises a flag that is read in the host wait for the boxes).
 * Stream and event ordering is the frictionless calls': b's qvel is read under the event that covers b's q. */
typedef struct fb_fem_contact_friction_params { double mu, slip_speed, damping, reserved; } fb_fem_contact_friction_params;
typedef struct fb_fem_contact_friction_info {
  int n_sticking[2], n_sliding[2], n_separating[2];     /* [0] / [1]: a into b / b into a; self contact uses [0] */
  double max_slip_speed, max_normal_force, max_stick_rate;
  double friction_on_points[2][3];                      /* per direction: the fp64 sum of (-f) over its contacts, ascending surface vertex */
} fb_fem_contact_friction_info;
int fb_fem_body_contact_friction(fb_fem_t a, fb_fem_t b, const fb_fem_body_contact_params* p, const fb_fem_contact_friction_params* fr,
                                 fb_fem_body_contact_info* out, fb_fem_contact_friction_info* fout);
int fb_fem_read_body_contact_friction(fb_fem_t a, int direction, double* normal_force, double* slip3, double* friction3);
int fb_fem_self_contact_friction(fb_fem_t h, const fb_fem_self_contact_params* p, const fb_fem_contact_friction_params* fr,
                                 fb_fem_self_contact_info* out, fb_fem_contact_friction_info* fout);
int fb_fem_read_self_contact_friction(fb_fem_t h, double* normal_force, double* slip3, double* friction3);

/* ---- Contact with a rigid tool, on the device ----
 * What a rigid instrument does to the tissue: a tool made of up to FB_TOOL_MAX_SHAPES spheres, capsules and oriented boxes -- the shapes
 * of fembrain_amd/erosion.py, with its inside tests -- pushes every point it holds out along the shape's normal, and the call hands back
 * the force and the torque the tissue returns to the tool.  The reference has only the axis-aligned probe box (fb_fem_contact_move); the
 * rule is this project's (tests/toolref.py restates it in numpy).  Unsharded handles only (FB_EINVAL otherwise); ids are
 * the CALLER's, also on renumbered handles.  The call uses the current state and ADDS into the external force vector (set gravity or
 * zero first), on the handle's stream.  A handle that never calls it allocates and launches nothing for it.  Every operation fp64, in
 * the order written, no contraction; dot(u, v) = (u0 v0 + u1 v1) + u2 v2:
 *  1. Points: FB_TOOL_SURFACE_VERTICES, fb_fem_surface's vertex_ids, ascending (the surface is built first where it is stale);
 *     FB_TOOL_ALL_NODES, every node, ascending.  A point sits at p = x0 + q.
 *  2. Per shape, whether it holds the point, the depth and the outward normal n:
 *     sphere (a, r): u = p - a, l2 = dot(u, u); held iff l2 <= r * r; l = sqrt(l2), depth = r - l, n = u / l; l == 0 is held with
 *       depth = r and is DEGENERATE (no normal);
 *     capsule (a, b, r): d = b - a, dd = dot(d, d), t = dd > 0 ? min(max(dot(p - a, d) / dd, 0), 1) : 0, c = a + t * d (a multiply,
 *       then an add); then the sphere rule about c;
 *     box (a, half, R): u = p - a, l_i = dot(row i of R, u); held iff |l_i| <= half_i for i = 0, 1, 2; e_i = half_i - |l_i|, the axis
 *       of the least e wins, the lowest i among equal ones; depth = e_i, n = row i of R, negated iff l_i < 0.  R is used as given.
 *  3. Of the shapes that hold the point the greatest depth wins, the lowest shape index among equal ones.  A point held by no shape is
 *     no contact.  A degenerate winner makes the contact degenerate: counted in n_contacts, contacts_by_shape and n_degenerate, it
 *     pushes nothing and enters no sum, maximum or class.  Nothing is culled.  Contacts are ordered by ascending point.
 *  4. Force: depth' = depth_cap > 0 ? min(depth, depth_cap) : depth, sd = stiffness * depth'.  Without fr, F_k = sd * n_k.  With fr:
 *     r = p - origin, vt = velocity + omega x r with the cross product written (w1 r2 - w2 r1, w2 r0 - w0 r2, w0 r1 - w1 r0),
 *     w_k = qvel[node][k] - vt_k, and from there the lines vn ... F_k of "Friction and damping of a contact" with this n and sd; the
 *     classes are its classes.  With mu == 0 and damping == 0 the force vector gets the bits of the frictionless call wherever the
 *     entry before the call is not -0: a record component that is -0 without fr (sd * n_k, n_k a negated zero of a box's row) is +0
 *     from N * n_k - 0 * t_k, the records agree as numbers, and only -0 + (-0) against -0 + (+0) shows the sign in the vector.
 *  5. +F is added to the node's entry of the external force vector, onto the value it had (the points are distinct nodes: no atomics,
 *     the same bits from call to call).  The host forms, in record order over the contacts that are not degenerate, force_on_body =
 *     sum F, force_on_tool = sum (-F), torque_on_tool = sum r x (-F) about origin (the cross product as above), max_depth (of depth'),
 *     and with fr the classes and maxima as fb_fem_contact_friction_info defines them (all zero without fr).
 * FB_EINVAL before anything is launched or written: a null tool or p; n_shapes outside 1 .. FB_TOOL_MAX_SHAPES; an unknown kind or
 * `points`; a non-zero reserved; a radius or half extent that is negative or not finite; any other number of the tool that the rule
 * reads (a; b of a capsule; R of a box; origin, velocity, omega) that is not finite; a box with |dot(R_i, R_j) - delta_ij| > 1e-9;
 * a stiffness or depth_cap that is negative or not finite; what the friction calls refuse in fr.  FB_EINVAL with the force vector
 * untouched: a position of a point that is not finite, and with fr a velocity of a point (the first kernel raises a flag that is read in
 * the host wait for the number of contacts; forces are added after it).  A refused call leaves the records of the last call in place.
 * fb_fem_read_tool_contact: per contact of the last adding call (n_contacts entries each, any pointer may be NULL) the node, the
 * winning shape, depth before the cap, n, F; and N, t[3], -f[3] of the friction law (zero after a frictionless call or for a degenerate
 * contact); fb_fem_num_tool_contacts is that number of entries, for a reader that did not make the call.  fb_fem_time_tool_contact: seconds of the three stages (points against shapes | compaction and the host wait | forces and
 * the records' way back), means of `reps` runs; it adds no force and leaves the records alone. */
#define FB_TOOL_SPHERE 0
#define FB_TOOL_CAPSULE 1
#define FB_TOOL_BOX 2
#define FB_TOOL_MAX_SHAPES 16
#define FB_TOOL_SURFACE_VERTICES 0
#define FB_TOOL_ALL_NODES 1
typedef struct fb_tool_shape { int kind, reserved; double a[3], b[3], size[3], R[9]; } fb_tool_shape;
    /* sphere: centre a, radius size[0] | capsule: a, b, radius size[0] | box: centre a, half extents size, row i of R = axis i */
typedef struct fb_tool { int n_shapes, reserved; fb_tool_shape shapes[FB_TOOL_MAX_SHAPES];
                         double origin[3], velocity[3], omega[3]; } fb_tool;      /* world frame, at the moment of the call */
typedef struct fb_fem_tool_contact_params { double stiffness, depth_cap; int points /* FB_TOOL_SURFACE_VERTICES | FB_TOOL_ALL_NODES */, reserved; } fb_fem_tool_contact_params;
typedef struct fb_fem_tool_contact_info {
  int n_points, n_contacts, n_degenerate, contacts_by_shape[FB_TOOL_MAX_SHAPES];
  int n_sticking, n_sliding, n_separating;          /* 0 without friction */
  double max_depth, max_slip_speed, max_normal_force, max_stick_rate;
  double force_on_body[3], force_on_tool[3], torque_on_tool[3];
} fb_fem_tool_contact_info;
int fb_fem_tool_contact(fb_fem_t h, const fb_tool* tool, const fb_fem_tool_contact_params* p,
                        const fb_fem_contact_friction_params* fr /* NULL: frictionless */, fb_fem_tool_contact_info* out /* may be NULL */);
int fb_fem_num_tool_contacts(fb_fem_t h);   /* entries fb_fem_read_tool_contact writes: n_contacts of the last adding call (negative: FB_E*) */
int fb_fem_read_tool_contact(fb_fem_t h, int* node, int* shape, double* depth, double* normal3, double* force3,
                             double* normal_force, double* slip3, double* friction3);   /* any pointer NULL */
int fb_fem_time_tool_contact(fb_fem_t h, const fb_tool* tool, const fb_fem_tool_contact_params* p,
                             const fb_fem_contact_friction_params* fr, int reps, double seconds[3]);  /* adds no force */

/* ---- Constrained motion: held nodes follow a tool, reaction forces on the device ----
 * A constrained DOF is otherwise nailed to q = 0 for life.  A MOTION SET is a subset of the handle's constrained DOFs, each with a
 * target displacement u_c: a grasper that drags tissue, a clamp that moves, a displacement-driven haptic device that is told what force
 * the tissue returns.  The reference has only the stub (IAvatar::grip() sets a flag, IScalpel.cpp:42-44, AvatarRing.cpp:177; its
 * integrator zeroes constrained DOFs as fb_fem_step does), so the rule is this library's (tests/motionref.py restates it
 * in NumPy on the oracle's matrices).  Unsharded handles with the default integrator only: a sharded handle and FB_INTEGRATOR_NEWMARK
 * return FB_EINVAL.  A handle with an empty set launches nothing new and steps bit for bit as before.
 *
 * The rule.  A constrained DOF outside the set behaves as ever (q = 0, qvel = 0 after a step).  For a DOF c of the set, the next
 * fb_fem_step ends with
 *     q_c = u_c  (the target's bits)      qvel_c = v*_c = (u_c - q_c_before) / h
 * and the target stays until it is changed, so the step after that has v* = 0.  dv_c = v*_c - qvel_c_before is known before the
 * solve, and the free rows solve the reference's system with the known part moved to the right:
 *     Keff_ff dv_f = rhs_f - Keff_fc dv_c,     Keff = s_k K + s_m M  (the UNMASKED matrix; s_k = h (h + cK), s_m = 1 + h cM)
 * Keff_fc couples free DOF f to moved DOF c -- the two other DOFs of the SAME node included where only one or two DOFs of a node are
 * in the set.  The stored matrix, its identity rows, the right-hand side on constrained rows (0) and the solution there (0) are
 * untouched: the solvers see only a different right-hand side.  fb_fem_system's rhs INCLUDES the correction while the handle has a set
 * (it is the right-hand side the step would solve; its matrix is bitwise that of a handle without a set).
 * The correction is formed from the elements, not from the matrix (whose columns are zeroed): every element with a node that has a DOF
 * in the set contributes (s_k K_e + s_m M_e) times the 12-vector that holds dv_c, K_e in the closed form the assembly sums (rotated
 * gradients of the step; under warp = 2 the symmetric part of the rotation-derivative terms), M_e = rho/20 V (1 + delta_ij), materials
 * per element where the handle has a map.  The 4 x 3 results are records 4p + k (corner k of the p-th such element, ascending), sorted
 * stably by node; a node's records are subtracted from its FREE DOFs in record order.  No floating-point atomics: two calls from one
 * state give the same bits.
 *
 * The REACTION on a DOF of the set is the force the constraint puts on the body during the step, from the unmasked row c and the full
 * dv (the moved DOFs included):
 *     lambda_c = (1/h) [Keff dv]_c + [(g_k K + g_m M) qvel + fint - fext]_c        (g_k = h + cK, g_m = cM; qvel before the step)
 * summed in the same record order.  What a haptic device is fed is -lambda, summed over the grasp: sum3 is the sum of lambda by axis
 * in one fixed tree.
 *
 * The targets are explicit: a target far from q means a large v* in ONE step ((u - q) / h), which is the caller's to bound (move the
 * target a little every step).  There are no velocity or acceleration limits, no sub-stepping, no friction at the jaws and no soft
 * grasp.  A target that is not finite is refused with FB_EINVAL where it is set; the step checks again on the device (a state that is
 * not finite at a moved DOF): it then returns FB_EINVAL and the moved DOFs hold what a step without the set writes (0).
 *
 * fb_fem_set_constrained_motion replaces the set: n caller DOF ids, ascending, each a constrained DOF of the handle, and their targets;
 * anything else is FB_EINVAL and nothing changes.  n = 0 clears.  fb_fem_num_constrained_motion / fb_fem_read_constrained_motion read it
 * back (either pointer may be NULL).  fb_fem_read_reactions: lambda of the last fb_fem_step in the set's order and its sum (either
 * may be NULL); zeros before a step with the set.  fb_fem_motion_info_get: the set's size, and of the element table the listed
 * elements, the touched nodes, the longest run of records of one node and how many times it was built (once per set and mesh
 * generation, at the first step that needs it; a change of targets alone builds nothing).  fb_fem_time_motion: seconds of the table
 * build | the correction | the reactions | the write of the moved DOFs, means of `reps` runs with a host wait each, written to
 * scratch (state, right-hand side, reactions and table_builds stay what they are); FB_EINVAL without a set.
 *
 * The grasp, on top: fb_fem_grasp adds the three DOFs of each node (caller ids, ascending) to the constrained list -- merged with what
 * the list held, masks rebuilt as fb_fem_set_constrained_dofs rebuilds them -- and to the set with target = their current q (bit for
 * bit, taken on the device; an entry the set already held keeps its target, and fb_fem_release gives it back as it was), and
 * remembers their current world positions p_grab = x0 + q.  One grasp per handle.  fb_fem_grasp_move
 * sets the targets of the grasped DOFs to R (p_grab - pivot) + pivot + t - x0 by a kernel (R row-major; no whole-mesh vector crosses
 * the bus).  fb_fem_release takes what fb_fem_grasp added out of the constrained list and out of the set; q and qvel stay, so the
 * tissue springs back as free DOFs.
 *
 * With the rest of the interface: fb_fem_set_constrained_dofs, fb_fem_resync_delta and fb_fem_cut keep the entries whose DOF is still
 * constrained, with their targets, and drop the others (a dropped DOF keeps its q and qvel where the call carries state; the table
 * is built again at the next step).  A cut does not move a held node's world-space target: fb_fem_cut(FB_CUT_BAKE), which adds q to the
 * rest positions and zeroes it, subtracts q_c from the targets first (u_c - q_c; a node held at its target keeps target 0).  An entry
 * on a node that no element uses any more (FB_DETACH_REMOVE) ends at its target with lambda_c = -fext_c, the rule's empty row.
 * fb_fem_resync and fb_fem_reset clear the set and the grasp.  A piece made by
 * fb_fem_detach_part starts with an empty set.  Renumbered handles map the ids at the boundary, as every entry point does. */
typedef struct fb_fem_motion_info {
  int n_dofs, n_listed_elements, n_touched_nodes, longest_run;
  int table_builds, table_valid, n_grasp_nodes, reserved;
} fb_fem_motion_info;
int fb_fem_set_constrained_motion(fb_fem_t h, int n, const int* dofs, const double* displacements);
int fb_fem_num_constrained_motion(fb_fem_t h);  /* -1: null or unusable handle */
int fb_fem_read_constrained_motion(fb_fem_t h, int* dofs, double* displacements);
int fb_fem_read_reactions(fb_fem_t h, double* forces, double* sum3);
int fb_fem_motion_info_get(fb_fem_t h, fb_fem_motion_info* out);
int fb_fem_time_motion(fb_fem_t h, int reps, double seconds[4]);
int fb_fem_grasp(fb_fem_t h, int n_nodes, const int* node_ids, fb_fem_motion_info* info);
int fb_fem_grasp_move(fb_fem_t h, const double R[9], const double t[3], const double pivot[3]);
int fb_fem_release(fb_fem_t h);

/* ---- Element stress and strain, on the device ----
 * The bracket of the corotational element force f_e,i = V R [lambda tr(H) I + mu (H + H^T)] b_i, which the assembly forms every step
 * (E B (R^T x - x0) of corotationalLinearFEM.cpp:107-137, 270-286) and does not keep.  Unsharded handles only (FB_EINVAL otherwise, as
 * fb_fem_read_mesh), device- or host-built plan alike, renumbered or not: elements keep the caller's order.  A handle that never calls
 * these allocates and launches nothing extra.
 *
 * For element e: b_k and V are its rest record (shape-function gradients, rest volume); P_k = x0 + q of its nodes; F = sum_k P_k b_k^T,
 * evaluated as the assembly evaluates it; (lambda_e, mu_e) what the next assembly would use -- the handle's E / nu, or the table entry
 * of the element's material where a map exists, fb_fem_set_internal_force_scaling folded in.  R = I on a handle created with linear != 0;
 * otherwise the rotation of the assembly's polar decomposition of F (same routine, tolerance 1e-6), negated when its determinant is
 * negative.  H = sum_j (R^T P_j - X_j) b_j^T, evaluated as (R^T - I) + R^T sum_j q_j b_j^T (the b_j sum to zero and sum_j X_j b_j^T = I), which keeps
 * the rounding of x0 + q away from the gradients of a flat element; strain = (H + H^T) / 2, stress = lambda_e tr(H) I + mu_e (H + H^T).  Six-vectors are
 * xx, yy, zz, xy, yz, zx -- the row order of the reference's B -- and hold TENSOR components: strain_xy is half the engineering shear
 * B produces.  von Mises = sqrt(((sxx-syy)^2 + (syy-szz)^2 + (szz-sxx)^2) / 2 + 3 (sxy^2 + syz^2 + szx^2)); energy density
 * psi = stress : strain / 2; J = det F by the plain cofactor expansion; an element is inverted when J < 0.  The tensors are in the
 * element's rest frame, the one the force model works in; with FB_STRESS_WORLD both are stored as R (.) R^T. */
#define FB_STRESS_WORLD   1   /* tensors rotated to the world frame */
#define FB_STRESS_TENSORS 2   /* keep stress6 / strain6 per element (96 B per element more) */
typedef struct fb_fem_stress_info {
  int n_elements, flags;
  double max_von_mises; int max_element;   /* of equal maxima the lowest element */
  double min_J;         int min_J_element; /* likewise */
  int n_inverted;
  double energy;        /* sum of V_e psi_e */
} fb_fem_stress_info;
/* Computes on the handle's stream from the current q.  von Mises, psi and J stay on the device per element, the tensors only with
 * FB_STRESS_TENSORS.  One copy of sizeof(fb_fem_stress_info) leaves the device.  Unknown flag bits return FB_EINVAL and change nothing.
 * No floating-point atomics: maxima and minima are lexicographic (value, element) folds over per-workgroup partials, `energy` is summed
 * in fb_fem_volume's fixed tree, which depends on the element count alone -- the same bits from call to call and under either numbering.
 * A mesh without elements gives zeros and elements -1. */
int fb_fem_stress(fb_fem_t h, int flags, fb_fem_stress_info* out);
/* The arrays of the last fb_fem_stress, elements first .. first + count - 1 in fb_fem_read_mesh's element order; any pointer may be
 * NULL.  stress6 / strain6: 6 doubles per element.  FB_EINVAL (text in fb_last_error) when there is no fb_fem_stress of the current
 * mesh (none yet, or the mesh changed since: fb_fem_resync, fb_fem_resync_delta, a fb_fem_cut returning FB_CUT_DONE), when the range
 * is bad, or when a tensor is asked for and the last call did not keep tensors. */
int fb_fem_read_stress(fb_fem_t h, int first, int count, double* von_mises, double* energy_density, double* J, double* stress6, double* strain6);
/* For every surface vertex, in fb_fem_read_surface's vertex_ids order: (float) of the mean von Mises stress of the elements behind the
 * vertex's faces (face_tets) -- an fp64 sum over the vertex's faces in ascending face order, divided by their number.  Builds the
 * surface first where it is stale, as fb_fem_surface_update does; FB_EINVAL when there is no stress of the current mesh.  One copy of
 * 4 n_vertices bytes leaves the device. */
int fb_fem_surface_stress(fb_fem_t h, float* von_mises);
/* Medians of `reps` HIP-event timings of fb_fem_stress(flags) and of fb_fem_surface_stress, copies included; either pointer may be
 * NULL.  Leaves the handle as a fb_fem_stress(flags) call does. */
int fb_fem_time_stress(fb_fem_t h, int reps, int flags, double* seconds_elements, double* seconds_surface);

/* ---- inspection entry points (what the parity tests compare against the oracle) ---- */
int fb_fem_num_nodes(fb_fem_t h);   /* global */
int fb_fem_num_tets(fb_fem_t h);    /* local (all for an unsharded handle) */
int fb_fem_num_blocks(fb_fem_t h);  /* 3x3 blocks of the stiffness pattern (owned rows) */
int fb_fem_matrix_precision(fb_fem_t h);  /* FB_MATRIX_F32 or FB_MATRIX_F64: the width the matrix values are stored in (what FB_MATRIX_AUTO chose) */
int fb_fem_owned_range(fb_fem_t h, int lo_hi[2]);  /* the node range this handle owns ([0, n_nodes) when unsharded); of the INTERNAL order when renumbered */
/* 1 when the handle works in an internal node order; widest element (largest id difference inside a tet) in the caller's and in the
 * internal order (equal when not renumbered; 0 when never measured: FB_RENUMBER_OFF).  Pointers may be NULL. */
int fb_fem_renumbering(fb_fem_t h, int* span_caller, int* span_internal);
/* a sharded handle's halo: nodes of other ranks its elements touch, and how many ranks own them (0, 0 when unsharded) */
int fb_fem_halo_info(fb_fem_t h, int* n_halo_nodes, int* n_neighbour_ranks);
/* caller ids of the nodes this handle owns, in internal order (hi - lo entries of fb_fem_owned_range; the identity range when not renumbered) */
int fb_fem_owned_nodes(fb_fem_t h, int* ids);
/* node-level pattern, ascending columns per row (corotationalLinearFEM.cpp:163-186, sparseMatrix.cpp:238-262):
 * bptr[n_owned+1], bcol[num_blocks] (global node ids) */
int fb_fem_pattern(fb_fem_t h, int* bptr, int* bcol);
/* per-element K0 = V B^T E B (144 fp64, row-major 12x12) and M^-1 (16 fp64, rows = [grad N_k | N_k(0)]) for
 * elements [first, first+count), computed by the batched MFMA kernel (corotationalLinearFEM.cpp:99-145) */
int fb_fem_element_stiffness(fb_fem_t h, int first, int count, double* K0, double* Minv);
/* raw corotational assembly at displacement u (3*n_nodes): internal force f (3*n_nodes, owned range filled) and
 * K as 9 values per block in fb_fem_pattern order (corotationalLinearFEM.cpp:219-470, warp = 1) */
int fb_fem_assemble(fb_fem_t h, const double* u, double* f, double* K_blocks);
/* Keff (blocks, constrained rows/cols replaced by identity) and right-hand side of the current state, as the
 * next fb_fem_step would solve them (PS_VolumeConservingIntegrator.cpp:84-123,160-162) */
int fb_fem_system(fb_fem_t h, double* Keff_blocks, double* rhs);
/* consistent mass scalar per block (generateMassMatrix.cpp:33-76, tetMesh.cpp:150-182) */
int fb_fem_mass(fb_fem_t h, double* m_blocks);
/* y = Keff x with the device SpMV kernel on the last assembled system (x, y: 3*n_nodes) */
int fb_fem_spmv(fb_fem_t h, const double* x, double* y);
/* Jacobi-PCG (CGSolver.cpp:129-190) on the last assembled system with a caller right-hand side; x starts at 0.
 * iterations_out: + converged / - not converged, as the reference returns. */
int fb_fem_pcg(fb_fem_t h, const double* rhs, double* x, double eps, int max_iter, int* iterations_out);

/* timing helpers for bench.py: `reps` launches of the PCG loop's SpMV kernel (k_spmv<MT,3>: q = A d plus the three
 * merged sums) / `reps` assemblies (k_tet_warp + k_assemble_tets / k_assemble_rows) on the current system; average device seconds per
 * launch measured with HIP events on the handle's stream. */
/* Plan arrays as the device holds them (what the per-step kernels read), for checking the device-side plan builder against
 * the host one (fembrain_hip_testing.h, fb_plan_get -- same names: bptr, bcol, blk_slot, slice_off, colidx, slot_coff,
 * slot_ccnt, contrib).  Copies at most `capacity` int32 words, returns the element count or a negative code.
 * Of a handle that solves in persistent launches also what that solver planned, where the plan has it: "pipe_wg_first" (the slices
 * dealt to the workgroups by slots: n_workgroups + 1 first slices, then n_workgroups counts), "pipe_tasks" (the task table, 16 rows of
 * four words per workgroup: an owner's resident slots, their place, the end of its stream and its helpers' mask; a helper's slice in the
 * workgroup, first and last slot and number) and "pipe_windows" (per slice: first slot of the LDS window, mirror layers, plain resident
 * slots).  A plan without one answers as for an unknown name. */
long long fb_fem_device_plan_get(fb_fem_t h, const char* name, int* out, long long capacity);
/* 1 if the plan of this handle was built on the device (unsharded handles, unless FEMBRAIN_PLAN_DEVICE=0), else 0 */
int fb_fem_plan_on_device(fb_fem_t h);
/* the assembly kernel of this handle: 2 = element-major, records staged in LDS by one wavefront and mass entries precomputed
 * (k_assemble_tets_st: FB_MATRIX_F32, warp = 1), 1 = element-major with every value wavefront fetching its records
 * (k_assemble_tets; slices of at most 31 slots; also FEMBRAIN_ASM_KERNEL=tets1), 0 = slot-major (k_assemble_rows; also
 * FEMBRAIN_ASM_KERNEL=rows).  All three write the same bits. */
int fb_fem_assembly_kernel(fb_fem_t h);
/* slices of more than 31 slots (hub nodes, hull nodes of a Delaunay mesh): the element-major kernel leaves those to a second launch of the
 * slot-major kernel (same bits); 0 when the slot-major kernel assembles everything anyway */
int fb_fem_assembly_wide_slices(fb_fem_t h);
int fb_fem_time_spmv(fb_fem_t h, int reps, double* seconds_per_spmv);
int fb_fem_time_assembly(fb_fem_t h, int reps, double* seconds_per_assembly);
/* COLLECTIVE on a sharded handle (every rank calls it with the same reps): average device seconds of one halo refresh of
 * a 3-vector and of one 3-scalar global sum, back to back on the handle's stream -- the two exchanges of a PCG
 * iteration, through whichever transport fb_fem_transport() reports.  Both 0 on an unsharded handle. */
int fb_fem_time_exchange(fb_fem_t h, int reps, double* seconds_per_halo, double* seconds_per_sum);
/* average device seconds of forming K0 = V B^T E B for ALL elements with the fp64 MFMA kernel behind
 * fb_fem_element_stiffness (results go to a device scratch, nothing is copied out): what materialising the reference's
 * KElementUndeformed array would cost per rebuild; the per-step path never forms K0. */
int fb_fem_time_element_stiffness(fb_fem_t h, int reps, double* seconds_per_pass);
/* FB_PCG_PERSISTENT (chosen by default where it is faster, see fb_fem_params.pcg_variant): returns 1 if this handle runs its
 * merged iterations inside persistent launches, else 0; wavefronts (= slices) per CU, workgroups, and how many slots of every
 * slice stay resident in LDS for a launch (any pointer may be NULL) */
int fb_fem_persist_info(fb_fem_t h, int* waves_per_cu, int* workgroups, int* lds_slots);
/* What ran: the FB_PCG_PATH_* of the last solve (return value); the persistent kernel instantiation this handle launches
 * ("k_pcg_pipe<float,c16,12,5>", "" when it has none) into name; persistent launches and fallbacks so far; the longest
 * producer list of a workgroup (-1: some workgroup polls all flags).  Any pointer may be NULL. */
int fb_fem_pcg_path(fb_fem_t h, char* name, int name_len, int* persist_launches, int* persist_fallbacks, int* max_producers);
/* A handle whose persistent launch timed out runs the two-launch iteration, but not for ever: after 32 such solves (doubling with
 * every further time-out; FEMBRAIN_PERSIST_REARM=n sets the first wait, 0 = never) an unsharded handle launches the persistent solver
 * again, and every re-sync re-arms it (sharded handles: at a re-sync only, the ranks switch together).  Returns how often this handle
 * was re-armed by the count. */
int fb_fem_persist_rearms(fb_fem_t h);
/* helper tasks of the persistent solver on this mesh (0: none): where a few slices are much wider than the rest (hull nodes of a Delaunay
 * mesh), wavefronts without a slice of their own multiply the upper part of a wide slice's slots and hand the partial sums over in LDS
 * (fembrain_amd/csrc/pcg_pipe.hip.h).  Chosen by the library from the slice widths; FEMBRAIN_PIPE_HELPERS=0/1 overrides. */
int fb_fem_persist_helpers(fb_fem_t h);
/* How the persistent solver lays out the vector its products gather from: 1 = node by node (x, y, z of a node side by side), 0 = three
 * planes.  Decided from the mesh: lines_planes / lines_records (either may be NULL) receive the cache lines the gathers of one matrix slot
 * touch on average in the two forms, sampled on the device when the handle was (re)built -- structured meshes ~12-20 / ~12-15 (planes: each
 * load touches 4 lines), unstructured ones ~80 / ~44 (node by node: 606k-tet Delaunay probe 18.9 -> 16.2 us per PCG iteration).  0 / 0 where
 * it was not measured (handles outside the one-row persistent kernel's range).  FEMBRAIN_PIPE_XYZ=0/1 overrides. */
int fb_fem_persist_gather(fb_fem_t h, double* lines_planes, double* lines_records);
/* The LDS window of the one-row persistent kernel (k_pcg_pipe (12, 6) / (12, 7), 9-12 slices per CU): per slice a contiguous run of slots is
 * kept in LDS, and its layers whose blocks have a lower row of the same workgroup as column are not stored again but read as the transposes of
 * those rows' resident blocks (A = A^T bitwise; the iterates do not change by a bit).  mirror_layers = such layers over all slices,
 * pool_entries = blocks kept transposed in the workgroups' pools (lanes of those layers whose partner block is not resident), plain_slots =
 * fewest plainly stored slots of any slice (never fewer than fb_fem_persist_info's lds_slots).  Returns 1 if some layer is mirrored, else 0
 * (0 / 0 / 0: no window -- other instantiations, FEMBRAIN_PIPE_MIRROR=0).  Any pointer may be NULL. */
int fb_fem_persist_mirror(fb_fem_t h, int* mirror_layers, int* pool_entries, int* plain_slots);
/* Register slots of the run-ahead LDS-window kernels (k_pcg_pipe (12, 6) / (12, 7) with a service wavefront, plain Jacobi): up to slots_per_slice
 * streamed slots of every slice, those next to its LDS window, keep their matrix values in registers for a whole launch (filled at the head of
 * every launch; the iterates do not change by a bit).  slots_per_slice (may be NULL) = what this handle's launches hold per slice at most: 3,
 * or what FEMBRAIN_PIPE_REGS=0|2|3 said when the plan was built; a slice holds that many or as many as it streams.  Returns the register slots over all slices (0 / 0: another instantiation, no window, FEMBRAIN_PIPE_REGS=0), < 0: an error. */
int fb_fem_persist_regs(fb_fem_t h, int* slots_per_slice);
/* Wavefront priority through the product of the persistent kernels that have a priority form (the register-slot kernels; the development build
 * with the phase clocks at (12, 6)): the form this handle's launches use -- 1 by progress, 2 static, 3 by progress with the service wavefront's
 * collection raised (FEMBRAIN_PIPE_PRIO when the plan was built; the iterates do not change by a bit) -- and 0 where the kernel has none. */
int fb_fem_persist_prio(fb_fem_t h);
/* average device seconds of ONE persistent launch that starts a solve of the current system and is cut after n_iters
 * iterations (tolerance out of reach), HIP events on the handle's stream around the launch; the difference of two lengths
 * prices an iteration without the launch's fixed cost */
int fb_fem_time_persist(fb_fem_t h, int reps, int n_iters, double* seconds_per_launch);
/* the persistent launches of the SOLVES this handle has made so far (fb_fem_step, fb_fem_pcg; not the timing helper above): how
 * many, their device seconds (HIP events on the handle's stream around each launch) and the PCG iterations they ran */
int fb_fem_persist_stats(fb_fem_t h, int* launches, double* seconds, long long* iterations);
/* algorithmic bytes of ONE Jacobi-PCG iteration on this system: BSR SpMV + the fused lower bound of the vector
 * traffic (9 fp64 vector streams) */
int fb_fem_iteration_bytes(fb_fem_t h, double* bytes);
/* algorithmic bytes moved by one SpMV launch / one assembly on this handle */
int fb_fem_spmv_bytes(fb_fem_t h, double* bytes);
int fb_fem_assembly_bytes(fb_fem_t h, double* bytes);

/* ------------------------------------------------------------------------------------------------------
 * Communicator for sharded handles: RCCL over xGMI, loaded lazily (a 1-GPU process never needs librccl).
 * unique_id: 128 bytes produced by fb_comm_unique_id on rank 0 and broadcast by the launcher.
 * ---------------------------------------------------------------------------------------------------- */
int fb_comm_unique_id(unsigned char id[128]);
int fb_comm_create(fb_comm_t* out, int rank, int n_ranks, const unsigned char id[128], int device);
int fb_comm_destroy(fb_comm_t c);
/* what the communicator is made of: *ranks = its size, *rccl_ranks = the rank count the RCCL communicator itself reports
 * (ncclCommCount; 0 when the communicator has no RCCL handle: the host-staged test transport), *transport = 0 none (one rank, no library),
 * 1 RCCL, 2 host-staged test transport.  Any pointer may be NULL. */
int fb_comm_info(fb_comm_t c, int* ranks, int* rccl_ranks, int* transport);

/* ------------------------------------------------------------------------------------------------------
 * BlobTree field / polygonizer handle = the GPU side of PS::SKETCH::GPUPoly (implicit/OclPolygonizer.h:45-231)
 * and PS::SKETCH::FieldComputer (implicit/FieldComputer.h:31-70).  Input is the LinearBlobTree flat layout
 * (implicit/LinearBlobTree.h:20-82): header 12 floats, 16 per operator, 20 per primitive, 12 per matrix.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct fb_poly_s* fb_poly_t;

/* GPUPoly::setBlob (OclPolygonizer.cpp:1602-1648): deep copy of the four arrays */
int fb_poly_create(fb_poly_t* out, int device, const float* header12, int n_ops, const float* ops16,
                   int n_prims, const float* prims20, int n_mtx, const float* mtx12);
int fb_poly_destroy(fb_poly_t h);

/* Which of the reference's field evaluations the handle follows (the reference has two that disagree):
 *   FB_FIELD_CPU      (default) FieldComputer::fieldValue / computePrimitiveField (implicit/Polygonizer.cpp:1544-2108) without
 *                     its primitive bounding-box cull: range operators sum, binary operators act by their type, instanced
 *                     nodes are evaluated.
 *   FB_FIELD_CPU_BOX  the same WITH computePrimitiveField's isOutsidePrim cull (Polygonizer.cpp:1485-1505,1548-1552), tested
 *                     per point: a primitive contributes 0 outside its box.  prim_boxes6 = lo.xyz, hi.xyz per primitive as
 *                     PrepareAllBoxes makes them (Polygonizer.cpp:210-540, offset ISO_VALUE; BlobReader.h / blobtree.py
 *                     compute them), copied.
 *   FB_FIELD_OPENCL   the OpenCL kernels GPUPoly actually runs (data/opencl/Polygonizer.cl:483-886): ComputeField over the
 *                     traversal route of LinearBlobTree::setTraversalRoute (implicit/LinearBlobTree.cpp:333-429), binary
 *                     operators through ComputeOpField(idxBranchOp, ...) -- the operator's INDEX where its type is meant
 *                     (:825) --, range operators by their own type, instanced nodes 0.  This is the evaluation that wrote the
 *                     reference's shipped outputs (data/models/blobtree/{tumor,peanut,dumbel,dumbelclose,eggshell}.veg): every
 *                     surface vertex of the five files is reproduced in order (tests/golden/surface_*.npz).  FB_EINVAL for
 *                     trees the reference's route builder cannot handle (an operator with two operator children).
 * Takes effect for every later sweep / field / surface call; grids swept before are dropped.  On failure the handle keeps
 * its previous semantics.  The colour pass (fb_poly_read_surface_colors, fb_poly_field_color_array) exists for FB_FIELD_CPU only. */
#define FB_FIELD_CPU 0
#define FB_FIELD_CPU_BOX 1
#define FB_FIELD_OPENCL 2
int fb_poly_set_field_semantics(fb_poly_t h, int semantics, const float* prim_boxes6);
int fb_poly_field_semantics(fb_poly_t h);

/* GPUPoly::computeFieldArray / FieldComputer::field(n,4,xyzf) (OclPolygonizer.cpp:943-986): xyzf is n*4 floats,
 * .w overwritten with the field value */
int fb_poly_field_array(fb_poly_t h, int n, float* xyzf);

/* GPUPoly::computeAllFields (OclPolygonizer.cpp:1358-1426) / FieldComputer::fieldsForVoxelGrid
 * (FieldComputer.cpp:143-231): sweeps the voxel grid of the model's bounding box (header[0..2] .. header[4..6]) at
 * `cellsize` -- points per axis = ceil(extent/cellsize)+2, origin = bbox lower -- and keeps the float4 (x,y,z,f)
 * grid on the device.  dims_out[3] = grid points per axis.  cellsize < 0.01 is refused as GPUPoly::run does. */
int fb_poly_sweep(fb_poly_t h, float cellsize, int dims_out[3]);
/* explicit grid (lower corner, cellsize, point counts) -- used by benches that name the grid size */
int fb_poly_sweep_grid(fb_poly_t h, const float lower[3], float cellsize, const int dims[3]);
/* GPUPoly::readBackVoxelGridSamples (OclPolygonizer.cpp:916-940): xyzf = 4 floats per grid point,
 * index = iz*gx*gy + iy*gx + ix */
int fb_poly_read_grid(fb_poly_t h, float* xyzf);

typedef struct fb_poly_counts {
  int grid[3];
  int n_points, n_cells;
  int n_crossed_edges;    /* = surface vertices, sum of ComputeEdgeTable counts (Polygonizer.cl:1353-1415) */
  int n_surface_cells;    /* cells with 0 < config < 255 */
  int n_included_cells;   /* config != 0 (Tetrahedralizer.cl:3-35) */
  int n_tet_vertices;     /* grid points touched by an included cell */
  int n_tets;             /* 6 per included cell */
  int n_surface_vertices; /* set by fb_poly_surface: = n_crossed_edges (m_ctVertices of GPUPoly::run) */
  int n_surface_indices;  /* set by fb_poly_surface: 3 per triangle (m_ctFaceElements) */
} fb_poly_counts;

/* ComputeEdgeTable + ComputeCellConfigs + TetMeshCells + the exclusive scans, all on the device
 * (OclPolygonizer.cpp:644-757 steps 2,3,5,6 and :762-819) */
int fb_poly_classify(fb_poly_t h, fb_poly_counts* counts);
/* per-point crossing flags (X=4,Y=2,Z=1) / counts and per-cell 8-bit configs, for parity tests; any may be NULL */
int fb_poly_read_classification(fb_poly_t h, unsigned char* edge_flags, unsigned int* edge_counts,
                                unsigned char* cell_configs);
/* GPUPoly::runTetrahedralizer (OclPolygonizer.cpp:762-819; Tetrahedralizer.cl:39-132): compacts the included grid
 * points in grid order and emits 6 tets per included cell; results stay on the device until read back. */
int fb_poly_tetrahedralize(fb_poly_t h, fb_poly_counts* counts);
/* xyz: 3 floats per tet-mesh vertex, tets: 4 uint32 per tet (both sized from fb_poly_counts) */
int fb_poly_read_tetmesh(fb_poly_t h, float* xyz, unsigned int* tets);

/* ---- marching-cubes surface: GPUPoly::run steps 3,4,6,7 (OclPolygonizer.cpp:663-757) ------------------------------
 * Replaces ComputeVertexAttribs (data/opencl/Polygonizer.cl:1429-1561, linear root + forward-difference normal,
 * 4 field evaluations per vertex), ComputeElements (:1610-1670) and the two host scans between them.  Needs
 * fb_poly_classify on a grid swept WITH stored samples.  Vertex colours: fb_poly_read_surface_colors. */
int fb_poly_surface(fb_poly_t h, fb_poly_counts* counts);
/* GPUPoly::readbackMeshV3T3 (OclPolygonizer.cpp:1696-1744): 3 floats per vertex / normal, 3 uint32 per triangle;
 * any pointer may be NULL */
int fb_poly_read_surface(fb_poly_t h, float* xyz, float* normals, unsigned int* indices);
/* the 256 x 16 triangle table (edge ids, 255 = end) and vertex counts the surface pass uses -- the data of
 * src/implicit/_CellConfigTable.h:58-317 / _CellConfigTableCompact.cpp, regenerated from Bloomenthal's cube-table
 * procedure at load time; host only, needs no device */
int fb_poly_cube_table(unsigned char tri[4096], unsigned char nvert[256]);

#define FB_MESH_SURFACE 0
#define FB_MESH_TET 1
/* GPUPoly::applyFemDisplacements (OclPolygonizer.cpp:1543-1596; ApplyVertexDeformations, Polygonizer.cl:1417-1426):
 * out = rest position + (float)displacement for every vertex of the surface or the tet mesh; the rest positions are
 * kept.  n_dof must be 3 x the mesh's vertex count (FB_EINVAL otherwise -- the reference does not check).  The
 * deformed positions stay on the device and are copied to xyz_out when it is not NULL. */
int fb_poly_apply_displacements(fb_poly_t h, int mesh, int n_dof, const double* displacements, float* xyz_out);

/* Render-loop coupling when the FEM mesh is the tet mesh of the SAME grid (fb_poly_tetrahedralize): every surface vertex
 * lies on a grid edge whose two end points are tet-mesh vertices a, b, at the weight t the root finder placed it.
 * out = rest + (float)u_a + t * ((float)u_b - (float)u_a).  (The reference indexes the FEM displacements by the
 * surface-vertex id, OclPolygonizer.cpp:1559-1563, which is only meaningful when both meshes share their vertices;
 * SURVEY 8f-2.)  n_tet_dof = 3 * n_tet_vertices; xyz_out (3 floats per surface vertex) may be NULL. */
int fb_poly_interpolate_displacements(fb_poly_t h, int n_tet_dof, const double* tet_displacements, float* xyz_out);
/* per surface vertex: the pair (a, b) of tet-mesh vertex ids and the weight t (either may be NULL) */
int fb_poly_read_surface_binding(fb_poly_t h, unsigned int* tet_vertex_pairs, float* weights);

/* Vertex colours of the surface mesh (the colour output of ComputeVertexAttribs / FieldComputer::fieldValueAndColor,
 * src/implicit/Polygonizer.cpp:2110-2410): 4 floats (r, g, b, 1) per surface vertex.  Needs fb_poly_surface. */
int fb_poly_read_surface_colors(fb_poly_t h, float* rgba);
/* FieldComputer::fieldValueAndColor for n points: xyzf (x, y, z, f) gets f, rgb 3 floats per point */
int fb_poly_field_color_array(fb_poly_t h, int n, float* xyzf, float* rgb);
/* GPUPoly::computeOffSurfacePointsAndFields (OclPolygonizer.cpp:1045-1107; kernel Polygonizer.cl:1329-1350): for every
 * surface vertex v with normal n the two points v + len n and v - len n with their field values; xyzf_pairs receives
 * 8 floats per vertex (x, y, z, f outside then inside).  Needs fb_poly_surface. */
int fb_poly_off_surface(fb_poly_t h, float len, float* xyzf_pairs);
/* average device seconds of the surface pass (counts + scans + vertex attributes + elements) on the current grid */
int fb_poly_time_surface(fb_poly_t h, int reps, double* seconds);
/* average device seconds of one sweep / one classify+tetrahedralize pipeline on the current grid */
int fb_poly_time_pipeline(fb_poly_t h, int reps, double* sweep_seconds, double* pipeline_seconds);
/* the sweep followed by the float4 (x, y, z, f) grid fb_poly_read_grid returns (16 bytes per point; the sweep itself stores f alone, 4 bytes
 * per point, and the grid is materialised only when it is asked for): SURVEY.md 8d's second figure */
int fb_poly_time_grid(fb_poly_t h, int reps, double* sweep_and_grid_seconds);
/* the same pipeline with HIP events between its stages (the events cost a little: fb_poly_time_pipeline is the rate to quote):
 * average device seconds of [0] the sweep, [1] classification + scans, [2] tet-mesh vertices, [3] tet elements (the dominant kernel:
 * 96 B written per included cell), [4] all of it */
int fb_poly_time_stages(fb_poly_t h, int reps, double seconds[5]);

/* Field grid -> tets -> FEM with no host hop: the tet mesh fb_poly_tetrahedralize left on the device becomes
 * the mesh of a new FEM handle -- node ids copied device to device, float positions widened to double, pattern / SELL-64
 * layout / contribution lists built on the device.  Same result as fb_fem_create on fb_poly_read_tetmesh's arrays.
 * params->device must be the polygonizer's device.  The constrained DOFs come from the host as for fb_fem_create. */
int fb_fem_create_from_poly(fb_fem_t* out, fb_poly_t poly, int n_fixed_dofs, const int* fixed_dofs, const fb_fem_params* params);
/* The current fb_poly_surface of `poly` as an embedding of h (fb_fem_embed), without a host copy: its vertices widened to double, and its
 * triangles.  poly must live on the handle's device and have a surface (FB_EINVAL otherwise).  Bit for bit what fb_fem_embed makes of
 * fb_poly_read_surface's arrays. */
int fb_fem_embed_from_poly(fb_fem_t h, fb_poly_t poly, const fb_fem_embed_params* p, int* id, fb_fem_embed_info* out);

/* ---- multi-GPU field path: z-slabs of one grid ---------------------------------------------------------------------
 * The grid's point planes are dealt to the ranks in contiguous runs.  A rank that owns planes [p0, p1) (and the cell layers
 * [p0, min(p1, planes - 1))) sweeps the slab [max(p0 - 1, 0), min(p1 + 1, planes - 1)] -- one plane below and two above,
 * so that the vertex marks of its own planes and of plane p1 are complete -- and runs fb_poly_classify and
 * fb_poly_tetrahedralize on it unchanged.  Point positions are lower + cellsize * GLOBAL index, so field samples, marks
 * and positions are bitwise those of the whole grid.  Vertices are numbered plane by plane: with vertex_base = the number
 * of owned vertices of all lower ranks (one all-gather of fb_poly_slab_counts' first number), fb_poly_read_tetmesh_slab
 * returns the rank's consecutive piece of the whole grid's tet mesh -- the pieces of all ranks concatenated ARE
 * fb_poly_read_tetmesh of the single-GPU run, bit for bit. */
int fb_poly_sweep_slab(fb_poly_t h, const float lower[3], float cellsize, const int dims[3], int z_first, int z_count);
int fb_poly_slab_counts(fb_poly_t h, int own_first_plane, int own_planes, int own_layers, int* n_vertices, int* n_tets);
int fb_poly_read_tetmesh_slab(fb_poly_t h, int own_first_plane, int own_planes, int own_layers, unsigned int vertex_base, float* xyz, unsigned int* tets);

/* ---- cutting tool: scalpel / tet-mesh intersection tests --------------------------------------------------------------------
 * Replaces the device half of PS::FEM::Cutting (src/deformable/Cutting.cpp:87-497) and the four kernels of
 * data/opencl/Cutting.cl (:158-341).  Face f of tet t is face 4 t + f with corners faceMask[f] = {0,1,2} {1,2,3} {2,3,0}
 * {0,1,3}; edge e of tet t is edge 6 t + e with ends {0,1} {1,2} {2,0} {0,3} {1,3} {2,3} (Cutting.cl:174-176, :290-292).
 * fp32 arithmetic, operation for operation that of the reference's IntersectSegmentTriangleF
 * (src/graphics/Intersections.cpp:12-64). */
typedef struct fb_cut_s* fb_cut_t;
#define FB_CUT_FACES 0
#define FB_CUT_EDGES 1
/* Cutting::createMemBuffers (Cutting.cpp:87-167): node positions (3 doubles each, rounded to float as there) and the
 * tets' node ids (4 each).  Ids are checked against n_vertices (FB_EINVAL; the reference does not check). */
int fb_cut_create(fb_cut_t* out, int device, int n_vertices, const double* xyz, int n_tets, const unsigned int* tets);
void fb_cut_destroy(fb_cut_t h);
/* new positions of the same nodes (the deformed mesh) */
int fb_cut_set_vertices(fb_cut_t h, int n_vertices, const double* xyz);
/* Cutting::computeFaceCentroids (Cutting.cpp:253-322; kernel ComputePerTetCentroids): every face flag 1, point = centroid */
int fb_cut_face_centroids(fb_cut_t h);
/* Cutting::computeFaceIntersections (Cutting.cpp:169-251; kernel ComputePerTetFaceIntersections): flag = the scalpel edge
 * s0-s1 (3 doubles each) crosses the face, point = the crossing (w = 1), the centroid otherwise; *n_hits = number of
 * flagged faces (what the reference's sum scan returns).  n_hits may be NULL. */
int fb_cut_face_intersections(fb_cut_t h, const double* s0, const double* s1, int* n_hits);
/* Cutting::computeEdgeIntersections (Cutting.cpp:442-497; kernel ComputePerTetEdgeIntersections): quad12 = the swept quad
 * q0..q3; an edge is tested against triangle (q0, q3, q1), then (q0, q2, q3).  Points of missed edges are (0, 0, 0, 1)
 * (the reference leaves them unwritten). */
int fb_cut_edge_intersections(fb_cut_t h, const double* quad12, int* n_hits);
/* flags (4 or 6 per tet) and points (x, y, z, w per face / edge) of the last pass; either pointer may be NULL */
int fb_cut_read(fb_cut_t h, int what, unsigned int* flags, float* points_xyzw);
/* the flagged faces / edges of the last pass in ascending id order (the compaction the reference's scan prepares):
 * ids and points (4 floats) of at most `capacity` hits, *n_out = number of hits.  ids / points may be NULL to query. */
int fb_cut_read_hits(fb_cut_t h, int what, int capacity, unsigned int* ids, float* points_xyzw, int* n_out);
/* kernel ComputeSegmentTriIntersections (Cutting.cl:321-341; Cutting::computeFaceSegmentIntersectionTest): loose
 * triangles (3 x float4 each) against the segment s0-s1 (3 floats each); out = crossing or (-1, -1, -1, 1) */
int fb_cut_segment_triangles(int device, int n_tris, const float* tri_xyzw, const float* s0, const float* s1, float* points_xyzw);
/* average device milliseconds of one face pass (a = s0, b = s1) or one edge pass (a = quad12, b ignored) */
int fb_cut_time(fb_cut_t h, int what, const double* a, const double* b, int reps, double* ms_per_pass);

#ifdef __cplusplus
}
#endif
#endif /* FEMBRAIN_HIP_H */
