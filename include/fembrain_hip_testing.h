/* fembrain_hip_testing.h -- host-only inspection hooks of libfembrain_hip.so used by the CPU test-suite
 * (no device call is made by any function in this header but fb_test_workgroup at its end).  They expose the per-rank plan that
 * fb_fem_create[_sharded] builds -- local numbering, halo/send lists, 3x3-block pattern, SELL-64 layout and the
 * element contribution lists -- so that the partition logic can be checked without a GPU, including with
 * world_size-2 gloo runs.  Not part of the reference-facing surface. */
#ifndef FEMBRAIN_HIP_TESTING_H
#define FEMBRAIN_HIP_TESTING_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct fb_plan_s* fb_plan_t;

int fb_plan_create(fb_plan_t* out, int n_nodes, int n_tets, const int* tets, int n_fixed_dofs, const int* fixed_dofs,
                   int n_ranks, int rank, const int* node_splits);
int fb_plan_destroy(fb_plan_t p);
/* info[0..11] = n_owned, n_halo, n_tets, n_blocks, n_slices, n_slots, n_crows, n_send, node_lo, node_hi,
 * n_fixed_owned, n_ranks */
int fb_plan_info(fb_plan_t p, int info[12]);
/* copies the named int32 array into out (capacity in elements); returns the element count or a negative code.
 * names: local2global, halo_off, send_off, send_local, tets, tet_global, bptr, bcol, slice_off, colidx, blk_slot,
 *        slot_coff, slot_ccnt, contrib (uint32 bits), dofmask (one int per DOF) */
int fb_plan_get(fb_plan_t p, const char* name, int* out, size_t capacity);

/* Host model of the persistent solver's LDS window planner (fembrain_amd/csrc/pcg_pipe_mirror.h, k_pipe_mirror_plan) over this plan, its slices
 * dealt in equal numbers to nb workgroups: out[0] = mirror layers over all slices, out[1] = pool entries, out[2] = fewest plain layers of a
 * slice, out[3] = workgroups that keep mirrors.  c16: 16-bit column words; klt: the instantiation's bound (6 or 7). */
int fb_plan_mirror_model(fb_plan_t p, int nb, int c16, int klt, int out[4]);
/* ... and of the register slots that go with that window (fembrain_amd/csrc/pcg_pipe_regs.hip.h; regs = 0..3 slots per slice at most): for every slice
 * parts[6 * slice + ...] = slots streamed in front | register slots in front | mirror layers | plain layers | register slots behind | slots
 * streamed behind, in slot order.  parts holds 6 ints per slice of the plan. */
int fb_plan_regs_model(fb_plan_t p, int nb, int c16, int klt, int regs, int* parts);

/* Host restatement of the handle's internal node order (fembrain_amd/csrc/renumber.h: slab order of the rest positions): the caller id of
 * every internal id, and the widest element (largest id difference inside a tet) in the caller's and in that order */
int fb_plan_slab_order(int n_nodes, const double* xyz, int n_tets, const int* tets, int* old_of_new, int* span_caller, int* span_internal);

/* Host restatement of one rank's vote on the node order of a sharded handle under FB_RENUMBER_AUTO (fem.hip vote_shard_order): out[0] =
 * the number of other ranks the elements with a node in this rank's range couple it to under the caller's numbering (-1: bad ranges
 * or node ids), out[1] = elements with a node of this rank, out[2] = those that also have a node of another rank.  node_splits may be
 * NULL (equal ranges). */
int fb_plan_shard_vote(int n_nodes, int n_tets, const int* tets, int n_ranks, int rank, const int* node_splits, int out[3]);

/* Host-staged communicator for tests: processes sharing ONE GPU (or none of them owning more than one) exchange through
 * the POSIX shared-memory segment `shm_name` with a process barrier per collective.  It drives exactly the sharded
 * solver path of fb_fem_create_sharded (halo lists, packing, rank-ordered sums) without RCCL, so the N > 1 path can be
 * run on a one-GPU box.  Every rank passes the same name, n_ranks and outbox_bytes; destroy with fb_comm_destroy. */
struct fb_comm_s;
int fb_comm_create_local(struct fb_comm_s** out, int rank, int n_ranks, const char* shm_name, size_t outbox_bytes, int device);
/* Rank 0 replaces a segment of the same name left by a killed run; every wait is bounded by FEMBRAIN_LOCAL_TIMEOUT_MS
 * (default 20000): a rank whose peers do not come gets FB_ECOMM and poisons the segment, which ends every other rank's
 * wait at once.  fb_comm_test_allgather (host only, no device call): `bytes` (<= 512) from every rank into `all`, in rank
 * order -- the barrier pair every collective of the transport is made of. */
int fb_comm_test_allgather(struct fb_comm_s* c, const void* mine, void* all, size_t bytes);

/* Host-only: 1 when the handle's last labelling of its parts (fb_fem_parts) sorted the faces in two passes (more than 2^21 nodes, or
 * FEMBRAIN_PARTS_WIDE_KEYS=1), 0 when in one, -1 when it has not labelled yet. */
struct fb_fem_s;
int fb_fem_parts_wide(struct fb_fem_s* h);

/* The one entry point of this header that DOES run on the device (the default stream of device 0): the in-workgroup primitives of the
 * mesh-side kernels (fembrain_amd/csrc/workgroup.hip.h) and the run bounds of a sorted key array (mesh_device.hip.h), each through the
 * two-launch pattern its users have -- a thread per item, per-workgroup partials, a single-workgroup final.  n items, `what`:
 *   FB_TEST_WG_SUM         values[n] -> out_d[0]: the fp64 sum in the fixed tree
 *   FB_TEST_WG_BEST_*      values[n], keys[n] -> out_d[0], out_i[0]: the lexicographic best (lowest / highest value, of equal values the
 *                          lowest key) with int or long long keys (_INT: the keys must fit an int); idle threads carry +-inf and the
 *                          key type's largest value
 *   FB_TEST_WG_RANKS       flags[n] -> out_i[n + 4]: per item the set flags in front of it, then the total, the items without a flag
 *                          (the scan's second counter), the total again as an integer workgroup sum, the most set flags of a workgroup
 *   FB_TEST_WG_BOX_*       values[3 n] (xyz) -> out_d[6]: lo[3], hi[3] of the points as float or double
 *   FB_TEST_WG_RUN_BOUNDS  keys[n] ascending in [0, m + FB_TEST_WG_GUARD) -> out_i[2 (m + FB_TEST_WG_GUARD)]: lo then hi of the m keys,
 *                          each followed by FB_TEST_WG_GUARD entries that start as -1 and that no key may write
 * FB_EINVAL for n < 1, a case that does not exist or a null array the case reads or writes; nothing is launched then. */
enum {
  FB_TEST_WG_SUM = 0, FB_TEST_WG_BEST_LOW_INT = 1, FB_TEST_WG_BEST_HIGH_INT = 2, FB_TEST_WG_BEST_LOW_LL = 3, FB_TEST_WG_BEST_HIGH_LL = 4,
  FB_TEST_WG_RANKS = 5, FB_TEST_WG_BOX_FLOAT = 6, FB_TEST_WG_BOX_DOUBLE = 7, FB_TEST_WG_RUN_BOUNDS = 8
};
#define FB_TEST_WG_GUARD 8
int fb_test_workgroup(int what, int n, int m, const double* values, const long long* keys, const unsigned char* flags, double* out_d, long long* out_i);

/* Host-only: compiles a BlobTree (operator walk order, slot allocation, expansion of instanced subtrees) exactly as
 * fb_poly_create does and reports the number of evaluation steps and of per-point value slots; needs no device.
 * Lets the CPU suite check every reference model's tree, including the instanced ones. */
int fb_poly_compile_info(int n_ops, const float* ops16, int n_prims, const float* prims20, int* n_steps, int* n_slots);

#ifdef __cplusplus
}
#endif
#endif
