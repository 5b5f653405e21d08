// Host-only test hooks over FemPlan (include/fembrain_hip_testing.h).
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fembrain_hip.h"
#include "../../include/fembrain_hip_testing.h"
#include "fem_plan.h"
#include "renumber.h"
#include "pcg_pipe_mirror.h"

namespace fb {
int fail(int code, const char* fmt, ...);
}

struct fb_plan_s {
  fb::FemPlan plan;
};

namespace {

// One workgroup of the host model of k_pipe_mirror_plan: the window of each of its slices (pipe_slices' deal).  Returns whether it keeps mirrors;
// *pool = its pool entries.
bool mirror_model_wg(const fb::FemPlan& P, int nb, int b, int c16, int klt, fb::MirWave* mw, int* first_out, int* count_out, int* pool) {
  const int* so = P.slice_off.data();
  const int* ci = P.colidx.data();
  // (pipe_slices, pcg_pipe.hip.h)
  const int xcd = b & 7, j = b >> 3, per = nb >> 3, chunk = (P.n_slices + 7) >> 3, lo_s = xcd * chunk;
  int len = P.n_slices - lo_s;
  len = len < 0 ? 0 : (len > chunk ? chunk : len);
  const int base = len / per, rem = len - base * per;
  const int first = lo_s + j * base + (j < rem ? j : rem);
  const int count = std::min(base + (j < rem ? 1 : 0), fb::kMirWaves);
  *first_out = first; *count_out = count < 0 ? 0 : count; *pool = 0;
  if (count <= 0) return false;
  const int lo = first * 64, hi = std::min((first + count) * 64, P.n_owned);
  for (int w = 0; w < count; w++) {
    const int sl = first + w, width = so[sl + 1] - so[sl];
    int hist[256] = {0};
    for (int l = 0; l < 64; l++) {
      const int dk = fb::mir_lane_diag(so, ci, sl, l, P.n_owned);
      if (dk >= 0 && dk < 256) hist[dk]++;
    }
    int d = -1, best = 0;
    for (int k = 0; k < width && k < 256; k++)
      if (hist[k] > best) { best = hist[k]; d = k; }
    int m = 0;
    if (d >= 0)
      for (; m < fb::kMirMax && d - 1 - m >= 0; m++) {
        int n = 0;
        for (int l = 0; l < 64; l++) n += fb::mir_lane_lower(so, ci, sl, d - 1 - m, l, lo, hi) ? 1 : 0;
        if (n < fb::kMirLanes) break;
      }
    mw[w].d = d; mw[w].m = m; mw[w].width = width;
  }
  auto misses = [&]() {
    int e = 0;
    for (int w = 0; w < count; w++)
      for (int k = 0; k < mw[w].m; k++)
        for (int l = 0; l < 64; l++) e += fb::mir_lane_addr(so, ci, first, mw, w, k, l, lo, hi, c16 != 0) < 0 ? 1 : 0;
    return e;
  };
  bool ok = fb::mir_wg_layout(mw, count, klt, c16 != 0, 0, false);
  int E = ok ? misses() : 0;
  ok = ok && E <= fb::kMirPoolMax && fb::mir_wg_layout(mw, count, klt, c16 != 0, E, true);
  if (ok) { E = misses(); ok = fb::mir_wg_gains(mw, count, klt, c16 != 0); }
  if (!ok) { fb::mir_wg_plain(mw, count, klt, c16 != 0); E = 0; }
  *pool = E;
  return ok;
}

}  // namespace


extern "C" {

int fb_plan_create(fb_plan_t* out, int n_nodes, int n_tets, const int* tets, int n_fixed_dofs, const int* fixed_dofs, int n_ranks,
                   int rank, const int* node_splits) {
  if (!out) return fb::fail(FB_EINVAL, "null output");
  fb_plan_s* p = new fb_plan_s;
  int rc = fb::build_fem_plan(p->plan, n_nodes, n_tets, tets, n_fixed_dofs, fixed_dofs, n_ranks, rank, node_splits);
  if (rc != FB_OK) {
    delete p;
    return rc;
  }
  *out = p;
  return FB_OK;
}

int fb_plan_destroy(fb_plan_t p) {
  delete p;
  return FB_OK;
}

int fb_plan_info(fb_plan_t p, int info[12]) {
  if (!p || !info) return fb::fail(FB_EINVAL, "null argument");
  const fb::FemPlan& P = p->plan;
  const int v[12] = {P.n_owned, P.n_halo, P.n_tets, P.n_blocks, P.n_slices, P.n_slots, P.n_crows, (int)P.send_local.size(),
                     P.node_lo, P.node_hi, P.n_fixed_owned, P.n_ranks};
  memcpy(info, v, sizeof v);
  return FB_OK;
}

int fb_plan_get(fb_plan_t p, const char* name, int* out, size_t capacity) {
  if (!p || !name) return fb::fail(FB_EINVAL, "null argument");
  const fb::FemPlan& P = p->plan;
  const std::string n(name);
  const std::vector<int>* v = nullptr;
  std::vector<int> tmp;
  if (n == "local2global") v = &P.local2global;
  else if (n == "halo_off") v = &P.halo_off;
  else if (n == "send_off") v = &P.send_off;
  else if (n == "send_local") v = &P.send_local;
  else if (n == "tets") v = &P.tets;
  else if (n == "tet_global") v = &P.tet_global;
  else if (n == "bptr") v = &P.bptr;
  else if (n == "bcol") v = &P.bcol;
  else if (n == "slice_off") v = &P.slice_off;
  else if (n == "colidx") v = &P.colidx;
  else if (n == "blk_slot") v = &P.blk_slot;
  else if (n == "slot_coff") v = &P.slot_coff;
  else if (n == "slot_ccnt") v = &P.slot_ccnt;
  else if (n == "contrib") { tmp.assign(P.contrib.begin(), P.contrib.end()); v = &tmp; }
  else if (n == "dofmask") { tmp.assign(P.dofmask.begin(), P.dofmask.end()); v = &tmp; }
  else return fb::fail(FB_EINVAL, "unknown plan array '%s'", name);
  if (out) {
    if (capacity < v->size()) return fb::fail(FB_EINVAL, "capacity %zu < %zu", capacity, v->size());
    memcpy(out, v->data(), v->size() * sizeof(int));
  }
  return (int)v->size();
}

int fb_plan_slab_order(int n_nodes, const double* xyz, int n_tets, const int* tets, int* old_of_new, int* span_caller, int* span_internal) {
  if (!xyz || !tets || !old_of_new || n_nodes < 1 || n_tets < 0) return fb::fail(FB_EINVAL, "bad argument");
  std::vector<int> o;
  const int rc = fb::host_slab_order(n_nodes, xyz, n_tets, tets, o, span_caller, span_internal);
  if (rc != FB_OK) return rc;
  memcpy(old_of_new, o.data(), sizeof(int) * (size_t)n_nodes);
  return FB_OK;
}

int fb_plan_shard_vote(int n_nodes, int n_tets, const int* tets, int n_ranks, int rank, const int* node_splits, int out[3]) {
  if (!tets || !out) return fb::fail(FB_EINVAL, "null argument");
  unsigned long long sum = 0;
  int splits_sum = 0;
  fb::shard_neighbour_count(n_nodes, n_tets, tets, n_ranks, rank, node_splits, &out[0], &sum, &splits_sum, &out[1], &out[2]);
  return FB_OK;
}

// Host model of k_pipe_mirror_plan (fem_persist.hip / pcg_pipe.hip.h) over the plan's SELL layout, the slices dealt in equal numbers to nb workgroups
// as pipe_slices does: the same functions of pcg_pipe_mirror.h, the wavefront-wide counts as loops over the 64 lanes.  out[0] = mirror layers,
// out[1] = pool entries, out[2] = fewest plain layers of a slice, out[3] = workgroups that keep mirrors.
int fb_plan_mirror_model(fb_plan_t p, int nb, int c16, int klt, int out[4]) {
  if (!p || !out || nb < 8 || (nb & 7) || (klt != 6 && klt != 7)) return fb::fail(FB_EINVAL, "bad argument");
  out[0] = out[1] = out[3] = 0;
  out[2] = 1 << 30;
  for (int b = 0; b < nb; b++) {
    fb::MirWave mw[fb::kMirWaves];
    int first = 0, count = 0, E = 0;
    const bool ok = mirror_model_wg(p->plan, nb, b, c16, klt, mw, &first, &count, &E);
    for (int w = 0; w < count; w++) { out[0] += mw[w].m; out[2] = std::min(out[2], mw[w].p); }
    out[1] += E;
    out[3] += ok ? 1 : 0;
  }
  return FB_OK;
}

// The register slots that go with that window (pcg_pipe_regs.hip.h; mir_reg_slots / mir_reg_split as k_pipe_mirror_plan and the kernel apply them), per
// slice: parts[slice][6] = slots streamed in front | register slots in front | mirror layers | plain layers (those the slice has) | register slots
// behind | slots streamed behind -- in slot order, they add up to the slice's width.
int fb_plan_regs_model(fb_plan_t p, int nb, int c16, int klt, int regs, int* parts) {
  if (!p || !parts || nb < 8 || (nb & 7) || (klt != 6 && klt != 7) || regs < 0 || regs > 3) return fb::fail(FB_EINVAL, "bad argument");
  for (int b = 0; b < nb; b++) {
    fb::MirWave mw[fb::kMirWaves];
    int first = 0, count = 0, E = 0;
    mirror_model_wg(p->plan, nb, b, c16, klt, mw, &first, &count, &E);
    for (int w = 0; w < count; w++) {
      const fb::MirWave& q = mw[w];
      int nf = 0, nbh = 0;
      fb::mir_reg_split(q, fb::mir_reg_slots(q, regs), &nf, &nbh);
      const int rest = std::max(q.width - q.a - q.m, 0), plain = std::min(q.p, rest);
      int* o = parts + (size_t)6 * (first + w);
      o[0] = q.a - nf; o[1] = nf; o[2] = q.m; o[3] = plain; o[4] = nbh; o[5] = rest - plain - nbh;
    }
  }
  return FB_OK;
}

}  // extern "C"
