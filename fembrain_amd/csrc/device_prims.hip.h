// The rocPRIM primitives of the mesh-side host drivers, each one call: the storage protocol lives in with_temp and nowhere else.
// (A header of its own: rocprim.hpp is most of the compile time of a unit that includes it, and haptic.hip and stress.hip do not.)
#pragma once
#include <rocprim/rocprim.hpp>

#include "common.h"

namespace fb {

// The two calls every rocPRIM primitive takes: call(nullptr, bytes) reports the temporary storage it needs, `temp` grows to it, and
// call(temp.p, bytes) runs in it (run == false: query and growth only, ahead of a timed path).  A primitive still in flight on the
// stream never loses its storage: DevBuf::reserve only grows, and growth goes through hipFree, which waits for the device.
template <class F>
int with_temp(DevBuf<char>& temp, const char* what, F call, bool run = true) {
  size_t bytes = 0;
  hipError_t e = call(nullptr, bytes);
  if (e == hipSuccess) {
    FB_TRY(temp.reserve(std::max<size_t>(bytes, 16)));
    if (run) e = call(temp.p, bytes);
  }
  if (e != hipSuccess) return fail(FB_EDEVICE, "rocprim::%s failed: %s", what, hipGetErrorString(e));
  return FB_OK;
}

// Iterator types pass through as the caller has them (counting and transform iterators, uint32_t views of 64-bit buffers).

// out[i] = init + in[0] + ... + in[i - 1]
template <class In, class Out, class T>
int exclusive_scan(DevBuf<char>& temp, hipStream_t s, In in, Out out, T init, size_t n) {
  return with_temp(temp, "exclusive_scan", [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, in, out, init, n, rocprim::plus<T>(), s); });
}

// stable, ascending in the key bits [0, bits)
template <class KeyIn, class KeyOut, class ValIn, class ValOut>
int sort_pairs(DevBuf<char>& temp, hipStream_t s, KeyIn keys, KeyOut keys_sorted, ValIn vals, ValOut vals_sorted, size_t n, unsigned bits, bool run = true) {
  return with_temp(temp, "radix_sort_pairs", [&](void* t, size_t& b) { return rocprim::radix_sort_pairs(t, b, keys, keys_sorted, vals, vals_sorted, n, 0u, bits, s); }, run);
}

// the in[i] with a non-zero flags[i], in order; their number to *count (device)
template <class In, class Flags, class Out, class Count>
int select_flagged(DevBuf<char>& temp, hipStream_t s, In in, Flags flags, Out out, Count count, size_t n) {
  return with_temp(temp, "select", [&](void* t, size_t& b) { return rocprim::select(t, b, in, flags, out, count, n, s); });
}

// the in[i] with pred(in[i]), in order; their number to *count (device)
template <class In, class Out, class Count, class Pred>
int select_if(DevBuf<char>& temp, hipStream_t s, In in, Out out, Count count, size_t n, Pred pred) {
  return with_temp(temp, "select", [&](void* t, size_t& b) { return rocprim::select(t, b, in, out, count, n, pred, s); });
}

// runs of equal values: the value and the length of each, their number to *n_runs (device)
template <class In, class Unique, class Counts, class Runs>
int run_length_encode(DevBuf<char>& temp, hipStream_t s, In in, unsigned int n, Unique unique, Counts counts, Runs n_runs) {
  return with_temp(temp, "run_length_encode", [&](void* t, size_t& b) { return rocprim::run_length_encode(t, b, in, n, unique, counts, n_runs, s); });
}

// *out (device) = the smallest of in[0 .. n), 1e300 for none
template <class In, class Out>
int min_reduce(DevBuf<char>& temp, hipStream_t s, In in, Out out, size_t n) {
  return with_temp(temp, "reduce", [&](void* t, size_t& b) { return rocprim::reduce(t, b, in, out, 1e300, n, rocprim::minimum<double>(), s); });
}

}  // namespace fb
