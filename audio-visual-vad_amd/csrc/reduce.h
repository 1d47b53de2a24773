// reduce.h -- the fixed-order reductions and the ragged row lengths of the signal and label kernels (scores, mix,
// spectral_loss, stoi, stats, target, lip, istft).  Those files promise results that are bit-identical run to run and
// between entry points that share a sum; the promise rests on two orders, and both live here and nowhere else:
//   across a wave      the xor butterfly over lane offsets 32, 16, 8, 4, 2, 1 (wave_fold)
//   across four waves  lane 0 of wave w puts its wave's value into red[w]; behind the caller's barrier the four meet as
//                      op(op(op(red[0], red[1]), red[2]), red[3])                                 (fold4_put, fold4_get)
// Changing either changes bits in every file above at once, which is the point of having one copy.
#pragma once
#include "common.h"

struct Add {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};

// every lane gets op over the wave's 64 values of v; `op` takes (own, other lane's)
template <class T, class Op>
__device__ __forceinline__ T wave_fold(T v, Op op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  return v;
}
template <class T>
__device__ __forceinline__ T wave_sum(T v) { return wave_fold(v, Add()); }      // double, float, int, long long

// The tail of a 256-thread workgroup.  The caller declares the LDS (`__shared__ double red[NC][4]`: a row per value, or
// `red[4]` for one), puts its values, has ONE __syncthreads() -- so a workgroup that leaves early must leave before the
// put -- and then any thread gets any row.
template <int NC, class T, class Op>
__device__ __forceinline__ void fold4_put(T (&red)[NC][4], const T (&v)[NC], Op op) {
  T s[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) s[c] = wave_fold(v[c], op);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c) red[c][threadIdx.x >> 6] = s[c];
  }
}
template <class T, class Op>
__device__ __forceinline__ void fold4_put(T (&red)[4], T v, Op op) {
  v = wave_fold(v, op);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
}
template <class T, class Op>
__device__ __forceinline__ T fold4_get(const T (&red)[4], Op op) { return op(op(op(red[0], red[1]), red[2]), red[3]); }

// acc + p[k0 * stride] + ... + p[(k1 - 1) * stride], added one by one in ascending k; UN loads are in flight at a time
template <int UN>
__device__ __forceinline__ double add_ascending(double acc, const double* __restrict__ p, long stride, int k0, int k1) {
  int k = k0;
  for (; k + UN <= k1; k += UN) {
    double t[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) t[u] = p[(long)(k + u) * stride];
#pragma unroll
    for (int u = 0; u < UN; ++u) acc += t[u];
  }
  for (; k < k1; ++k) acc += p[(long)k * stride];
  return acc;
}

// What row b holds of at most `hi`: everything without a count array, else n[b] clamped to [0, hi] -- a wrong count cannot
// reach outside a buffer.  row_len for sample counts (long), row_count for frame counts (int).
__device__ __forceinline__ long row_len(const int* __restrict__ n, int b, long hi) {
  if (!n) return hi;
  const int v = n[b];
  return v < 0 ? 0 : (v > hi ? hi : v);
}
__device__ __forceinline__ int row_count(const int* __restrict__ n, int b, int hi) { return n ? clamp_count(n[b], hi) : hi; }

// chunks of `chunk` that cover n: the kernels' grids and the host's workspace sizes count them the same way
__host__ __device__ inline long chunks_of(long n, long chunk) { return (n + chunk - 1) / chunk; }
