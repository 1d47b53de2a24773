// stream_product.h -- the basis-streaming product of the two streaming transforms (stft_stream.hip, istft_stream.hip):
// M = a few frames (1 .. a few hundred) of K = n_fft values each against NP planes of a basis, 16 output columns per
// workgroup.  Not a tile GEMM: workgroup blockIdx.x reads its slab of the basis (NP x 16 x K floats, packed so that a wave's
// operand load is 1 KiB contiguous) once per pass of 16 NG frames, which its kernel has staged in LDS.  The planes of a
// column are accumulators of the same lane.  This header knows the product and nothing of the transform around it: a
// kernel supplies the rows' frame counts, stages the frames and finishes the sums.
//
// SUMMATION ORDER.  One output value is always summed the same way, whatever M, the row or the frame's place in the call:
// wave w of 8 accumulates the 16-value groups kk = w, w + 8, ... of its K-slice in that order (an MFMA column does not see
// the other columns), and the 8 partial sums are added in wave order.  Nothing else enters: no atomics, no second kernel
// form above a size.  This is what makes any split of a stream into calls give the same bits.
//
// LDS.  All of it is the dynamic region, so that its base is offset 0 and every 16-byte access is aligned: the frames
// [16 NG][K + 4]; after the product the same space takes the waves' partial sums [NG][NP][8 waves][64 lanes] x 4; behind
// both (Plan::tab floats in) the pass's per-frame tables.
#pragma once
#include "frames.h"

namespace sprod {

constexpr int NT = 512;             // threads per workgroup: 8 waves over K
constexpr int NW = NT / 64;
constexpr int PAD = 4;              // frame pitch K + 4 floats: the 16 frames of a ds_read_b128 lane group sit on 16 different slots
constexpr size_t LDS_MAX = 150 * 1024;
constexpr int K_MAX = 2048;        // the documented limit of both transforms (include/avvad.h); plan() alone would take what LDS takes, 2368

// index within K that lane-quarter q reads in MFMA j of group kk: both operands use it, so the product is a plain sum
__device__ __forceinline__ int operand_index(int K, int kk, int q, int j) { return (K >> 2) * q + 4 * kk + j; }

// The per-frame tables of a pass of FP frames, TI ints per frame slot: the row, the frame of the row, then TI - 2 arrays
// of the kernel's own; behind them the call's frame count.
template <int FP, int TI>
struct Tables {
  int *fb, *ft;
  __device__ __forceinline__ explicit Tables(float* tab) : fb(reinterpret_cast<int*>(tab)), ft(fb + FP) {}
  __device__ __forceinline__ int* own(int j) const { return fb + (2 + j) * FP; }
  __device__ __forceinline__ int& M() const { return fb[TI * FP]; }
};

// Frame m of the call -> (row, frame of the row) for the pass's frames m0 .. m0 + FP - 1: wave 0 takes a running sum of
// the rows' frame counts, one 64-lane inclusive scan per 64 rows.  count(b) is row b's clamped frame count; the lane that
// owns the row calls own(slot) for each of its frame slots, to fill the kernel's own arrays from what count(b) read.
// Ends in a barrier.  -> the frames of this pass, <= 0 when the call has none left (uniform).
template <int FP, int TI, class Count, class Own>
__device__ __forceinline__ int map_frames(const Tables<FP, TI>& t, int B, int m0, Count count, Own own) {
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < 64) {
    int base = 0;
    for (int c0 = 0; c0 < B; c0 += 64) {
      const int b = c0 + lane;
      const int nf = b < B ? count(b) : 0;
      int incl = nf;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
      }
      const int excl = base + incl - nf;
      const int lo = excl > m0 ? excl : m0, hi = excl + nf < m0 + FP ? excl + nf : m0 + FP;
      for (int m = lo; m < hi; ++m) {
        t.fb[m - m0] = b;
        t.ft[m - m0] = m - excl;
        own(m - m0);
      }
      base += __shfl(incl, 63, 64);
    }
    if (lane == 0) t.M() = base;
  }
  __syncthreads();
  const int left = t.M() - m0;
  return left < FP ? left : FP;
}

// The product of the pass's nfp staged frames with this workgroup's slab (w: plane 0, this lane's first operand; plane p
// lies p K/16 groups behind), handed over through LDS.  Frame rows of a 16-frame group that the pass does not fill keep
// what LDS held: an MFMA column does not see the other columns, and theirs is never finished.  Between its two barriers
// the partial sums replace the frames.
template <int NG, int NP>
__device__ __forceinline__ void product(float* lds, const f32x4* w, int K, int nfp) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int P = K + PAD, KQ = K >> 4;
  f32x4 acc[NG][NP];
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[g][p] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* frow = lds + (lane & 15) * P + (K >> 2) * (lane >> 4);
  for (int kk = wave; kk < KQ; kk += NW) {
    f32x4 c[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) c[p] = w[((long)p * KQ + kk) * 64];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (16 * g < nfp) {                        // uniform
        const f32x4 x = *reinterpret_cast<const f32x4*>(frow + 16 * g * P + 4 * kk);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int p = 0; p < NP; ++p) acc[g][p] = __builtin_amdgcn_mfma_f32_16x16x4f32(c[p][j], x[j], acc[g][p], 0, 0, 0);
      }
    }
  }
  __syncthreads();                               // every wave has read the frames
  f32x4* part = reinterpret_cast<f32x4*>(lds);
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int p = 0; p < NP; ++p) part[((g * NP + p) * NW + wave) * 64 + lane] = acc[g][p];
  __syncthreads();
}

// One finished value: the eight partial sums of register r of `lane`, plane p of frame group g, in wave order.  Register
// r of lane (i, q) is column 4 q + r of frame 16 g + i.  The kernel syncs before it stages the next pass over them.
template <int NP>
__device__ __forceinline__ float finish(const float* lds, int g, int p, int lane, int r) {
  const float* pf = lds + ((g * NP + p) * NW * 64 + lane) * 4 + r;
  float v = pf[0];
  for (int w = 1; w < NW; ++w) v += pf[w * 256];
  return v;
}

// ---- host side: the launch plan of a call with about `hint` frames; tab_ints = ints per frame slot of the kernel's tables
struct Plan {
  int NG;       // 16-frame groups per pass: 2 above 16 frames where LDS takes them; 0: K does not fit at all
  int ny;       // the grid's second dimension: the passes beyond 16 walk it
  size_t lds;   // dynamic LDS bytes
  int tab;      // float offset of the tables
};
static inline size_t lds_bytes(int K, int NP, int tab_ints, int NG, int* tab) {
  const size_t frames = (size_t)16 * NG * (K + PAD) * sizeof(float), parts = (size_t)NG * NP * NW * 64 * sizeof(f32x4);
  const size_t front = frames > parts ? frames : parts;      // both multiples of 16 bytes
  *tab = (int)(front / sizeof(float));
  return front + align_up((size_t)(tab_ints * 16 * NG + 1) * sizeof(int), 16);
}
static inline Plan plan(int K, int NP, int tab_ints, long hint) {
  Plan p;
  p.NG = hint > 16 ? 2 : 1;
  p.lds = lds_bytes(K, NP, tab_ints, p.NG, &p.tab);
  if (p.NG == 2 && p.lds > LDS_MAX) p.lds = lds_bytes(K, NP, tab_ints, p.NG = 1, &p.tab);
  const long ny = (hint + 16 * p.NG - 1) / (16 * p.NG);
  p.ny = (int)(ny < 1 ? 1 : (ny > 16 ? 16 : ny));
  if (p.lds > LDS_MAX) p.NG = 0;
  return p;
}

template <auto Kernel, class Args>
int launch(const Args& a, dim3 grid, size_t lds, hipStream_t s) {
  if (int rc = allow_large_lds<Kernel>(lds, LDS_MAX)) return rc;
  hipLaunchKernelGGL(Kernel, grid, dim3(NT), lds, s, a);
  return AVVAD_OK;
}

}  // namespace sprod
