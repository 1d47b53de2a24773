// wn_block.h -- device toolkit shared by every R = D = 32, fw = 2 residual-block kernel of wavenet.hip:
// the LDS weight image and its stagers, the tile decode, and the cross-tile ping-pong loop.  (The tile walk is
// xcd_walk / xcd_walk_i in common.h.)
#pragma once
#include "common.h"

// ---- LDS weight image.  The per-lane MFMA fragment pattern is a 128- or 256-byte-strided gather, so a workgroup first
// copies the 3072 weights coalesced into padded (conflict-free) LDS rows and picks its fragments from there:
//   [WIMG_DIL,   + 32 * 65)  W_dil[d][c][k]  as rows of 64 (+1 pad): element (d, c, k) at d * 65 + 2 c + k
//   [WIMG_DENSE, + 32 * 33)  W_dense[r][d]   as rows of 32 (+1 pad): element (r, d) at r * 33 + d
//   [WIMG_BDIL,  + 32)       b_dil   (zeros without a bias)
//   [WIMG_BDENSE, + 32)      b_dense (zeros without a bias)
// The biases stay in LDS and seed the accumulators per tile (32 registers saved).  A kernel that needs only a prefix of
// the image declares only that prefix; the fused backward's image has no dense part and keeps b_dil right behind W_dil.
constexpr int WIMG_DIL_PITCH = 65, WIMG_DENSE_PITCH = 33;
constexpr int WIMG_DIL = 0;
constexpr int WIMG_DENSE = WIMG_DIL + 32 * WIMG_DIL_PITCH;          // 2080
constexpr int WIMG_BDIL = WIMG_DENSE + 32 * WIMG_DENSE_PITCH;       // 3136
constexpr int WIMG_BDENSE = WIMG_BDIL + 32;                         // 3168
constexpr int WIMG_SIZE = WIMG_BDENSE + 32;                         // 3200 floats
constexpr int WIMG_DIL_SIZE = WIMG_DENSE;                           // W_dil alone
constexpr int WIMG_DENSE_SIZE = 32 * WIMG_DENSE_PITCH;              // W_dense alone (an image of its own)

// Stagers: thread `tid` of `nthreads` copies its share; the caller places the barrier.
__device__ __forceinline__ void stage_w_dil(float* img, const float* __restrict__ w_dil, int tid, int nthreads) {
  for (int i = tid; i < 2048; i += nthreads) img[(i >> 6) * WIMG_DIL_PITCH + (i & 63)] = w_dil[i];
}
__device__ __forceinline__ void stage_w_dense(float* img, const float* __restrict__ w_dense, int tid, int nthreads) {
  for (int i = tid; i < 1024; i += nthreads) img[(i >> 5) * WIMG_DENSE_PITCH + (i & 31)] = w_dense[i];
}
__device__ __forceinline__ void stage_bias(float* img, const float* __restrict__ b, int tid) {
  if (tid < 32) img[tid] = b ? b[tid] : 0.f;
}
// the whole image
__device__ __forceinline__ void stage_block_weights(float* img, const float* __restrict__ w_dil, const float* __restrict__ b_dil,
                                                    const float* __restrict__ w_dense, const float* __restrict__ b_dense,
                                                    int tid, int nthreads) {
  stage_w_dil(img + WIMG_DIL, w_dil, tid, nthreads);
  stage_w_dense(img + WIMG_DENSE, w_dense, tid, nthreads);
  stage_bias(img + WIMG_BDIL, b_dil, tid);
  stage_bias(img + WIMG_BDENSE, b_dense, tid);
}

// ---- tile decode: tile index -> sequence b, first sample t0 of the W-sample tile, this lane's sample t = t0 + lane_off and
// whether it exists (t < L).  Tiles are counted per sequence over L: the forward and the fused backward count output
// samples (Lo), the input gradient counts input samples (Lin), the wide forward takes W = 128.
template <int W>
__device__ __forceinline__ int tiles_per_sequence(int L) { return (L + W - 1) >> __builtin_ctz(W); }
struct TilePos { int b, t0, t; bool ok; };
template <int W = 32, class I>
__device__ __forceinline__ TilePos tile_pos(I tile, int tiles_per_seq, int lane_off, int L) {
  TilePos p;
  p.b = (int)(tile / tiles_per_seq);
  p.t0 = (int)(tile - (I)p.b * tiles_per_seq) * W;
  p.t = p.t0 + lane_off;
  p.ok = p.t < L;
  return p;
}

// ---- cross-tile ping-pong: "issue tile + stride into the other register set, compute this one".  Set `a` already holds
// the requests of tile w.first (the caller issues them wherever its prologue wants them in flight); a tile past w.last is
// requested (issue() clamps it to an existing one) and never used.  PIN puts a scheduling barrier between an issue and the
// compute behind it, for bodies whose loads hipcc would otherwise sink down to their consumers.
template <bool PIN, class Set, class Issue, class Compute>
__device__ __forceinline__ void pingpong_tiles(const TileWalkI& w, Set& a, Set& b, Issue issue, Compute compute) {
  for (int tile = w.first; tile < w.last; tile += 2 * w.stride) {
    issue(tile + w.stride, b);             // in flight during the MFMAs below
    if (PIN) __builtin_amdgcn_sched_barrier(0);
    compute(tile, a);
    if (tile + w.stride >= w.last) break;
    issue(tile + 2 * w.stride, a);
    if (PIN) __builtin_amdgcn_sched_barrier(0);
    compute(tile + w.stride, b);
  }
}
// the plain loop of the forms that hold nothing across tiles (the other waves of the SIMD hide the loads)
template <bool PIN, class Set, class Issue, class Compute>
__device__ __forceinline__ void plain_tiles(const TileWalkI& w, Issue issue, Compute compute) {
  for (int tile = w.first; tile < w.last; tile += w.stride) {
    Set a;
    issue(tile, a);
    if (PIN) __builtin_amdgcn_sched_barrier(0);
    compute(tile, a);
  }
}
