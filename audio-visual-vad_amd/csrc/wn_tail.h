// wn_tail.h -- device code of the encoder's tail (bottleneck 1x1 + ReLU + adaptive average pool) and the fixed-order slab
// reduce, included by wavenet.hip only: a toolkit whose pieces are each written once, the tail kernels built from it, and the
// constexpr sizes that the kernels' LDS carve-ups and the launchers share.  (Form choice and launchers: wavenet.hip.)
#pragma once
#include "common.h"

namespace {

// ---- sizes.  The fused backward forms leave one slab of partial sums per workgroup: dW_b[bn][c] at bn * 32 + c, then db[bn].
constexpr int TAIL_MAXBLK = 256;        // workgroups (= slabs) of a fused tail backward: 1 workgroup / CU is resident, one round
constexpr int TAIL_PITCH = 33;          // padded row of a 32-float LDS row (conflict-free both ways)
constexpr int TAIL_TILE = 32 * TAIL_PITCH;
constexpr int tail_wimg_floats(int Bn) { return Bn * TAIL_PITCH; }
constexpr int tail_slab_floats(int Bn) { return Bn * 32 + Bn; }
// dynamic LDS of a fused form, 4 * WPT waves: weight image, slab, two transpose tiles per wave, (WPT = 2) a hand-off tile per pair
constexpr int tail_fused_lds_floats(int Bn, int WPT) {
  return tail_wimg_floats(Bn) + tail_slab_floats(Bn) + 4 * WPT * 2 * TAIL_TILE + (WPT == 2 ? 4 * TAIL_TILE : 0);
}

// ---- toolkit
__device__ __forceinline__ void pool_bin(int p, int Lv, int P, int& a, int& e) {
  a = (int)(((long)p * Lv) / P);
  e = (int)((((long)(p + 1)) * Lv + P - 1) / P);
}
// The bottleneck weights (Bn x 32) go coalesced into padded LDS, element (bn, c) at bn * 33 + c, once per workgroup (the caller
// places the barrier): the per-lane fragment pattern, a 128-byte-strided gather from memory, made these kernels TA-bound.
__device__ __forceinline__ void stage_tail_weights(float* img, const float* __restrict__ wb, int Bn, int tid, int nthreads) {
  for (int i = tid; i < Bn * 32; i += nthreads) img[(i >> 5) * TAIL_PITCH + (i & 31)] = wb[i];
}
// Pool bins that contain sample t, P <= Lv (see tail_bwd_form): candidate j is bin floor(t P / Lv) - 1 + j, pb[j] the bin
// clamped to a valid one, pc[j] = 1 / its length, or 0 when t is not a member.
struct PoolWindow { int pb[3]; float pc[3]; };
__device__ __forceinline__ PoolWindow pool_window(int t, bool ok, int Lv, int P) {
  PoolWindow w;
  const int c0 = ok ? (int)(((long)t * P) / Lv) : 0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int p = c0 - 1 + j;
    int a = 0, e = 0;
    const bool in = ok && p >= 0 && p < P;
    if (in) pool_bin(p, Lv, P, a, e);
    const bool hit = in && t >= a && t < e;
    w.pb[j] = hit ? p : 0;
    w.pc[j] = hit ? 1.f / (float)(e - a) : 0.f;
  }
  return w;
}
// z tile of rows nb .. nb + 31 (D layout: row mfma32_row(r, lh), column = time on the lane) from the s tile x[k] = s[2k + lh][t]
__device__ __forceinline__ f32x16 tail_z_tile(const float* wl, const float* __restrict__ bb, int nb, const float (&x)[16], int li, int lh) {
  f32x16 accZ;
#pragma unroll
  for (int r = 0; r < 16; ++r) accZ[r] = bb ? bb[nb + mfma32_row(r, lh)] : 0.f;
  float wz[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) wz[k] = wl[(nb + li) * TAIL_PITCH + 2 * k + lh];   // A[i = bn][k = c]
#pragma unroll
  for (int k = 0; k < 16; ++k) accZ = mfma32(wz[k], x[k], accZ);
  return accZ;
}
// dz = (z > 0) * pooled upstream gradient; fetch(r) is that gradient for register r's row
template <class Fetch>
__device__ __forceinline__ void tail_dz_tile(const f32x16& accZ, Fetch fetch, float (&dz)[16]) {
#pragma unroll
  for (int r = 0; r < 16; ++r) { const float g = fetch(r); dz[r] = accZ[r] > 0.f ? g : 0.f; }     // (fetched whatever z is)
}
// dS[c][t] += sum_bn Wb[bn][c] dz[bn][t] over rows nb .. nb + 31 (16 MFMAs, the dz tile in place as the B operand); a form
// reads the weight fragment where its register budget wants it
__device__ __forceinline__ void tail_wt_frag(const float* wl, int nb, int li, int lh, float (&wt)[16]) {
#pragma unroll
  for (int k = 0; k < 16; ++k) wt[k] = wl[(nb + mfma32_row(k, lh)) * TAIL_PITCH + li];   // A[i = c][k = bn]
}
__device__ __forceinline__ void tail_ds_product(f32x16& accS, const float (&wt)[16], const float (&dz)[16]) {
#pragma unroll
  for (int r = 0; r < 16; ++r) accS = mfma32(wt[r], dz[r], accS);
}
// tile (time on the lane; register k holds row 2k + lh, or row mfma32_row(k, lh) with DLAYOUT) -> fragment
// f[q] = tile[row = li][t = 2q + lh], through this wave's own 32 x 33 LDS tile
template <bool DLAYOUT>
__device__ __forceinline__ void tile_to_fragment(float* T, const float (&v)[16], float (&f)[16], int li, int lh) {
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int k = 0; k < 16; ++k) T[(DLAYOUT ? mfma32_row(k, lh) : 2 * k + lh) * TAIL_PITCH + li] = v[k];
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int q = 0; q < 16; ++q) f[q] = T[li * TAIL_PITCH + 2 * q + lh];
}
// The waves' sums meet in LDS in WAVE ORDER: plain adds between barriers, not LDS atomics in arrival order.
template <class Add>
__device__ __forceinline__ void meet_in_wave_order(int nwaves, int wave, Add add) {
  for (int w = 0; w < nwaves; ++w) {
    __syncthreads();
    if (wave == w) add();
  }
}
// Fixed-order sum of one element (el_ptr: in slab 0) over `nslab` slabs of `pitch` floats.  A workgroup of 256 = 32 elements x
// 8 slab groups: ascending slabs inside a group, the groups combined in LDS in order; the total goes to threadIdx.x < 32.
__device__ __forceinline__ float slab_sum_fixed_order(const float* __restrict__ el_ptr, int nslab, int pitch) {
  __shared__ float sm[8][32];
  const int el = threadIdx.x & 31, grp = threadIdx.x >> 5;
  float s = 0.f;
#pragma unroll 4
  for (int b = grp; b < nslab; b += 8) s += el_ptr[(long)b * pitch];
  sm[grp][el] = s;
  __syncthreads();
  if (grp == 0) {
#pragma unroll
    for (int k = 1; k < 8; ++k) s += sm[k][el];
  }
  return s;
}

// ---- generic direct kernels (any R, Bn, P)
// out[b][bn][p] = mean_{t in bin p} relu(bb[bn] + sum_c Wb[bn][c] s[b][c][t])
__global__ void __launch_bounds__(256)
    tail_fwd_generic(const float* __restrict__ s, const float* __restrict__ wb, const float* __restrict__ bb,
                     float* __restrict__ out, int R, int Bn, int Lv, int P) {
  const int b = blockIdx.y, p = blockIdx.x;
  int a, e;
  pool_bin(p, Lv, P, a, e);
  const float* sb = s + (long)b * R * Lv;
  for (int bn = threadIdx.x; bn < Bn; bn += 256) {
    const float* wr = wb + (long)bn * R;
    const float bias = bb ? bb[bn] : 0.f;
    float sum = 0.f;
    for (int t = a; t < e; ++t) {
      float z = bias;
      for (int c = 0; c < R; ++c) z = fmaf(wr[c], sb[(long)c * Lv + t], z);
      sum += fmaxf(z, 0.f);
    }
    out[((long)b * Bn + bn) * P + p] = sum / (float)(e - a);
  }
}

// dz[b][bn][t] = (z>0) * sum_{p: t in bin p} dout[b][bn][p] / len_p
__global__ void tail_bwd_dz_generic(const float* __restrict__ s, const float* __restrict__ wb, const float* __restrict__ bb,
                                    const float* __restrict__ dout, float* __restrict__ dz, int B, int R, int Bn, int Lv, int P) {
  const long n = (long)B * Bn * Lv;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int t = (int)(i % Lv);
    const int bn = (int)((i / Lv) % Bn);
    const int b = (int)(i / ((long)Lv * Bn));
    float z = bb ? bb[bn] : 0.f;
    const float* sb = s + (long)b * R * Lv + t;
    for (int c = 0; c < R; ++c) z = fmaf(wb[(long)bn * R + c], sb[(long)c * Lv], z);
    float g = 0.f;
    if (z > 0.f) {
      // the bins that contain t are exactly floor(t P / Lv) .. ceil((t + 1) P / Lv) - 1: two at the most while P <= Lv,
      // any number beyond (Lv = 3, P = 5: sample 1 is in bins 1, 2, 3)
      const int p0 = (int)(((long)t * P) / Lv), p1 = (int)((((long)t + 1) * P + Lv - 1) / Lv);
      for (int p = p0; p < p1; ++p) {
        int a, e;
        pool_bin(p, Lv, P, a, e);
        g += dout[((long)b * Bn + bn) * P + p] / (float)(e - a);
      }
    }
    dz[i] = g;
  }
}

// ---- MFMA forward (R = 32, Bn % 32 == 0)
// One wave per (sequence, pool bin, group of NT bn-tiles).  Transposed product z^T[t][bn] = s^T . Wb^T: the
// activation tile is the A operand (lane = time, loaded as it lies in memory), the weights the B operand, so the
// accumulator has TIME IN ITS REGISTERS and bn on the lane: the pool is 16 register adds + one lane-half swap.
template <int NT>
__global__ void __launch_bounds__(256)
    tail_fwd_mfma(const float* __restrict__ s, const float* __restrict__ wb, const float* __restrict__ bb,
                  float* __restrict__ out, int B, int Bn, int Lv, int P) {
  const int lane = threadIdx.x & 63;
  const int li = lane & 31, lh = lane >> 5;
  const int ngrp = Bn / (32 * NT);
  const long nitems = (long)B * P * ngrp;
  const long nwaves = ((long)gridDim.x * blockDim.x) >> 6;
  for (long item = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; item < nitems; item += nwaves) {
    const int grp = (int)(item % ngrp);
    const int p = (int)((item / ngrp) % P);
    const int b = (int)(item / ((long)ngrp * P));
    const int bn0 = grp * 32 * NT;
    int a, e;
    pool_bin(p, Lv, P, a, e);
    float w[NT][16], bias[NT], sum[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
#pragma unroll
      for (int k = 0; k < 16; ++k) w[n][k] = wb[(long)(bn0 + n * 32 + li) * 32 + 2 * k + lh];
      bias[n] = bb ? bb[bn0 + n * 32 + li] : 0.f;
      sum[n] = 0.f;
    }
    const float* sp = s + (long)b * 32 * Lv;
    for (int t0 = a; t0 < e; t0 += 32) {
      const int t = t0 + li;
      const bool ok = t < e;
      const int tcl = ok ? t : a;
      float x[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) x[k] = sp[(long)(2 * k + lh) * Lv + tcl];
#pragma unroll
      for (int k = 0; k < 16; ++k) x[k] = ok ? x[k] : 0.f;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        f32x16 acc = {};
#pragma unroll
        for (int k = 0; k < 16; ++k) acc = mfma32(x[k], w[n][k], acc);
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (t0 + mfma32_row(r, lh) < e) sum[n] += relu1(acc[r] + bias[n]);
      }
    }
    const float inv = 1.f / (float)(e - a);
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const float v = sum[n] + __shfl_xor(sum[n], 32, 64);
      if (lh == 0) out[((long)b * Bn + bn0 + n * 32 + li) * P + p] = v * inv;
    }
  }
}

// ---- MFMA backward, unfused (R = 32, Bn % 32 == 0): one 32-sample tile per wave; dz is written out as dz_t for the engine's
// weight gradients.  Flat loads (buffer descriptors would put a length limit on this form), always the sum of three candidates.
__global__ void __launch_bounds__(256)
    tail_bwd_mfma(const float* __restrict__ s, const float* __restrict__ wb, const float* __restrict__ bb,
                  const float* __restrict__ dout, float* __restrict__ dzt, float* __restrict__ dS, int B, int Bn, int Lv, int P) {
  const int lane = threadIdx.x & 63;
  const int li = lane & 31, lh = lane >> 5;
  const int tiles_per_seq = (Lv + 31) >> 5;
  const long ntiles = (long)B * tiles_per_seq;
  const long nwaves = ((long)gridDim.x * blockDim.x) >> 6;
  extern __shared__ float wl[];
  stage_tail_weights(wl, wb, Bn, threadIdx.x, 256);
  __syncthreads();
  for (long tile = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; tile < ntiles; tile += nwaves) {
    const int b = (int)(tile / tiles_per_seq);
    const int t = (int)(tile - (long)b * tiles_per_seq) * 32 + li;
    const bool ok = t < Lv;
    const float* sp = s + (long)b * 32 * Lv + (ok ? t : 0);
    float x[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) x[k] = sp[(long)(2 * k + lh) * Lv];
#pragma unroll
    for (int k = 0; k < 16; ++k) x[k] = ok ? x[k] : 0.f;
    const PoolWindow pw = pool_window(t, ok, Lv, P);
    f32x16 accS = {};
    for (int nb = 0; nb < Bn; nb += 32) {
      const f32x16 accZ = tail_z_tile(wl, bb, nb, x, li, lh);
      float dz[16];
      tail_dz_tile(accZ, [&](int r) {
        const long o = ((long)b * Bn + nb + mfma32_row(r, lh)) * P;
        float g = 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) g = fmaf(dout[o + pw.pb[j]], pw.pc[j], g);
        return g;
      }, dz);
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (ok) dzt[((long)b * Bn + nb + mfma32_row(r, lh)) * Lv + t] = dz[r];
      float wt[16];
      tail_wt_frag(wl, nb, li, lh, wt);
      tail_ds_product(accS, wt, dz);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (ok) dS[((long)b * 32 + mfma32_row(r, lh)) * Lv + t] = accS[r];
  }
}

// ---- tail backward + bottleneck weight/bias gradients in ONE pass (Bn = 32 NBT; measurements: DESIGN.md section 4)
// tail_bwd_mfma writes dz_t (268 MB at the bench shape) only for a GEMM and a column sum to read it back.  Here each dz tile
// goes from the accumulator through a per-wave 32x33 LDS transpose straight into resident 32x32 weight-gradient accumulators
// (dW_b[bn][c], one per bn tile); the s tile is transposed once per time tile.  Partial sums leave through per-workgroup slabs.
// ONE body, WPT waves per time tile: 1 -- a wave keeps all NBT accumulators (one wave per SIMD at NBT = 8); 2 -- waves 2p and
// 2p + 1 share tile after tile, each takes HALF of the bottleneck rows and a partial sum of d s over them, which wave 2p + 1
// hands through LDS to wave 2p: half the registers, twice the waves, two chains interleave on every SIMD.
template <int NBT, int WPT>
__device__ __forceinline__ void tail_bwd_wgrad_body(const float* __restrict__ s, const float* __restrict__ wb,
                                                    const float* __restrict__ bb, const float* __restrict__ dout,
                                                    float* __restrict__ dS, float* __restrict__ slab, int B, int Lv, int P) {
  static_assert((WPT == 1 || WPT == 2) && NBT % WPT == 0, "one wave per time tile, or two that halve the bottleneck rows");
  constexpr int Bn = NBT * 32, NH = NBT / WPT, NWAVES = 4 * WPT, NTHREADS = 64 * NWAVES, SLAB = tail_slab_floats(Bn);
  extern __shared__ float wl[];                 // Bn x 33 padded weights
  float* red = wl + tail_wimg_floats(Bn);       // SLAB partial sums of this workgroup
  float* tiles = red + SLAB;                    // per wave 2 transpose tiles of 32 x 33, then (WPT = 2) one tile per pair
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int pair = wave >> 1, half = WPT == 2 ? wave & 1 : 0;
  const int tiles_per_seq = (Lv + 31) >> 5;
  const long ntiles = (long)B * tiles_per_seq;
  float *T0 = tiles + wave * 2 * TAIL_TILE, *T1 = T0 + TAIL_TILE;     // this wave's s tile and dz tile
  float* PS = tiles + (NWAVES * 2 + pair) * TAIL_TILE;     // the odd wave's partial d s
  stage_tail_weights(wl, wb, Bn, threadIdx.x, NTHREADS);
  for (int i = threadIdx.x; i < SLAB; i += NTHREADS) red[i] = 0.f;
  __syncthreads();
  f32x16 accW[NH] = {};
  float bsum[NH] = {};
  // buffer addressing: the flat form spent ~1150 VALU instructions per tile on the addresses of the 384 pooled-gradient gathers
  const int rowV = Lv * 4;
  const bool single = (Lv % P) == 0;
  auto one_tile = [&](long tile, bool live) __attribute__((always_inline)) {
    const int b = __builtin_amdgcn_readfirstlane((int)((live ? tile : 0) / tiles_per_seq));
    const int t = (int)((live ? tile : 0) - (long)b * tiles_per_seq) * 32 + li;
    const bool ok = live && t < Lv;
    const __amdgpu_buffer_rsrc_t rs = brsrc(s + (long)b * 32 * Lv, 32 * rowV);
    const __amdgpu_buffer_rsrc_t rd = brsrc(dS + (long)b * 32 * Lv, 32 * rowV);
    const __amdgpu_buffer_rsrc_t rg = brsrc(dout + (long)b * Bn * P, Bn * P * 4);
    const int offs = ok ? t * 4 + lh * rowV : BUF_OOB;            // s row 2k + lh
    const int offd = ok ? t * 4 + 4 * lh * rowV : BUF_OOB;        // dS row mfma32_row(r, lh)
    float x[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) x[k] = bload(rs, offs, 2 * k * rowV);   // 0 past the sequence
    __builtin_amdgcn_sched_barrier(0);     // keep the 16 loads together (see wn_block_bwd_dz_wgrad_body)
    const PoolWindow pw = pool_window(t, ok, Lv, P);
    int pbo[3];       // byte offset of (row 4 lh, bin pb[j]) inside this sequence's dout slab; the row of register r is scalar
#pragma unroll
    for (int j = 0; j < 3; ++j) pbo[j] = (pw.pb[j] + 4 * lh * P) * 4;
    float fs[16];     // fs[q] = s[c = li][t = 2q + lh]  (B operand of the weight-gradient products)
    tile_to_fragment<false>(T0, x, fs, li, lh);
    f32x16 accS = {};
#pragma unroll
    for (int n = 0; n < NH; ++n) {
      const int nb = (half * NH + n) * 32;
      float wt[16];     // one wave: read ahead of the z rebuild (behind it hipcc spills one more scalar register)
      if constexpr (WPT == 1) tail_wt_frag(wl, nb, li, lh, wt);
      const f32x16 accZ = tail_z_tile(wl, bb, nb, x, li, lh);
      if constexpr (WPT == 2) __builtin_amdgcn_sched_barrier(0);      // (phase by phase: hoisted, the next phases' operands spill)
      float dz[16];
      tail_dz_tile(accZ, [&](int r) {
        const int row = (nb + mfma32_row(r, 0)) * P * 4;
        // Lv % P == 0: the bins do not overlap, candidate 1 (bin t P / Lv) is the only member
        if (single) return bload(rg, pbo[1], row) * pw.pc[1];
        float g = 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) g = fmaf(bload(rg, pbo[j], row), pw.pc[j], g);
        return g;                                                      // (0 outside the sequence: pc = 0)
      }, dz);
      if constexpr (WPT == 2) {
        __builtin_amdgcn_sched_barrier(0);
        tail_wt_frag(wl, nb, li, lh, wt);
      }
      tail_ds_product(accS, wt, dz);
      if constexpr (WPT == 2) __builtin_amdgcn_sched_barrier(0);
      float fz[16];     // fz[q] = dz[bn = li][t = 2q + lh]
      tile_to_fragment<true>(T1, dz, fz, li, lh);
#pragma unroll
      for (int q = 0; q < 16; ++q) bsum[n] += fz[q];
#pragma unroll
      for (int q = 0; q < 16; ++q) accW[n] = mfma32(fz[q], fs[q], accW[n]);
    }
    if constexpr (WPT == 2) {
      // d s = (rows of the first half) + (rows of the second half): the odd wave's partial crosses LDS, the even wave adds and stores
      if (half == 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) PS[mfma32_row(r, lh) * TAIL_PITCH + li] = accS[r];
      }
      __syncthreads();
      if (half == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) bstore(accS[r] + PS[mfma32_row(r, lh) * TAIL_PITCH + li], rd, offd, mfma32_row(r, 0) * rowV);
      }
      __syncthreads();                     // (PS is free for the next round)
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) bstore(accS[r], rd, offd, mfma32_row(r, 0) * rowV);
    }
  };
  if constexpr (WPT == 2) {
    // every pair of the workgroup runs the same number of rounds (one_tile's barriers are workgroup barriers)
    const long npairs = (long)gridDim.x * 4;
    const long rounds = (ntiles + npairs - 1) / npairs;
    for (long rd_ = 0; rd_ < rounds; ++rd_) {
      const long tile = rd_ * npairs + (long)blockIdx.x * 4 + pair;
      one_tile(tile, tile < ntiles);
    }
  } else {
    const long nwaves = ((long)gridDim.x * blockDim.x) >> 6;
    for (long tile = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; tile < ntiles; tile += nwaves) one_tile(tile, true);
  }
  meet_in_wave_order(NWAVES, wave, [&] {
#pragma unroll
    for (int n = 0; n < NH; ++n) {
#pragma unroll
      for (int r = 0; r < 16; ++r) red[((half * NH + n) * 32 + mfma32_row(r, lh)) * 32 + li] += accW[n][r];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {      // the bias sums: both lane halves hold partial sums of the same 32 rows -> half 0 first
      if (h == 1) __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int n = 0; n < NH; ++n)
        if (lh == h) red[Bn * 32 + (half * NH + n) * 32 + li] += bsum[n];
    }
  });
  __syncthreads();
  float* out = slab + (long)blockIdx.x * SLAB;
  for (int i = threadIdx.x; i < SLAB; i += NTHREADS) out[i] = red[i];
}

// one wave per time tile (option wn_no_tail_pair)
template <int NBT>
__global__ void __launch_bounds__(256)
    tail_bwd_wgrad_mfma(const float* __restrict__ s, const float* __restrict__ wb, const float* __restrict__ bb,
                        const float* __restrict__ dout, float* __restrict__ dS, float* __restrict__ slab, int B, int Lv, int P) {
  tail_bwd_wgrad_body<NBT, 1>(s, wb, bb, dout, dS, slab, B, Lv, P);
}

// two waves per time tile (8 waves per workgroup, two per SIMD): the default
template <int NBT>
__global__ void __launch_bounds__(512, 2)
    tail_bwd_wgrad_pair(const float* __restrict__ s, const float* __restrict__ wb, const float* __restrict__ bb,
                        const float* __restrict__ dout, float* __restrict__ dS, float* __restrict__ slab, int B, int Lv, int P) {
  tail_bwd_wgrad_body<NBT, 2>(s, wb, bb, dout, dS, slab, B, Lv, P);
}

// dW_b[bn][c] += sum_blocks slab[bn*32 + c]; db[bn] += slab[Bn*32 + bn], in the fixed order of slab_sum_fixed_order
__global__ void __launch_bounds__(256)
    tail_wgrad_reduce(const float* __restrict__ slab, int nslab, int Bn, float* __restrict__ dW, float* __restrict__ db) {
  const int n = tail_slab_floats(Bn);
  const int i = blockIdx.x * 32 + (threadIdx.x & 31);
  const float sum = slab_sum_fixed_order(slab + i, i < n ? nslab : 0, n);
  if (threadIdx.x >= 32 || i >= n) return;
  if (i < Bn * 32) { if (dW) dW[i] += sum; }
  else if (db) db[i - Bn * 32] += sum;
}

}  // namespace
