// wavenet.hip -- WaveNet-style encoder (valid dilated Conv1d stack): forward and backward.
//
// Replaces wavenet_autoencoder._encode, packages/models/wavenet_autoencoder.py:74-93:
//   s0 = causal(wave)                                            (:75)
//   s_{i+1} = dense_i(relu(dil_i(relu(s_i)))) + s_i[:, :, -len:]   (:78-86)
//   out = AdaptiveAvgPool1d(P)(relu(bottleneck(s_N)))            (:88-92)
// Layout: [B][C][L] fp32, time contiguous (the reference's NCL).
//
// Production shape (R = D = 32, filter_width 2) runs a fused MFMA kernel per
// residual block: one wave owns a 32-sample time tile; lane half h of the wave
// streams tap h (x[c][t + h*d]) straight from HBM into the B operand of
// v_mfma_f32_32x32x2_f32 -- the dilation gather is the lane-half assignment,
// no LDS, no shuffles -- and the first GEMM's accumulator tile (rows = dilation
// channels in registers, column = time on the lane) is consumed in place as the
// B operand of the 1x1 "dense" GEMM (k-order permuted to the accumulator's row
// order).  ReLUs, both biases and the left-cropped residual are fused; each
// activation is read once (+ once for the residual, an L2 hit) and written once.
// The block kernels come in several forms of the same arithmetic (options wn_flat,
// wn_dx, wn_bwd_t): buffer-addressed with the weights read
// from LDS and 4 waves per SIMD (the default for short planes), 16-byte memory
// instructions over 128-sample super-tiles (long planes), resident weights with a
// cross-tile prefetch (beside another stream's kernels), flat addressing (round 1).
// Any other (R, D, filter_width) runs generic direct kernels.
// Weight gradients contract over (sequence, time) on the igemm engine.
// The tail (bottleneck 1x1, ReLU, adaptive average pool) has its device code in wn_tail.h; its form choice and launchers are here.
#include "gemm_api.h"
#include "wn_block.h"
#include "wn_tail.h"

namespace {

static inline int grid1(long n) { long b = (n + 255) / 256; return (int)(b > 8192 ? 8192 : (b < 1 ? 1 : b)); }

// ------------------------------------------------------------------ generic direct kernels
// y[b][co][t] = bias[co] + sum_{ci,k} w[co][ci][k] * f(x[b][ci][t + k*dil])  (+ res[b][co][t + res_off])
__global__ void conv1d_fwd_generic(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                   const float* __restrict__ res, float* __restrict__ y, int B, int Cin, int Cout, int Lin,
                                   int Lout, int fw, int dil, int relu_in, int res_off, int res_L) {
  const long n = (long)B * Cout * Lout;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int t = (int)(i % Lout);
    const int co = (int)((i / Lout) % Cout);
    const int b = (int)(i / ((long)Lout * Cout));
    float acc = bias ? bias[co] : 0.f;
    const float* xb = x + (long)b * Cin * Lin + t;
    const float* wr = w + (long)co * Cin * fw;
    for (int ci = 0; ci < Cin; ++ci)
      for (int k = 0; k < fw; ++k) {
        float v = xb[(long)ci * Lin + k * dil];
        if (relu_in) v = fmaxf(v, 0.f);
        acc = fmaf(wr[ci * fw + k], v, acc);
      }
    if (res) acc += res[((long)b * Cout + co) * res_L + t + res_off];
    y[i] = acc;
  }
}

// dx[b][ci][ti] = mask(xmask>0) * sum_{co,k} w[co][ci][k] dy[b][co][ti - k*dil]   (+ res[b][ci][ti - res_off])
__global__ void conv1d_bwd_data_generic(const float* __restrict__ dy, const float* __restrict__ w,
                                        const float* __restrict__ xmask, const float* __restrict__ res, float* __restrict__ dx,
                                        int B, int Cin, int Cout, int Lin, int Lout, int fw, int dil, int res_off, int res_L) {
  const long n = (long)B * Cin * Lin;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int ti = (int)(i % Lin);
    const int ci = (int)((i / Lin) % Cin);
    const int b = (int)(i / ((long)Lin * Cin));
    float acc = 0.f;
    if (!xmask || xmask[i] > 0.f) {
      for (int k = 0; k < fw; ++k) {
        const int to = ti - k * dil;
        if (to < 0 || to >= Lout) continue;
        const float* dyb = dy + (long)b * Cout * Lout + to;
        for (int co = 0; co < Cout; ++co) acc = fmaf(w[((long)co * Cin + ci) * fw + k], dyb[(long)co * Lout], acc);
      }
    }
    if (res && ti >= res_off && ti - res_off < res_L) acc += res[((long)b * Cin + ci) * res_L + ti - res_off];
    dx[i] = acc;
  }
}

// db[c] += sum_{b,t} dy[b][c][t]
__global__ void __launch_bounds__(256) chan_sum_acc(const float* __restrict__ dy, float* __restrict__ db, int B, int C, int L) {
  __shared__ float sm[256];
  const int c = blockIdx.x;
  float s = 0.f;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const float* p = dy + ((long)b * C + c) * L;
    for (int t = threadIdx.x; t < L; t += 256) s += p[t];
  }
  sm[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) db[c] += sm[0];     // gridDim.y == 1: one workgroup per channel, a fixed summation order
}

// Causal layer (few input channels, Cin*fw <= 4 weights per output channel): weight AND bias gradient in one pass over dy
//   dw[co][ci][k] += sum_{b,t} dy[b][co][t] x[b][ci][t + k]      db[co] += sum_{b,t} dy[b][co][t]
// (the engine's 64x64 tile on this 32 x 2 product ran 168 us; this reads dy once at HBM rate)
__global__ void __launch_bounds__(256)
    narrow_conv1d_grads(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ part,
                        int B, int Cout, int Cin, int Lout, int Lin, int fw) {
  __shared__ float sm[5][256];
  const int co = blockIdx.x, nw = Cin * fw;
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const float* p = dy + ((long)b * Cout + co) * Lout;
    const float* xb = x + (long)b * Cin * Lin;
    for (int t = threadIdx.x; t < Lout; t += 256) {
      const float g = p[t];
      acc[4] += g;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nw) acc[j] = fmaf(g, xb[(long)(j / fw) * Lin + t + (j % fw)], acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 5; ++j) sm[j][threadIdx.x] = acc[j];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o)
#pragma unroll
      for (int j = 0; j < 5; ++j) sm[j][threadIdx.x] += sm[j][threadIdx.x + o];
    __syncthreads();
  }
  // partial sums of this (channel, sequence group); narrow_conv1d_grads_sum adds the groups in order (deterministic)
  if (threadIdx.x < 5) part[((long)blockIdx.y * Cout + co) * 5 + threadIdx.x] = sm[threadIdx.x][0];
}
__global__ void narrow_conv1d_grads_sum(const float* __restrict__ part, int ny, int Cout, int nw, float* __restrict__ dw,
                                        float* __restrict__ db) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Cout * 5) return;
  const int co = i / 5, j = i - co * 5;
  float s = 0.f;
  for (int y = 0; y < ny; ++y) s += part[((long)y * Cout + co) * 5 + j];
  if (j < 4) { if (j < nw && dw) dw[(long)co * nw + j] += s; }
  else if (db) db[co] += s;
}

// ------------------------------------------------------------------ fused MFMA residual block (R = D = 32, fw = 2)
// The device toolkit every block kernel below stands on -- the LDS weight image and its stagers, the tile decode, the
// ping-pong loop -- is wn_block.h; the tile walk is xcd_walk in common.h.
// FLAT-ADDRESSED form (round 1; the fallback for planes of >= 2 GiB).  MODE 0: write s_out; MODE 2: write z (the pre-ReLU
// dilation output) only, for the unfused backward.
template <int MODE>
__global__ void __launch_bounds__(256)
    wn_block_fwd_mfma(const float* __restrict__ s_in, const float* __restrict__ w_dil, const float* __restrict__ b_dil,
                      const float* __restrict__ w_dense, const float* __restrict__ b_dense, float* __restrict__ s_out,
                      float* __restrict__ z_out, int B, int Lin, int dil) {
  static_assert(MODE == 0 || MODE == 2, "s_out only, or z only");
  const int lane = threadIdx.x & 63;
  const int li = lane & 31, lh = lane >> 5;
  const int Lo = Lin - dil;
  const int tiles_per_seq = tiles_per_sequence<32>(Lo);
  const long ntiles = (long)B * tiles_per_seq;
  const long wave0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long nwaves = ((long)gridDim.x * blockDim.x) >> 6;

  // A operands, resident for the whole kernel, picked from the LDS weight image
  __shared__ float wl[WIMG_SIZE];
  stage_block_weights(wl, w_dil, b_dil, w_dense, b_dense, threadIdx.x, 256);
  __syncthreads();
  float wd[32];   // W_dil[d = li][c = s][tap = lh]
#pragma unroll
  for (int s = 0; s < 32; ++s) wd[s] = wl[WIMG_DIL + li * WIMG_DIL_PITCH + s * 2 + lh];
  float we[16];   // W_dense[r = li][d = row(r', lh)]
#pragma unroll
  for (int r = 0; r < 16; ++r) we[r] = wl[WIMG_DENSE + li * WIMG_DENSE_PITCH + mfma32_row(r, lh)];
  const float* bzl = wl + WIMG_BDIL;
  const float* bsl = wl + WIMG_BDENSE;

  // Software pipeline across tiles: the NEXT tile's 48 loads are issued before the current tile's 48 MFMAs, so
  // HBM latency hides under the matrix work inside one wave (the kernel is balanced HBM <-> MFMA).
  // Loads are UNCONDITIONAL on a clamped (always valid) address and masked afterwards: a per-element
  // "ok ? load : 0" makes hipcc branch around every load and wait for each one (32 serial round trips).
  float xn[32], rn[16];
  auto issue = [&](long tile) {
    const TilePos p = tile_pos(tile < ntiles ? tile : ntiles - 1, tiles_per_seq, li, Lo);
    const int b = p.b, tcl = p.ok ? p.t : 0;
    const float* xp = s_in + (long)b * 32 * Lin + tcl + lh * dil;
#pragma unroll
    for (int c = 0; c < 32; ++c) xn[c] = xp[(long)c * Lin];
    if (MODE == 0) {
      const float* rp = s_in + (long)b * 32 * Lin + tcl + dil;
#pragma unroll
      for (int r = 0; r < 16; ++r) rn[r] = rp[(long)mfma32_row(r, lh) * Lin];
    }
  };
  if (wave0 < ntiles) issue(wave0);
  for (long tile = wave0; tile < ntiles; tile += nwaves) {
    const TilePos p = tile_pos(tile, tiles_per_seq, li, Lo);
    const int b = p.b, t = p.t;
    const bool ok = p.ok;
    float x[32], rv[16];
#pragma unroll
    for (int c = 0; c < 32; ++c) x[c] = ok ? xn[c] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) rv[r] = (MODE == 0 && ok) ? rn[r] : 0.f;
    issue(tile + nwaves);     // in flight during the MFMAs below (clamped to the last tile when there is none)
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = bzl[mfma32_row(r, lh)];
#pragma unroll
    for (int s = 0; s < 32; ++s) acc = mfma32(wd[s], relu1(x[s]), acc);
    if (MODE == 2) {
      float* zp = z_out + (long)b * 32 * Lo + t;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (ok) zp[(long)mfma32_row(r, lh) * Lo] = acc[r];
    }
    if (MODE == 0) {
      f32x16 acc2;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc2[r] = bsl[mfma32_row(r, lh)] + rv[r];
#pragma unroll
      for (int r = 0; r < 16; ++r) acc2 = mfma32(we[r], relu1(acc[r]), acc2);
      float* op = s_out + (long)b * 32 * Lo + t;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (ok) op[(long)mfma32_row(r, lh) * Lo] = acc2[r];
    }
  }
}

// BUFFER-ADDRESSED forms of the same block (option "wn_flat" selects the kernel above).  On this chip the fp32
// MFMA runs on the vector lanes: every VALU instruction costs ~4 matrix-pipe cycles whatever the occupancy (tools/lab/
// mfvar_lab.py: a wave's MFMA chain at 0.90 of the pipe with ~50 VALU per tile, 0.71 with ~220, the same at 1, 2 and 3
// waves/SIMD).  The flat kernel above carries 718 VALU instructions per 48 MFMAs -- 139 64-bit address adds, 96 v_max (two
// per ReLU), 85 validity selects -- i.e. as many vector cycles as matrix cycles.  Here a tile's addressing is wave-uniform:
//   * one buffer descriptor per tensor and tile (SALU), ONE per-lane byte offset, the row in the instruction's scalar offset;
//   * lanes past the end of a sequence carry an out-of-range offset: their loads return 0 and their stores are dropped by
//     the bounds check, so no select touches the data;
//   * ReLU is one integer max (relu1).
// ONE body, two schedules of it (wn_block_fwd_buf and wn_block_fwd_occ below):
//   RESIDENT   the 48 weight fragments live in registers and the cross-tile prefetch alternates between two register sets
//              (instead of copying): a tile's memory latency hides under this wave's own MFMAs;
//   otherwise  nothing is held across tiles -- weights read from LDS per MFMA, no prefetch registers -- so the kernel fits
//              4 waves per SIMD (< 128 VGPRs) and the latency hides under the OTHER waves' MFMAs.
// The tiles are walked XCD-aware (xcd_walk, common.h): the second tap and the residual of a tile (the same plane, `dil`
// samples later) are then lines that a neighbouring wave of the SAME XCD fetched a moment ago.
struct FwdTile { float x[32], r[16]; };      // a tile's 32 operand rows (tap lh) and 16 residual rows, as requested
template <bool RESIDENT>
__device__ __forceinline__ void wn_block_fwd_body(float* wl, const float* __restrict__ s_in, const float* __restrict__ w_dil,
                                                  const float* __restrict__ b_dil, const float* __restrict__ w_dense,
                                                  const float* __restrict__ b_dense, float* __restrict__ s_out, int B, int Lin,
                                                  int dil) {
  const int lane = threadIdx.x & 63;
  const int li = lane & 31, lh = lane >> 5;
  const int Lo = Lin - dil;
  const int tiles_per_seq = tiles_per_sequence<32>(Lo);
  const int ntiles = B * tiles_per_seq;
  const float* wdl = wl + WIMG_DIL + li * WIMG_DIL_PITCH + lh;             // W_dil[d = li][c = s][tap = lh] at wdl[2 s]
  const float* wel = wl + WIMG_DENSE + li * WIMG_DENSE_PITCH + 4 * lh;     // W_dense[r = li][d = row(r', lh)] at wel[row(r', 0)]
  const float* bzl = wl + WIMG_BDIL + 4 * lh;
  const float* bsl = wl + WIMG_BDENSE + 4 * lh;
  const int rowL = Lin * 4, rowO = Lo * 4;     // bytes per row of the input / output tensors
  float wd[32], we[16];                        // RESIDENT: the fragments themselves

  // request tile `tile`'s 48 values (the prefetch clamps to the last tile when there is none: the values are then never used)
  auto issue = [&](int tile, FwdTile& n) __attribute__((always_inline)) {
    const TilePos p = tile_pos(RESIDENT && tile >= ntiles ? ntiles - 1 : tile, tiles_per_seq, li, Lo);
    const __amdgpu_buffer_rsrc_t rx = brsrc(s_in + (long)p.b * 32 * Lin, 32 * rowL);
    const int offx = p.ok ? (p.t + lh * dil) * 4 : BUF_OOB;
#pragma unroll
    for (int c = 0; c < 32; ++c) n.x[c] = bload(rx, offx, c * rowL);
    const int offr = p.ok ? (p.t + dil) * 4 + 4 * lh * rowL : BUF_OOB;
#pragma unroll
    for (int r = 0; r < 16; ++r) n.r[r] = bload(rx, offr, mfma32_row(r, 0) * rowL);
  };
  auto compute = [&](int tile, const FwdTile& c) __attribute__((always_inline)) {
    const TilePos p = tile_pos(tile, tiles_per_seq, li, Lo);
    const int offo = p.ok ? p.t * 4 + 4 * lh * rowO : BUF_OOB;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = bzl[mfma32_row(r, 0)];
#pragma unroll
    for (int s = 0; s < 32; ++s) acc = mfma32(RESIDENT ? wd[s] : wdl[2 * s], relu1(c.x[s]), acc);
    f32x16 acc2;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[r] = bsl[mfma32_row(r, 0)] + c.r[r];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2 = mfma32(RESIDENT ? we[r] : wel[mfma32_row(r, 0)], relu1(acc[r]), acc2);
    const __amdgpu_buffer_rsrc_t ro = brsrc(s_out + (long)p.b * 32 * Lo, 32 * rowO);
#pragma unroll
    for (int r = 0; r < 16; ++r) bstore(acc2[r], ro, offo, mfma32_row(r, 0) * rowO);
  };
  const TileWalkI w = xcd_walk_i(ntiles);
  FwdTile ta, tb;
  // RESIDENT: the first tile's requests are on their way while the block's weights make their own round trip (global -> LDS
  // -> registers): at the bench shape a launch lasts ~37 us and each of the two latencies is ~2 us of it
  if (RESIDENT && w.first < w.last) issue(w.first, ta);
  stage_block_weights(wl, w_dil, b_dil, w_dense, b_dense, threadIdx.x, 256);
  __syncthreads();
  if (RESIDENT) {
#pragma unroll
    for (int s = 0; s < 32; ++s) wd[s] = wdl[2 * s];
#pragma unroll
    for (int r = 0; r < 16; ++r) we[r] = wel[mfma32_row(r, 0)];
    pingpong_tiles<false>(w, ta, tb, issue, compute);
  } else {
    plain_tiles<false, FwdTile>(w, issue, compute);
  }
}

// resident weights + cross-tile prefetch: the form picked beside another stream's kernels (wn_flat = 2)
__global__ void __launch_bounds__(256)
    wn_block_fwd_buf(const float* __restrict__ s_in, const float* __restrict__ w_dil, const float* __restrict__ b_dil,
                     const float* __restrict__ w_dense, const float* __restrict__ b_dense, float* __restrict__ s_out, int B,
                     int Lin, int dil) {
  __shared__ float wl[WIMG_SIZE];
  wn_block_fwd_body<true>(wl, s_in, w_dil, b_dil, w_dense, b_dense, s_out, B, Lin, dil);
}

// HIGH-OCCUPANCY form (the default for planes shorter than 8192 samples).  Measured (tools/lab/clk_lab2.py, same body):
// bench-shape layer 28.4 us at 4 waves/SIMD, 28.5 at 3, 31.0 at 2; C2-shape layer 273 / 303 / 380 us.  Earlier attempts at
// this shape (round 2, first half) ran the flat addressing: with ~700 VALU instructions per tile the extra waves only queued
// for the vector ALUs.
__global__ void __launch_bounds__(256, 4)
    wn_block_fwd_occ(const float* __restrict__ s_in, const float* __restrict__ w_dil, const float* __restrict__ b_dil,
                     const float* __restrict__ w_dense, const float* __restrict__ b_dense, float* __restrict__ s_out, int B,
                     int Lin, int dil) {
  __shared__ float wl[WIMG_SIZE];
  wn_block_fwd_body<false>(wl, s_in, w_dil, b_dil, w_dense, b_dense, s_out, B, Lin, dil);
}

// LDS-DMA form.  What bounds the dword kernels above is the CU's ADDRESS unit, shared by the four SIMDs: a wave memory
// instruction costs it ~16 cycles whatever its width, a 32-sample tile issues 64 of them (32 operand loads, 16 residual loads,
// 16 stores) = ~1000 cycles per tile and CU against 768 cycles of matrix work (48 MFMAs x 64 cycles / 4 SIMDs) -- the memory
// phase alone takes 20 us per bench-shape layer (12 200 tiles / 256 CUs x 1024 cycles), and at launch every resident wave
// queues its 48 loads at once, so the first MFMA of a CU waits for ~12 000 cycles of address work.  Here a tile's operands
// arrive by EIGHT buffer_load_dwordx4 ... lds instructions (1 KiB each: 8 channel rows x 128 B, straight into the wave's own
// 8 KB LDS tile, no VGPR destination): tap 0 and tap 1 as two [32 channels][32 samples] images.  The MFMA B operand of
// k-step s is then one conflict-free ds_read_b32 (lane half h = tap h, row s), the residual rows are 16 more reads of the
// tap-1 image, and the address unit sees 8 + 16 instructions per tile (384 cycles) -- the kernel is bound by the matrix
// pipe.  Same MFMA sequence and accumulator initialisation as wn_block_fwd_occ: the results agree bit for bit.
// One workgroup = 8 waves (weights once per workgroup in LDS, 64 KB of wave tiles): two per CU = 4 waves per SIMD.
__global__ void __launch_bounds__(512, 4)
    wn_block_fwd_dma(const float* __restrict__ s_in, const float* __restrict__ w_dil, const float* __restrict__ b_dil,
                     const float* __restrict__ w_dense, const float* __restrict__ b_dense, float* __restrict__ s_out, int B, int Lin,
                     int dil) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int Lo = Lin - dil;
  const int tiles_per_seq = tiles_per_sequence<32>(Lo);
  const int ntiles = B * tiles_per_seq;
  __shared__ __attribute__((aligned(16))) float wl[8 * 2048 + WIMG_SIZE];     // wave tiles first (16-byte aligned DMA targets)
  float* const wts = wl + 8 * 2048;
  stage_block_weights(wts, w_dil, b_dil, w_dense, b_dense, threadIdx.x, 512);
  __syncthreads();
  const float* wdl = wts + WIMG_DIL + li * WIMG_DIL_PITCH + lh;             // W_dil[d = li][c = s][tap = lh] at wdl[2 s]
  const float* wel = wts + WIMG_DENSE + li * WIMG_DENSE_PITCH + 4 * lh;     // W_dense[r = li][d = row(r', lh)] at wel[row(r', 0)]
  const float* bzl = wts + WIMG_BDIL + 4 * lh;
  const float* bsl = wts + WIMG_BDENSE + 4 * lh;
  const int rowL = Lin * 4, rowO = Lo * 4;
  float* const tb = wl + __builtin_amdgcn_readfirstlane(wave) * 2048;        // this wave's tile: [tap][32 channels][32 samples]
  const float* const xs = tb + lh * 1024 + li;                               // B operand of k-step s: xs[32 s]
  const float* const rs = tb + 1024 + 4 * lh * 32 + li;                       // residual row (r, lh): rs[32 row(r, 0)]
  // the DMA's per-lane source: channel row (lane >> 3) of the instruction's 8, samples 4 (lane & 7) .. + 3
  const int dvo = (lane >> 3) * rowL + (lane & 7) * 16;
  const TileWalkI w = xcd_walk_i(ntiles, 8);             // 8 waves per workgroup here
  for (int tile = w.first; tile < w.last; tile += w.stride) {
    const TilePos p = tile_pos(tile, tiles_per_seq, li, Lo);
    const int b = p.b, t0 = p.t0;
    const __amdgpu_buffer_rsrc_t rx = brsrc(s_in + (long)b * 32 * Lin, 32 * rowL);
    // samples past the end of a row read into the next row, past the slab nothing is written: garbage COLUMNS, whose
    // results are never stored (an output column depends on its own input columns only)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(tb + q * 256), 16, dvo + t0 * 4,
                                               8 * q * rowL, 0, 0);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(tb + 1024 + q * 256), 16,
                                               dvo + (t0 + dil) * 4, 8 * q * rowL, 0, 0);
    const int offo = p.ok ? p.t * 4 + 4 * lh * rowO : BUF_OOB;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = bzl[mfma32_row(r, 0)];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the tile has landed (and the previous tile's stores have drained)
    __builtin_amdgcn_sched_barrier(0);
    // Operands of 8 k-steps at a time, the NEXT group's LDS reads in flight under this group's MFMAs (pinned: left alone,
    // hipcc issues two reads, waits for them and multiplies twice -- the LDS latency in front of every MFMA pair)
    float wv[2][8], xv[2][8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { wv[0][k] = wdl[2 * k]; xv[0][k] = xs[32 * k]; }
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      if (gq < 3) {
#pragma unroll
        for (int k = 0; k < 8; ++k) { wv[(gq + 1) & 1][k] = wdl[2 * (8 * (gq + 1) + k)]; xv[(gq + 1) & 1][k] = xs[32 * (8 * (gq + 1) + k)]; }
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc = mfma32(wv[gq & 1][k], relu1(xv[gq & 1][k]), acc);
    }
    // the 1x1 product: its 16 weights and the 16 residual rows are read while the last dilated MFMAs run
    float we16[16];
    f32x16 acc2;
#pragma unroll
    for (int r = 0; r < 16; ++r) { we16[r] = wel[mfma32_row(r, 0)]; acc2[r] = bsl[mfma32_row(r, 0)] + rs[32 * mfma32_row(r, 0)]; }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2 = mfma32(we16[r], relu1(acc[r]), acc2);
    const __amdgpu_buffer_rsrc_t ro = brsrc(s_out + (long)b * 32 * Lo, 32 * rowO);
#pragma unroll
    for (int r = 0; r < 16; ++r) bstore(acc2[r], ro, offo, mfma32_row(r, 0) * rowO);
    // (the next tile's DMA overwrites this wave's LDS tile: every read of it above has been consumed by an MFMA or an add
    //  that precedes the DMA in program order)
    __builtin_amdgcn_sched_barrier(0);
  }
}

// WIDE form (the default for planes of >= 128 samples): the same block with 16-byte memory instructions.  The dword
// kernels above are ISSUE-bound in the memory pipe -- 64 one-dword wave-instructions per 32-sample tile keep the CU's
// address unit busier (~1000 cycles) than the tile's 48 MFMAs keep the matrix pipe (768), and a wave that is stuck issuing
// its loads issues no MFMAs behind them either -- so here one wave owns a 128-sample SUPER-tile as four interleaved
// sub-tiles (sub-tile j = samples t0 + 4n + j: columns are independent, so any set of 32 columns is a valid MFMA tile):
// lane n holds 4 consecutive samples, every load / store is a dwordx4 (rows start at any sample: 4-byte aligned 16-byte
// accesses), and the instruction count per sample drops 4x.  The weights come from LDS per MFMA group (one ds_read feeds
// four MFMAs), the residual is fetched (an L1/L2 hit: the tap-1 lanes just read those lines) into the x registers once the
// dilated product is done.
__global__ void __launch_bounds__(256, 2)
    wn_block_fwd_w4(const float* __restrict__ s_in, const float* __restrict__ w_dil, const float* __restrict__ b_dil,
                    const float* __restrict__ w_dense, const float* __restrict__ b_dense, float* __restrict__ s_out, int B,
                    int Lin, int dil) {
  const int lane = threadIdx.x & 63;
  const int li = lane & 31, lh = lane >> 5;
  const int Lo = Lin - dil;
  const int tiles_per_seq = tiles_per_sequence<128>(Lo);
  const int ntiles = B * tiles_per_seq;
  __shared__ float wl[WIMG_SIZE];
  stage_block_weights(wl, w_dil, b_dil, w_dense, b_dense, threadIdx.x, 256);
  __syncthreads();
  const float* wdl = wl + WIMG_DIL + li * WIMG_DIL_PITCH + lh;             // W_dil[d = li][c = s][tap = lh] at wdl[2 s]
  const float* wel = wl + WIMG_DENSE + li * WIMG_DENSE_PITCH + 4 * lh;     // W_dense[r = li][d = row(r', lh)] at wel[row(r', 0)]
  const float* bzl = wl + WIMG_BDIL + 4 * lh;
  const float* bsl = wl + WIMG_BDENSE + 4 * lh;
  const int rowL = Lin * 4, rowO = Lo * 4;

  const TileWalkI w = xcd_walk_i(ntiles);
  for (int tile = w.first; tile < w.last; tile += w.stride) {
    const TilePos p = tile_pos<128>(tile, tiles_per_seq, 4 * li, Lo);
    const int b = p.b, t0 = p.t0, t = p.t;         // t: this lane's first sample
    const __amdgpu_buffer_rsrc_t rx = brsrc(s_in + (long)b * 32 * Lin, 32 * rowL);
    const __amdgpu_buffer_rsrc_t ro = brsrc(s_out + (long)b * 32 * Lo, 32 * rowO);
    // samples past the end of a row read into the next row (or return 0 past the slab): garbage columns, never stored
    const int offx = (t + lh * dil) * 4;
    f4v x[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) x[c] = bload4(rx, offx, c * rowL);
    // all 32 requests go out BEFORE the first MFMA (left alone, hipcc hoists the weights into 48 registers, has too few left
    // for x and re-fetches it two loads at a time between the MFMAs: a memory round trip per four MFMAs).  The weight
    // pointers are laundered per tile so that their LDS reads stay inside the loop.
    __builtin_amdgcn_sched_barrier(0);
    const float* wd_t = wdl;
    const float* we_t = wel;
    asm volatile("" : "+v"(wd_t), "+v"(we_t));
    f32x16 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = bzl[mfma32_row(r, 0)];
#pragma unroll
    for (int s = 0; s < 32; ++s) {
      const float w = wd_t[2 * s];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = mfma32(w, relu1(x[s][j]), acc[j]);
    }
    // residual rows (same plane, `dil` samples later: the lines the tap-1 half just read), into registers x no longer needs
    const int offr = (t + dil) * 4 + 4 * lh * rowL;
    f4v rv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) rv[r] = bload4(rx, offr, mfma32_row(r, 0) * rowL);
    __builtin_amdgcn_sched_barrier(0);
    f32x16 acc2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc2[j][r] = bsl[mfma32_row(r, 0)];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float w = we_t[mfma32_row(r, 0)];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc2[j] = mfma32(w, relu1(acc[j][r]), acc2[j]);
    }
    const int offo = t * 4 + 4 * lh * rowO;
    if (t0 + 128 <= Lo) {
      // All 16 sums first (in place of rv), THEN the 16 stores, nothing writing their data registers behind them.
      // gfx950 hazard the compiler does not know: a buffer_store_dwordx4 whose soffset is an SGPR still reads its data
      // registers a moment after issue, exactly like the immediate-soffset form hipcc pads with a wait state.  With the sum
      // of row r+1 computed into the registers of row r's store right behind it, 16 lanes of the store's first dword were
      // the NEXT row's value -- only with two waves per SIMD (the other wave's traffic delays the read), only rows whose
      // store had an SGPR soffset and a successor: r = 1..14 (tests: test_wavenet_block_kernel_forms_agree).
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const f4v o = {acc2[0][r] + rv[r][0], acc2[1][r] + rv[r][1], acc2[2][r] + rv[r][2], acc2[3][r] + rv[r][3]};
        rv[r] = o;
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int r = 0; r < 16; ++r) bstore4(rv[r], ro, offo, mfma32_row(r, 0) * rowO);
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_nop 1");
    } else {          // last super-tile of a sequence: element-wise, out-of-range samples dropped by the bounds check
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int oj = t + j < Lo ? offo + 4 * j : BUF_OOB;
#pragma unroll
        for (int r = 0; r < 16; ++r) bstore(acc2[j][r] + rv[r][j], ro, oj, mfma32_row(r, 0) * rowO);
      }
    }
  }
}

// (Round 2 also tried two other shapes of the FLAT kernel -- tools/lab/mem_lab.py holds the measurements: a 3-waves-per-SIMD form
//  with the weight fragments read from LDS and no cross-tile prefetch, and one with wave-uniform scalar/buffer addressing
//  (the flat form spends ~1900 VALU cycles per tile on 64-bit per-lane address arithmetic, and on this chip VALU time adds
//  to fp32-MFMA time: the matrix instruction runs on the vector lanes).  Both timed within 3 % of this kernel at the bench
//  and C2 shapes: its ~36 us per bench-shape layer are the SUM of the access pattern's streaming time (20 us alone) and the
//  matrix time (15 us alone), and neither occupancy nor fewer VALU instructions made the two overlap.  Nor did pinning the
//  next tile's 48 loads in front of this tile's MFMAs with sched_barrier -- hipcc sinks them below the first 32 MFMAs
//  otherwise -- which timed 3 % slower.)

// ------------------------------------------------------------------ fused MFMA backward of a residual block (R = D = 32, fw = 2)
// (A)  dz[d][t] = (z[d][t] > 0) * sum_r W_dense[r][d] * dS[r][t]            -- 16 MFMAs per 32-sample tile
// Same lane geometry as the forward: column = time on the lane; the K index r = 2s+h is fed by lane half h.
__global__ void __launch_bounds__(256)
    wn_block_bwd_dz_mfma(const float* __restrict__ dS, const float* __restrict__ Z, const float* __restrict__ w_dense,
                         float* __restrict__ DZ, int B, int Lo) {
  const int lane = threadIdx.x & 63;
  const int li = lane & 31, lh = lane >> 5;
  const int tiles_per_seq = tiles_per_sequence<32>(Lo);
  const long ntiles = (long)B * tiles_per_seq;
  const long wave0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long nwaves = ((long)gridDim.x * blockDim.x) >> 6;
  __shared__ float wl[WIMG_DENSE_SIZE];
  stage_w_dense(wl, w_dense, threadIdx.x, 256);
  __syncthreads();
  float wt[16];  // A[i = d = li][k = r = 2s+lh] = W_dense[r][d]
#pragma unroll
  for (int s = 0; s < 16; ++s) wt[s] = wl[(2 * s + lh) * WIMG_DENSE_PITCH + li];
  for (long tile = wave0; tile < ntiles; tile += nwaves) {
    const TilePos p = tile_pos(tile, tiles_per_seq, li, Lo);
    const int b = p.b, t = p.t;
    const bool ok = p.ok;
    const long base = (long)b * 32 * Lo + (ok ? t : 0);   // clamped: loads are unconditional, masked below
    float g[16], z[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) g[s] = dS[base + (long)(2 * s + lh) * Lo];
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = Z[base + (long)mfma32_row(r, lh) * Lo];
#pragma unroll
    for (int s = 0; s < 16; ++s) g[s] = ok ? g[s] : 0.f;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int s = 0; s < 16; ++s) acc = mfma32(wt[s], g[s], acc);
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (ok) DZ[base + (long)mfma32_row(r, lh) * Lo] = z[r] > 0.f ? acc[r] : 0.f;
  }
}

// (B)  dS_in[c][t'] = (s_in[c][t'] > 0) * sum_{d,k} W_dil[d][c][k] * dz[d][t' - k*dil]  +  dS_out[c][t' - dil]
//      (terms whose index falls outside [0, Lo) are zero)                        -- 32 MFMAs per tile
__global__ void __launch_bounds__(256)
    wn_block_bwd_dx_mfma(const float* __restrict__ DZ, const float* __restrict__ s_in, const float* __restrict__ dS_out,
                         const float* __restrict__ w_dil, float* __restrict__ dS_in, int B, int Lin, int dil) {
  const int lane = threadIdx.x & 63;
  const int li = lane & 31, lh = lane >> 5;
  const int Lo = Lin - dil;
  const int tiles_per_seq = tiles_per_sequence<32>(Lin);
  const long ntiles = (long)B * tiles_per_seq;
  __shared__ float wl[WIMG_DIL_SIZE];
  stage_w_dil(wl, w_dil, threadIdx.x, 256);
  __syncthreads();
  float wt[32];  // A[i = c = li][k = (d = s, tap = lh)] = W_dil[d][c][tap]
#pragma unroll
  for (int s = 0; s < 32; ++s) wt[s] = wl[s * WIMG_DIL_PITCH + li * 2 + lh];
  // software pipeline across tiles (see wn_block_fwd_mfma): next tile's loads fly under this tile's MFMAs
  float dzn[32], svn[16], rvn[16];
  auto issue = [&](long tile) {
    const TilePos p = tile_pos(tile < ntiles ? tile : ntiles - 1, tiles_per_seq, li, Lin);
    const int b = p.b, t = p.t;
    const bool ok = p.ok;
    const int to = t - lh * dil;
    const bool okz = ok && to >= 0 && to < Lo;
    const float* zp = DZ + (long)b * 32 * Lo + (okz ? to : 0);
#pragma unroll
    for (int s = 0; s < 32; ++s) dzn[s] = zp[(long)s * Lo];
    const bool okr = ok && t >= dil;
    const float* sp = s_in + (long)b * 32 * Lin + (ok ? t : 0);
    const float* rp = dS_out + (long)b * 32 * Lo + (okr ? t - dil : 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) { svn[r] = sp[(long)mfma32_row(r, lh) * Lin]; rvn[r] = rp[(long)mfma32_row(r, lh) * Lo]; }
  };
  const TileWalk tw = xcd_walk(ntiles);
  if (tw.first < tw.last) issue(tw.first);
  for (long tile = tw.first; tile < tw.last; tile += tw.stride) {
    const TilePos p = tile_pos(tile, tiles_per_seq, li, Lin);
    const int b = p.b, t = p.t;                                       // t' (input time)
    const bool ok = p.ok;
    const int to = t - lh * dil;                                      // dz time of this lane half's tap
    const bool okz = ok && to >= 0 && to < Lo;
    const bool okr = ok && t >= dil;                                  // residual: dS_out[c][t' - dil]
    float dz[32], sv[16], rv[16];
#pragma unroll
    for (int s = 0; s < 32; ++s) dz[s] = okz ? dzn[s] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { sv[r] = svn[r]; rv[r] = okr ? rvn[r] : 0.f; }
    issue(tile + tw.stride);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int s = 0; s < 32; ++s) acc = mfma32(wt[s], dz[s], acc);
    float* op = dS_in + (long)b * 32 * Lin + t;
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (ok) op[(long)mfma32_row(r, lh) * Lin] = (sv[r] > 0.f ? acc[r] : 0.f) + rv[r];
  }
}

// BUFFER-ADDRESSED forms of (B): ONE body, the two schedules of the forward pair (see wn_block_fwd_body).  Same arithmetic,
// same summation order as the flat kernel above -- which carries 720 VALU instructions per 32 MFMAs, most of them 64-bit
// address arithmetic and validity selects.
struct DxTile { float dz[32], sv[16], rv[16]; };   // dz rows (tap lh), s_in rows (the ReLU mask), dS_out rows (the residual)
template <bool RESIDENT>
__device__ __forceinline__ void wn_block_bwd_dx_body(float* wl, const float* __restrict__ DZ, const float* __restrict__ s_in,
                                                     const float* __restrict__ dS_out, const float* __restrict__ w_dil,
                                                     float* __restrict__ dS_in, int B, int Lin, int dil) {
  const int lane = threadIdx.x & 63;
  const int li = lane & 31, lh = lane >> 5;
  const int Lo = Lin - dil;
  const int tiles_per_seq = tiles_per_sequence<32>(Lin);
  const int ntiles = B * tiles_per_seq;
  const float* wtl = wl + li * 2 + lh;   // A[i = c = li][k = (d = s, tap = lh)] = W_dil[d][c][tap] at wtl[65 s]
  const int rowL = Lin * 4, rowO = Lo * 4;
  float wt[32];                          // RESIDENT: the fragment itself
  // request tile `tile` (the prefetch clamps to the last tile when there is none: the values are then never used)
  auto issue = [&](int tile, DxTile& n) __attribute__((always_inline)) {
    const TilePos p = tile_pos(RESIDENT && tile >= ntiles ? ntiles - 1 : tile, tiles_per_seq, li, Lin);
    const int t = p.t;                                    // t' (input time)
    const int to = t - lh * dil;                          // dz time of this lane half's tap
    const bool okz = p.ok && to >= 0 && to < Lo;
    const bool okr = p.ok && t >= dil;                    // residual: dS_out[c][t' - dil]
    const __amdgpu_buffer_rsrc_t rz = brsrc(DZ + (long)p.b * 32 * Lo, 32 * rowO);
    const __amdgpu_buffer_rsrc_t rs = brsrc(s_in + (long)p.b * 32 * Lin, 32 * rowL);
    const __amdgpu_buffer_rsrc_t rg = brsrc(dS_out + (long)p.b * 32 * Lo, 32 * rowO);
    const int offz = okz ? to * 4 : BUF_OOB;
    const int offs = p.ok ? t * 4 + 4 * lh * rowL : BUF_OOB;
    const int offg = okr ? (t - dil) * 4 + 4 * lh * rowO : BUF_OOB;
#pragma unroll
    for (int s = 0; s < 32; ++s) n.dz[s] = bload(rz, offz, s * rowO);
#pragma unroll
    for (int r = 0; r < 16; ++r) { n.sv[r] = bload(rs, offs, mfma32_row(r, 0) * rowL); n.rv[r] = bload(rg, offg, mfma32_row(r, 0) * rowO); }
  };
  auto compute = [&](int tile, const DxTile& c) __attribute__((always_inline)) {
    const TilePos p = tile_pos(tile, tiles_per_seq, li, Lin);
    const __amdgpu_buffer_rsrc_t ro = brsrc(dS_in + (long)p.b * 32 * Lin, 32 * rowL);
    const int offs = p.ok ? p.t * 4 + 4 * lh * rowL : BUF_OOB;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int s = 0; s < 32; ++s) acc = mfma32(RESIDENT ? wt[s] : wtl[WIMG_DIL_PITCH * s], c.dz[s], acc);
#pragma unroll
    for (int r = 0; r < 16; ++r) bstore((c.sv[r] > 0.f ? acc[r] : 0.f) + c.rv[r], ro, offs, mfma32_row(r, 0) * rowL);
  };
  const TileWalkI w = xcd_walk_i(ntiles);
  DxTile ta, tb;                                             // (RESIDENT only)
  if (RESIDENT && w.first < w.last) issue(w.first, ta);      // in flight while the weights are staged
  stage_w_dil(wl, w_dil, threadIdx.x, 256);
  __syncthreads();
  if (RESIDENT) {
#pragma unroll
    for (int s = 0; s < 32; ++s) wt[s] = wtl[WIMG_DIL_PITCH * s];
    pingpong_tiles<false>(w, ta, tb, issue, compute);
  } else {
    plain_tiles<false, DxTile>(w, issue, compute);
  }
}

// resident weights, the next tile's requests in flight under this tile's MFMAs (option wn_dx = 1)
__global__ void __launch_bounds__(256)
    wn_block_bwd_dx_buf(const float* __restrict__ DZ, const float* __restrict__ s_in, const float* __restrict__ dS_out,
                        const float* __restrict__ w_dil, float* __restrict__ dS_in, int B, int Lin, int dil) {
  __shared__ float wl[WIMG_DIL_SIZE];
  wn_block_bwd_dx_body<true>(wl, DZ, s_in, dS_out, w_dil, dS_in, B, Lin, dil);
}

// HIGH-OCCUPANCY form, the default (see wn_block_fwd_occ): nothing held across tiles -> < 128 VGPRs, 4 waves per SIMD
__global__ void __launch_bounds__(256, 4)
    wn_block_bwd_dx_occ(const float* __restrict__ DZ, const float* __restrict__ s_in, const float* __restrict__ dS_out,
                        const float* __restrict__ w_dil, float* __restrict__ dS_in, int B, int Lin, int dil) {
  __shared__ float wl[WIMG_DIL_SIZE];
  wn_block_bwd_dx_body<false>(wl, DZ, s_in, dS_out, w_dil, dS_in, B, Lin, dil);
}

constexpr int WG_SLAB = 3 * 1024 + 64;   // per-workgroup partial sums of wn_block_wgrad_mfma
constexpr int WG_MAXBLK = 512;

// ------------------------------------------------------------------ fused MFMA weight/bias gradients of a residual block (R = D = 32, fw = 2)
//   dW_dil[d][c][k] += sum_t dz[d][t] relu(s_in[c][t + k*dil])      db_dil[d]   += sum_t dz[d][t]
//   dW_dense[r][d]  += sum_t dS[r][t] relu(z[d][t])                 db_dense[r] += sum_t dS[r][t]
// The contraction index is TIME, so the MFMA wants channel-on-lane fragments (A[i = channel][k = t]).  Tiles are
// loaded the coalesced way (lane = time), transposed through a per-wave 32x33 LDS tile (conflict-free both ways)
// and fed to three 32x32 accumulators that live in registers across the wave's whole time range; one LDS +
// global float-atomic reduction per workgroup at the end.  Replaces two split-K GEMM launches and two bias
// reductions per layer.
__global__ void __launch_bounds__(256)
    wn_block_wgrad_mfma(const float* __restrict__ dS, const float* __restrict__ Z, const float* __restrict__ DZ,
                        const float* __restrict__ s_in, float* __restrict__ slab, int B, int Lin, int dil) {
  __shared__ float tile[4][32 * 33];
  __shared__ float red[WG_SLAB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int Lo = Lin - dil;
  const int tiles_per_seq = tiles_per_sequence<32>(Lo);
  const long ntiles = (long)B * tiles_per_seq;
  const long wave0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long nwaves = ((long)gridDim.x * blockDim.x) >> 6;
  float* T = tile[wave];
  for (int i = threadIdx.x; i < WG_SLAB; i += 256) red[i] = 0.f;

  f32x16 acc0, acc1, acc2;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; acc2[r] = 0.f; }
  float bs_dz = 0.f, bs_ds = 0.f;

  // fragment of X: f[s] = X[channel = li][t0 + 2s + lh]; X is read as X[c][t0 + li] (c = 2s' + lh), coalesced,
  // unconditionally from a clamped address (masked afterwards: no per-load branches / waits)
  auto gl = [&](const float* base, long rstride, float (&v)[16]) {
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = base[(long)(2 * q + lh) * rstride];
  };
  auto xpose = [&](const float (&v)[16], bool ok, bool relu, float (&f)[16]) {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float x = ok ? v[q] : 0.f;
      T[(2 * q + lh) * 33 + li] = relu ? relu1(x) : x;
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int q = 0; q < 16; ++q) f[q] = T[li * 33 + 2 * q + lh];
    __builtin_amdgcn_wave_barrier();
  };

  for (long tl = wave0; tl < ntiles; tl += nwaves) {
    const TilePos p = tile_pos(tl, tiles_per_seq, li, Lo);
    const int b = p.b, t = p.t;
    const bool ok = p.ok;
    const long oo = (long)b * 32 * Lo + (ok ? t : 0);
    const long oi = (long)b * 32 * Lin + (ok ? t : 0);
    float v0[16], v1[16], v2[16], v3[16], v4[16];   // all five operand tiles in flight at once
    gl(DZ + oo, Lo, v0);
    gl(s_in + oi, Lin, v1);
    gl(s_in + oi + dil, Lin, v2);
    gl(dS + oo, Lo, v3);
    gl(Z + oo, Lo, v4);
    float fa[16], fb[16];
    xpose(v0, ok, false, fa);
#pragma unroll
    for (int q = 0; q < 16; ++q) bs_dz += fa[q];
    xpose(v1, ok, true, fb);
#pragma unroll
    for (int q = 0; q < 16; ++q) acc0 = mfma32(fa[q], fb[q], acc0);
    xpose(v2, ok, true, fb);
#pragma unroll
    for (int q = 0; q < 16; ++q) acc1 = mfma32(fa[q], fb[q], acc1);
    xpose(v3, ok, false, fa);
#pragma unroll
    for (int q = 0; q < 16; ++q) bs_ds += fa[q];
    xpose(v4, ok, true, fb);
#pragma unroll
    for (int q = 0; q < 16; ++q) acc2 = mfma32(fa[q], fb[q], acc2);
  }

  __syncthreads();  // red[] zeroed
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = mfma32_row(r, lh);
    atomicAdd(&red[row * 32 + li], acc0[r]);
    atomicAdd(&red[1024 + row * 32 + li], acc1[r]);
    atomicAdd(&red[2048 + row * 32 + li], acc2[r]);
  }
  atomicAdd(&red[3072 + li], bs_dz);
  atomicAdd(&red[3104 + li], bs_ds);
  __syncthreads();
  // one slab of 3136 partial sums per workgroup (plain stores); wn_wgrad_reduce adds the slabs in a fixed order.
  // (640 workgroups doing float atomics onto the SAME 3136 addresses ran at the contended-atomic rate: 90 us.)
  float* out = slab + (long)blockIdx.x * WG_SLAB;
  for (int i = threadIdx.x; i < WG_SLAB; i += 256) out[i] = red[i];
}

// ------------------------------------------------------------------ (A) + weight gradients in ONE pass, z recomputed
// wn_block_bwd_dz_mfma and wn_block_wgrad_mfma fused, and the forward no longer stores z: per 32-sample tile a wave loads
// dS (16 values) and the two dilation taps of s_in (lane half h = tap h, 32 channels: the forward's own operand), rebuilds
// z = b + W_dil (*) relu(s_in) with the forward's exact MFMA sequence (bit-identical, so the ReLU masks agree), forms
// dz = (z>0) * W_dense^T dS, stores it, and pushes dz / relu(s taps) / dS / relu(z) through per-wave 32x33 LDS
// transposes into the three resident weight-gradient accumulators.  Per layer this replaces 350 MB of HBM traffic
// (z written by the forward, dS + Z read twice, DZ re-read) by 150 MB; the encoder shares HBM with the trunk's
// convolutions running on the other stream, so the bytes matter beyond this kernel's own time.
// ONE body, two schedules (wn_block_bwd_dz_wgrad_mfma and wn_block_bwd_dz_wgrad_occ below):
//   RESIDENT   both weight fragments in registers (W_dense reaches its transposed fragment through the wave's own transpose
//              tile), the next tile's 48 loads in flight under this tile's 96 MFMAs: one wave per SIMD;
//   otherwise  weights read from LDS per MFMA (W_dense from an image of its own, `wtl`), no cross-tile prefetch -> under
//              256 registers, two waves per SIMD (two workgroups per CU).  (Tried for the beside-the-trunk case: this schedule
//              WITH the cross-tile prefetch, 243 registers and no AGPR shuffling, one workgroup per CU -- 0.2-0.5 ms/step
//              slower than the resident-weights form.)
struct DzwTile { float g[16], x[32]; };      // dS rows 2q + lh, s_in rows of tap lh
template <bool RESIDENT>
__device__ __forceinline__ void wn_block_bwd_dz_wgrad_body(float* tiles, float* red, float* wl, float* wtl,
                                                           const float* __restrict__ dS, const float* __restrict__ w_dil,
                                                           const float* __restrict__ b_dil, const float* __restrict__ w_dense,
                                                           const float* __restrict__ s_in, float* __restrict__ DZ,
                                                           float* __restrict__ slab, int B, int Lin, int dil) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int Lo = Lin - dil;
  const int tiles_per_seq = tiles_per_sequence<32>(Lo);
  const int ntiles = B * tiles_per_seq;
  float* T = tiles + wave * 2 * 1056;   // this wave's two 32 x 33 transpose tiles
  float* T1 = T + 1056;
  float* Th = T + lh * 1056;            // this lane half's tile for the two-tap transpose
  stage_w_dil(wl, w_dil, threadIdx.x, 256);
  stage_bias(wl + WIMG_DIL_SIZE, b_dil, threadIdx.x);       // (no dense part in this image: b_dil follows W_dil)
  // W_dense[r][d], padded rows: A[i = d = li][k = r = 2s+lh] = image[(2s+lh)*33 + li].  RESIDENT: through this wave's
  // transpose tile into registers
  if (RESIDENT) stage_w_dense(T, w_dense, lane, 64);
  else stage_w_dense(wtl, w_dense, threadIdx.x, 256);
  for (int i = threadIdx.x; i < WG_SLAB; i += 256) red[i] = 0.f;
  __syncthreads();
  const float* wtp = (RESIDENT ? T : wtl) + lh * WIMG_DENSE_PITCH + li;   // + 66 s
  const float* wdp = wl + li * WIMG_DIL_PITCH + lh;                        // + 2 s: W_dil[d = li][c = s][tap = lh]  (the forward's fragment)
  const float* bzl = wl + WIMG_DIL_SIZE + 4 * lh;
  float wt[16], wd[32];
  if (RESIDENT) {
#pragma unroll
    for (int s = 0; s < 16; ++s) wt[s] = wtp[2 * WIMG_DENSE_PITCH * s];
#pragma unroll
    for (int s = 0; s < 32; ++s) wd[s] = wdp[2 * s];
  }
  __builtin_amdgcn_wave_barrier();

  f32x16 acc0, acc1, acc2;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; acc2[r] = 0.f; }
  float bs_dz = 0.f, bs_ds = 0.f;
  const int rowL = Lin * 4, rowO = Lo * 4;

  // One wave per SIMD is resident (RESIDENT; two otherwise), so VALU instructions add to the 96 MFMAs of a tile one for one
  // (~4 cycles each): the flat-addressed version of this kernel carried 1225 of them per tile -- 64-bit address arithmetic
  // for 64 memory instructions, a validity select on every loaded value, two-instruction ReLUs.  Buffer addressing
  // (common.h): samples past the end of a sequence carry an out-of-range offset, their loads return 0 and their stores are
  // dropped; a zero dS column makes every product of that column zero, so nothing downstream needs masking.
  // RESIDENT, software pipeline across tiles: the NEXT tile's 48 loads are issued before this tile's 96 MFMAs and LDS
  // transposes (nothing else hides their latency), alternating between two register sets instead of copying.
  auto issue = [&](int tile, DzwTile& n) __attribute__((always_inline)) {
    const TilePos p = tile_pos(tile < ntiles ? tile : ntiles - 1, tiles_per_seq, li, Lo);
    const __amdgpu_buffer_rsrc_t rg = brsrc(dS + (long)p.b * 32 * Lo, 32 * rowO);
    const __amdgpu_buffer_rsrc_t rx = brsrc(s_in + (long)p.b * 32 * Lin, 32 * rowL);
    const int offg = p.ok ? p.t * 4 + lh * rowO : BUF_OOB;
    const int offx = p.ok ? (p.t + lh * dil) * 4 : BUF_OOB;
#pragma unroll
    for (int q = 0; q < 16; ++q) n.g[q] = bload(rg, offg, 2 * q * rowO);
#pragma unroll
    for (int c = 0; c < 32; ++c) n.x[c] = bload(rx, offx, c * rowL);
  };
  auto compute = [&](int tidx, const DzwTile& c) __attribute__((always_inline)) {
    const TilePos p = tile_pos(tidx, tiles_per_seq, li, Lo);
    const int offo = p.ok ? p.t * 4 + 4 * lh * rowO : BUF_OOB;
    const __amdgpu_buffer_rsrc_t rz = brsrc(DZ + (long)p.b * 32 * Lo, 32 * rowO);
    float x[32];
#pragma unroll
    for (int s = 0; s < 32; ++s) x[s] = relu1(c.x[s]);      // relu(s tap lh); 0 outside the sequence
    // z exactly as the forward builds it
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = bzl[mfma32_row(r, 0)];
#pragma unroll
    for (int s = 0; s < 32; ++s) z = mfma32(RESIDENT ? wd[s] : wdp[2 * s], x[s], z);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc = mfma32(RESIDENT ? wt[q] : wtp[2 * WIMG_DENSE_PITCH * q], c.g[q], acc);
    float f0[16], f1[16];
    // ---- dz (D layout: rows mfma32_row(r, lh), column = time li) -> store, transpose
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float dz = z[r] > 0.f ? acc[r] : 0.f;            // (a column past the sequence has dS = 0, so acc = 0)
      bstore(dz, rz, offo, mfma32_row(r, 0) * rowO);
      T[mfma32_row(r, lh) * 33 + li] = dz;
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int q = 0; q < 16; ++q) { f0[q] = T[li * 33 + 2 * q + lh]; bs_dz += f0[q]; }   // f0 = dz[d = li][t = 2q+lh]
    __builtin_amdgcn_wave_barrier();
    // ---- both taps of relu(s): lane half h writes its 32 channels into tile h
#pragma unroll
    for (int s = 0; s < 32; ++s) Th[s * 33 + li] = x[s];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int q = 0; q < 16; ++q) f1[q] = T[li * 33 + 2 * q + lh];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc0 = mfma32(f0[q], f1[q], acc0);
#pragma unroll
    for (int q = 0; q < 16; ++q) f1[q] = T1[li * 33 + 2 * q + lh];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc1 = mfma32(f0[q], f1[q], acc1);
    __builtin_amdgcn_wave_barrier();
    // ---- dS (channel 2q+lh on register q) and relu(z) (D layout; multiplied by dS = 0 past the sequence)
#pragma unroll
    for (int q = 0; q < 16; ++q) T[(2 * q + lh) * 33 + li] = c.g[q];
#pragma unroll
    for (int r = 0; r < 16; ++r) T1[mfma32_row(r, lh) * 33 + li] = relu1(z[r]);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int q = 0; q < 16; ++q) { f0[q] = T[li * 33 + 2 * q + lh]; bs_ds += f0[q]; }
#pragma unroll
    for (int q = 0; q < 16; ++q) f1[q] = T1[li * 33 + 2 * q + lh];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc2 = mfma32(f0[q], f1[q], acc2);
    __builtin_amdgcn_wave_barrier();
  };
  const TileWalkI w = xcd_walk_i(ntiles);
  DzwTile ta, tb;
  // the loads are PINNED in front of the compute (both schedules): left alone hipcc sinks each one down to its consumer
  // (load, wait, mfma, load, wait, ...), 32 serial memory round trips per tile -- the kernel ran 2.5x slower than the two
  // it replaces
  if (RESIDENT) {
    if (w.first < w.last) issue(w.first, ta);
    pingpong_tiles<true>(w, ta, tb, issue, compute);
  } else {
    plain_tiles<true, DzwTile>(w, issue, compute);    // nothing held across tiles: the other wave of the SIMD hides the loads
  }

  // the four waves' sums meet in LDS in WAVE ORDER (plain adds between barriers: float atomics here added them in
  // arrival order, the one place left where this kernel's result could differ in the last bit from run to run)
  for (int wv = 0; wv < 4; ++wv) {
    __syncthreads();
    if (wave == wv) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = mfma32_row(r, lh);
        red[row * 32 + li] += acc0[r];
        red[1024 + row * 32 + li] += acc1[r];
        red[2048 + row * 32 + li] += acc2[r];
      }
      // the bias sums: both lane halves hold partial sums of the same 32 channels -> half 0 first, then half 1
      if (lh == 0) { red[3072 + li] += bs_dz; red[3104 + li] += bs_ds; }
      __builtin_amdgcn_wave_barrier();
      if (lh == 1) { red[3072 + li] += bs_dz; red[3104 + li] += bs_ds; }
    }
  }
  __syncthreads();
  float* out = slab + (long)blockIdx.x * WG_SLAB;
  for (int i = threadIdx.x; i < WG_SLAB; i += 256) out[i] = red[i];
}

// resident weights + cross-tile prefetch (option wn_bwd_t = 3; the default beside another stream's kernels)
__global__ void __launch_bounds__(256)
    wn_block_bwd_dz_wgrad_mfma(const float* __restrict__ dS, const float* __restrict__ w_dil, const float* __restrict__ b_dil,
                               const float* __restrict__ w_dense, const float* __restrict__ s_in, float* __restrict__ DZ,
                               float* __restrict__ slab, int B, int Lin, int dil) {
  __shared__ float tile[4 * 2 * 32 * 33];
  __shared__ float red[WG_SLAB];
  __shared__ float wl[WIMG_DIL_SIZE + 32];
  wn_block_bwd_dz_wgrad_body<true>(tile, red, wl, nullptr, dS, w_dil, b_dil, w_dense, s_in, DZ, slab, B, Lin, dil);
}

// HIGH-OCCUPANCY form of the fused pass (option wn_bwd_t = 2; the default alone on the device)
__global__ void __launch_bounds__(256, 2)
    wn_block_bwd_dz_wgrad_occ(const float* __restrict__ dS, const float* __restrict__ w_dil, const float* __restrict__ b_dil,
                               const float* __restrict__ w_dense, const float* __restrict__ s_in, float* __restrict__ DZ,
                               float* __restrict__ slab, int B, int Lin, int dil) {
  __shared__ float tile[4 * 2 * 32 * 33];
  __shared__ float red[WG_SLAB];
  __shared__ float wl[WIMG_DIL_SIZE + 32];
  __shared__ float wtl[WIMG_DENSE_SIZE];
  wn_block_bwd_dz_wgrad_body<false>(tile, red, wl, wtl, dS, w_dil, b_dil, w_dense, s_in, DZ, slab, B, Lin, dil);
}

// ------------------------------------------------------------------ the same pass with TRANSPOSED products: no LDS transposes
// wn_block_bwd_dz_wgrad_mfma pushes five 32x32 tiles per time tile through LDS to turn "time on the lane" (how the data
// lies in memory) into "channel on the lane" (what a contraction over TIME wants), holds 368 registers and runs one wave
// per SIMD.  Here z and dz are formed TRANSPOSED instead -- the activation tile is the A operand (lane = time, loaded
// coalesced exactly as before), the weights are the B operand:
//     zT[t][d]  = b_dil[d] + sum_{c,k} relu(s[c][t + k*dil]) * W_dil[d][c][k]      (bit-identical to the forward's z: same
//     dzT[t][d] = (z > 0) * sum_r dS[r][t] * W_dense[r][d]                          products, same accumulation order)
// so the accumulators come out with the CHANNEL on the lane and time in the registers (register r of lane-half h is sample
// t0 + mfma32_row(r, h)) -- which is precisely the A / B fragment of the weight-gradient products, whose k-steps may
// enumerate the 32 samples of the tile in any order:
//     dW_dil[d][c][k] += sum_t dzT[t][d] * relu(s[c][t + k*dil])      A = dzT registers,  B = s, channel on the lane
//     dW_dense[r][d]  += sum_t dS[r][t]  * relu(zT[t][d])             A = dS, channel on the lane,  B = relu(zT) registers
// The three channel-on-lane operands (dS, both taps of s) are a SECOND load of lines the time-on-lane loads fetch anyway:
// lane c reads its own row as four 16-byte pieces (samples 8q + 4h .. +3), L1/L2 hits.  dz leaves as four 16-byte stores
// per lane.  No LDS traffic inside the loop, under 256 registers: two waves per SIMD cover each other's memory latency.
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));   // rows start at any sample: 4-byte aligned 16-byte accesses

__global__ void __launch_bounds__(256, 2)
    wn_block_bwd_dzw_t(const float* __restrict__ dS, const float* __restrict__ w_dil, const float* __restrict__ b_dil,
                       const float* __restrict__ w_dense, const float* __restrict__ s_in, float* __restrict__ DZ,
                       float* __restrict__ slab, int B, int Lin, int dil) {
  __shared__ float red[WG_SLAB];
  __shared__ float wl[WIMG_BDENSE];          // the image without b_dense
  const int lane = threadIdx.x & 63;
  const int li = lane & 31, lh = lane >> 5;
  const int Lo = Lin - dil;
  const int tiles_per_seq = tiles_per_sequence<32>(Lo);
  const long ntiles = (long)B * tiles_per_seq;
  const long wave0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long nwaves = ((long)gridDim.x * blockDim.x) >> 6;
  stage_w_dil(wl + WIMG_DIL, w_dil, threadIdx.x, 256);
  stage_w_dense(wl + WIMG_DENSE, w_dense, threadIdx.x, 256);
  stage_bias(wl + WIMG_BDIL, b_dil, threadIdx.x);
  for (int i = threadIdx.x; i < WG_SLAB; i += 256) red[i] = 0.f;
  __syncthreads();
  // The weight fragments stay in LDS and are read per k-step (one conflict-free ds_read_b32 each, 48 per tile against 96
  // MFMAs of 64 cycles): 48 registers less than keeping them resident -- that is what brings the kernel under the 256
  // registers of two waves per SIMD.
  //   wdp[2s]  : B[k = (c = s, tap = lh)][j = d = li] = W_dil[d][c][tap]   (the forward's A fragment)
  //   wtp[66s] : B[k = r = 2s+lh][j = d = li]         = W_dense[r][d]
  const float* wdp = wl + WIMG_DIL + li * WIMG_DIL_PITCH + lh;
  const float* wtp = wl + WIMG_DENSE + lh * WIMG_DENSE_PITCH + li;
  const float bz = wl[WIMG_BDIL + li];

  f32x16 acc0, acc1, acc2;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; acc2[r] = 0.f; }
  float bs_dz = 0.f, bs_ds = 0.f;

  for (long tl = wave0; tl < ntiles; tl += nwaves) {
    const TilePos p = tile_pos(tl, tiles_per_seq, li, Lo);
    const int b = p.b, t0 = p.t0, t = p.t;
    const bool ok = p.ok;
    const int tcl = ok ? t : 0;
    const bool full = t0 + 32 <= Lo;                        // wave-uniform: every sample of the tile exists
    // ---- time on the lane (coalesced; unconditional loads from a clamped address, masked below)
    float x[32], g[16];
    {
      const float* xp = s_in + (long)b * 32 * Lin + tcl + lh * dil;
#pragma unroll
      for (int c = 0; c < 32; ++c) x[c] = xp[(long)c * Lin];
      const float* gp = dS + (long)b * 32 * Lo + tcl;
#pragma unroll
      for (int q = 0; q < 16; ++q) g[q] = gp[(long)(2 * q + lh) * Lo];
    }
    // ---- channel on the lane: lane li reads its own row, samples t0 + mfma32_row(s, lh) = t0 + 8q + 4lh + e (s = 4q + e)
    float gc[16], xc0[16], xc1[16];
    const float* rowS = dS + ((long)b * 32 + li) * Lo + t0 + 4 * lh;
    const float* rowX = s_in + ((long)b * 32 + li) * Lin + t0 + 4 * lh;
    if (full) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f4u a = *reinterpret_cast<const f4u*>(rowS + 8 * q);
        const f4u u = *reinterpret_cast<const f4u*>(rowX + 8 * q);
        const f4u v = *reinterpret_cast<const f4u*>(rowX + dil + 8 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) { gc[4 * q + e] = a[e]; xc0[4 * q + e] = u[e]; xc1[4 * q + e] = v[e]; }
      }
    } else {                                                // ragged last tile of a sequence: element-wise, clamped + masked
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int o = 8 * (s >> 2) + (s & 3);
        const bool in = t0 + 4 * lh + o < Lo;
        const int oc = in ? o : -(t0 + 4 * lh);             // clamp to the row's first sample
        const float a = rowS[oc], u = rowX[oc], v = rowX[oc + dil];
        gc[s] = in ? a : 0.f; xc0[s] = in ? u : 0.f; xc1[s] = in ? v : 0.f;
      }
    }
    __builtin_amdgcn_sched_barrier(0);                      // keep every load of the tile above the MFMAs
#pragma unroll
    for (int c = 0; c < 32; ++c) x[c] = ok ? relu1(x[c]) : 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) g[q] = ok ? g[q] : 0.f;
    // ---- zT, dzT
    f32x16 zT;
#pragma unroll
    for (int r = 0; r < 16; ++r) zT[r] = bz;
#pragma unroll
    for (int s = 0; s < 32; ++s) zT = mfma32(x[s], wdp[2 * s], zT);
    f32x16 dzT;
#pragma unroll
    for (int r = 0; r < 16; ++r) dzT[r] = 0.f;
#pragma unroll
    for (int s = 0; s < 16; ++s) dzT = mfma32(g[s], wtp[66 * s], dzT);
#pragma unroll
    for (int r = 0; r < 16; ++r) dzT[r] = zT[r] > 0.f ? dzT[r] : 0.f;     // rows of samples beyond the sequence are zero (g = 0)
    // ---- dz out: lane li owns row d = li
    float* rowZ = DZ + ((long)b * 32 + li) * Lo + t0 + 4 * lh;
    if (full) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f4u o = {dzT[4 * q], dzT[4 * q + 1], dzT[4 * q + 2], dzT[4 * q + 3]};
        *reinterpret_cast<f4u*>(rowZ + 8 * q) = o;
      }
    } else {
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int o = 8 * (s >> 2) + (s & 3);
        if (t0 + 4 * lh + o < Lo) rowZ[o] = dzT[s];
      }
    }
    // ---- parameter gradients: k-step s stands for sample t0 + mfma32_row(s, lh) on both operands
#pragma unroll
    for (int s = 0; s < 16; ++s) { bs_dz += dzT[s]; bs_ds += gc[s]; }
#pragma unroll
    for (int s = 0; s < 16; ++s) acc2 = mfma32(gc[s], relu1(zT[s]), acc2);
#pragma unroll
    for (int s = 0; s < 16; ++s) acc0 = mfma32(dzT[s], relu1(xc0[s]), acc0);
#pragma unroll
    for (int s = 0; s < 16; ++s) acc1 = mfma32(dzT[s], relu1(xc1[s]), acc1);
  }

#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = mfma32_row(r, lh);
    atomicAdd(&red[row * 32 + li], acc0[r]);
    atomicAdd(&red[1024 + row * 32 + li], acc1[r]);
    atomicAdd(&red[2048 + row * 32 + li], acc2[r]);
  }
  atomicAdd(&red[3072 + li], bs_dz);
  atomicAdd(&red[3104 + li], bs_ds);
  __syncthreads();
  float* out = slab + (long)blockIdx.x * WG_SLAB;
  for (int i = threadIdx.x; i < WG_SLAB; i += 256) out[i] = red[i];
}

// dW_dil[d][c][k] += sum_blocks slab[k*1024 + d*32 + c]; dW_dense[r][d] += slab[2048 + r*32 + d]; biases likewise.
// ALL residual blocks in one launch behind the last of them (blockIdx.y = layer; 20 launches of ~5 us before), and in the
// FIXED order of slab_sum_fixed_order (wn_tail.h); one thread adds the total onto the gradient.  (The per-layer version
// spread the slabs over gridDim.y and added with float atomics: the last place where the encoder's weight gradients could
// differ in the last bit from run to run.)
constexpr int WN_MAXL = 64;       // residual blocks one reduce launch covers
struct WgradTab {
  const float* slab[WN_MAXL];
  int nslab[WN_MAXL];
  float* dW_dil[WN_MAXL];
  float* db_dil[WN_MAXL];
  float* dW_dense[WN_MAXL];
  float* db_dense[WN_MAXL];
};
__global__ void __launch_bounds__(256) wn_wgrad_reduce_all(const WgradTab tab) {
  const int l = blockIdx.y;
  const int i = blockIdx.x * 32 + (threadIdx.x & 31);     // WG_SLAB = 98 * 32
  const int nslab = tab.nslab[l];
  const float s = slab_sum_fixed_order(tab.slab[l] + i, nslab, WG_SLAB);
  if (threadIdx.x >= 32 || nslab <= 0) return;
  if (i < 2048) { if (tab.dW_dil[l]) tab.dW_dil[l][(i & 1023) * 2 + (i >> 10)] += s; }   // every pointer may be NULL (frozen)
  else if (i < 3072) { if (tab.dW_dense[l]) tab.dW_dense[l][i - 2048] += s; }
  else if (i < 3104) { if (tab.db_dil[l]) tab.db_dil[l][i - 3072] += s; }
  else if (tab.db_dense[l]) tab.db_dense[l][i - 3104] += s;
}

// ------------------------------------------------------------------ plan / workspace
struct Plan {
  int n;
  int L[66];        // L[0] = causal output length, L[i+1] = after block i
  size_t s[66];     // offsets of s_i (floats); without save_for_backward only 2 ping-pong buffers
  size_t z, dz, ga, gb, dzt;
  size_t zs[66];    // per-layer pre-ReLU dilation outputs kept for backward (MFMA shape); else 0
  size_t slab;      // weight-gradient partial slabs
  size_t gslab;     // GEMM engine scratch (weight gradients of shapes / switches that go through igemm)
  size_t total;
};
static int make_plan(const avvad_wavenet_desc* d, Plan* p) {
  if (!d || d->n_layers < 0 || d->n_layers > 64 || d->B <= 0 || d->fw < 1 || d->qc < 1 || d->R < 1 || d->D < 1 ||
      d->Bn < 1 || d->P < 1 || (d->n_layers > 0 && !d->dilations_h))
    return AVVAD_EINVAL;
  p->n = d->n_layers;
  p->L[0] = d->L - (d->fw - 1);
  for (int i = 0; i < p->n; ++i) p->L[i + 1] = p->L[i] - d->dilations_h[i] * (d->fw - 1);
  if (p->L[p->n] < 1) return AVVAD_EINVAL;
  size_t off = 0;
  auto take = [&](size_t n) { size_t o = off; off += align_up(n, 64); return o; };
  const size_t B = d->B;
  if (d->save_for_backward) {
    for (int i = 0; i <= p->n; ++i) p->s[i] = take(B * d->R * p->L[i]);
    const size_t big = B * (size_t)(d->R > d->D ? d->R : d->D) * p->L[0];
    p->z = take(big); p->dz = take(big); p->ga = take(big); p->gb = take(big);
    p->dzt = take(B * d->Bn * p->L[p->n]);
    {   // one scratch z buffer (only the unfused backward fallback rebuilds z into it)
      const size_t zb = (d->R == 32 && d->D == 32 && d->fw == 2 && p->n > 0) ? take(B * d->D * p->L[1]) : 0;
      for (int i = 0; i < p->n; ++i) p->zs[i] = zb;
    }
    {   // weight-gradient slabs: residual blocks (WG_MAXBLK x WG_SLAB) or the tail (TAIL_MAXBLK x tail_slab_floats)
      const bool perlayer = d->R == 32 && d->D == 32 && d->fw == 2;      // one slab set per residual block: ONE reduce launch
      const size_t a = (size_t)WG_MAXBLK * WG_SLAB * (perlayer ? (size_t)p->n : 1), b2 = (size_t)TAIL_MAXBLK * tail_slab_floats(d->Bn);
      p->slab = take(a > b2 ? a : b2);
    }
    p->gslab = take(igemm::SLAB_FLOATS);
  } else {
    for (int i = 0; i < p->n; ++i) p->zs[i] = 0;
    const size_t a = take(B * d->R * p->L[0]), b2 = take(B * d->R * p->L[0]);
    for (int i = 0; i <= p->n; ++i) p->s[i] = (i & 1) ? b2 : a;
    p->z = take(B * d->D * p->L[0]);  // scratch of the generic (non-MFMA-shape) block path
    p->dz = p->ga = p->gb = p->dzt = 0;
  }
  p->total = off;
  return AVVAD_OK;
}

static inline bool mfma_shape(const avvad_wavenet_desc* d) { return d->R == 32 && d->D == 32 && d->fw == 2; }
// the buffer-addressed block kernels index a sequence's [32][L] slab with 31-bit byte offsets and count tiles in an int
static inline bool buf_ok(int B, int Lin) {
  return avvad_tune().wn_flat != 1 && (long)Lin * 32 * 4 + 4096 < (1L << 31) && (long)B * cdiv(Lin, 32) < (1L << 31);
}

// ------------------------------------------------------------------ kernel-form choice: one per product and call
// Which form of a product runs, and on how many workgroups, is decided HERE and nowhere else: pure functions of the
// shape, the descriptor's shared_device hint, the gradients wanted and the options table (the only readers of avvad_tune()
// in this file, with buf_ok).  The launchers switch on the result.  Options (common.h / include/avvad.h): wn_flat, wn_dx,
// wn_bwd_t, wn_grid, wn_no_fused_wgrad, wn_no_fused_tail, wn_no_tail_pair.
enum class FwdForm { FLAT, BUF, OCC, WIDE, DMA };
enum class DxForm { FLAT, BUF, OCC };
enum class BwdForm { RESIDENT, OCC, TRANSPOSED, UNFUSED };
enum class TailFwdForm { GENERIC, MFMA1, MFMA4 };     // MFMAn: tail_fwd_mfma<n>, n bn-tiles per wave
enum class TailBwdForm { PAIR, FUSED, MFMA, GENERIC };
struct FwdChoice { FwdForm form; int grid; };
struct DxChoice { DxForm form; int grid; };
struct BwdChoice { BwdForm form; int grid; int grid_z, grid_dz; };   // grid: weight-gradient workgroups = slabs; UNFUSED also runs z and dz
struct TailFwdChoice { TailFwdForm form; int grid; };
struct TailBwdChoice { TailBwdForm form; int grid; };                // PAIR, FUSED: grid = slabs

// Workgroups of a persistent grid: `per_wg` tiles' worth of waves per workgroup, at most `cap` (and at most wn_grid when
// that tuning option is set), then whole XCD groups of 8 for the XCD-aware walk.  Rounding UP leaves surplus waves that
// find no tile; the fused backward rounds DOWN because its workgroup count is its slab count (the summation order).
enum class XcdRound { NONE, UP, UP_FROM_8, DOWN_FROM_8 };
static int wn_grid_size(long tiles, int per_wg, long cap, int wn_grid, XcdRound r) {
  long g = (tiles + per_wg - 1) / per_wg;
  if (g > cap) g = cap;
  if (wn_grid > 0 && g > wn_grid) g = wn_grid;
  if (r == XcdRound::UP || (r == XcdRound::UP_FROM_8 && g >= 8)) g = (g + 7) / 8 * 8;
  if (r == XcdRound::DOWN_FROM_8 && g >= 8) g = g / 8 * 8;
  return (int)(g < 1 ? 1 : g);
}

constexpr int WIDE_FROM = 8192;    // plane length from which the dwordx4 kernel runs
// Forward of one block.  Wide kernel for long planes (C2's one-second chunks: 290 vs 363 us per layer); at the bench shape
// (64 planes of ~6000 samples, 3008 super-tiles) the dword kernel's finer tiles balance better and the two time the same
// (37-38 us).  The choice depends on the plane LENGTH only: the two forms round the residual add differently (last bit),
// and a sequence's result must not depend on how many others share its batch.
static FwdChoice fwd_form(int B, int Lin, int dil) {
  const AvvadTune& t = avvad_tune();
  const int Lo = Lin - dil;
  const bool buf = buf_ok(B, Lin);
  if (buf && (t.wn_flat == 0 || t.wn_flat == 3) && Lo >= 128 && (Lo >= WIDE_FROM || t.wn_flat == 3))     // wn_grid REPLACES this cap
    return {FwdForm::WIDE, wn_grid_size((long)B * cdiv(Lo, 128), 4, t.wn_grid > 0 ? t.wn_grid : 1024, 0, XcdRound::UP)};
  const long ntiles = (long)B * cdiv(Lo, 32);
  if (buf && t.wn_flat == 5 && Lo >= 32)            // 8 waves per workgroup, two workgroups per CU
    return {FwdForm::DMA, wn_grid_size(ntiles, 8, 512, t.wn_grid, XcdRound::UP_FROM_8)};
  if (buf && (t.wn_flat == 0 || t.wn_flat == 4))    // 4 waves per SIMD resident: 1024 workgroups
    return {FwdForm::OCC, wn_grid_size(ntiles, 4, 1024, t.wn_grid, XcdRound::UP_FROM_8)};
  // 2 waves per SIMD resident; each wave walks >= 5 tiles at the bench shape
  return {buf ? FwdForm::BUF : FwdForm::FLAT, wn_grid_size(ntiles, 4, 512, t.wn_grid, XcdRound::NONE)};
}

// Input gradient of one block: the high-occupancy kernel everywhere.  (Round 2 measured it 0.16 ms/step SLOWER beside the
// trunk's backward on another stream, and the shared_device hint picked the resident-weights form there; with round 3's
// trunk kernels -- layer 1 off the persistent engine, fewer and longer class launches -- the same A/B reads 0.06 ms FASTER:
// bench.py --ab wn_dx=1.)
static DxChoice dx_form(int B, int Lin) {
  const AvvadTune& t = avvad_tune();
  const long ntiles = (long)B * cdiv(Lin, 32);
  if (buf_ok(B, Lin) && (t.wn_dx == 0 || t.wn_dx == 2))      // 4 waves per SIMD resident
    return {DxForm::OCC, wn_grid_size(ntiles, 4, 1024, 0, XcdRound::UP_FROM_8)};
  return {buf_ok(B, Lin) && t.wn_dx != 3 ? DxForm::BUF : DxForm::FLAT, wn_grid_size(ntiles, 4, 512, 0, XcdRound::NONE)};
}

// dz + the four parameter gradients of one block (Lo output samples per sequence).  Alone on the device the
// two-waves-per-SIMD form wins (encoder fwd+bwd 3.09 -> 2.90 ms); beside the trunk's backward on the other stream it costs
// the STEP 0.25 ms (same-process A/B), hence the descriptor's shared_device hint.  >= 4 tiles per wave in every form.
static BwdChoice bwd_form(int B, int Lo, bool shared_device, bool any_grad) {
  const AvvadTune& t = avvad_tune();
  const long ntiles = (long)B * cdiv(Lo, 32);
  if (!any_grad || t.wn_no_fused_wgrad)     // frozen weights / tuning switch: z, dz and the weight gradients as separate kernels
    return {BwdForm::UNFUSED, wn_grid_size(ntiles, 16, WG_MAXBLK, 0, XcdRound::NONE), wn_grid_size(ntiles, 4, 512, 0, XcdRound::NONE),
            wn_grid_size(ntiles, 4, 768, 0, XcdRound::NONE)};
  switch (t.wn_bwd_t == 0 ? (shared_device ? 3 : 2) : t.wn_bwd_t) {
    case 3:
      // one workgroup per CU is resident: ONE round of 256, not two of 512 -- every workgroup pays a weight staging
      // prologue and a 12.5 KB slab epilogue (step 22.57 -> 22.06 ms; 128..256 workgroups time the same)
      return {BwdForm::RESIDENT, wn_grid_size(ntiles, 16, 256, 0, XcdRound::NONE), 0, 0};
    case 2:
      return {BwdForm::OCC, wn_grid_size(ntiles, 16, WG_MAXBLK, 0, XcdRound::DOWN_FROM_8), 0, 0};
    default:    // under 256 registers, two workgroups per CU (one wave per SIMD each)
      return {BwdForm::TRANSPOSED, wn_grid_size(ntiles, 16, WG_MAXBLK, 0, XcdRound::NONE), 0, 0};
  }
}

// forward of the tail: one wave per (sequence, pool bin, group of 1 or 4 bn-tiles); GENERIC: one workgroup per (bin, sequence)
static TailFwdChoice tail_fwd_form(int B, int R, int Bn, int P) {
  if (!(R == 32 && Bn % 32 == 0)) return {TailFwdForm::GENERIC, 0};
  const int nt = Bn % 128 == 0 ? 4 : 1;
  return {nt == 4 ? TailFwdForm::MFMA4 : TailFwdForm::MFMA1, wn_grid_size((long)B * P * (Bn / (32 * nt)), 4, 2048, 0, XcdRound::NONE)};
}

// backward of the tail (bottleneck + ReLU + pool) over Lv samples per sequence.  The three MFMA forms look for the bins of
// sample t in the three-register window c0 - 1 .. c0 + 1, c0 = floor(t P / Lv); the bins that contain t are
// c0 .. ceil((t + 1) P / Lv) - 1, which is inside the window exactly when P <= Lv ((t + 1) P / Lv <= t P / Lv + 1).  A pool
// with more bins than samples (fewer than P samples per sequence: not a shape to tune for) takes the generic form, whose loop walks
// the whole range.
static TailBwdChoice tail_bwd_form(int B, int Lv, int R, int Bn, int P, bool any_grad) {
  const AvvadTune& t = avvad_tune();
  const long ntiles = (long)B * cdiv(Lv, 32);
  if (!(R == 32 && Bn % 32 == 0 && Bn <= 1024) || P > Lv) return {TailBwdForm::GENERIC, 0};
  if (Bn == 256 && any_grad && !t.wn_no_fused_tail)        // one slab per workgroup: the plan holds TAIL_MAXBLK of them
    return {t.wn_no_tail_pair ? TailBwdForm::FUSED : TailBwdForm::PAIR, wn_grid_size(ntiles, 4, TAIL_MAXBLK, 0, XcdRound::NONE)};
  return {TailBwdForm::MFMA, wn_grid_size(ntiles, 4, 2048, 0, XcdRound::NONE)};
}

// forward of one residual block, MFMA shape
static void launch_block_fwd(const float* s_in, const float* wd, const float* bd, const float* we, const float* be, float* s_out,
                             int B, int Lin, int dil, hipStream_t s) {
  const FwdChoice c = fwd_form(B, Lin, dil);
  const dim3 grid(c.grid);
  switch (c.form) {
    case FwdForm::WIDE: hipLaunchKernelGGL(wn_block_fwd_w4, grid, dim3(256), 0, s, s_in, wd, bd, we, be, s_out, B, Lin, dil); break;
    case FwdForm::DMA: hipLaunchKernelGGL(wn_block_fwd_dma, grid, dim3(512), 0, s, s_in, wd, bd, we, be, s_out, B, Lin, dil); break;
    case FwdForm::OCC: hipLaunchKernelGGL(wn_block_fwd_occ, grid, dim3(256), 0, s, s_in, wd, bd, we, be, s_out, B, Lin, dil); break;
    case FwdForm::BUF: hipLaunchKernelGGL(wn_block_fwd_buf, grid, dim3(256), 0, s, s_in, wd, bd, we, be, s_out, B, Lin, dil); break;
    case FwdForm::FLAT:
      hipLaunchKernelGGL(wn_block_fwd_mfma<0>, grid, dim3(256), 0, s, s_in, wd, bd, we, be, s_out, (float*)nullptr, B, Lin, dil);
      break;
  }
}

// dw[co][ci][k] += sum_{b,t} dy[b][co][t] * f(x[b][ci][t + k*dil])  for every tap, on the engine
static int wgrad_conv1d(const float* dy, const float* x, float* dw, int B, int Cout, int Cin, int Lout, int Lin, int fw,
                        int dil, int relu_in, hipStream_t s, float* slab) {
  const long K = (long)B * Lout;
  if (K > 0x7fffffffL) return AVVAD_EINVAL;
  const int ktiles = cdiv(K, igemm::BK);
  int split = 1024 / (cdiv(Cout, 64) * cdiv(Cin * fw, 64));
  if (split > ktiles) split = ktiles;
  if (split < 1) split = 1;
  // one launch for all taps: column n = ci*fw + k is exactly the [Cout][Cin][fw] weight layout
  igemm::RowSegK a{dy, Lout, (long)Cout * Lout, Cout, (int)K, Lout, 0, 0, 1, 0};
  igemm::RowSegK b{x, Lin, (long)Cin * Lin, Cin * fw, (int)K, Lout, 0, relu_in, fw, dil};
  igemm::EpiStore e{dw, (long)Cin * fw, nullptr, 1};     // dw += (split tiles combined by the engine's fix-up kernel)
  return igemm::launch<64, 64>(a, b, e, Cout, Cin * fw, (int)K, split, s, slab);
}

static void bias_grad(const float* dy, float* db, int B, int C, int L, hipStream_t s) {
  if (!db) return;
  // (one workgroup per channel: with several per channel adding atomically the sum depended on their arrival order --
  //  the one gradient of the generic encoder path that was not bit-reproducible run to run)
  hipLaunchKernelGGL(chan_sum_acc, dim3(C, 1), dim3(256), 0, s, dy, db, B, C, L);
}

// forward of the tail: out = pool(relu(bb + Wb s_N))
static void launch_tail_fwd(const float* sN, const float* wb, const float* bb, float* out, int B, int R, int Bn, int Lv, int P,
                            hipStream_t s) {
  const TailFwdChoice c = tail_fwd_form(B, R, Bn, P);
  switch (c.form) {
    case TailFwdForm::MFMA4: hipLaunchKernelGGL(tail_fwd_mfma<4>, dim3(c.grid), dim3(256), 0, s, sN, wb, bb, out, B, Bn, Lv, P); break;
    case TailFwdForm::MFMA1: hipLaunchKernelGGL(tail_fwd_mfma<1>, dim3(c.grid), dim3(256), 0, s, sN, wb, bb, out, B, Bn, Lv, P); break;
    case TailFwdForm::GENERIC: hipLaunchKernelGGL(tail_fwd_generic, dim3(P, B), dim3(256), 0, s, sN, wb, bb, out, R, Bn, Lv, P); break;
  }
}

// backward of the tail: dS = d s_N, dW / db += the bottleneck's gradients (either may be NULL); dzt, slab, gslab: workspace
static int launch_tail_bwd(const float* sN, const float* wb, const float* bb, const float* dout, float* dW, float* db, float* dS,
                           float* dzt, float* slab, float* gslab, int B, int R, int Bn, int Lv, int P, hipStream_t s) {
  const TailBwdChoice c = tail_bwd_form(B, Lv, R, Bn, P, dW || db);
  int rc;
  if (c.form == TailBwdForm::PAIR || c.form == TailBwdForm::FUSED) {      // one pass + the slab reduce; dz_t is never materialised
    const bool pair = c.form == TailBwdForm::PAIR;
    const size_t lds = (size_t)tail_fused_lds_floats(Bn, pair ? 2 : 1) * sizeof(float);
    if ((rc = pair ? allow_large_lds<tail_bwd_wgrad_pair<8>>(lds, lds) : allow_large_lds<tail_bwd_wgrad_mfma<8>>(lds, lds))) return rc;
    hipLaunchKernelGGL(pair ? tail_bwd_wgrad_pair<8> : tail_bwd_wgrad_mfma<8>, dim3(c.grid), dim3(pair ? 512 : 256), lds, s, sN, wb,
                       bb, dout, dS, slab, B, Lv, P);
    hipLaunchKernelGGL(tail_wgrad_reduce, dim3(cdiv(tail_slab_floats(Bn), 32)), dim3(256), 0, s, slab, c.grid, Bn, dW, db);
    return AVVAD_OK;
  }
  if (c.form == TailBwdForm::MFMA)
    hipLaunchKernelGGL(tail_bwd_mfma, dim3(c.grid), dim3(256), (size_t)tail_wimg_floats(Bn) * sizeof(float), s, sN, wb, bb, dout,
                       dzt, dS, B, Bn, Lv, P);
  else
    hipLaunchKernelGGL(tail_bwd_dz_generic, dim3(grid1((long)B * Bn * Lv)), dim3(256), 0, s, sN, wb, bb, dout, dzt, B, R, Bn, Lv, P);
  if (dW && (rc = wgrad_conv1d(dzt, sN, dW, B, Bn, R, Lv, Lv, 1, 1, 0, s, gslab))) return rc;
  bias_grad(dzt, db, B, Bn, Lv, s);
  if (c.form == TailBwdForm::GENERIC)
    hipLaunchKernelGGL(conv1d_bwd_data_generic, dim3(grid1((long)B * R * Lv)), dim3(256), 0, s, dzt, wb, (const float*)nullptr,
                       (const float*)nullptr, dS, B, R, Bn, Lv, Lv, 1, 1, 0, 0);
  return AVVAD_OK;
}

}  // namespace

extern "C" size_t avvad_wavenet_workspace(const avvad_wavenet_desc* d) {
  Plan p;
  if (make_plan(d, &p)) return 0;
  return p.total * sizeof(float);
}

extern "C" int avvad_wavenet_fwd(const float* wave, const avvad_wavenet_params* prm, float* out, const avvad_wavenet_desc* d,
                                 void* wsv, size_t ws_bytes, avvad_stream_t sv) {
  AVVAD_ENTER();
  Plan p;
  if (!wave || !prm || !out || !wsv || ws_misaligned(wsv) || make_plan(d, &p)) return AVVAD_EINVAL;
  if (ws_bytes < p.total * sizeof(float)) return AVVAD_EWORKSPACE;
  hipStream_t s = (hipStream_t)sv;
  float* ws = (float*)wsv;
  const int B = d->B, R = d->R, D = d->D, fw = d->fw;
  // causal layer: Conv1d(qc -> R, k = fw), no input ReLU   (:75)
  hipLaunchKernelGGL(conv1d_fwd_generic, dim3(grid1((long)B * R * p.L[0])), dim3(256), 0, s, wave, prm->causal_w,
                     d->use_bias ? prm->causal_b : (const float*)nullptr, (const float*)nullptr, ws + p.s[0], B, d->qc, R,
                     d->L, p.L[0], fw, 1, 0, 0, 0);
  for (int i = 0; i < p.n; ++i) {
    const int dil = d->dilations_h[i];
    const float* bd = d->use_bias ? prm->dil_b_h[i] : nullptr;
    const float* be = d->use_bias ? prm->dense_b_h[i] : nullptr;
    if (mfma_shape(d)) {
      // z (pre-ReLU dilation output) is NOT kept: backward rebuilds it from s_i inside its fused kernel, bit-identically
      launch_block_fwd(ws + p.s[i], prm->dil_w_h[i], bd, prm->dense_w_h[i], be, ws + p.s[i + 1], B, p.L[i], dil, s);
    } else {
      float* z = ws + p.z;
      hipLaunchKernelGGL(conv1d_fwd_generic, dim3(grid1((long)B * D * p.L[i + 1])), dim3(256), 0, s, ws + p.s[i],
                         prm->dil_w_h[i], bd, (const float*)nullptr, z, B, R, D, p.L[i], p.L[i + 1], fw, dil, 1, 0, 0);
      hipLaunchKernelGGL(conv1d_fwd_generic, dim3(grid1((long)B * R * p.L[i + 1])), dim3(256), 0, s, z, prm->dense_w_h[i], be,
                         ws + p.s[i], ws + p.s[i + 1], B, D, R, p.L[i + 1], p.L[i + 1], 1, 1, 1, p.L[i] - p.L[i + 1], p.L[i]);
    }
  }
  launch_tail_fwd(ws + p.s[p.n], prm->bott_w, d->use_bias ? prm->bott_b : (const float*)nullptr, out, B, R, d->Bn, p.L[p.n],
                  d->P, s);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

// One residual block alone (the layer-at-a-time kernel the large dilations run on): what bench.py times per launch for
// the HBM roofline entry, like avvad_conv2d_fwd for the MFMA one.
extern "C" int avvad_wavenet_block_fwd(const float* s_in, const float* w_dil, const float* b_dil, const float* w_dense,
                                       const float* b_dense, float* s_out, int B, int Lin, int dil, avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!s_in || !w_dil || !w_dense || !s_out || B <= 0 || dil < 1 || Lin - dil < 1) return AVVAD_EINVAL;
  launch_block_fwd(s_in, w_dil, b_dil, w_dense, b_dense, s_out, B, Lin, dil, (hipStream_t)sv);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

extern "C" int avvad_wavenet_bwd(const float* wave, const avvad_wavenet_params* prm, const float* dout,
                                 const avvad_wavenet_grads* g, float* dwave, const avvad_wavenet_desc* d, void* wsv,
                                 size_t ws_bytes, avvad_stream_t sv) {
  AVVAD_ENTER();
  Plan p;
  if (!wave || !prm || !dout || !g || !wsv || ws_misaligned(wsv) || make_plan(d, &p) || !d->save_for_backward) return AVVAD_EINVAL;
  if (ws_bytes < p.total * sizeof(float)) return AVVAD_EWORKSPACE;
  hipStream_t s = (hipStream_t)sv;
  float* ws = (float*)wsv;
  const int B = d->B, R = d->R, D = d->D, fw = d->fw, Bn = d->Bn;
  int rc;
  float* Z = ws + p.z;
  float* DZ = ws + p.dz;
  float* GA = ws + p.ga;  // d s_{i+1}
  float* GB = ws + p.gb;  // d s_i
  // ---- tail: d s_N into GA, the bottleneck's gradients
  if ((rc = launch_tail_bwd(ws + p.s[p.n], prm->bott_w, d->use_bias ? prm->bott_b : (const float*)nullptr, dout, g->bott_w,
                            d->use_bias ? g->bott_b : (float*)nullptr, GA, ws + p.dzt, ws + p.slab, ws + p.gslab, B, R, Bn,
                            p.L[p.n], d->P, s)))
    return rc;
  // ---- residual blocks, last to first
  WgradTab wtab;
  bool any_slab = false;
  for (int l = 0; l < WN_MAXL; ++l) {
    wtab.slab[l] = nullptr; wtab.nslab[l] = 0;
    wtab.dW_dil[l] = wtab.db_dil[l] = wtab.dW_dense[l] = wtab.db_dense[l] = nullptr;
  }
  auto note_slabs = [&](int i, float* slab_i, int wb) {
    wtab.slab[i] = slab_i; wtab.nslab[i] = wb;
    wtab.dW_dil[i] = g->dil_w_h[i]; wtab.dW_dense[i] = g->dense_w_h[i];
    wtab.db_dil[i] = d->use_bias ? g->dil_b_h[i] : (float*)nullptr;
    wtab.db_dense[i] = d->use_bias ? g->dense_b_h[i] : (float*)nullptr;
    any_slab = true;
  };
  for (int i = p.n - 1; i >= 0; --i) {
    float* const slab_i = ws + p.slab + (size_t)i * WG_MAXBLK * WG_SLAB;     // this block's partial sums (reduced at the end)
    const int dil = d->dilations_h[i];
    const int Li = p.L[i], Lo = p.L[i + 1];
    const float* si = ws + p.s[i];
    const float* bd = d->use_bias ? prm->dil_b_h[i] : nullptr;
    const bool fast = mfma_shape(d);
    float* Zi = fast ? ws + p.zs[i] : Z;
    if (!fast)  // recompute z = dil_i(relu(s_i)) (pre-ReLU)
      hipLaunchKernelGGL(conv1d_fwd_generic, dim3(grid1((long)B * D * Lo)), dim3(256), 0, s, si, prm->dil_w_h[i], bd,
                         (const float*)nullptr, Zi, B, R, D, Li, Lo, fw, dil, 1, 0, 0);
    if (fast) {
      // dz = (z>0) * W_dense^T dS and all four parameter gradients (one pass, or three kernels) ; then d s_i.
      // A block's four parameter gradients are wanted independently (partially frozen blocks): the fused kernels always
      // form all four sums, the reduce skips the NULL destinations
      const bool any_grad = g->dil_w_h[i] || g->dense_w_h[i] || (d->use_bias && (g->dil_b_h[i] || g->dense_b_h[i]));
      const BwdChoice bc = bwd_form(B, Lo, d->shared_device != 0, any_grad);
      switch (bc.form) {
        case BwdForm::RESIDENT:
          hipLaunchKernelGGL(wn_block_bwd_dz_wgrad_mfma, dim3(bc.grid), dim3(256), 0, s, GA, prm->dil_w_h[i], bd,
                             prm->dense_w_h[i], si, DZ, slab_i, B, Li, dil);
          break;
        case BwdForm::OCC:
          hipLaunchKernelGGL(wn_block_bwd_dz_wgrad_occ, dim3(bc.grid), dim3(256), 0, s, GA, prm->dil_w_h[i], bd,
                             prm->dense_w_h[i], si, DZ, slab_i, B, Li, dil);
          break;
        case BwdForm::TRANSPOSED:
          hipLaunchKernelGGL(wn_block_bwd_dzw_t, dim3(bc.grid), dim3(256), 0, s, GA, prm->dil_w_h[i], bd, prm->dense_w_h[i], si,
                             DZ, slab_i, B, Li, dil);
          break;
        case BwdForm::UNFUSED:      // z is not kept by the forward -> rebuild it first
          hipLaunchKernelGGL(wn_block_fwd_mfma<2>, dim3(bc.grid_z), dim3(256), 0, s, si, prm->dil_w_h[i], bd, prm->dense_w_h[i],
                             (const float*)nullptr, (float*)nullptr, Zi, B, Li, dil);
          hipLaunchKernelGGL(wn_block_bwd_dz_mfma, dim3(bc.grid_dz), dim3(256), 0, s, GA, Zi, prm->dense_w_h[i], DZ, B, Lo);
          if (any_grad)
            hipLaunchKernelGGL(wn_block_wgrad_mfma, dim3(bc.grid), dim3(256), 0, s, GA, Zi, DZ, si, slab_i, B, Li, dil);
          break;
      }
      if (any_grad) note_slabs(i, slab_i, bc.grid);
      const DxChoice dc = dx_form(B, Li);
      switch (dc.form) {
        case DxForm::OCC:
          hipLaunchKernelGGL(wn_block_bwd_dx_occ, dim3(dc.grid), dim3(256), 0, s, DZ, si, GA, prm->dil_w_h[i], GB, B, Li, dil);
          break;
        case DxForm::BUF:
          hipLaunchKernelGGL(wn_block_bwd_dx_buf, dim3(dc.grid), dim3(256), 0, s, DZ, si, GA, prm->dil_w_h[i], GB, B, Li, dil);
          break;
        case DxForm::FLAT:
          hipLaunchKernelGGL(wn_block_bwd_dx_mfma, dim3(dc.grid), dim3(256), 0, s, DZ, si, GA, prm->dil_w_h[i], GB, B, Li, dil);
          break;
      }
    } else {
      // dense (1x1) layer: d W_dense = GA . relu(z)^T ; d b ; dz = (z>0) * W_dense^T GA
      if (g->dense_w_h[i] && (rc = wgrad_conv1d(GA, Zi, g->dense_w_h[i], B, R, D, Lo, Lo, 1, 1, 1, s, ws + p.gslab))) return rc;
      if (d->use_bias) bias_grad(GA, g->dense_b_h[i], B, R, Lo, s);
      hipLaunchKernelGGL(conv1d_bwd_data_generic, dim3(grid1((long)B * D * Lo)), dim3(256), 0, s, GA, prm->dense_w_h[i], Zi,
                         (const float*)nullptr, DZ, B, D, R, Lo, Lo, 1, 1, 0, 0);
      // dilated layer: d W_dil = dz . relu(s_i shifted)^T ; d b ; d s_i = (s_i>0) * W_dil^T (*) dz + left-padded GA
      if (g->dil_w_h[i] && (rc = wgrad_conv1d(DZ, si, g->dil_w_h[i], B, D, R, Lo, Li, fw, dil, 1, s, ws + p.gslab))) return rc;
      if (d->use_bias) bias_grad(DZ, g->dil_b_h[i], B, D, Lo, s);
      hipLaunchKernelGGL(conv1d_bwd_data_generic, dim3(grid1((long)B * R * Li)), dim3(256), 0, s, DZ, prm->dil_w_h[i], si, GA,
                         GB, B, R, D, Li, Lo, fw, dil, Li - Lo, Lo);
    }
    float* t = GA; GA = GB; GB = t;
  }
  if (any_slab) hipLaunchKernelGGL(wn_wgrad_reduce_all, dim3(WG_SLAB / 32, p.n), dim3(256), 0, s, wtab);
  // ---- causal layer
  if (d->qc * fw <= 4) {   // narrow causal layer: weight + bias gradient in one pass over GA
    if (g->causal_w || (d->use_bias && g->causal_b))
    {
      const int ny = B < 32 ? B : 32;
      float* part = ws + p.gslab;          // the engine scratch is idle here
      hipLaunchKernelGGL(narrow_conv1d_grads, dim3(R, ny), dim3(256), 0, s, GA, wave, part, B, R, d->qc, p.L[0], d->L, fw);
      hipLaunchKernelGGL(narrow_conv1d_grads_sum, dim3(cdiv(R * 5, 256)), dim3(256), 0, s, part, ny, R, d->qc * fw, g->causal_w,
                         d->use_bias ? g->causal_b : (float*)nullptr);
    }
  } else {
    if (g->causal_w && (rc = wgrad_conv1d(GA, wave, g->causal_w, B, R, d->qc, p.L[0], d->L, fw, 1, 0, s, ws + p.gslab))) return rc;
    if (d->use_bias) bias_grad(GA, g->causal_b, B, R, p.L[0], s);
  }
  if (dwave)
    hipLaunchKernelGGL(conv1d_bwd_data_generic, dim3(grid1((long)B * d->qc * d->L)), dim3(256), 0, s, GA, prm->causal_w,
                       (const float*)nullptr, (const float*)nullptr, dwave, B, d->qc, R, d->L, p.L[0], fw, 1, 0, 0);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}
