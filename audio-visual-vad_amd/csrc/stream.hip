// stream.hip -- stateful, chunked inference: an LSTM layer with (h, c) in and out, and the encoder as a streaming
// kernel that keeps every layer's left context between calls.  Inference only (nothing is saved for a backward pass),
// deterministic (no float atomics, fixed summation orders), and no kernel here waits on another workgroup: a time step
// is a launch, and one encoder row is one workgroup.
//
// Why chunked evaluation equals the whole-utterance forward: the encoder is a valid (left-context-only) Conv1d stack, the
// trunk / concat fusion / final Linear are per frame, the LSTMs are unidirectional (Audio_Net.py:50-59,
// Video_Net.py:102-116, AV_Net.py:124-140, wavenet_autoencoder.py:74-93).
#include "gemm_api.h"
#include "lstm_cell.h"
#include <stdlib.h>

namespace {

// ==================================================================== LSTM layer with state
__global__ void st_copy(const float* __restrict__ src, float* __restrict__ dst, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

template <bool VEC>
__device__ __forceinline__ float4 ld4(const float* __restrict__ p, int k, int K) {
  if (VEC) return k < K ? *reinterpret_cast<const float4*>(p + k) : float4{0.f, 0.f, 0.f, 0.f};   // K % 4 == 0: all or nothing
  float4 v;
  v.x = k < K ? p[k] : 0.f;
  v.y = k + 1 < K ? p[k + 1] : 0.f;
  v.z = k + 2 < K ? p[k + 2] : 0.f;
  v.w = k + 3 < K ? p[k + 3] : 0.f;
  return v;
}

// One time step of one layer for the few-rows regime: a weight-streaming product, not a tile GEMM.  Workgroup blockIdx.x
// owns hidden units 4 blk .. 4 blk + 3, i.e. the 16 rows {gate * H + unit} of W_hh in the order 4 * u + gate of
// lstm_cell.h, and reads them ONCE per launch with 16-byte loads; blockIdx.y owns a run of 16 * NG batch rows ("columns"
// of the product), each group of 16 one v_mfma_f32_16x16x4_f32 column block, padded by clamping.  The four waves take the
// 16-float chunks of K round-robin; their partial sums meet in LDS and are added in wave order, then wave g finishes
// column group g: gate arithmetic in registers on top of the input projection G, then c (in place: only this workgroup
// touches its units), h into ANOTHER buffer than it was read from (every workgroup reads all of h_{t-1}) and y.  G holds
// x W_ih^T + b_ih; b_hh is added here.  hprev / cin may be NULL: a zero state (the product is skipped).  cin and cout are
// the same buffer except at the first step of a call whose c0 and cT differ.  A row with t >= lengths[b] passes h and c
// through and writes a zero output: length 0 keeps the state bit for bit.
// A column's result does not depend on NG, VEC or on what the other columns hold.
template <int NG, bool VEC>
__global__ void __launch_bounds__(256)
    lstm_state_step(const float* __restrict__ G, const float* __restrict__ w_hh, const float* __restrict__ b_hh,
                    const float* __restrict__ hprev, float* __restrict__ hnext, const float* cin, float* cout,
                    float* __restrict__ y, const int* __restrict__ lengths, int B, int T, int H, int t) {
  __shared__ f32x4 part[NG][4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int cb = blockIdx.y * (16 * NG);
  int unit = lstm_cell::quad_unit(i, blockIdx.x);
  if (unit > H - 1) unit = H - 1;                            // H % 4 != 0: the surplus rows repeat the last unit, never stored
  const float* wrow = w_hh + (long)lstm_cell::whh_row(i, unit, H) * H;
  const float* hrow[NG];
  f32x4 acc[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    int b = cb + 16 * g + i;
    if (b > B - 1) b = B - 1;
    hrow[g] = hprev ? hprev + (long)b * H : nullptr;
    acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int nkc = (H + 15) >> 4;
  for (int kk = wave; hprev && kk < nkc; kk += 4) {
    const int k = 16 * kk + 4 * q;
    const float4 a = ld4<VEC>(wrow, k, H);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      acc[g] = lstm_cell::mfma4(a, ld4<VEC>(hrow[g], k, H), acc[g]);
    }
  }
#pragma unroll
  for (int g = 0; g < NG; ++g) part[g][wave][lane] = acc[g];
  __syncthreads();
  if (wave >= NG) return;
  // r[gate] = recurrent part of the gate of unit j for batch row b
  const f32x4 r = lstm_cell::add_slices(part[wave][0][lane], &part[wave][0][lane], 4, 64);
  const int b = cb + 16 * wave + i, j = 4 * blockIdx.x + q;
  if (b >= B || j >= H) return;
  const long o = (long)b * H + j, oy = ((long)b * T + t) * H + j;
  const float cp = cin ? cin[o] : 0.f;
  if (t >= lengths[b]) {
    y[oy] = 0.f;
    hnext[o] = hprev ? hprev[o] : 0.f;
    if (cout != cin) cout[o] = cp;
    return;
  }
  const float* g = G + ((long)b * T + t) * 4 * H;
  const lstm_cell::Fwd c = lstm_cell::fwd([&](int e) { return g[e * H + j] + (r[e] + b_hh[e * H + j]); }, cp);
  cout[o] = c.c;
  hnext[o] = c.h;
  y[oy] = c.h;
}

struct LWs {
  float *G, *hbuf, *slab;
  size_t total;
};
LWs lcarve(const avvad_lstm_desc* d, float* base) {
  LWs w;
  size_t off = 0;
  auto take = [&](size_t n) { size_t o = off; off += align_up(n, 64); return base ? base + o : (float*)nullptr; };
  const size_t B = d->B, T = d->T, H = d->H;
  w.G = take(B * T * 4 * H);
  w.hbuf = take(2 * align_up(B * H, 64));
  w.slab = take(igemm::SLAB_FLOATS);
  w.total = off;
  return w;
}

// The form of lstm_state_step: NG groups of 16 batch rows per workgroup (as many as cover B, four at the most), and VEC,
// 16-byte loads of W_hh and h: rows of H % 4 == 0 floats from 16-byte bases -- w_hh, h0 (read at step 0) and hT (read by
// a later call); the workspace buffers between them are aligned by the entry point's check.
struct StateChoice { int NG; bool vec; };
StateChoice state_form(int B, int H, const float* w_hh, const float* h0, const float* hT) {
  return {B <= 16 ? 1 : (B <= 32 ? 2 : 4),
          H % 4 == 0 && ((uintptr_t)w_hh & 15) == 0 && (!h0 || ((uintptr_t)h0 & 15) == 0) && ((uintptr_t)hT & 15) == 0};
}
using StateKernel = void (*)(const float*, const float*, const float*, const float*, float*, const float*, float*, float*,
                             const int*, int, int, int, int);
template <bool VEC>
StateKernel state_kernel(int NG) {
  return NG == 1 ? lstm_state_step<1, VEC> : (NG == 2 ? lstm_state_step<2, VEC> : lstm_state_step<4, VEC>);
}

// ==================================================================== streaming encoder
// State block of one row (floats): [0..3] header -- words 0/1 hold the 64-bit count of columns consumed since the
// reset, the rest is zero -- then the causal layer's last (fw-1) input columns [qc][fw-1], then per residual layer its
// last h_i = (fw-1) d_i input columns [R][h_i].  Every history is a RING indexed by the absolute column number modulo
// its length, so a call moves no old column; an all-zero block is "start of utterance".
constexpr int WS_HDR = 4;
constexpr int WS_NT = 512;       // threads per workgroup
constexpr int WS_NC_MFMA = 256;  // columns per pass of the MFMA form: one 32-column tile per wave

struct WsTab {
  int n;
  int dil[64];
  const float* dw[64];
  const float* db[64];
  const float* ew[64];
  const float* eb[64];
  const float *cw, *cb, *bw, *bb;
};

__device__ __forceinline__ int ring_wrap(int v, int h) { return v < 0 ? v + h : v; }

// One workgroup per row walks causal layer -> residual stack -> bottleneck -> ReLU -> mean over k columns for the row's
// n_valid new columns, NC columns per pass.  The pass's columns stay in LDS (cur [R][NC], updated in place layer by
// layer: s_{i+1}[j] = dense(relu(z))[j] + s_i[j]); taps that reach behind the pass read the layer's ring, and the pass's
// last h_i columns go back into it once every wave has read.  __syncthreads() separates the layers.  Column c of the call
// is dropped while c < skip (warm-up, computed from the zero history); the others fill frames of k columns; a frame that
// straddles two passes is carried in LDS (pacc).  MF: R = D = 32, fw = 2 on v_mfma_f32_32x32x2_f32, NC = 256; the dilation
// product's D tile feeds the dense product as its B operand straight from registers (the contraction index of MFMA step
// r is the D row of register r).  Otherwise the plain direct form with z in LDS.
template <bool MF>
__global__ void __launch_bounds__(WS_NT)
    wn_stream_kernel(const float* __restrict__ chunk, float* state, const int* __restrict__ n_valid,
                     const int* __restrict__ skip_, float* __restrict__ out, const WsTab tab, int L, int qc, int R, int D,
                     int Bn, int fw, int k, int out_frames, long state_floats, int NC) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int BT = NC + 1;                              // pitch of the bottleneck tile
  float* cur = lds;                                   // [R][NC]
  float* zb = cur + (long)R * NC;                     // [D][NC]  (direct form only)
  float* bt = zb + (MF ? 0 : (long)D * NC);           // [32][NC + 1]
  float* psum = bt + 32 * BT;                         // [WS_NT / 32][32]
  float* pacc = psum + WS_NT;                         // [Bn]
  float* wdl = pacc + Bn;                             // MFMA form: the layer's W_dil as [(ci, tap)][33], W_dense as [dc][33]
  float* wel = wdl + 64 * 33;
  float* st = state + (long)b * state_floats;
  int n = n_valid[b];
  n = n < 0 ? 0 : (n > L ? L : n);
  int skip = skip_[b];
  skip = skip < 0 ? 0 : skip;
  const int nf_all = n > skip ? (n - skip) / k : 0;
  const int nf = nf_all < out_frames ? nf_all : out_frames;
  float* orow = out + (long)b * out_frames * Bn;
  for (long i = (long)nf * Bn + tid; i < (long)out_frames * Bn; i += WS_NT) orow[i] = 0.f;   // frames this row does not fill
  if (n == 0) return;                                 // the state is not touched
  for (int i = tid; i < Bn; i += WS_NT) pacc[i] = 0.f;
  const unsigned long long count0 = *reinterpret_cast<const unsigned long long*>(st);
  const float* x = chunk + (long)b * qc * L;
  const int hc = fw - 1;
  float* ring_c = st + WS_HDR;
  const int pool_end = skip + nf * k;                 // columns [skip, pool_end) of the call fill frames

  for (int p0 = 0; p0 < n; p0 += NC) {
    const int np = n - p0 < NC ? n - p0 : NC;
    const unsigned long long count = count0 + (unsigned long long)p0;
    // ---- causal layer: Conv1d(qc -> R, fw), no input ReLU
    {
      const int base = hc > 0 ? (int)(count % (unsigned long long)hc) : 0;
      for (int idx = tid; idx < R * np; idx += WS_NT) {
        const int r = idx / np, j = idx - r * np;
        float acc = tab.cb ? tab.cb[r] : 0.f;
        for (int ci = 0; ci < qc; ++ci)
          for (int kk = 0; kk < fw; ++kk) {
            const int o = j - (hc - kk);
            const float v = o >= 0 ? x[(long)ci * L + p0 + o] : ring_c[ci * hc + ring_wrap(base + o, hc)];
            acc = fmaf(tab.cw[(r * qc + ci) * fw + kk], v, acc);
          }
        cur[r * NC + j] = acc;
      }
      __syncthreads();
      for (int idx = tid; idx < qc * hc; idx += WS_NT) {      // the last hc input columns, wherever they come from
        const int ci = idx / hc, e = idx - ci * hc;
        const int j = np - hc + e;                            // pass-local column of the e-th newest-history column
        if (j >= 0) ring_c[ci * hc + (base + j) % hc] = x[(long)ci * L + p0 + j];
      }
      __syncthreads();
    }
    // ---- residual stack
    float* ring = ring_c + (long)qc * hc;
    for (int i = 0; i < tab.n; ++i) {
      const int dil = tab.dil[i], h = hc * dil;
      const int base = h > 0 ? (int)(count % (unsigned long long)h) : 0;
      const float *wd = tab.dw[i], *bd = tab.db[i], *we = tab.ew[i], *be = tab.eb[i];
      if (MF) {
        const int lane = tid & 63, wave = tid >> 6;
        const int jl = lane & 31, kh = lane >> 5;
        const int j = 32 * wave + jl, o = j - dil;
        const int ridx = o < 0 ? ring_wrap(base + o, h) : 0;
        // the layer's 12 KB of weights go through LDS, transposed so that a wave's operand read is one row: read
        // straight from memory, lane i's A operand is row i of a [32][64] matrix, 64 cache lines per load
        for (int e = tid; e < 2048; e += WS_NT) wdl[(e & 63) * 33 + (e >> 6)] = wd[e];
        for (int e = tid; e < 1024; e += WS_NT) wel[(e & 31) * 33 + (e >> 5)] = we[e];
        __syncthreads();
        f32x16 z;
#pragma unroll
        for (int r = 0; r < 16; ++r) z[r] = 0.f;
#pragma unroll
        for (int m = 0; m < 16; ++m) {
          const int ci = 2 * m + kh;
          const float x1 = cur[ci * NC + j];
          // both loads are issued, with clamped addresses, and the VALUES are selected: a branch per operand would
          // put the 16 ring loads' latencies one behind the other
          const float xc = cur[ci * NC + (o >= 0 ? o : 0)], xr = ring[(long)ci * h + ridx];
          const float x0 = o >= 0 ? xc : xr;
          z = mfma32(wdl[(ci * 2) * 33 + jl], relu1(x0), z);
          z = mfma32(wdl[(ci * 2 + 1) * 33 + jl], relu1(x1), z);
        }
        f32x16 yv;
#pragma unroll
        for (int r = 0; r < 16; ++r) yv[r] = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = mfma32_row(r, kh);
          yv = mfma32(wel[row * 33 + jl], relu1(z[r] + (bd ? bd[row] : 0.f)), yv);
        }
        float ov[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = mfma32_row(r, kh);
          ov[r] = cur[row * NC + j];
          yv[r] = yv[r] + (be ? be[row] : 0.f) + ov[r];
        }
        __syncthreads();                                      // every wave has read cur and the ring
        const bool keep = j < np && j >= np - h;
        const int widx = keep ? (base + j) % h : 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = mfma32_row(r, kh);
          cur[row * NC + j] = yv[r];
          if (keep) ring[(long)row * h + widx] = ov[r];
        }
        __syncthreads();
      } else {
        for (int idx = tid; idx < D * np; idx += WS_NT) {
          const int dc = idx / np, j = idx - dc * np;
          float acc = bd ? bd[dc] : 0.f;
          for (int ci = 0; ci < R; ++ci)
            for (int kk = 0; kk < fw; ++kk) {
              const int o = j - (hc - kk) * dil;
              float v = cur[ci * NC + (o >= 0 ? o : 0)];
              if (o < 0) v = ring[(long)ci * h + ring_wrap(base + o, h)];
              acc = fmaf(wd[(dc * R + ci) * fw + kk], fmaxf(v, 0.f), acc);
            }
          zb[dc * NC + j] = fmaxf(acc, 0.f);
        }
        __syncthreads();                                      // z complete; every read of the ring is done
        for (int idx = tid; idx < R * np; idx += WS_NT) {
          const int r = idx / np, j = idx - r * np;
          float acc = be ? be[r] : 0.f;
          for (int dc = 0; dc < D; ++dc) acc = fmaf(we[r * D + dc], zb[dc * NC + j], acc);
          const float old = cur[r * NC + j];
          if (j >= np - h) ring[(long)r * h + (base + j) % h] = old;      // h == 0: never true
          cur[r * NC + j] = acc + old;
        }
        __syncthreads();
      }
      ring += (long)R * h;
    }
    // ---- bottleneck -> ReLU -> mean over the frames' columns
    const int ja = skip - p0 > 0 ? skip - p0 : 0;
    const int je = pool_end - p0 < np ? pool_end - p0 : np;
    if (ja >= je) continue;                                   // warm-up (or surplus) columns only: uniform
    const int f_first = (p0 + ja - skip) / k, f_last = (p0 + je - 1 - skip) / k;
    for (int bn0 = 0; bn0 < Bn; bn0 += 32) {
      if (MF) {
        const int lane = tid & 63, wave = tid >> 6;
        const int jl = lane & 31, kh = lane >> 5;
        const int j = 32 * wave + jl;
        const int arow = bn0 + jl < Bn ? bn0 + jl : Bn - 1;
        f32x16 a;
#pragma unroll
        for (int r = 0; r < 16; ++r) a[r] = 0.f;
#pragma unroll
        for (int m = 0; m < 16; ++m) a = mfma32(tab.bw[arow * 32 + 2 * m + kh], cur[(2 * m + kh) * NC + j], a);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = mfma32_row(r, kh);
          const int bn = bn0 + row < Bn ? bn0 + row : Bn - 1;
          bt[row * BT + j] = fmaxf(a[r] + (tab.bb ? tab.bb[bn] : 0.f), 0.f);
        }
      } else {
        for (int idx = tid; idx < 32 * np; idx += WS_NT) {
          const int row = idx / np, j = idx - row * np;
          const int bn = bn0 + row < Bn ? bn0 + row : Bn - 1;
          float acc = tab.bb ? tab.bb[bn] : 0.f;
          for (int r = 0; r < R; ++r) acc = fmaf(tab.bw[bn * R + r], cur[r * NC + j], acc);
          bt[row * BT + j] = fmaxf(acc, 0.f);
        }
      }
      __syncthreads();
      // frame by frame: WS_NT / 32 threads per bottleneck row each add a contiguous run of the frame's columns, then one
      // thread per row adds the runs in order onto what earlier passes carried
      const int row = tid & 31, slot = tid >> 5, bn = bn0 + row;
      for (int f = f_first; f <= f_last; ++f) {
        const int fs = skip + f * k - p0, fe = fs + k;        // the frame's columns, pass-local
        const int a0 = fs > ja ? fs : ja, e0 = fe < je ? fe : je;
        const int per = (e0 - a0 + WS_NT / 32 - 1) / (WS_NT / 32);
        const int lo = a0 + slot * per;
        const int hi = lo + per < e0 ? lo + per : e0;
        float s = 0.f;
        for (int j = lo; j < hi; ++j) s += bt[row * BT + j];
        psum[slot * 32 + row] = s;
        __syncthreads();
        if (slot == 0 && bn < Bn) {
          float tot = pacc[bn];
          for (int s2 = 0; s2 < WS_NT / 32; ++s2) tot += psum[s2 * 32 + row];
          if (fe <= np) {                                     // the frame ends in this pass
            orow[(long)f * Bn + bn] = tot / (float)k;
            pacc[bn] = 0.f;
          } else {
            pacc[bn] = tot;
          }
        }
        __syncthreads();
      }
    }
  }
  if (tid == 0) *reinterpret_cast<unsigned long long*>(st) = count0 + (unsigned long long)n;
}

bool stream_desc_ok(const avvad_wavenet_desc* d) {
  if (!d || d->n_layers < 0 || d->n_layers > 64 || d->B <= 0 || d->L < 1 || d->fw < 1 || d->qc < 1 || d->R < 1 || d->D < 1 ||
      d->Bn < 1 || (d->n_layers > 0 && !d->dilations_h) || d->save_for_backward)
    return false;
  for (int i = 0; i < d->n_layers; ++i)
    if (d->dilations_h[i] < 1) return false;
  return true;
}
size_t stream_state_floats(const avvad_wavenet_desc* d) {
  size_t sum = 0;
  for (int i = 0; i < d->n_layers; ++i) sum += (size_t)d->dilations_h[i];
  return align_up((size_t)WS_HDR + (size_t)(d->fw - 1) * ((size_t)d->qc + (size_t)d->R * sum), 4);
}
constexpr size_t WS_LDS_MAX = 150 * 1024;      // of the CU's 160 KiB
size_t stream_lds_bytes(const avvad_wavenet_desc* d, bool mf, int NC) {
  return ((size_t)d->R * NC + (mf ? 96 * 33 : (size_t)d->D * NC) + 32 * (size_t)(NC + 1) + WS_NT + (size_t)d->Bn) * sizeof(float);
}

}  // namespace

extern "C" size_t avvad_lstm_state_workspace(const avvad_lstm_desc* d) {
  if (!d || d->B <= 0 || d->T <= 0 || d->H <= 0 || d->In <= 0 || d->save_for_backward) return 0;
  return lcarve(d, nullptr).total * sizeof(float);
}

extern "C" int avvad_lstm_layer_fwd_state(const float* x, const float* w_ih, const float* w_hh, const float* b_ih,
                                          const float* b_hh, const float* h0, const float* c0, float* y, float* hT, float* cT,
                                          const avvad_lstm_desc* d, void* wsv, size_t ws_bytes, avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!x || !w_ih || !w_hh || !b_ih || !b_hh || !y || !hT || !cT || !d || !wsv || !d->lengths || d->B <= 0 || d->T <= 0 ||
      d->In <= 0 || d->H <= 0 || d->save_for_backward || ((uintptr_t)wsv & 15))     // the h buffers are read 16 bytes at a time
    return AVVAD_EINVAL;
  hipStream_t s = (hipStream_t)sv;
  LWs w = lcarve(d, (float*)wsv);
  if (ws_bytes < w.total * sizeof(float)) return AVVAD_EWORKSPACE;
  const int B = d->B, T = d->T, H = d->H, In = d->In;
  const long BH = (long)B * H;
  float* hb[2] = {w.hbuf, w.hbuf + align_up((size_t)BH, 64)};
  // the input projection of all steps of the chunk as one product over B * T columns (the engine stages its operands
  // through LDS, so W_ih rows of In = 513 / 1025 floats, off every 16-byte boundary, need no special case here)
  avvad_gemm_desc gd = gemm_desc(B * T, 4 * H, In, In, In, 4 * H, 0, 1, 0, 1);
  int rc;
  if ((rc = avvad_gemm_impl(x, w_ih, b_ih, w.G, &gd, s, w.slab))) return rc;
  const StateChoice c = state_form(B, H, w_hh, h0, hT);
  const StateKernel step = c.vec ? state_kernel<true>(c.NG) : state_kernel<false>(c.NG);
  const dim3 grid(cdiv(H, 4), cdiv(B, 16 * c.NG));
  if (grid.y > 65535) return AVVAD_EINVAL;
  // step t reads h from where step t - 1 wrote it and writes somewhere else: the last step into hT, the others into the
  // two workspace buffers in turn.  Only a one-step call with hT == h0 needs a copy behind it.
  const float* hp = h0;
  for (int t = 0; t < T; ++t) {
    float* hn = t == T - 1 ? hT : hb[t & 1];
    const bool staged = hn == hp;                        // T == 1 and in place
    if (staged) hn = hb[0];
    const float* ci = t == 0 ? c0 : cT;
    hipLaunchKernelGGL(step, grid, dim3(256), 0, s, w.G, w_hh, b_hh, hp, hn, ci, cT, y, d->lengths, B, T, H, t);
    if (staged) hipLaunchKernelGGL(st_copy, dim3(cdiv(BH, 256)), dim3(256), 0, s, hb[0], hT, BH);
    hp = hn;
  }
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

extern "C" size_t avvad_wavenet_stream_state_bytes(const avvad_wavenet_desc* d) {
  if (!stream_desc_ok(d)) return 0;
  return stream_state_floats(d) * sizeof(float);
}

extern "C" size_t avvad_wavenet_stream_workspace(const avvad_wavenet_desc* d) {
  if (!stream_desc_ok(d)) return 0;
  return 256;      // the kernel keeps a pass in LDS and needs no scratch; a constant so that callers size it like every other
}

extern "C" int avvad_wavenet_stream_fwd(const float* chunk, const avvad_wavenet_params* prm, float* state, const int* n_valid,
                                        const int* skip, int k, float* out, int out_frames, const avvad_wavenet_desc* d,
                                        void* wsv, size_t ws_bytes, avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!chunk || !prm || !state || !n_valid || !skip || !stream_desc_ok(d) || k < 1 || out_frames < 0 ||
      (out_frames > 0 && !out) || (long)d->qc * d->L >= (1L << 31) / d->B)
    return AVVAD_EINVAL;
  if (ws_misaligned(wsv)) return AVVAD_EINVAL;
  if (!wsv || ws_bytes < 256) return AVVAD_EWORKSPACE;
  hipStream_t s = (hipStream_t)sv;
  WsTab tab;
  tab.n = d->n_layers;
  for (int i = 0; i < d->n_layers; ++i) {
    if ((long)(d->fw - 1) * d->dilations_h[i] >= (1L << 30)) return AVVAD_EINVAL;
    tab.dil[i] = d->dilations_h[i];
    tab.dw[i] = prm->dil_w_h[i];
    tab.ew[i] = prm->dense_w_h[i];
    tab.db[i] = d->use_bias ? prm->dil_b_h[i] : nullptr;
    tab.eb[i] = d->use_bias ? prm->dense_b_h[i] : nullptr;
    if (!tab.dw[i] || !tab.ew[i]) return AVVAD_EINVAL;
  }
  tab.cw = prm->causal_w; tab.bw = prm->bott_w;
  tab.cb = d->use_bias ? prm->causal_b : nullptr;
  tab.bb = d->use_bias ? prm->bott_b : nullptr;
  if (!tab.cw || !tab.bw) return AVVAD_EINVAL;
  const bool mf = d->R == 32 && d->D == 32 && d->fw == 2;
  int NC = WS_NC_MFMA;
  if (!mf) {   // the longest pass that fits: a multiple of 32 where possible
    while (NC > 32 && stream_lds_bytes(d, false, NC) > WS_LDS_MAX) NC -= 32;
    while (NC > 1 && stream_lds_bytes(d, false, NC) > WS_LDS_MAX) NC -= 1;
  }
  const size_t lds = stream_lds_bytes(d, mf, NC);
  if (lds > WS_LDS_MAX) return AVVAD_EINVAL;
  if (int rc = mf ? allow_large_lds<wn_stream_kernel<true>>(lds, WS_LDS_MAX) : allow_large_lds<wn_stream_kernel<false>>(lds, WS_LDS_MAX))
    return rc;
  const long sf = (long)stream_state_floats(d);
  if (mf)
    hipLaunchKernelGGL(wn_stream_kernel<true>, dim3(d->B), dim3(WS_NT), lds, s, chunk, state, n_valid, skip, out, tab, d->L,
                       d->qc, d->R, d->D, d->Bn, d->fw, k, out_frames, sf, NC);
  else
    hipLaunchKernelGGL(wn_stream_kernel<false>, dim3(d->B), dim3(WS_NT), lds, s, chunk, state, n_valid, skip, out, tab, d->L,
                       d->qc, d->R, d->D, d->Bn, d->fw, k, out_frames, sf, NC);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}
