// lstm_cell.h -- what the LSTM kernels share: the cell arithmetic in both directions and the pieces of the skinny
// recurrent product W_hh h_{t-1} on v_mfma_f32_16x16x4_f32.  lstm.hip (training: lstm_gates_fwd, lstm_step_fwd_mfma,
// lstm_persistent_fwd, lstm_gates_bwd, EpiLstmBwd) and stream.hip (lstm_state_step) call these; what differs between the
// kernels -- how the pre-activation sum is associated, where h goes, the schedule of the loads -- stays with each kernel.
#pragma once
#include "common.h"

namespace lstm_cell {

// ------------------------------------------------------------------ forward
struct Fwd { float ig, fg, gg, og, c, h; };

// The live cell on four FINISHED pre-activations: pre(gate) is the caller's, which forms the sum (g + r, g + (r + b_hh) or
// g alone) -- the association is the kernel's own, and adding a zero is not neutral (tanhf(-0.f + 0.f) and tanhf(-0.f)
// differ in sign).  Each is asked for where its gate is activated, so a kernel's loads stay where it staged them.  That
// staging shows in the bits: hipcc contracts f * c_prev + i * g to ONE fma and rounds the other product, and which one
// follows the order in which the caller's operands become ready (lstm_gates_fwd rounds f * c_prev while it loads its four
// gates first; reading each gate where it is activated, behind an early c_prev, made it round i * g).  A kernel that
// changes its staging can change its last bit: compare with the previous build's bits.
template <class Pre>
__device__ __forceinline__ Fwd fwd(Pre pre, float cp) {
  Fwd r;
  r.ig = sigmoidf_(pre(0)); r.fg = sigmoidf_(pre(1)); r.gg = tanhf(pre(2)); r.og = sigmoidf_(pre(3));
  r.c = r.fg * cp + r.ig * r.gg;
  r.h = r.og * tanhf(r.c);
  return r;
}

// A gate row g = G[b][t] holds the four gates of unit j at g[gate * H + j].
__device__ __forceinline__ void load_gates(const float* g, int H, int j, float (&v)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = g[e * H + j];
}
__device__ __forceinline__ void store_gates(float* g, int H, int j, float ig, float fg, float gg, float og) {
  g[j] = ig; g[H + j] = fg; g[2 * H + j] = gg; g[3 * H + j] = og;
}
// what the training forward leaves of a live step for the backward, and the layer's output (o: index of (b, t, j))
__device__ __forceinline__ void store_live(float* g, float* Cs, float* y, int H, int j, long o, const Fwd& r) {
  store_gates(g, H, j, r.ig, r.fg, r.gg, r.og);
  Cs[o] = r.c;
  y[o] = r.h;
}
// a step at or past the sequence's length: zero gates (so its gate gradients vanish), zero state, zero output
__device__ __forceinline__ void store_dead(float* g, float* Cs, float* y, int H, int j, long o) {
  store_gates(g, H, j, 0.f, 0.f, 0.f, 0.f);
  Cs[o] = 0.f;
  y[o] = 0.f;
}

// ------------------------------------------------------------------ backward
// The cell at (b, j, t), idx = b * H + j, o = index of (b, t, j), given dhr = the recurrent dh arriving from step t + 1.
// in: activated gates in g, the cell states, dy, DC[idx] (dc from step t + 1)
// out: d(pre-activation gates) in g (in place), DC[idx] for step t - 1
__device__ __forceinline__ void bwd(float* g, const float* Cs, const float* dy, float* DC, int H, int j, int idx, long o,
                                    int t, bool live, float dhr) {
  if (!live) {
    store_gates(g, H, j, 0.f, 0.f, 0.f, 0.f);
    DC[idx] = 0.f;
    return;
  }
  const float ig = g[j], fg = g[H + j], gg = g[2 * H + j], og = g[3 * H + j];
  const float c = Cs[o], cp = t > 0 ? Cs[o - H] : 0.f;
  const float tc = tanhf(c);
  const float dh = dy[o] + dhr;
  const float dc = DC[idx] + dh * og * (1.f - tc * tc);
  store_gates(g, H, j, dc * gg * ig * (1.f - ig), dc * cp * fg * (1.f - fg), dc * ig * (1.f - gg * gg), dh * tc * og * (1.f - og));
  DC[idx] = dc * fg;
}

// ------------------------------------------------------------------ recurrent product
// D[16 gate rows][16 sequences] per v_mfma_f32_16x16x4_f32: lane (i = l & 15, q = l >> 4) feeds A = W_hh[row(i)][k] and
// B = h_{t-1}[sequence i][k].  Row order i = 4 * u + gate over a quad of units puts the four gate sums of unit q in the four
// accumulator registers of lane (sequence, q), so the cell runs in registers.
__device__ __forceinline__ int quad_unit(int i, int quad) { return 4 * quad + (i >> 2); }
// W_hh row of lane i whose unit is `unit` (quad_unit(), or that clamped): gate * H + unit < 4 H (an int: W_hh has 4 H * H floats)
__device__ __forceinline__ int whh_row(int i, int unit, int H) { return (i & 3) * H + unit; }

// Both operands are read as float4 along k and the 4 elements go to 4 MFMAs: k-slot q of MFMA e stands for
// k = 16 * kk + 4 * q + e on both operands, a permutation of the contraction order only.
__device__ __forceinline__ f32x4 mfma4(const float4& a, const float4& h, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, h.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, h.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, h.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, h.w, acc, 0, 0, 0);
  return acc;
}

// r (slice 0's partial sum) plus the partial sums of K-slices 1 .. n - 1 in slice order; p[s * stride] is slice s's
__device__ __forceinline__ f32x4 add_slices(f32x4 r, const f32x4* p, int n, int stride) {
  for (int s = 1; s < n; ++s) {
    const f32x4 v = p[s * stride];
    r[0] += v[0]; r[1] += v[1]; r[2] += v[2]; r[3] += v[3];
  }
  return r;
}

}  // namespace lstm_cell
