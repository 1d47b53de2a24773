/* avvad.h -- C ABI of libavvad_hip.so: the MI355X (gfx950) kernels behind the
 * per-frame classification hot path of sp-uhh/audio-visual-vad.
 *
 * The reference has no FFI / operator registry (it is pure Python on torch.nn,
 * SURVEY.md 8b); every entry point below replaces a stock torch / torchvision
 * call site of the reference, cited as file:line relative to the reference root.
 * The Python host (audio-visual-vad_amd/avvad) binds these with ctypes; a
 * maintainer of the reference would add the same ctypes stub.
 *
 * Conventions (all entry points):
 *   - plain C types only; every pointer is a DEVICE pointer unless the
 *     parameter name ends in _h (host);
 *   - the caller allocates every buffer, including the workspace
 *     (size from the matching *_workspace() query, bytes).  The contract
 *     (tests/test_abi_contract_gpu.py runs every entry-point family under it):
 *       * contents on entry are unspecified: what a workspace or an output
 *         buffer holds when the call starts never reaches a result.  Outputs
 *         are written in full -- padded steps, frames behind a row's length and
 *         gradients of masked rows are stored as zeros, not left alone.
 *         (In/out arguments are what their entry point says: C with
 *         accumulate, gradient pointers that are accumulated into (+=),
 *         running statistics, float64 statistics accumulators, stream state.)
 *       * nothing outside [ws, ws + ws_bytes) and outside the stated extent of
 *         an output is written;
 *       * a workspace below the queried size is refused (AVVAD_EWORKSPACE)
 *         before anything is launched: no buffer has changed (tested per
 *         entry point, forward and backward).  The one
 *         exception is the optional engine scratch of avvad_gemm_f32 /
 *         avvad_conv2d_*: ws == NULL or fewer than avvad_engine_workspace()
 *         bytes select the whole-tile schedule and the scratch is not touched;
 *       * a backward entry point takes the workspace its forward filled
 *         (save_for_backward), unmodified in between, at the same address or
 *         copied as a whole; it may overwrite it (one backward per forward);
 *       * alignment is per pointer class, checked before anything is launched
 *         where a wrong one would be an error (AVVAD_EINVAL):
 *           workspace                      16 bytes, every entry point (avvad_score_accumulate: 256)
 *           float64 statistics and score accumulators, score ratios, int64 confusion counts  8 bytes
 *           ratio / energies / clip_off of avvad_mix                                        8 bytes
 *           c_speech / c_noise and the spectra of avvad_target_noise_aware*                 8 bytes
 *           d and taps of avvad_stoi and avvad_stoi_loss, taps of avvad_resample*           8 bytes
 *           int64 / int32 index arrays      their natural alignment
 *           bf16 operands, avvad_lip_decode's coef, the avvad_stft_stream basis,
 *           (checked by avvad_stft_stream_fwd / _fwd_spec), the avvad_istft_stream
 *           basis (checked by avvad_istft_stream),
 *           activations, weights, outputs and gradients of the encoder, the
 *           trunk, the convolutions and the fusion: 16 bytes (the base address
 *           of any allocation; not checked unless the entry point says so)
 *           any 4-byte aligned float pointer (a contiguous slice such as
 *           wave + 3): A / B of avvad_gemm_f32, the four vectors of
 *           avvad_adam_step, wave / vad / ibm / out of avvad_target_*, wave of
 *           avvad_stft*, clean / bank / noisy / noise_out of avvad_mix,
 *           w_hh / h0 / hT of the LSTM entry points, and every
 *           argument of the element-wise helpers (loss, copy, transpose,
 *           standardise, peak).  These pick a vector form when the pointer
 *           (and the shape) allows it and a scalar form otherwise: same
 *           values up to the fp32 summation order;
 *   - asynchronous on the given hipStream_t, never synchronises, never
 *     allocates, keeps no per-call state -> re-entrant across streams and
 *     devices, capturable into a hipGraph.  The only process-wide state is the
 *     table of schedule options below (avvad_set_option): it is filled ONCE
 *     from the AVVAD_* environment variables on first use and never re-read;
 *   - returns AVVAD_OK or a negative AVVAD_E* code, never throws;
 *   - fp32 storage and fp32 arithmetic (fp32-input MFMA == ordered fmaf chain).
 */
#ifndef AVVAD_H
#define AVVAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* avvad_stream_t; /* hipStream_t */

#define AVVAD_OK 0
#define AVVAD_EINVAL (-1)     /* bad descriptor / unsupported shape */
#define AVVAD_EWORKSPACE (-2) /* workspace too small */
#define AVVAD_ELAUNCH (-3)    /* hipGetLastError() != hipSuccess after a launch */

/* library / build identification ("gfx950", ABI version).  AVVAD_ABI_VERSION is what THIS header describes; a binding
 * must refuse a library whose avvad_abi_version() differs (signatures changed incompatibly between versions:
 * 2 = (ws, ws_bytes) in front of the stream of avvad_gemm_f32 / avvad_conv2d_*, avvad_wavenet_desc.shared_device). */
#define AVVAD_ABI_VERSION 3   /* 3 = + avvad_conv2d_*_bf16.  Added entry points alone (the avvad_target_* labels) change no
                                 existing signature, so they keep the version: a version-3 binding still describes the
                                 library exactly for every symbol it binds.  The avvad_stats_* section is such an addition, and so
                                 are the avvad_score_* / avvad_confusion_* scores, and avvad_istft_bwd / avvad_resynth_bwd /
                                 avvad_si_sdr_loss, and avvad_mix_workspace / avvad_mix, and the
                                 avvad_target_noise_aware* masks, and avvad_spectral_loss_workspace /
                                 avvad_spectral_loss, and avvad_stoi_workspace / avvad_stoi, and
                                 avvad_stoi_loss_workspace / avvad_stoi_loss, and the avvad_resample* entries. */
const char* avvad_version(void);
int avvad_abi_version(void);

/* Schedule options (tuning / debugging; production leaves them alone).  Names:
 *   "no_streamk" (1 = whole-tile GEMM schedule), "igemm_variant", "kmajor", "no_tall", "no_stem_kernel",
 *   "no_fixup1" (1 = always the four-wave fix-up kernel), "no_buf" (1 = convolution gathers with flat addressing + validity selects, the form operands >= 2 GiB use),
 *   "lstm_no_fused_step", "lstm_no_persistent", "wn_no_fused_tail", "wn_no_fused_wgrad",
 *   "wn_flat" (encoder block forward: 0 by plane length -- the wide kernel from 8192 samples, else the high-occupancy
 *   kernel; 1 flat dword kernel, which also makes the input gradient flat; 2 buffer dword kernel with resident weights and
 *   cross-tile prefetch; 3 wide dwordx4 kernel; 4 high-occupancy kernel; 5 LDS-DMA kernel),
 *   "wn_dx" (encoder block input gradient: 0 and 2 high-occupancy kernel; 1 resident weights and cross-tile prefetch;
 *   3 flat kernel),
 *   "wn_bwd_t" (encoder block dz + weight gradients in one pass: 0 by the descriptor's shared_device hint -- 3 beside
 *   another stream's kernels, else 2; 1 transposed products; 2 high occupancy; 3 resident weights),
 *   "wn_grid" (workgroup cap of the encoder block forward kernels),
 *   "bf16" (BASELINE config 5's mixed precision, never the default.  1: the trunk runs its bf16 DATA PATH -- activations
 *   between convolutions, the gradients that feed convolutions and the packed weights are stored as bf16, the convolutions
 *   run on the bf16 engine -- and the dense GEMMs of the heads round their fp32 operands to bf16 on their way into LDS;
 *   2: round 2's form, fp32 storage everywhere and operands rounded while staging.  BatchNorm statistics, LSTM cell, loss,
 *   Adam and every accumulation stay fp32 in both),
 *   "max_cus" (cap on the CUs a persistent grid occupies, so that RCCL's kernels find free CUs during data-parallel
 *   training), "bwd_max_cus" (the same cap applied only while a backward entry point runs: the gradient all-reduce overlaps
 *   the backward pass, the forward keeps the whole chip), "no_cls" (1 = 3x3 convolutions multiply their zero padding like
 *   everything else instead of running position-major), "cls_cap", "no_fused_stats" (1 = BatchNorm statistics by separate
 *   column-reduction passes instead of the producing kernels' epilogues), "no_conv64" (1 = the 64 -> 64 channel 3x3
 *   convolutions on the GEMM engine instead of their weights-stationary / output-stationary kernels), "no_s2_cls" (1 = a
 *   stride-2 data gradient as four accumulating parity-class launches instead of one position-class product).
 * Initial values come from AVVAD_<NAME> in the environment, read once.  Returns AVVAD_EINVAL for an unknown name. */
int avvad_set_option(const char* name, int value);
int avvad_get_option(const char* name);

/* ------------------------------------------------------------------------
 * Dense GEMM on fp32 MFMA:  C[M,N] (+)= op(A) . op(B) (+ bias[N])
 *   transA=0: A is [M,K] row-major (lda);  transA=1: A is stored [K,M] (lda)
 *   transB=0: B is [K,N] row-major (ldb);  transB=1: B is stored [N,K] (ldb)
 *   accumulate: C += result.
 * Replaces: nn.LSTM input / recurrent projections and nn.Linear
 *   (packages/models/Audio_Net.py:30-35,51-59, Video_Net.py:45-51,102-116,
 *    AV_Net.py:53-58,128-140) and their autograd backward.
 * ---------------------------------------------------------------------- */
typedef struct {
  int M, N, K;
  int lda, ldb, ldc;
  int transA, transB;
  int accumulate;
  int split_k; /* >= 1: hint that K is long and the tiles few (needs accumulate) */
  int relu_a;  /* apply max(.,0) to A elements on load */
  int relu_b;
} avvad_gemm_desc;
/* Scratch of the GEMM engine, bytes (a constant: one tile per persistent worker, or -- the larger -- one [576][64] partial
 * weight gradient per CU for the 64-channel convolutions' own kernel).  Tiles whose K range is cut between
 * workers (the engine's stream-K round) leave their partial sums there and a fix-up kernel adds them in a fixed
 * order: results are bit-reproducible run to run, there are no float atomics.  Every entry point that runs a single
 * GEMM / convolution takes (ws, ws_bytes); ws == NULL (or too small) selects whole-tile scheduling -- same results up
 * to summation order, slower where the tile count quantises badly against the 256 CUs. */
size_t avvad_engine_workspace(void);
int avvad_gemm_f32(const float* A, const float* B, const float* bias, float* C,
                   const avvad_gemm_desc* d, void* ws, size_t ws_bytes, avvad_stream_t s);

/* ------------------------------------------------------------------------
 * WaveNet-style encoder (valid dilated Conv1d stack)
 * Replaces: wavenet_autoencoder._encode, packages/models/wavenet_autoencoder.py:74-93
 * Layout: activations [B][C][L] (torch NCL, time contiguous); weights exactly as
 * in the state_dict: Conv1d weight [Cout][Cin][fw], bias [Cout].
 * ---------------------------------------------------------------------- */
typedef struct {
  int B;   /* sequences                                                */
  int L;   /* input samples per sequence                               */
  int qc;  /* quantization_channel (input channels)                    */
  int R;   /* en_residual_channel                                      */
  int D;   /* en_dilation_channel                                      */
  int Bn;  /* en_bottleneck_width                                      */
  int fw;  /* filter_width                                             */
  int P;   /* en_pool_kernel_size (used as pool OUTPUT size, :91)      */
  int n_layers;
  const int* dilations_h; /* host array [n_layers]                     */
  int use_bias;
  int save_for_backward; /* forward keeps every s_i in the workspace (z_i is rebuilt by the backward) */
  int shared_device;     /* hint: another stream's kernels run beside this call (the AV model's trunk on the main stream):
                            prefer the kernel forms that interfere least with them.  0 = the device is ours        */
} avvad_wavenet_desc;

/* parameter pointers, host arrays of device pointers */
typedef struct {
  const float* causal_w;
  const float* causal_b;
  const float* const* dil_w_h; /* [n_layers] */
  const float* const* dil_b_h;
  const float* const* dense_w_h;
  const float* const* dense_b_h;
  const float* bott_w;
  const float* bott_b;
} avvad_wavenet_params;

typedef struct {
  float* causal_w;
  float* causal_b;
  float* const* dil_w_h;
  float* const* dil_b_h;
  float* const* dense_w_h;
  float* const* dense_b_h;
  float* bott_w;
  float* bott_b;
} avvad_wavenet_grads;

size_t avvad_wavenet_workspace(const avvad_wavenet_desc* d);
/* wave [B][qc][L] -> out [B][Bn][P] */
int avvad_wavenet_fwd(const float* wave, const avvad_wavenet_params* p, float* out,
                      const avvad_wavenet_desc* d, void* ws, size_t ws_bytes, avvad_stream_t s);
/* needs the workspace of a forward run with save_for_backward=1.
 * grads are ACCUMULATED (+=) into g; dwave may be NULL.  Every shape the forward accepts is supported, a pool with more
 * bins than samples (P > Lv, a sample in more than two bins) included. */
int avvad_wavenet_bwd(const float* wave, const avvad_wavenet_params* p, const float* dout,
                      const avvad_wavenet_grads* g, float* dwave, const avvad_wavenet_desc* d,
                      void* ws, size_t ws_bytes, avvad_stream_t s);

/* One residual block of the R = D = 32, filter_width 2 encoder on its own (wavenet_autoencoder.py:80-86):
 *   s_out[b][r][t] = b_dense[r] + sum_d W_dense[r][d] relu(b_dil[d] + sum_{c,k} W_dil[d][c][k] relu(s_in[b][c][t + k*dil]))
 *                    + s_in[b][r][t + dil]          s_in [B][32][Lin] -> s_out [B][32][Lin - dil]
 * The layer-at-a-time kernel of the large dilations; bench.py times it per launch for its HBM roofline entry.
 * Biases may be NULL. */
int avvad_wavenet_block_fwd(const float* s_in, const float* w_dil, const float* b_dil, const float* w_dense,
                            const float* b_dense, float* s_out, int B, int Lin, int dil, avvad_stream_t s);

/* ------------------------------------------------------------------------
 * ResNet-18 trunk over gray lip crops
 * Replaces: self.features(video).squeeze() with the 3x channel repeat in front,
 *   packages/models/Video_Net.py:60-81, packages/models/AV_Net.py:78-94
 *   (torchvision.models.resnet18 children [:-1]).
 * Layout: input frames [N][H][W] (1 channel; the reference's 3 identical
 * channels are folded into conv1's weights), activations NHWC inside, output
 * [N][512].  Parameters are passed in torchvision state_dict layout (OIHW).
 * ---------------------------------------------------------------------- */
#define AVVAD_TRUNK_NCONV 20 /* conv1 + 16 block convs + 3 downsample convs */

typedef struct {
  int N, H, W;
  int training;   /* batch statistics + running-stat update */
  float momentum; /* 0.1 */
  float eps;      /* 1e-5 */
  int save_for_backward;
} avvad_trunk_desc;

/* conv index order: 0 = conv1; then per stage s (0..3), per block b (0..1):
 * conv1, conv2, [downsample if s>0 and b==0].  The i-th BatchNorm follows the
 * i-th conv.  (torchvision order: features.0/1, features.{4..7}.{0,1}.{conv1,bn1,conv2,bn2,downsample}) */
typedef struct {
  const float* conv_w[AVVAD_TRUNK_NCONV]; /* OIHW */
  const float* bn_w[AVVAD_TRUNK_NCONV];
  const float* bn_b[AVVAD_TRUNK_NCONV];
  float* bn_rm[AVVAD_TRUNK_NCONV]; /* running_mean (updated when training) */
  float* bn_rv[AVVAD_TRUNK_NCONV]; /* running_var                          */
} avvad_trunk_params;

typedef struct {
  float* conv_w[AVVAD_TRUNK_NCONV]; /* OIHW, accumulated (+=) */
  float* bn_w[AVVAD_TRUNK_NCONV];
  float* bn_b[AVVAD_TRUNK_NCONV];
} avvad_trunk_grads;

/* Single convolution on the implicit-GEMM engine (the trunk's building block; also what bench.py times
 * per launch for the roofline).  x [N][H][W][C] NHWC, y [N][Ho][Wo][Co]; square kernel KS, stride 1|2.
 * Weights are packed once from OIHW: wf [(kh,kw,c)][co] (forward) and wd [(kh,kw,co)][c] (dgrad; may be
 * NULL).  C must be 1 (stem, forward/wgrad only) or a multiple of 32; Co a multiple of 4.
 * dgrad also needs Co % 32 == 0; forward and dgrad a kernel of at most 32 taps (C > 1); dgrad with stride 2 needs KS <= 4.
 * A shape outside these limits, or one in which no window fits (H + 2 pad < KS), is refused with AVVAD_EINVAL before
 * anything is launched: the output buffer keeps every bit.
 * wgrad writes the packed layout [(kh,kw,c)][co] (overwritten).  ws: avvad_engine_workspace() bytes.  Replaces nn.Conv2d inside
 * torchvision's resnet18 (packages/models/Video_Net.py:35-37). */
typedef struct {
  int N, H, W, C, Co, KS, stride, pad;
} avvad_conv_desc;
int avvad_conv2d_pack_weights(const float* w_oihw, float* wf, float* wd, const avvad_conv_desc* d,
                              avvad_stream_t s);
int avvad_conv2d_fwd(const float* x, const float* wf, float* y, const avvad_conv_desc* d, void* ws,
                     size_t ws_bytes, avvad_stream_t s);
int avvad_conv2d_dgrad(const float* dy, const float* wd, float* dx, const avvad_conv_desc* d,
                       int accumulate, void* ws, size_t ws_bytes, avvad_stream_t s);
int avvad_conv2d_wgrad(const float* x, const float* dy, float* dw_packed, const avvad_conv_desc* d, void* ws,
                       size_t ws_bytes, avvad_stream_t s);

/* The same convolutions on the bf16 data path (BASELINE configs[4]; what the trunk runs when option "bf16" is 1): operands
 * are bf16 IN MEMORY -- x16 / dy16 NHWC bf16, weights in the K-contiguous bf16 packs
 *   wf16[co][(cc * T + tap) * 64 + r] = w[co][cc * 64 + r][tap]     (forward; T = KS * KS taps, 64-channel chunks cc)
 *   wd16[c][(cc * T + tap) * 64 + r]  = w[cc * 64 + r][c][tap]      (data gradient; may be NULL in the pack call)
 * -- multiplied by v_mfma_f32_32x32x16_bf16 with fp32 accumulation; results (y, dx, the packed weight gradient
 * [(kh,kw,c)][co]) are fp32.  C and Co must be multiples of 64.  Same replaced call site as above. */
int avvad_conv2d_pack_weights_bf16(const float* w_oihw, void* wf16, void* wd16, const avvad_conv_desc* d, avvad_stream_t s);
int avvad_conv2d_fwd_bf16(const void* x16, const void* wf16, float* y, const avvad_conv_desc* d, void* ws, size_t ws_bytes,
                          avvad_stream_t s);
int avvad_conv2d_dgrad_bf16(const void* dy16, const void* wd16, float* dx, const avvad_conv_desc* d, int accumulate,
                            void* ws, size_t ws_bytes, avvad_stream_t s);
int avvad_conv2d_wgrad_bf16(const void* x16, const void* dy16, float* dw_packed, const avvad_conv_desc* d, void* ws,
                            size_t ws_bytes, avvad_stream_t s);

/* A trunk descriptor needs N > 0 and H, W >= 32.  For any other the size query answers 0 and the three calls below
 * AVVAD_EINVAL, before anything is computed or launched. */
size_t avvad_trunk_workspace(const avvad_trunk_desc* d);
/* Test support: offset (floats), channels and spatial size of the post-ReLU activation `index` that a forward run with
 * save_for_backward keeps in its workspace, NHWC.  index 0: pooled stem output; 1 + 2k: block k's first activation
 * (bn1 + ReLU); 2 + 2k: block k's output (k = 0..7).  The parity tests compare sign patterns with the oracle's.
 * index 17 (save_for_backward only): the max pool's arg-max plane, N*H*W*16 32-bit words at `offset_floats` (C = 64, H x W
 * the pooled grid).  Byte k of word q of a pooled position is the window position dh*3+dw (0..8, the window starts one
 * row and one column before 2*ph, 2*pw) that holds the maximum of channel 4q+k: the first one in row-major scan order. */
int avvad_trunk_activation(const avvad_trunk_desc* d, int index, size_t* offset_floats, int* C, int* H, int* W);
int avvad_trunk_fwd(const float* frames, const avvad_trunk_params* p, float* feat /* [N][512] */,
                    const avvad_trunk_desc* d, void* ws, size_t ws_bytes, avvad_stream_t s);
int avvad_trunk_bwd(const float* frames, const avvad_trunk_params* p, const float* dfeat,
                    const avvad_trunk_grads* g, const avvad_trunk_desc* d, void* ws, size_t ws_bytes,
                    avvad_stream_t s);

/* ------------------------------------------------------------------------
 * Packed-sequence multi-layer LSTM (unidirectional) -- batch_first padded input,
 * padded output steps are zero, (h,c) stop at each sequence's length.
 * Replaces: pack_padded_sequence -> nn.LSTM -> pad_packed_sequence(total_length)
 *   packages/models/Audio_Net.py:50-56, Video_Net.py:102-113, AV_Net.py:127-137
 * x [B][T][In], y [B][T][H]; weights in state_dict layout: w_ih [4H][In],
 * w_hh [4H][H], b_ih/b_hh [4H], gate order i,f,g,o.
 * ---------------------------------------------------------------------- */
typedef struct {
  int B, T, In, H;
  const int* lengths; /* device int32 [B] */
  int save_for_backward;
} avvad_lstm_desc;
size_t avvad_lstm_workspace(const avvad_lstm_desc* d);
int avvad_lstm_layer_fwd(const float* x, const float* w_ih, const float* w_hh, const float* b_ih,
                         const float* b_hh, float* y, const avvad_lstm_desc* d, void* ws,
                         size_t ws_bytes, avvad_stream_t s);
/* dx may be NULL; parameter grads are accumulated (+=). dy is [B][T][H]. */
int avvad_lstm_layer_bwd(const float* x, const float* w_ih, const float* w_hh, const float* y,
                         const float* dy, float* dx, float* dw_ih, float* dw_hh, float* db_ih,
                         float* db_hh, const avvad_lstm_desc* d, void* ws, size_t ws_bytes,
                         avvad_stream_t s);

/* ------------------------------------------------------------------------
 * Streaming (stateful, chunked) inference.  Inference only: nothing is kept for a backward pass, and a descriptor with
 * save_for_backward set is refused (AVVAD_EINVAL).  Deterministic: no float atomics, fixed summation orders.  No kernel
 * of this section waits on another workgroup; a time step is a launch.
 * Replaces: nothing the reference has -- it scores whole utterances (scripts/evaluate_*_net.py).  Fed an utterance in
 * chunks, these entry points compute what the whole-utterance forward computes (same call sites as the sections above),
 * because the encoder is left-context-only, the LSTMs are unidirectional and everything else is per frame.
 * ---------------------------------------------------------------------- */
/* One LSTM layer over the next T steps of B independent rows, with the state in and out.  x [B][T][In], y [B][T][H],
 * h0 / c0 / hT / cT [B][H].  h0 / c0 may be NULL (zeros); hT / cT may be the same buffers as h0 / c0.  Row b advances
 * lengths[b] steps (0 <= lengths[b] <= T): later output steps are zero, its state stops there, and length 0 passes the
 * state through bit for bit.  Any B, T, In, H >= 1; ws must be 16-byte aligned.  A row's results do not depend on the
 * other rows' values.
 * Form: the input projection of all steps is one product on the GEMM engine; then one launch per step in which
 * workgroups own four hidden units each, stream their 16 rows of W_hh once and contract them against up to 64 rows per
 * workgroup in MFMA column blocks of 16 (few rows: a weight-streaming product, not a tile GEMM). */
size_t avvad_lstm_state_workspace(const avvad_lstm_desc* d);
int avvad_lstm_layer_fwd_state(const float* x, const float* w_ih, const float* w_hh, const float* b_ih,
                               const float* b_hh, const float* h0, const float* c0, float* y, float* hT, float* cT,
                               const avvad_lstm_desc* d, void* ws, size_t ws_bytes, avvad_stream_t s);

/* The encoder on a stream of samples.  d describes the network as for avvad_wavenet_fwd (every configuration that accepts
 * is accepted here; R = D = 32 with filter_width 2 runs on MFMA, the others in a plain direct form); d->L is the column
 * pitch of the chunk, d->P is ignored (a whole-utterance output count has no meaning here), save_for_backward must be 0.
 * state: B opaque blocks of avvad_wavenet_stream_state_bytes(d) each -- per row the number of columns consumed, the
 * causal layer's last (fw-1) input columns and each residual layer's last (fw-1) d_i input columns.  ALL ZEROS means
 * "start of utterance"; there is no other special case: the first RF-1 output columns are computed from the zero
 * history and dropped by the caller's skip count.
 * chunk [B][qc][L]; n_valid / skip: device int32 [B].  Row b consumes its first n_valid[b] columns (0 leaves its state
 * untouched).  Its output columns c < skip[b] are dropped (remaining warm-up); the others are averaged in runs of k:
 *   out[b][f][:] = mean over the k columns of frame f of relu(bottleneck(s_N)),  f < (n_valid[b] - skip[b]) / k,
 * frame-major [B][out_frames][Bn] -- the layout the fusion and the LSTM read; frames a row does not fill are written
 * as 0.  The caller keeps n_valid[b] <= skip[b] or (n_valid[b] - skip[b]) % k == 0, so no frame straddles two calls.
 * One workgroup per row walks the whole stack in one launch, up to 256 columns per pass held in LDS (more than 64 KB of
 * it: the entry point clears the kernel for that once per device). */
size_t avvad_wavenet_stream_state_bytes(const avvad_wavenet_desc* d);
size_t avvad_wavenet_stream_workspace(const avvad_wavenet_desc* d);
int avvad_wavenet_stream_fwd(const float* chunk, const avvad_wavenet_params* p, float* state, const int* n_valid,
                             const int* skip, int k, float* out, int out_frames, const avvad_wavenet_desc* d, void* ws,
                             size_t ws_bytes, avvad_stream_t s);

/* ------------------------------------------------------------------------
 * Multimodal compact bilinear fusion + signed sqrt + whole-tensor L2 normalisation + BatchNorm1d
 * Replaces: the use_mcb branch of DeepVAD_AV.forward, packages/models/AV_Net.py:109-121, i.e.
 *   CompactBilinearPooling (packages/models/compact_bilinear_pooling.py:7-27,140-220: count sketches
 *   psi(x,h,s)[h_i] += s_i x_i, circular convolution of the two sketches) -> sign(y)sqrt(|y|+eps) ->
 *   y / ||y||_2 (detached norm of the whole tensor) -> BatchNorm1d(D, eps) over all rows.
 * audio [rows][A], video [rows][V], out [rows][D]; rows = B*T; h1/h2 int64 bucket per input channel
 * (values in [0, D)), s1/s2 = +-1.  D % 4 == 0, D <= 1024.  bwd accumulates (+=) dbn_w / dbn_b and
 * overwrites daudio / dvideo (either may be NULL).
 * ---------------------------------------------------------------------- */
typedef struct {
  int rows, A, V, D;
  float eps;      /* used for the signed sqrt AND as the BatchNorm eps (AV_Net.py:49,114) */
  int training;
  float momentum;
  int save_for_backward;
} avvad_mcb_desc;
size_t avvad_mcb_workspace(const avvad_mcb_desc* d);
int avvad_mcb_fusion_fwd(const float* audio, const float* video, const int64_t* h1, const float* s1,
                         const int64_t* h2, const float* s2, const float* bn_w, const float* bn_b,
                         float* bn_rm, float* bn_rv, float* out, const avvad_mcb_desc* d, void* ws,
                         size_t ws_bytes, avvad_stream_t s);
int avvad_mcb_fusion_bwd(const float* audio, const float* video, const int64_t* h1, const float* s1,
                         const int64_t* h2, const float* s2, const float* bn_w, const float* dout,
                         float* daudio, float* dvideo, float* dbn_w, float* dbn_b,
                         const avvad_mcb_desc* d, void* ws, size_t ws_bytes, avvad_stream_t s);

/* The bare modules of packages/models/compact_bilinear_pooling.py, for callers that use them outside DeepVAD_AV:
 *   CountSketch.forward (:59-114 -> CountSketchFn_forward :7-27):  out[row][h[i]] += s[i] * x[row][i]
 *   CountSketchFn_backward (:30-38):                               dx[row][i] = s[i] * dout[row][h[i]]
 *   CompactBilinearPooling.forward (:222-263 -> CompactBilinearPoolingFn.forward :140-173): the raw vector
 *     y = irfft(rfft(psi(a,h1,s1)) * rfft(psi(v,h2,s2))) = circular convolution of the two sketches, [rows][D]
 *   CompactBilinearPoolingFn.backward (:175-220): da, dv (either may be NULL; overwritten).
 * D <= 2048. */
int avvad_count_sketch_fwd(const float* x, const int64_t* h, const float* s, float* out, int rows, int In, int D,
                           avvad_stream_t st);
int avvad_count_sketch_bwd(const float* dout, const int64_t* h, const float* s, float* dx, int rows, int In, int D,
                           avvad_stream_t st);
int avvad_mcb_fwd(const float* a, const float* v, const int64_t* h1, const float* s1, const int64_t* h2,
                  const float* s2, float* y, int rows, int A, int V, int D, avvad_stream_t st);
int avvad_mcb_bwd(const float* a, const float* v, const int64_t* h1, const float* s1, const int64_t* h2,
                  const float* s2, const float* dy, float* da, float* dv, int rows, int A, int V, int D,
                  avvad_stream_t st);

/* ------------------------------------------------------------------------
 * STFT log-power front-end: framing + periodic Hann + real DFT (one MFMA GEMM) + |X|^2 (+ log)
 * Replaces: stft_pytorch packages/processing/stft.py:102-151 (center=False; the optional one-hop zero pad at
 *   the end is implied by T: frames may run at most one hop past L and read zeros there) and the callers'
 *   power / log, scripts/evaluate_audio_net.py:141-148, packages/data_handling.py:454-457.
 * wave [B][L].  mode 0: out [B][T][F] = log(|X|^2 + eps); mode 1: out = |X|^2; mode 2 (B == 1): out [F][T][2] =
 * (re, im), the legacy torch.stft real view the reference's callers index.  F = n_fft/2 + 1, n_fft % 32 == 0.
 * ---------------------------------------------------------------------- */
typedef struct {
  int B;
  long L;
  int n_fft, hop, T;
  float eps;
} avvad_stft_desc;
size_t avvad_stft_workspace(const avvad_stft_desc* d);
int avvad_stft(const float* wave, float* out, const avvad_stft_desc* d, int mode, void* ws, size_t ws_bytes,
               avvad_stream_t s);

/* The evaluate scripts' feature chain in one call (scripts/evaluate_audio_net.py:131-163): STFT -> |X|^2 ->
 * log(. + d->eps) -> (x - mean[f]) / (std[f] + norm_eps), the standardisation folded into the DFT's epilogue pass.
 * mean / std: [F] train-set statistics.  out [B][T][F]. */
int avvad_stft_features(const float* wave, const float* mean, const float* std_, float* out,
                        const avvad_stft_desc* d, float norm_eps, void* ws, size_t ws_bytes, avvad_stream_t s);
/* The same front-end on a STREAM of samples (inference; nothing the reference has: it transforms whole utterances).
 * Row b's logical stream is its pending tail -- the n_pending[b] < n_fft samples that earlier calls left without a
 * complete frame, or that later frames still overlap -- followed by chunk[b][0 .. n_valid[b]).  The call emits the row's
 * next n_frames[b] frames, frame t from samples [t hop, t hop + n_fft) of that stream, each sample divided by peak[b]
 * (a division: a peak of 1 changes no bit; peak == NULL is 1 everywhere):
 *   out[b][t][f] = log(re^2 + im^2 + eps),  then with mean / std (both or neither)  (v - mean[f]) / (std[f] + norm_eps),
 * and the rest of out [B][T][F] is zero.  Samples past the end of a stream read as zero -- the reference's one-hop end
 * padding -- and only a row with pad_frames[b] != 0 (it ends here) may emit the one frame that does so.  The stream from
 * sample n_frames[b] hop on is the new tail: state_out[b] (raw samples, zero behind them).  A row with no new sample and
 * no frame keeps its state bit for bit.
 * state_in / state_out: plain float [B][n_fft], different buffers (every workgroup reads tails while others are written:
 * the caller swaps, as for h / c); all zeros with n_pending 0 is "start of utterance".  chunk [B][L] is never written.
 * n_valid / n_pending / n_frames / pad_frames: device int32 [B]; the counts are the caller's bookkeeping (frames after N
 * samples: max(0, (N - n_fft) / hop + 1)); the kernel clamps them so that wrong ones cannot leave a buffer: n_valid to
 * [0, d->L], n_pending to [0, n_fft], n_frames to [0, min(d->T, the complete frames of the n_pending + n_valid samples,
 * plus one where pad_frames[b] != 0)].  d->M is the
 * HOST's sum of n_frames (0: unknown, B T is assumed); it sizes the grid and selects nothing that changes a value.
 * basis: avvad_stft_stream_basis_bytes(n_fft) bytes filled ONCE by avvad_stft_stream_basis (16-byte aligned) -- the
 * windowed basis of avvad_stft (periodic Hann, exact phase reduction, evaluated in double) packed per block of 16 bins,
 * real and imaginary columns apart.  n_fft % 32 == 0, 1 <= hop <= n_fft, n_fft <= 2048 (a pass of frames sits in LDS).
 * No workspace.
 * DETERMINISM: the order in which one output value is summed depends on (n_fft, bin) alone -- not on the number of
 * frames, the row, the frame's place in the call or n_pending.  One kernel serves every size: workgroups own 16 bins,
 * 8 waves split K round-robin in groups of 16 samples on v_mfma_f32_16x16x4_f32 and their partial sums are added in wave
 * order.  Any split of a stream into calls therefore gives the same bits. */
typedef struct {
  int B;         /* rows */
  int L;         /* pitch of chunk (floats), >= 1 */
  int n_fft, hop;
  int T;         /* frame pitch of out (>= every n_frames[b]); 0: no row emits a frame, out may be NULL */
  int M;         /* host's sum of n_frames, or 0 */
  float eps, norm_eps;
} avvad_stft_stream_desc;
/* out[b] = max|x[b][:]|, x [B][L]: the peak avvad_peak_normalize divides by, as a value -- what a caller hands to
 * avvad_stft_stream_fwd when it knows the whole utterance (the evaluators) */
int avvad_abs_max(const float* x, float* out, int B, long L, avvad_stream_t s);
size_t avvad_stft_stream_basis_bytes(int n_fft);
int avvad_stft_stream_basis(int n_fft, float* out, avvad_stream_t s);
int avvad_stft_stream_fwd(const float* chunk, const int* n_valid, const int* n_pending, const int* n_frames,
                          const int* pad_frames, const float* peak, const float* state_in, float* state_out,
                          const float* basis, const float* mean, const float* std_, float* out,
                          const avvad_stft_stream_desc* d, avvad_stream_t s);
/* The same call, which also hands out the complex spectrum it holds anyway: spec [B][T][F][2], (re, im) adjacent, of the
 * samples divided by peak[b]; frames a row does not fill are zero, like out.  Written in the epilogue that writes out, in the
 * forward's summation order, so it is bit-identical for every split of a stream; out has the bits of avvad_stft_stream_fwd.
 * spec: plain float, 8-byte aligned (AVVAD_EINVAL otherwise), may be NULL when d->T == 0.  What avvad_istft_stream takes. */
int avvad_stft_stream_fwd_spec(const float* chunk, const int* n_valid, const int* n_pending, const int* n_frames,
                               const int* pad_frames, const float* peak, const float* state_in, float* state_out,
                               const float* basis, const float* mean, const float* std_, float* out, float* spec,
                               const avvad_stft_stream_desc* d, avvad_stream_t s);
/* ------------------------------------------------------------------------
 * Masked inverse STFT: mask x spectrum -> waveform
 * Replaces: istft packages/processing/stft.py:63-99 (librosa.core.istft: per-frame irfft, periodic Hann, overlap-add,
 *   division by the window sum of squares where it exceeds float32 tiny, centre trim, length fix), and the
 *   "mask x noisy spectrum" product in front of it, which is never written to memory.
 * The inverse DFT and the synthesis window are ONE fp32-MFMA GEMM, Y[(b,t)][n] = sum_c A[(b,t)][c] Winv[c][n]
 * (c = 2f + {re,im}; the forward transform's flop count), then a gather per output sample in ascending frame order:
 *   out[b][s] = scale[b] * (sum_t Y[b,t][s + start - t hop]) / wss(s + start),   wss(s') = sum_t hann^2[s' - t hop]
 * over the frames t < n_frames[b] that cover s' (the division only where wss > 1.17549435e-38).  No float atomics:
 * results are bit-identical run to run.  Samples at or beyond out_len[b], beyond the row's natural length
 * n_fft + hop (n_frames[b] - 1) - start, and rows without frames are written as exact zeros.
 * spec: interleaved (re, im) pairs, bin (b, t, f) at spec[b * stride_b + t * stride_t + f * stride_f] (float strides): a
 * batched [B][T][F][2] tensor (T F 2, F 2, 2), the legacy [F][T][2] view of ONE utterance (0, 2, 2 T) and the forward
 * transform's workspace rows go in as they are.  F = n_fft/2 + 1, n_fft % 32 == 0, n_fft >= 32, 1 <= hop <= n_fft (hop
 * need not divide n_fft).  The last element of spec and of mask lies below 2^31 floats (32-bit offsets in the operand
 * load; AVVAD_EINVAL otherwise).
 * mask_mode 0: none (mask may be NULL); 1: multiply by mask [B][T][F]; 2: by sigmoid(mask) (a soft mask from logits);
 * 3: by (mask > 0 ? 1 : 0) (the evaluators' sigmoid > 0.5).
 * n_frames / out_len: device int32 [B], NULL = T frames / out_pitch samples for every row (values are clamped to those).
 * scale: device float [B] or NULL (undoes the evaluators' peak normalisation).  out [B][out_pitch].  start = n_fft/2
 * for librosa's center=True, else 0.  ws: 16-byte aligned.
 * ---------------------------------------------------------------------- */
typedef struct {
  int B, T;        /* rows, frame pitch of spec / mask                       */
  int n_fft, hop;
  int start;       /* samples trimmed at the front (0 <= start < n_fft)      */
  int out_pitch;   /* floats per row of out                                  */
  int mask_mode;   /* 0 .. 3                                                 */
} avvad_istft_desc;
size_t avvad_istft_workspace(const avvad_istft_desc* d);   /* 0 on a bad descriptor */
int avvad_istft(const float* spec, long stride_b, long stride_t, long stride_f, const float* mask, const int* n_frames,
                const int* out_len, const float* scale, float* out, const avvad_istft_desc* d, void* ws, size_t ws_bytes,
                avvad_stream_t s);
/* wave [B][L] -> out [B][out_pitch] in one call: the forward DFT of avvad_stft (sd), the masked inverse and the
 * overlap-add; the spectrum stays in the workspace.  sd and d must agree in B, T, n_fft and hop. */
size_t avvad_resynth_workspace(const avvad_stft_desc* sd, const avvad_istft_desc* d);
int avvad_resynth(const float* wave, const float* mask, const int* n_frames, const int* out_len, const float* scale,
                  float* out, const avvad_stft_desc* sd, const avvad_istft_desc* d, void* ws, size_t ws_bytes,
                  avvad_stream_t s);
/* The adjoint of the masked inverse with respect to the mask (mode 1) or its logits (mode 2), for training on a loss
 * of the waveform.  With a cotangent dout [B][out_pitch] of avvad_istft's out:
 *   q[b][s']      = scale[b] dout[b][s' - start] / wss(s')   where the forward wrote a sum (0 <= s' - start below
 *                   out_len[b] and the row's natural length; the division as in the forward), exactly 0 elsewhere;
 *   G             = the framed DFT of q taken as a [B][(T - 1) hop + n_fft] waveform -- the inverse basis is w_f / N times
 *                   the forward one, so the adjoint of the inverse GEMM IS the forward transform's GEMM (same M, N, K);
 *   dmask[b,t,f]  = (w_f / N) (G_re S_re + G_im S_im), in mode 2 times sigmoid'(mask[b,t,f]);  w_f = 1 for DC and
 *                   Nyquist, else 2.  Frames t >= n_frames[b] are written as exact zeros.
 * dmask [B][T][F] is overwritten.  Nothing of dout at or behind a row's length, and neither spectrum nor mask of a frame
 * t >= n_frames[b], is read: they may hold anything.  There is no gradient for spec (it is data) and no second derivative.
 * mask_mode 0 and 3 have no gradient: AVVAD_EINVAL, as is B ((T - 1) hop + n_fft) >= 2^31.  Every other argument and
 * limit as for avvad_istft; no float atomics, bit-identical run to run.  ws: 16-byte aligned; q, G and the basis live
 * only there. */
size_t avvad_istft_bwd_workspace(const avvad_istft_desc* d);   /* 0 on a bad descriptor or mask_mode 0 / 3 */
int avvad_istft_bwd(const float* spec, long stride_b, long stride_t, long stride_f, const float* mask, const int* n_frames,
                    const int* out_len, const float* scale, const float* dout, float* dmask, const avvad_istft_desc* d,
                    void* ws, size_t ws_bytes, avvad_stream_t s);
/* The same from the waveform: avvad_resynth keeps no spectrum, so this call transforms wave again into the workspace and
 * proceeds as avvad_istft_bwd on those rows (bit for bit what avvad_stft_complex + avvad_istft_bwd give): two
 * forward-size GEMMs. */
size_t avvad_resynth_bwd_workspace(const avvad_stft_desc* sd, const avvad_istft_desc* d);
int avvad_resynth_bwd(const float* wave, const float* mask, const int* n_frames, const int* out_len, const float* scale,
                      const float* dout, float* dmask, const avvad_stft_desc* sd, const avvad_istft_desc* d, void* ws,
                      size_t ws_bytes, avvad_stream_t s);
/* The masked inverse on a STREAM of frames (inference; center = False, no start trim, like the streaming forward).  Row b
 * has n_before[b] frames behind it; the call takes its next n_frames[b] frames, spec / mask [B][T][F]([2]) as
 * avvad_stft_stream_fwd_spec and the model hand them out (mask_mode as for avvad_istft; modes 2 and 3 take logits), and
 * writes n_out[b] samples: out[b][p], p < n_out[b], is the absolute sample s' = n_before[b] hop + p,
 *   out[b][p] = scale[b] * (state_in[b][p] + sum_i Y[b,i][p - i hop]) / wss(s'),   i ascending over the call's frames,
 * wss(s') the double sum of hann^2 over the absolute frames t < n_before[b] + n_frames[b] that cover s', ascending (the
 * division only where (float)wss > 1.17549435e-38); a sample no frame covers is +0, and out [B][L] is zero from n_out[b] on.
 * state_out[b][q] is the partial sum of the absolute sample (n_before[b] + n_frames[b]) hop + q (zero for q >= n_fft - hop).
 * A row that goes on emits n_out[b] = n_frames[b] hop samples -- those no later frame can cover: a sample leaves up to
 * n_fft - 1 samples after it came in.  A row with n_out[b] != n_frames[b] hop ENDS with this call (the final flush: a
 * stream of N samples has written n_before[b] hop so far and takes n_out[b] = N - that, cropped or zero-filled like
 * avvad_resynth's rows); its new state is all zero.  A row with n_frames[b] == 0 and n_out[b] == 0 keeps its state bit for
 * bit.  The sum of a sample is the ascending chain of avvad_istft's overlap-add cut at the call boundaries, and Y is summed
 * in an order that depends on (n_fft, n) alone, so ANY split of a stream into calls gives the same bits.
 * n_frames / n_before / n_out: device int32 [B], clamped in the kernel (to T, to >= 0, to L) so that wrong counts cannot
 * leave a buffer.  state_in / state_out: plain float [B][n_fft], different buffers; all zeros is "start of utterance".
 * basis: avvad_istft_stream_basis_bytes(n_fft) bytes filled ONCE by avvad_istft_stream_basis (16-byte aligned): the basis
 * of avvad_istft with the contraction packed to K = n_fft rows (re[0], re[n_fft/2], then re[f], im[f]), per block of 16
 * samples, and hann^2 in double behind it.  n_fft % 32 == 0, 32 <= n_fft <= 2048, 1 <= hop <= n_fft.  T == 0 (no row has
 * a frame; spec and mask may be NULL) with L > 0 is the final flush of rows that complete no frame; L == 0: out may be
 * NULL.  d->M: the host's sum of n_frames (0: unknown); it sizes the grid and selects nothing that changes a value.
 * ws: avvad_istft_stream_workspace(d) bytes, 16-byte aligned (the per-frame inverses Y). */
typedef struct {
  int B, T;        /* rows, frame pitch of spec / mask                       */
  int n_fft, hop;
  int L;           /* floats per row of out (>= every n_out[b])              */
  int M;           /* host's sum of n_frames, or 0                           */
  int mask_mode;   /* 0 .. 3                                                 */
} avvad_istft_stream_desc;
size_t avvad_istft_stream_basis_bytes(int n_fft);          /* 0 on an unsupported n_fft */
int avvad_istft_stream_basis(int n_fft, float* out, avvad_stream_t s);
size_t avvad_istft_stream_workspace(const avvad_istft_stream_desc* d);   /* 0 on a bad descriptor */
int avvad_istft_stream(const float* spec, const float* mask, const int* n_frames, const int* n_before, const int* n_out,
                       const float* scale, const float* state_in, float* state_out, const float* basis, float* out,
                       const avvad_istft_stream_desc* d, void* ws, size_t ws_bytes, avvad_stream_t s);
/* The batched complex spectrum of avvad_stft's DFT: out [B][T][F][2] = (re, im).  ws: avvad_stft_workspace(d). */
int avvad_stft_complex(const float* wave, float* out, const avvad_stft_desc* d, void* ws, size_t ws_bytes,
                       avvad_stream_t s);

/* out[b][:] = x[b][:] / max|x[b][:]|   (peak normalisation, scripts/evaluate_audio_net.py:125-127); out may alias x */
int avvad_peak_normalize(const float* x, float* out, int B, long L, avvad_stream_t s);
/* out[r][f] = (x[r][f] - mean[f]) / (std[f] + eps)  -- input standardisation of the train / evaluate loops
 * (scripts/train_AV_net.py:286-291, evaluate_audio_net.py:158-163).  nstat == F: per-bin statistics (audio,
 * 513 x 1 in the reference); nstat == 1: one scalar pair (video, 1 x 1).  out may alias x. */
int avvad_standardize(const float* x, const float* mean, const float* std_, float* out, size_t rows, int F,
                      int nstat, float eps, avvad_stream_t s);

/* ------------------------------------------------------------------------
 * Train-set standardisation statistics: the producers of the mean / std that avvad_standardize and
 * avvad_stft_features apply
 * Replaces: scripts/create_audio_train_files.py:196-214, 273-280, 340-392 (per file n_samples, channels_sum,
 *   channels_squared_sum of the log-power spectrogram, then mean = sum / n, std = sqrt((sumsq - n mean^2) / (n - 1)),
 *   513 x 1 each) and the same triples over all pixels in scripts/create_video_train_files_upsampled.py (1 x 1), which
 *   the reference computes offline and stores in HDF5.
 * An accumulator is caller-owned device memory of 2 * nstat + 1 doubles: sum[nstat], sumsq[nstat], count.  nstat is the
 * feature width F (per-column statistics: audio) or 1 (one scalar pair over all values: video), as for
 * avvad_standardize.  The caller zeroes it; every call ADDS to it, so a training set is a sequence of batches into one
 * accumulator, and accumulators of several ranks add element-wise.
 * Deliberate difference from the reference: it keeps sum and sumsq in float32 (`0. + float32 array` stays float32; numpy's
 * pairwise sum per file, left to right across files), which degrades with the size of the set.  Here every step behind
 * the float32 feature value is double.
 * Reductions use no floating-point atomics: rows are cut into chunks whose size depends on the shape only, per-chunk
 * double partials go to the workspace and are added in a fixed order that depends on the chunk count only (sixteen
 * contiguous segments of chunks, ascending inside, then the segments ascending), so results are bit-identical run to
 * run and independent of the "max_cus" option.
 * ---------------------------------------------------------------------- */
/* Bytes of workspace of avvad_stats_accumulate for rows = B * T rows; 0 on rows == 0, rows >= 2^31 or nstat <= 0. */
size_t avvad_stats_workspace(size_t rows, int nstat);
/* x [B][T][F] materialised features (spectrogram batches of a loader; video frames with F = H*W, nstat = 1);
 * lengths: device int32 [B], rows t >= lengths[b] are not counted (NULL: every row counts).  nstat must be F or 1. */
int avvad_stats_accumulate(const float* x, const int* lengths, double* acc, int B, int T, int F, int nstat, void* ws,
                           size_t ws_bytes, avvad_stream_t s);
/* Fused from the waveform: wave [B][L] ragged (rows zero-padded), n_frames device int32 [B] valid frames per row, d as
 * for avvad_stft.  Runs the STFT's DFT GEMM, then ONE pass over the spectrum that forms log(re^2 + im^2 + d->eps) (the
 * expression of avvad_stft mode 0, bit for bit), widens to double and accumulates x and x^2 per bin over the frames
 * t < n_frames[b]; the [B][T][F] feature tensor is never written.  nstat = F = n_fft/2 + 1.  The workspace holds the
 * STFT's (the spectrum is live while the partials are written) followed by the partials: avvad_stft_stats_workspace,
 * 0 on a bad descriptor.  avvad_stft_workspace is unchanged. */
size_t avvad_stft_stats_workspace(const avvad_stft_desc* d);
int avvad_stft_stats(const float* wave, const int* n_frames, double* acc, const avvad_stft_desc* d, void* ws,
                     size_t ws_bytes, avvad_stream_t s);
/* mean[i] = sum[i] / n, std[i] = sqrt(max((sumsq[i] - n mean[i]^2) / (n - 1), 0)) (the reference's "empirical std"),
 * computed in double and written as float [nstat].  The clamp keeps constant data (where the difference can round to a
 * tiny negative number) from producing a NaN; n < 2 gives NaN as numpy would. */
int avvad_stats_finalize(const double* acc, int nstat, float* mean, float* std_, avvad_stream_t s);

/* ------------------------------------------------------------------------
 * Scores: SI-SDR / SI-SIR / SI-SAR of the enhanced speech, confusion counts of the classifier
 * Replaces: packages/metrics.py:12-60 (si_sdr_components, energy_ratios: numpy on the host, three planes per utterance)
 *   and the four sums of f1_loss, packages/models/utils.py:191-194.
 * With the estimate e, the clean reference r and the noise n, every norm the reference takes is a quadratic form of six
 * inner products G = (e.e, e.r, e.n, r.r, n.n, r.n); a_s = e.r / r.r, a_n = e.n / n.n:
 *   |s_target|^2 = a_s e.r    |e_noise + e_art|^2 = e.e - a_s e.r    |e_noise|^2 = a_n e.n
 *   |e_art|^2 = e.e - a_s e.r - a_n e.n + 2 a_s a_n r.n
 *   si_sdr, si_sir, si_sar = 10 log10(|s_target|^2 / |e_noise + e_art|^2, / |e_noise|^2, / |e_art|^2)
 * One pass reads the three signals (12 bytes per sample), widens every value to double before it is multiplied and sums
 * G; the planes n, s_target, e_noise, e_art are never written.  An accumulator is caller-owned device memory of [B][6]
 * doubles in the order of G.  The caller zeroes it; every call ADDS to it, so an utterance may arrive in packets.
 * Rows are cut into chunks of AVVAD_SCORE_CHUNK samples (a function of the row length alone), per-chunk double partials
 * go to the workspace in a fixed cross-lane and cross-wave order and are added to the accumulator in ascending chunk
 * order: no floating-point atomics, bit-identical run to run and independent of the "max_cus" option.
 * ---------------------------------------------------------------------- */
#define AVVAD_SCORE_CHUNK 4096
/* Bytes of workspace of avvad_score_accumulate; 0 on a bad shape (B outside 1..65535, L < 1). */
size_t avvad_score_workspace(int B, long L);                       /* 0 on a bad shape */
/* est / ref / third: B rows of L samples, each with its own row pitch in floats (ld_* >= L), so a column slice of a wider
 * tensor is read in place; any 4-byte aligned float pointer.  third_mode 0: third must be NULL, only SI-SDR is defined;
 * 1: third is the noise n; 2: third is the noisy mixture x and n = (double)x - (double)r is formed in the kernel.
 * lengths: device int32 [B], clamped to [0, L]; nothing at or behind a row's length is read (NULL: L each).
 * ws: 256-byte aligned, acc: 8-byte aligned. */
int avvad_score_accumulate(const float* est, long ld_est, const float* ref, long ld_ref,
                           const float* third, long ld_third, int third_mode /* 0 none, 1 noise, 2 mixture */,
                           const int* lengths /* NULL: L each */, double* acc /* [B][6], added to */,
                           int B, long L, void* ws, size_t ws_bytes, avvad_stream_t s);
/* ratios[b] = (si_sdr, si_sir, si_sar) in dB, alpha[b] = (a_s, a_n), with the reference's IEEE behaviour: an empty row
 * gives NaN, a zero denominator inf, and a denominator that cancellation drove slightly negative counts as 0.
 * third_mode 0: si_sir, si_sar and a_n are NaN.  ratios / alpha: 8-byte aligned. */
int avvad_score_finalize(const double* acc, int B, int third_mode, double* ratios /* [B][3] */,
                         double* alpha /* [B][2] or NULL */, avvad_stream_t s);
/* The SI-SDR loss of a ragged batch and its gradient in the estimate, for training.  Per row, over its first lengths[b]
 * samples, with the sums a = e.r, r = r.r, e = e.e of avvad_score_accumulate's pass (third_mode 0: the same chunks, the
 * same order, in double), P = a^2 / r and D = e - P:
 *   SI-SDR_b = 10 log10(P / D)   (avvad_score_finalize's value, bit for bit)
 *   loss[0]  = -sum_b SI-SDR_b   (summed in double in ascending row order, rounded once to float)
 *   dest[b][i] = c1 ref[b][i] + c2 est[b][i],   c2 = (20 / ln 10) / D,   c1 = -(20 / ln 10) (1 / a + a / (r D))
 * the two coefficients formed in double and rounded once each.  dest [B][ld_dest] is overwritten in columns 0 .. L - 1,
 * with exact zeros at and behind lengths[b] (clamped to [0, L]; NULL: L each); nothing of est / ref there is read.
 * ratios: NULL or [B] doubles (8-byte aligned), SI-SDR_b in dB.
 * Degenerate rows: a row with an empty window (lengths[b] <= 0) adds 0 to the loss and has a zero gradient (its ratios
 * entry is NaN, as avvad_score_finalize has it).  Any other non-finite value -- a silent reference (r = 0), an estimate
 * orthogonal to it (a = 0) or a perfect one (D = 0) -- propagates to loss, ratios and dest as IEEE arithmetic gives it.
 * The pass runs one workgroup per chunk of AVVAD_SCORE_CHUNK samples and row; no float atomics, bit-identical run to
 * run.  est / ref / dest: any 4-byte aligned float pointers with their own row pitches (>= L).  ws: 16-byte aligned. */
size_t avvad_si_sdr_loss_workspace(int B, long L);                 /* 0 on a bad shape */
int avvad_si_sdr_loss(const float* est, long ld_est, const float* ref, long ld_ref, const int* lengths /* NULL: L each */,
                      float* loss /* [1] */, double* ratios /* [B] or NULL */, float* dest, long ld_dest, int B, long L,
                      void* ws, size_t ws_bytes, avvad_stream_t s);
/* pred, target [B][T][Y] contiguous; target values are 0 / 1; pred_mode 0: pred values are 0 / 1, 1: pred values are
 * logits and the prediction is logit > 0 (sigmoid > 0.5).  counts[b] = (tp, tn, fp, fn) as int64, ADDED to (64-bit
 * integer atomics: exact in any order, no workspace); values at t >= lengths[b] (clamped to [0, T]; NULL: T each) are
 * not read. */
int avvad_confusion_accumulate(const float* pred, int pred_mode, const float* target, const int* lengths,
                               long long* counts /* [B][4], added to */, int B, int T, int Y, avvad_stream_t s);

/* ------------------------------------------------------------------------
 * Intelligibility: STOI and ESTOI of the enhanced speech (csrc/stoi.hip)
 * Replaces: nothing the reference has; the papers of this model family report both scores from a host-side package.
 * Signal order: clean x, processed y, both cropped to the row's length.  Every constant is fixed:
 *   1. fs 16000: both are resampled to 10 kHz, polyphase up 5 / down 8 with the 161 taps the caller uploads (doubles;
 *      avvad.ops.stoi_taps(): 5 firwin(161, 1/8, kaiser 5.0)), zero-extended edges, ceil(5 len / 8) samples centred as
 *      scipy.signal.resample_poly centres them; each sample is a double sum in tap order rounded once to float32.
 *      fs 10000 skips the stage; any other rate is refused.
 *   2. frames of 256 at hop 128 with starts i < len - 256 (strict), window w = hanning(258)[1:-1];
 *      e_i = 20 log10(|w x_i| + 2^-52) of the CLEAN signal in double; frame i is kept iff (max e - 40) - e_i < 0; the kept
 *      windowed frames of both signals are overlap-added at hop 128 (double sum, rounded once).
 *   3. the result is framed again by the same rule and window (M = kept - 1 frames), 512-point real DFT as one fp32-MFMA
 *      product, and the 15 third-octave band magnitudes sqrt(sum |.|^2) over bins (7,9) (9,11) (11,14) (14,17) (17,22) (22,27)
 *      (27,34) (34,43) (43,55) (55,69) (69,87) (87,109) (109,138) (138,174) (174,219), upper bin excluded, in double.
 *   4. for m = 30 .. M the 15 x 30 blocks of frames m - 30 .. m - 1, in double.  STOI per band row: a = |x| / (|y| + eps),
 *      y' = min(a y, x (1 + 10^(15/20))), both rows' means removed, each divided by (its norm + eps), products summed;
 *      d = mean over bands and segments.  ESTOI: rows normalised the same way over time, then columns over bands;
 *      d = mean over segments of sum(x_n y_n) / 30.
 *   5. a row with fewer than 30 frames after removal (or no full frame) scores 1e-5 with 0 segments; anything else
 *      propagates as IEEE arithmetic gives it.
 * d [B][2] = (STOI, ESTOI); the one `which` does not ask for is NaN.  info [B][3] = (frames, kept frames, segments).
 * clean / proc: B rows with their own pitches in floats (ld_* >= L), any 4-byte aligned float pointers; lengths: device int32
 * [B], clamped to [0, L], nothing at or behind a row's length is read (NULL: L each).  taps: 8-byte aligned device doubles
 * [161] (may be NULL at fs 10000); d: 8-byte aligned; ws: 16-byte aligned.  No floating-point atomics and every sum in a
 * fixed order of the row alone: bit-identical run to run, a row's bits independent of its batch and of "max_cus".
 * ---------------------------------------------------------------------- */
size_t avvad_stoi_workspace(int B, long L, int fs);                /* 0 on a bad shape (B outside 1..32767, L < 1) or rate */
int avvad_stoi(const float* clean, long ld_clean, const float* proc, long ld_proc, const int* lengths /* NULL: L each */,
               const double* taps /* [161] */, int B, long L, int fs, int which /* 1 STOI, 2 ESTOI, 3 both */,
               double* d /* [B][2] */, int* info /* [B][3]: frames, kept, segments */, void* ws, size_t ws_bytes,
               avvad_stream_t s);
/* STOI / ESTOI as a training loss: the row loss is -d_b, with d_b avvad_stoi's STOI (which 1) or ESTOI (which 2) bit for
 * bit (the same forward passes in the same order), and dproc its gradient in the PROCESSED signal.  The clean signal gets
 * no gradient; the 40 dB keep decision is made from the clean signal alone, so it and the kept-frame list are constants of
 * the backward.  The chain resample -> overlap-add of the kept windowed frames -> frame, window, banded DFT -> band
 * magnitudes -> segments is differentiated stage by stage, every adjoint a gather with fixed-order sums, in double where
 * the forward sums in double; no float atomics; a row's sums depend on the row alone.
 *   unit map u(v) = c / (n + eps), c = v - mean(v), n = |c|, cotangent g on u:
 *       dc = g / (n + eps) - c (g.c) / (n (n + eps)^2)   (second term 0 when n == 0),   dv = dc - mean(dc)
 *   STOI, per band row of a segment: a = |x| / (|y| + eps), p_t = a y_t where a y_t < C x_t, else C x_t (C = 1 + 10^(15/20);
 *       the tie goes to the clip branch as the forward's minimum has it, so m_t = [a y_t < C x_t] strictly).  g_p = the unit
 *       map's dv for u(p) under the cotangent u(x) / (15 S);
 *       dy_t = a m_t g_p,t - (|x| y_t / (|y| (|y| + eps)^2)) sum_k m_k g_p,k y_k   (second term 0 when |y| == 0)
 *   ESTOI: the unit map over time, then over bands; its adjoint twice in reverse, from the cotangent x_n / (30 S).
 *   (the loss is -d: both cotangents enter with a minus sign)
 *   segments: frame m belongs to segments max(0, m - 29) .. min(S - 1, m); their contributions to dY[m][j] are summed in
 *       ascending segment order (each segment writes a 15 x 30 block of its own, then a gather).
 *   band magnitude: dS[m][f] = dY[m][band(f)] S[m][f] / Y[m][band(f)], 0 where the magnitude is 0; the 15 bands tile bins
 *       7 .. 218, so this is one pass that writes the float32 operand of
 *   the banded DFT's adjoint: ONE fp32-MFMA product dframes [M x 256] = dS [M x 424] . basis^T (the window is in the
 *       basis), in whole tiles: a row's bits depend neither on its batch nor on "max_cus".
 *   framing, kept-frame overlap-add (through the inverse of the kept list: frame -> position, or dropped) and the 5/8
 *       resampler: each sample gathers the one or two frames, or the about 20 taps, that touch it, in ascending order, in
 *       double, rounded once.  fs 10000 skips the resampler, as the forward does.
 * dproc [B][ld_dproc] float32 is overwritten in columns 0 .. L - 1, with exact zeros at and behind lengths[b]; nothing of
 * either input there is read.  A row without a segment scores 1e-5 and has an all-zero gradient.
 * loss[0] = -sum_b d_b, summed in double in ascending row order and rounded once to float (as avvad_si_sdr_loss).
 * d: NULL or [B] doubles, d_b; info: NULL or [B][3] as avvad_stoi's.  Non-finite inputs propagate as IEEE arithmetic
 * gives them.  Pointers, pitches (ld_dproc >= L too), alignments and return codes as for avvad_stoi; loss and dproc: any
 * 4-byte aligned float pointers.  The workspace is the caller's; nothing is allocated and nothing synchronises. */
size_t avvad_stoi_loss_workspace(int B, long L, int fs);           /* 0 on a bad shape or rate, as avvad_stoi_workspace */
int avvad_stoi_loss(const float* clean, long ld_clean, const float* proc, long ld_proc, const int* lengths /* NULL: L each */,
                    const double* taps /* [161] */, int B, long L, int fs, int which /* 1 STOI, 2 ESTOI */,
                    float* loss /* [1] */, double* d /* [B] or NULL */, int* info /* [B][3] or NULL */, float* dproc,
                    long ld_dproc, void* ws, size_t ws_bytes, avvad_stream_t s);

/* ------------------------------------------------------------------------
 * Mask-regression training losses of a (B, T, F) mask head: mask MSE, signal approximation, spectrum approximation
 * Replaces: packages/models/utils.py:151-162 (mean_square_error_signal, mean_square_error_mask,
 *   magnitude_spectrum_approxiamation_loss), each a torch composition over one utterance.
 * pred [B][T][F] contiguous.  pred_mode 1: pred is the mask m itself and dpred the gradient in the mask; 2: m =
 * sigmoid(pred) and dpred the gradient in the logits (the numbers of avvad_istft_desc.mask_mode).  Per cell (b, t, f):
 *   kind 0 (mask):      (y - m)^2                          y = target[b][t][f]
 *   kind 1 (signal):    ((y - m) x)^2                      x = |X|, the magnitude of the mixture's complex bin
 *   kind 2 (spectrum):  |S - m X|^2                        the complex difference, real(d conj(d))
 *   row_b = (1 / len_b) sum_{t < len_b} sum_f term         (the reference's mean(sum(., axis=-1)) over the valid frames)
 *   loss[0] = sum_b row_b                                  (a fixed order that depends on B alone, in double, rounded once to float)
 *   dpred = d loss / d pred, exact zeros on frames t >= len_b; the whole [B][T][F] buffer is written (NULL: skipped)
 * len_b = n_frames[b] clamped to [0, T] (NULL: T each); a row with len_b == 0 adds nothing and divides by nothing.
 * Terms and gradients are evaluated in float32, every sum is in double.  row_loss: NULL or [B] doubles, 8-byte aligned.
 * target [B][T][F] contiguous (kind 0, 1; not read for kind 2 and may be NULL).  mix (kind 1, 2) and speech (kind 2) hold
 * interleaved (re, im) float pairs, bin (b, t, f) at p[b * stride_b + t * stride_t + f * stride_f] (float strides: even,
 * stride_t and stride_f positive, stride_b positive unless B == 1; the pointer 8-byte aligned) -- a [B][T][F][2] tensor,
 * the legacy [F][T][2] view of one utterance and a complex (F, T) tensor go in as they are.  Nothing of pred, target or
 * the spectra at or behind len_b is read.  pred / target / dpred: any 4-byte aligned float pointers.
 * A row's T * F cells are cut into chunks of AVVAD_SPECTRAL_CHUNK cells (a function of (T, F) alone), one workgroup per
 * chunk and row; per-chunk double partials are summed in a fixed lane and wave order, then a second launch adds a row's
 * partials in a fixed order that depends on its chunk count alone.
 * Guarantees: no floating-point atomics; the same bits from run to run; a row's row_loss and dpred bits are the same at
 * B = 1 and inside any batch; the loss bits do not depend on whether dpred is asked for.
 * ws: 16-byte aligned.  A bad shape (B outside 1..65535, T or F < 1, T * F > 2^30), a needed pointer that is NULL, an
 * unknown kind or pred_mode, bad strides or alignment: AVVAD_EINVAL; a workspace below the query: AVVAD_EWORKSPACE; both
 * before anything is launched or written.
 * ---------------------------------------------------------------------- */
#define AVVAD_SPECTRAL_CHUNK 2048
size_t avvad_spectral_loss_workspace(int B, int T, int F);     /* 0 on a bad shape */
int avvad_spectral_loss(const float* pred, int pred_mode /* 1 mask, 2 logits */, int kind /* 0 mask, 1 signal, 2 spectrum */,
                        const float* target /* [B][T][F]: kind 0, 1; NULL for kind 2 */,
                        const float* mix, long mb, long mt, long mf /* complex (re,im) pairs, strides in floats: kind 1, 2 */,
                        const float* speech, long sb, long st, long sf /* kind 2 */,
                        const int* n_frames /* NULL: T each */, float* loss /* [1] */, double* row_loss /* [B] or NULL */,
                        float* dpred /* [B][T][F] or NULL */, int B, int T, int F, void* ws, size_t ws_bytes, avvad_stream_t s);

/* ------------------------------------------------------------------------
 * Mixing clean speech and noise at a target SNR, for training
 * Replaces: nothing the reference has -- its corpus module leaves the noise-aware dataset as a TODO
 *   (packages/dataset/ntcd_timit.py:13, 246) and training reads mixtures that were made offline at fixed SNRs.
 * A ragged batch clean [B][ld_clean], row b holding len_b = n_samples[b] (clamped to [0, L]; NULL: L each) samples s, and
 * a noise BANK: one flat buffer of n_bank floats that holds K clips, clip k at bank[clip_off[k] .. + clip_len[k]),
 * clip_off int64 [K], clip_len int32 [K] (>= 1).  Per row a clip index clip[b], a start start[b] (int32 [B] each) and a
 * linear power ratio ratio[b] = 10^(snr_db / 10), a DOUBLE computed on the host like avvad_target_desc.vad_coef: no pow
 * runs on the device.  The row's noise is its clip read circularly,
 *   n[i] = bank[clip_off[k] + (start[b] + i) mod clip_len[k]],   0 <= i < len_b
 *   Es = sum_i s[i]^2,  En = sum_i n[i]^2  over i < len_b (En over the segment actually read, not the whole clip),
 *        every value widened to double before it is squared
 *   g_b = (float) sqrt(Es / (En ratio[b]))      formed in double and rounded once;
 *         g_b = 0 (noisy = clean, bit for bit) when len_b <= 0, Es == 0, En == 0 or ratio[b] is not finite and positive
 *   noise_out[b][i] = g_b n[i]                  one float product
 *   noisy[b][i]     = s[i] + noise_out[b][i]    one float addition (never contracted into an fma)
 * Columns len_b .. L - 1 of noisy and noise_out hold exact zeros; columns from L to the pitch are not touched.  Optional
 * outputs (each NULL or): gain [B] float g_b; energies [B][2] double (Es, En); peak [B] float max |noisy[b][:]|, equal to
 * avvad_abs_max of the written mixture bit for bit.  Nothing is rescaled here.
 * Rows are cut into chunks of AVVAD_MIX_CHUNK samples (a function of the row length alone); per-chunk double partials are
 * summed in a fixed lane and wave order and then in ascending chunk order; the peak is an integer maximum on |x|'s bits.
 * Guarantees:
 *   - no floating-point atomics; the same bits from run to run and under any "max_cus";
 *   - a row's outputs depend on that row alone: the same bits at B = 1;
 *   - nothing of clean at or behind len_b is read;
 *   - nothing outside [0, n_bank) is read, whatever the device arrays hold: clip[b] is clamped to [0, K), start[b] is
 *     taken mod the clip's length, a clip that would run past n_bank is cut there, and a clip whose offset lies outside
 *     the bank or whose length is below 1 is silent (nothing is read, g_b = 0);
 *   - clean, noisy, noise_out and bank are any 4-byte aligned float pointers, the first three each with its own row pitch
 *     >= L; no load assumes a 16-byte aligned row base;
 *   - noisy may not alias clean, nor noise_out either of them (equal pointers: AVVAD_EINVAL);
 *   - ws 16-byte aligned; ratio, energies and clip_off 8-byte aligned: AVVAD_EINVAL otherwise, before anything is launched;
 *   - a workspace below avvad_mix_workspace(B, L) bytes: AVVAD_EWORKSPACE before anything is launched.
 * ---------------------------------------------------------------------- */
#define AVVAD_MIX_CHUNK 4096
size_t avvad_mix_workspace(int B, long L);     /* 0 on a bad shape: B outside 1..65535, L < 1 */
int avvad_mix(const float* clean, long ld_clean, const int* n_samples /* NULL: L each */,
              const float* bank, long n_bank, const long long* clip_off, const int* clip_len, int K,
              const int* clip, const int* start, const double* ratio,
              float* noisy, long ld_noisy, float* noise_out /* or NULL */, long ld_noise,
              float* gain, double* energies, float* peak,      /* each NULL or as above */
              int B, long L, void* ws, size_t ws_bytes, avvad_stream_t s);

/* ------------------------------------------------------------------------
 * Rational-rate resampling: waveforms and streams of any rate into the 16 kHz signal chain (csrc/resample.hip)
 * Replaces: nothing the reference has -- its corpus scripts read audio that was resampled offline.
 * For rates fs_in -> fs_out: g = gcd, up = fs_out / g, down = fs_in / g, m = max(up, down), half = 10 m.  The filter is
 * scipy.signal.resample_poly's default, h[t] = up w[t] / sum(w), w[t] = (1/m) sinc((t - half) / m) kaiser(2 half + 1, 5.0)[t],
 * built on the host in float64 (avvad.ops.resample_taps).  Per row of len inputs x:
 *   out[n] = (float) sum_m h[n down + half - m up] x[m],   0 <= n < ceil(len up / down),
 *   m ascending over max(0, ceil((n down - half) / up)) .. min(len - 1, floor((n down + half) / up)):
 * inputs that do not exist are skipped, not multiplied; every product and the chain are double fma, rounded to float once.
 * A value depends on its own inputs alone: not on the tile, the row, the batch, "max_cus", the form of the kernel or how a
 * stream was split into calls.  No atomics, no workspace.
 * taps: 8-byte aligned device doubles, avvad_resample_taps_len(up, down) = up T of them with T = 2 half / up + 1, PHASE-MAJOR:
 *   taps[p T + j] = h[p + j up], and 0 where p + j up > 2 half (never read).
 * avvad_resample: x [B][ld_x], row b holding lengths[b] (device int32, clamped to [0, L]; NULL: L each) samples, any
 *   4-byte aligned float pointer; nothing at or behind a row's length is read.  out [B][ld_out]: columns
 *   0 .. avvad_resample_length(L, up, down) - 1 are written, +0 from the row's own count on; columns from there to the pitch
 *   are not touched.  n_out: NULL or device int32 [B], the rows' counts ceil(len up / down).
 * avvad_resample_stream: row b has taken in_before[b] inputs and emitted out_before[b] outputs since its reset, takes the
 *   first n_valid[b] samples of chunk [B][ld_chunk] (n_in columns; chunk may be NULL when n_in == 0) and writes its outputs
 *   out_before[b] .. out_before[b] + n_emit[b] - 1 to out [B][ld_out]; columns n_emit[b] .. n_max - 1 are +0 (out may be NULL
 *   when n_max == 0).  The four count arrays are device int64 [B] (a stream that runs for hours passes 2^31), clamped in the
 *   kernel (to n_in, to n_max, to [0, 2^50]) so that wrong counts cannot leave a buffer.  The host decides n_emit: a row that
 *   goes on emits the outputs whose every tap has arrived, E(N) = floor((N up - 1 - half) / down) + 1 of them after N inputs
 *   (0 while N up - 1 - half < 0); a row that ENDS with the call emits up to ceil(N up / down), the inputs that never came
 *   skipped like those behind a whole utterance's end -- so a stream of N samples yields avvad_resample's samples and count.
 *   state_in / state_out: float [B][H], H = avvad_resample_hist(up, down) = 2 half / up + 2, different buffers:
 *   state_out[b] = the last H of (state_in[b] ++ chunk[b][:n_valid[b]]), so a row with nothing to do copies its state.  Inputs
 *   in front of a row's reset are never read: any state content is "start of utterance" when in_before[b] == 0.
 * Refused (AVVAD_EINVAL) before anything is launched: up or down < 1 or > AVVAD_RESAMPLE_MAX_RATE, gcd(up, down) != 1,
 * up == down == 1 (16 kHz passes through untouched in the Python layer), B outside 1..65535, L < 1 or L or the output
 * length >= 2^31, a pitch below its row, taps not 8-byte aligned, NULL where a buffer is needed, state_in == state_out.
 * The three queries return 0 on a bad ratio.
 * ---------------------------------------------------------------------- */
#define AVVAD_RESAMPLE_TILE 256       /* outputs of one workgroup */
#define AVVAD_RESAMPLE_MAX_RATE 1024  /* largest up and down */
long avvad_resample_length(long L, int up, int down);      /* ceil(L up / down) */
long avvad_resample_taps_len(int up, int down);            /* doubles of the phase-major table */
int avvad_resample_hist(int up, int down);                 /* H: floats per row of the stream state */
int avvad_resample(const float* x, long ld_x, const int* lengths /* NULL: L each */, const double* taps, int up, int down,
                   float* out, long ld_out, int* n_out /* int32 [B] or NULL */, int B, long L, avvad_stream_t s);
int avvad_resample_stream(const float* chunk, long ld_chunk, const long long* n_valid, const long long* in_before,
                          const long long* out_before, const long long* n_emit, const float* state_in, float* state_out,
                          const double* taps, int up, int down, float* out, long ld_out, int B, int n_in, int n_max,
                          avvad_stream_t s);

/* ------------------------------------------------------------------------
 * Training labels from clean speech: framed-energy VAD and ideal binary mask (IBM)
 * Replaces: packages/processing/target.py clean_speech_VAD (:5-56), clean_speech_IBM (:58-70) and
 *   noise_robust_clean_speech_IBM (:72-107), which the reference runs offline into HDF5 label files
 *   (scripts/create_audio_train_files.py:96-160); here they run in the training step next to the features.
 * A ragged batch: wave [B][L] (rows zero-padded past each utterance), n_samples / n_frames device int32 [B] computed
 * on the host with the reference's rules:
 *   n_samples[b] = L_b, plus one hop of zeros when ceil(L_b/fs/wlen_sec/hop_percent) != int(...) (the end pad);
 *   n_frames[b]  = 1 + (n_samples[b] + 2 * (center ? n_fft/2 : 0) - n_fft) / hop  (librosa.util.frame).
 * Outputs are batch-first with frame pitch d->T; frames t >= n_frames[b] are written as 0.  No reduction crosses an
 * utterance.  Results are bit-identical run to run (fp64 energies in a fixed order; maxima by integer atomics).
 * ---------------------------------------------------------------------- */
typedef struct {
  int B;           /* utterances                                                          */
  long L;          /* sample pitch of wave [B][L]                                         */
  int n_fft, hop;  /* frame length and hop, samples                                      */
  int T;           /* frame pitch of the outputs (the largest n_frames[b])                */
  int center;      /* 0: no centring; n_fft/2 samples per side of 1: reflect, 2: zero padding (VAD only) */
  float eps;       /* IBM: 20 log10(|S| + eps)                                            */
  double vad_coef; /* 10**vad_threshold: vad = E_t > vad_coef * min_t E_t (compared in double)          */
  double ibm_coef; /* 10**(-ibm_threshold/20): ibm = |S| > (max|S| + eps) * ibm_coef - eps            */
} avvad_target_desc;
/* Bytes of workspace for the descriptor (the largest need of the entry points below); 0 on a bad descriptor
 * (B <= 0, hop <= 0, T beyond the frames that L, one hop of end pad and the centring allow, ...). */
size_t avvad_target_workspace(const avvad_target_desc* d);
/* vad [B][T] = framed-energy VAD: energies accumulated in fp64 from the wave itself (no padded copy). */
int avvad_target_vad(const float* wave, const int* n_samples, const int* n_frames, float* vad, const avvad_target_desc* d,
                     void* ws, size_t ws_bytes, avvad_stream_t s);
/* ibm [B][T][F] (F = n_fft/2 + 1, batch-first like the collates' targets) from the waveform: the STFT front-end's DFT
 * (periodic Hann, center = 0 only, n_fft % 32 == 0), the per-utterance maximum of |S|, one threshold pass; robust != 0
 * multiplies each frame by the utterance's VAD (noise_robust_clean_speech_IBM with the same framing). */
int avvad_target_ibm(const float* wave, const int* n_samples, const int* n_frames, int robust, float* ibm,
                     const avvad_target_desc* d, void* ws, size_t ws_bytes, avvad_stream_t s);
/* IBM of ONE given spectrum (d->B == 1; only n_fft, T, eps, ibm_coef are read): spec holds interleaved (re, im) float
 * pairs, bin (t, f) at spec[t * stride_t + f * stride_f] (float strides, even) -- the legacy (F, T, 2) view of
 * stft_pytorch and torch.view_as_real of a complex (F, T) tensor go in as they are.  out [F][T]; vad [T] (may be
 * NULL) multiplies each frame.  ws: at least 8 bytes (the workspace query of a descriptor always covers it), 16-byte
 * aligned like every workspace. */
int avvad_target_ibm_from_spectrum(const float* spec, long stride_t, long stride_f, const float* vad, float* out,
                                   const avvad_target_desc* d, void* ws, size_t ws_bytes, avvad_stream_t s);
/* Noise-aware masks from the two components of a mixture, the speech X and the noise N (target.py noise_aware_IBM :151-202,
 * threshold_IBM :205-251), and the ideal ratio mask of the same pair.  Per cell (b, t, f), every step in double:
 *   p2 = (double)peak[b] * peak[b]   (1 when peak is NULL or p2 is not finite and positive: no scaling)
 *   xP = ((double)re re + (double)im im) / p2 of X, nP likewise of N; nP = noise_psd when the noise spectrum is NULL
 *        (threshold_IBM: 10)
 *   speech = (xP / c_speech[f] > nP) && (xP / c_speech[f] > floor),  forced to 0 for f < low_cut - 1 and f >= high_cut
 *   noise  = (xP / c_noise[f]  < nP) || (xP / c_noise[f]  < floor),  forced to 1 on the same bins
 *   irm    = (float)(xP / (xP + nP)), 0 where xP + nP == 0; no cuts
 * strict comparisons and cut indices as the reference writes them (floor: its 0.005).  c_speech / c_noise: DOUBLE [F]
 * tables 10^(threshold_f / 10) computed on the host (no pow runs on the device), 8-byte aligned.  speech / noise / irm
 * [B][T][F] float32, each may be NULL but not all three; frames t >= n_frames[b] (int32 [B], clamped to 0..T; NULL: T
 * each) are written as zeros in all three.  peak: float [B] or NULL.  1 <= low_cut, high_cut <= F.  A pure function of
 * its inputs: no atomics, no reduction.
 * From spectra: interleaved (re, im) pairs, bin (b, t, f) at spec[b * stride_b + t * stride_t + f * stride_f] (float
 * strides: even, stride_t and stride_f positive, stride_b positive unless B == 1; the pointer 8-byte aligned), the
 * noise spectrum with strides of its own -- a [B][T][F][2] tensor, the legacy [F][T][2] view of one utterance and a
 * column slice of a wider tensor go in as they are.  No workspace.
 * From waveforms: speech_wave / noise_wave [B][d->L] (one pitch, rows zero-padded past each utterance; n_samples is not
 * read and may be NULL), d as for the waveform IBM (center == 0, n_fft % 32 == 0; eps and the two coefficients are not
 * read), F = n_fft/2 + 1.  The DFT runs once per wave with the batch's own (B, T), so both spectra are bit for bit those
 * of the complex-spectrum entry point of the STFT front-end for the same batch.  ws: 16-byte aligned, at least the
 * bytes of the query below (0 on a bad descriptor).
 * Bad arguments are AVVAD_EINVAL and a short workspace AVVAD_EWORKSPACE, before anything is launched. */
size_t avvad_target_noise_aware_workspace(const avvad_target_desc* d);
int avvad_target_noise_aware_from_spectrum(const float* spec, long stride_b, long stride_t, long stride_f,
                                           const float* noise_spec /* or NULL */, long nstride_b, long nstride_t,
                                           long nstride_f, const int* n_frames, const float* peak, const double* c_speech,
                                           const double* c_noise, int low_cut, int high_cut, double floor, double noise_psd,
                                           float* speech, float* noise, float* irm, int B, int T, int F, avvad_stream_t s);
int avvad_target_noise_aware(const float* speech_wave, const float* noise_wave, const int* n_samples, const int* n_frames,
                             const float* peak, const double* c_speech, const double* c_noise, int low_cut, int high_cut,
                             double floor, float* speech, float* noise, float* irm, const avvad_target_desc* d, void* ws,
                             size_t ws_bytes, avvad_stream_t s);

/* ------------------------------------------------------------------------
 * Video front-end: lip-region DCT coefficients -> the 67 x 67 crops of the trunk, at the STFT's frame rate
 * Replaces: scripts/create_video_train_files_upsampled.py:105-173 (process_write_video: scipy's unnormalised type-2 idct
 *   along both axes of every frame, (A - min over the utterance) / (largest per-frame max - min) * 255, np.rot90(., 3),
 *   ffmpeg's `fps` filter through a temporary mp4) and the pixel statistics of :294-310, :350-361.
 * coef [rows][W*H] holds the utterances' coefficient frames; utterance b owns the n_in[b] rows from starts[b] on (a
 * packed or a padded batch alike).  video [B][T][H][W]; output frame k of utterance b shows input frame i for
 *   s(i) <= k < s(i+1),  s(i) = (2 i p + q) / (2 q)   (i p / q rounded half away from zero),
 * p / q = fs / (hop * fps_in) in lowest terms (25 / 12 for 16 kHz, hop 256, 30 frames/s), up to
 * out_len[b] = min(s(n_in[b]), n_out[b], T); frames k >= out_len[b] are written as 0.  n_out may be NULL (no cap).
 * quantize != 0: clip to [0, 255] and round towards zero (the uint8 conversion of the reference's frame writer); the
 * codec round trip that follows there is not modelled.  An utterance whose frames are all constant (range 0, a division
 * by zero in the reference) is written as 0.  No reduction crosses an utterance.
 * Fused extras: acc (may be NULL) is a statistics accumulator with nstat == 1 (avvad_stats_*): the written frames'
 * sum, sum of squares and pixel count are ADDED to it, exactly what avvad_stats_accumulate(video, out_len, nstat = 1)
 * adds, taken before the standardisation; mean / std_ (one float each on the device, both or neither) store
 * (x - mean) / (std + norm_eps) instead of x.  Double accumulation in a fixed order, no floating-point atomics:
 * bit-identical run to run and independent of "max_cus".
 * starts / n_in / n_out / out_len are device int32 [B]; coef and ws are 16-byte aligned.  The workspace holds the
 * un-normalised frames between the two passes (rows * W * H floats) besides per-frame minima, maxima and partial sums:
 * the utterance's minimum and range are needed before a frame can be written, and re-reading the frames measured faster
 * than forming them twice.
 * ---------------------------------------------------------------------- */
typedef struct {
  int B;           /* utterances                                                          */
  int n_max;       /* the largest n_in[b] (sizes the grid only)                           */
  long rows;       /* rows of coef                                                        */
  int T;           /* frame pitch of video (at least the largest out_len[b])              */
  int W, H;        /* 67, 67                                                              */
  int p, q;        /* output frames per input frame, in lowest terms                      */
  int quantize;    /* clip and truncate to 8-bit levels                                   */
  float norm_eps;  /* eps of the fused standardisation                                    */
} avvad_lip_desc;
/* Bytes of workspace; 0 on a bad descriptor (B, rows, n_max, T, p, q <= 0, W or H != 67, B or T > 65535, ...). */
size_t avvad_lip_decode_workspace(const avvad_lip_desc* d);
int avvad_lip_decode(const float* coef, const int* starts, const int* n_in, const int* n_out, float* video, int* out_len,
                     double* acc, const float* mean, const float* std_, const avvad_lip_desc* d, void* ws, size_t ws_bytes,
                     avvad_stream_t s);

/* ------------------------------------------------------------------------
 * Masked BCE-with-eps loss, summed over sequences
 * Replaces: binary_cross_entropy packages/models/utils.py:108-113 and its caller
 *   loop scripts/train_AV_net.py:298-301  (per-sequence mean over valid frames
 *   and y_dim, summed over the batch).
 * logits/targets [B][T][Y]; loss: one float (overwritten); dlogits [B][T][Y]
 * (d loss / d logits, zero on padded steps), may be NULL.
 * ---------------------------------------------------------------------- */
int avvad_bce_masked(const float* logits, const float* targets, const int* lengths, float* loss,
                     float* dlogits, int B, int T, int Y, float eps, avvad_stream_t s);

/* Two-output-unit BCE on probabilities: binary_cross_entropy_2classes packages/models/utils.py:115-116
 * (imported by scripts/train_video_net.py:18):
 *   loss = -mean_rows( sum_y [ x log(r1 + eps) + (1 - x) log(r2 + eps) ] ).
 * r1, r2, x [rows][Y]; loss one float; dr1 / dr2 (d loss / d r, may be NULL) [rows][Y]. */
int avvad_bce_2classes(const float* r1, const float* r2, const float* x, float* loss, float* dr1, float* dr2,
                       long rows, int Y, float eps, avvad_stream_t s);

/* ------------------------------------------------------------------------
 * Fused Adam step over a flat parameter buffer
 * Replaces: torch.optim.Adam(lr, betas=(0.9,0.999)).step()  scripts/train_AV_net.py:238,306
 * (torch semantics: eps added to sqrt(v_hat); no weight decay, no amsgrad).
 * ---------------------------------------------------------------------- */
int avvad_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                    float lr, float beta1, float beta2, float eps, int step, avvad_stream_t s);

/* ------------------------------------------------------------------------
 * Small fused elementwise helpers used by the Python host
 * ---------------------------------------------------------------------- */
/* dst[r][dst_off + c] = src[r][src_off + c], c < ncols (row strides src_ld / dst_ld) -- writes a
 * branch into the concat buffer (torch.cat, AV_Net.py:124) and splits its gradient back */
int avvad_copy_cols(const float* src, float* dst, size_t rows, int ncols, int src_ld, int src_off,
                    int dst_ld, int dst_off, avvad_stream_t s);
/* out[c] += sum_r X[r][c]   (bias gradient of nn.Linear) */
int avvad_colsum_acc(const float* X, size_t rows, int cols, float* out, avvad_stream_t s);
/* x[i] *= *scalar  (scalar lives on the device: upstream gradient of the loss) */
int avvad_scale_by_device_scalar(float* x, const float* scalar, size_t n, avvad_stream_t s);
/* out[b][t][c] = in[b][c][t]  (encoder output (B,Bn,P) -> (B,P,Bn)) and back */
int avvad_transpose_last2(const float* in, float* out, int B, int C, int T, avvad_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* AVVAD_H */
