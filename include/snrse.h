/* snrse.h — C-ABI of libsnrse_hip.so, the MI355X (gfx950) kernels of the
 * reverse-diffusion speech-enhancement path of yh-jun/SNR-Aligned_diffSE
 * (ScoreModel.enhance() / PC sampler, sgmse-bbed/sgmse/model.py:702-839).
 *
 * Conventions
 *   - Plain pointers to DEVICE memory, sizes as int, a hipStream_t (NULL = legacy stream);
 *     every launch is stream-ordered and asynchronous, nothing is allocated inside except
 *     where a caller-provided workspace is named.
 *   - Reentrancy: entries without a snrse_ctx argument keep no state.  The four with one
 *     (snrse_conv2d, snrse_gn_stats, snrse_input_conv, snrse_gn_resample) read their switches and
 *     split-K workspace from it and write their read-backs into it, so calls through DISTINCT
 *     contexts may run concurrently from any host threads / streams; give each concurrently issuing
 *     thread or stream its own context.  A NULL context is the process default one (edited by
 *     snrse_set_option / snrse_set_workspace; for single-stream callers).
 *   - Return 0 on success or a hipError_t code (hipErrorInvalidValue = 1 for a bad
 *     argument); snrse_error_string() maps it to text.  The Python host maps non-zero to
 *     RuntimeError, as the reference's TORCH_CHECK does (op/upfirdn2d.cpp:8-19).
 *   - dtype: SNRSE_F32 = 0 (exact fp32 "parity" mode), SNRSE_F16 = 2 (IEEE fp16 storage and MFMA
 *     operands, fp32 accumulation: the 16-bit fast path's default since round 6, whose error against the
 *     reference is ~9x below bf16's), SNRSE_BF16 = 1 (the same kernels on bf16; every entry
 *     that takes SNRSE_BF16 takes SNRSE_F16 too), SNRSE_F32X3 = 4 (snrse_conv2d only: fp32 activations and output, weights
 *     pre-split into bf16 hi / lo halves, three bf16 MFMA products per K-tile -- the fast fp32
 *     parity mode).  Activations are NHWC: [B, F(=H), T(=W), C].
 *   - Range: SNRSE_F16 holds magnitudes up to 65504 and every 16-bit store rounds to nearest, so a larger
 *     value is stored as +-inf (SNRSE_BF16 has fp32's exponent range).  No entry checks this on its own;
 *     snrse_range_stats reads a stored tensor back and reports its peak and its inf / NaN count per batch
 *     row.  The Python host runs it once per enhancement and recomputes a damaged utterance in bf16.
 *   - Complex spectrograms are interleaved complex64 [B, F, T] (= the reference's
 *     [B, 1, F, T] tensors).
 */
#ifndef SNRSE_H_
#define SNRSE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* hipStream_t;

enum { SNRSE_F32 = 0, SNRSE_BF16 = 1, SNRSE_F16 = 2, SNRSE_F64 = 3, SNRSE_F32X3 = 4 };

int snrse_abi_version(void); /* 2: snrse_ctx arguments */
/* sha256 (hex) of the sources the library was compiled from: csrc/*.hip, *.cpp, *.h and the build
 * script (snrse/build.py source_hash()), compiled in; "unknown" for a build made without it. */
const char* snrse_build_id(void);
const char* snrse_error_string(int code);
int snrse_device_name(char* buf, int len);

/* Caller-owned launch context: tuning switches (the names of snrse_set_option), the split-K
 * workspace and the read-backs of the latest launch through it (the names of snrse_get_option).
 * Host memory only; create copies the process default's switches, with no workspace. */
typedef struct snrse_ctx snrse_ctx;
snrse_ctx* snrse_ctx_create(void);
void snrse_ctx_destroy(snrse_ctx* ctx);
int snrse_ctx_set_workspace(snrse_ctx* ctx, void* ptr, size_t bytes);
int snrse_ctx_set_option(snrse_ctx* ctx, const char* name, int value);
int snrse_ctx_get_option(const snrse_ctx* ctx, const char* name, int* value);
/* Diagnostic timing (bench.py's roofline probe): from now on every snrse_conv2d call through ctx is
 * bracketed by a pair of HIP events (created here, without the system-scope fence), up to `capacity`
 * calls; capacity 0 stops and frees them.  snrse_ctx_probe_read waits for the recorded calls and writes,
 * in call order, each call's device time in ms and the kernel generation that ran ("last_kernel"). */
int snrse_ctx_probe_begin(snrse_ctx* ctx, int capacity);
int snrse_ctx_probe_read(snrse_ctx* ctx, float* ms, int* kernel, int max, int* n);

/* Generic FIR resampling on [major, in_h, in_w, minor] — replaces the reference's only
 * native op binding, upfirdn2d(input, kernel, up_x, up_y, down_x, down_y, pad_x0, pad_x1,
 * pad_y0, pad_y1) (op/upfirdn2d.cpp:12-23, op/upfirdn2d_kernel.cu:209-369, semantics of
 * upfirdn2d_native op/upfirdn2d.py:159-200).  `kernel` is [kh, kw] f32 on the device;
 * `out` is caller-allocated [major, out_h, out_w, minor] with
 * out_h = (in_h*up_y + pad_y0 + pad_y1 - kh)/down_y + 1 (out_w likewise).
 * dtype: SNRSE_F32 / SNRSE_F16 / SNRSE_F64, the reference's float / half / double dispatch
 * (upfirdn2d_kernel.cu:311), plus SNRSE_BF16; f64 accumulates in f64, the others in f32. */
int snrse_upfirdn2d(const void* in, void* out, const float* kernel, int major, int in_h, int in_w,
                    int minor, int kh, int kw, int up_x, int up_y, int down_x, int down_y,
                    int pad_x0, int pad_x1, int pad_y0, int pad_y1, int dtype, hipStream_t stream);

/* Implicit-GEMM convolution (3x3 pad 1 or 1x1), stride 1, NHWC, on MFMA.
 * Replaces ddpm_conv3x3 / ddpm_conv1x1 / NIN (ncsnpp_utils/layers.py:100-124, 546-555).
 *   input channels = concat(src0 [.., C0], src1 [.., C1]) (torch.cat, ncsnpp.py:337)
 *   wgt    [Npad][ksize*ksize*(C0+C1)] packed (Cout, ky, kx, Cin), dtype; Npad = Cout
 *          rounded up to 128 (Cout >= 64) or 16 (Cout <= 16, zero rows)
 *   sc_src/sc_src1 (optional): 1x1 shortcut input(s) appended as extra K; sc_wgt [Npad][Csc+Csc1]
 *   out[m][n] = ((acc + bias[n] + temb[b][n] + res[m][n]) * out_scale)
 *               + (comb_src ? comb_src[m][0:4] . comb_w[n][0:4] + comb_b[n] : 0)
 *   out_f32: write float output (bf16 mode pyramid heads); res then is float too.
 *   stats (optional): per-channel (sum, sumsq) of out, [B][SNRSE_STAT_SLOTS][Cout][2] double
 *          (atomics spread over the slots; consumers fold them), for the next GroupNorm
 *          (zeroed by the call unless the context's "stats_zeroed" switch is set).
 *   gn_scale/gn_shift (optional, [B][C0+C1] f32, from snrse_gn_scale_shift): the main input
 *          is consumed as SiLU(x*scale+shift) (gn_act=1) or x*scale+shift (gn_act=0), i.e. the
 *          ResBlock's GroupNorm+SiLU fused into the GEMM's halo load (bf16, 3x3, H%4==0,
 *          W%64==0, and the pyramid heads Cout<=16 with f32 output; otherwise
 *          hipErrorInvalidValue).
 *   dtype SNRSE_F32X3: src/res/out fp32; wgt [Npad][2*ksize*ksize*(C0+C1)] and sc_wgt [Npad][2*(Csc+Csc1)]
 *          bf16, each 32-element K-tile of the fp32 packing stored as 32 hi = bf16(w) then 32
 *          lo = bf16(w - hi); Cout % 128 == 0 or Cout <= 16 (Npad 16); gn_scale only on the halo form
 *          (3x3, H % 4 == 0, >= 256 tiles or option x3_tile 4) and the pyramid head (3x3, Cout <= 16,
 *          H % 8 == 0, W % 32 == 0, C0 / C1 % 32 == 0, no stats / temb / shortcut / combine), else
 *          hipErrorInvalidValue; out_f32 ignored. */
int snrse_conv2d(snrse_ctx* ctx, const void* src0, int C0, const void* src1, int C1, int B, int H, int W, int ksize,
                 const void* wgt, const void* sc_src, int Csc, const void* sc_src1, int Csc1,
                 const void* sc_wgt, const float* bias, const float* temb, int temb_stride,
                 const void* res, int res_ld, float out_scale, const float* comb_src,
                 const float* comb_w, const float* comb_b, void* out, int Cout, int out_ld,
                 double* stats, const float* gn_scale, const float* gn_shift, int gn_act, int dtype,
                 int out_f32, hipStream_t stream);

/* Statistics buffers of the GroupNorm entries: [B][SNRSE_STAT_SLOTS][C][2] double. */
#define SNRSE_STAT_SLOTS 16

/* GroupNorm statistics (nn.GroupNorm, layerspp.py:221,233): per-channel (sum, sumsq) over
 * H*W of src0 into sums and of src1 into sums1 (slotted layout above; zeroed by the call). */
int snrse_gn_stats(snrse_ctx* ctx, const void* src0, int C0, const void* src1, int C1, int B, int HW, double* sums,
                   double* sums1, int dtype, hipStream_t stream);

/* Per-(b, c) GroupNorm scale/shift from per-channel sums (of src0 | src1, H*W pixels each). */
int snrse_gn_scale_shift(const double* sums0, int C0, const double* sums1, int C1, int B, int HW,
                         const float* gamma, const float* beta, int groups, float eps, float* scale,
                         float* shift, hipStream_t stream);

/* Fused GroupNorm-apply (+SiLU) (+FIR [1,3,3,1] down/up x2) (layerspp.py:245-257,
 * up_or_down_sampling.py:195-257).  sums == NULL: identity normalisation (plain FIR of x).
 * mode: 0 none, 1 down (out H/2 x W/2), 2 up (out 2H x 2W).  out [B][Ho][Wo][C0+C1]. */
int snrse_gn_apply(const void* src0, int C0, const void* src1, int C1, int B, int H, int W,
                   const double* sums, const double* sums1, const float* gamma, const float* beta,
                   int groups, float eps, int act, int mode, void* out, int dtype, hipStream_t stream);

/* LDS-tiled GroupNorm-apply + SiLU + FIR x2 of a ResBlock with up/down (layerspp.py:245-257):
 * out_act = FIR(act(x*scale+shift)) and, when out_raw != NULL, out_raw = FIR(x) (the shortcut input,
 * layerspp.py:249/255), both [B][Ho][Wo][C] from one pass over x.  scale/shift [B][C] f32 from
 * snrse_gn_scale_shift, or both NULL (identity).  mode 1 down (H, W even), 2 up.  dtype SNRSE_BF16: C % 8 == 0
 * with C / 8 dividing 64 (the row-strip kernel), otherwise C % 16 == 0 (the LDS-tiled kernel); SNRSE_F32
 * (the fp32 parity modes): C % 4 == 0 with C / 4 dividing 64 (row strips).  act = 1 computes SiLU in both
 * dtypes as z * rcp(-(1 + 2^z) / ln 2) on the affine prescaled by -log2(e) (v_exp_f32 + v_rcp_f32, each 1 ulp:
 * a few fp32 ulp, ~4e-7 relative), not the IEEE-division silu_exact of snrse_gn_act / snrse_gn_apply; in the
 * exact fp32 mode that is 2-3 orders below its 1e-4 tolerance (tests/test_gpu_kernels.py resample cases). */
int snrse_gn_resample(snrse_ctx* ctx, const void* src, int C, int B, int H, int W, const float* scale, const float* shift,
                      int act, int mode, void* out_act, void* out_raw, int dtype, hipStream_t stream);

/* Elementwise GroupNorm-apply (+SiLU) of the channel concatenation (src0 | src1), dtype SNRSE_BF16 or
 * SNRSE_F32 (exact SiLU), from precomputed scale/shift [B][C0+C1] (snrse_gn_scale_shift; both NULL:
 * identity).  out [B][HW][C0+C1]. */
int snrse_gn_act(const void* src0, int C0, const void* src1, int C1, int B, int HW, const float* scale,
                 const float* shift, int act, void* out, int dtype, hipStream_t stream);

/* Split-K workspace of the small-image conv GEMMs (levels whose tile grid underfills the CUs) of the
 * process default context (per context: snrse_ctx_set_workspace): a device buffer of `bytes` the
 * caller keeps alive and leaves untouched while convs run; the library keeps [splits][M][Cout] f32
 * partial sums there and splits only when they fit.  NULL disables splitting (the default).  Launches
 * that may run concurrently must be issued through contexts with different workspaces. */
int snrse_set_workspace(void* ptr, size_t bytes);

/* Tuning switches of the process default context (per context: snrse_ctx_set_option; A/B experiments;
 * the Python host also reads SNRSE_OPTS="name=value,..." at load):
 * "conv_variant" 0 auto, 1 register-staged v1, 2 LDS-DMA v2, 5 halo GEMM v5 (the default halo kernel);
 * "splitk" 0 disables the split-K small-image GEMMs, "splitk_target" workgroups a split launch aims for;
 * "epi_nt" 0 / 1 / 2 (auto above "epi_nt_mb" = 256 MB of output) non-temporal halo-GEMM output stores;
 * "h5_specialise" 1 compile-time epilogue flags for the NCSN++ ResBlock configurations (16-bit halo GEMM, and the
 *   fp32x3 halo GEMM's pair schedule);
 * "h5_tw" halo-GEMM tile: 0 auto (8 rows x 32 px where H % 8 == 0, else 4 x 64), 64 forces 4 x 64;
 * "resample_variant" 0 row-strip / 1 LDS-tiled gn_resample, "resample_nt" non-temporal stores there,
 * "resample_down_rows" 1 / 2 / 4 (default) output rows per down-sampling row strip (bit-identical results);
 * "x3_tile" split-bf16 fp32 GEMM: 0 auto (the halo kernel on 3x3 convs with H % 4 == 0 and >= 256 tiles of
 *   4 x 64 px x 128 couts, any W, else register-staged 128 x 128), register-staged tiles 1 128 px x 128 couts,
 *   2 256 x 128, 3 128 x 256 (Cout % 256 == 0), 4 the halo kernel wherever its shape conditions hold;
 * "stats_zeroed" 1 = the statistics buffers handed to snrse_conv2d / snrse_gn_stats are already zero (the
 * caller clears one arena per network evaluation), so they skip their per-call memset;
 * "ic_lds" the bf16 input conv (W <= 1024): 3 (default) its workgroup's input rows staged in LDS and its output
 *   staged through LDS for whole-KB stores, 1 input rows only, 2 with the channels split over wave pairs, 0 the
 *   streaming form (all bit-identical but 2's statistics fold order);
 * "x3_tw" fp32x3 halo GEMM tile: 0 (default) 8 x 32 px where H % 8 == 0 and W % 32 == 0, else 4 x 64; 64 forces
 *   4 x 64; "x3_nt" 1 (default) its fp32 output stores non-temporal under the "epi_nt" rule;
 * "x3_spread" fp32x3 halo GEMM schedule: 2 (default) two taps per barrier phase where its tiles are 8 x 32 px and the
 *   main input has an even number of 32-channel chunks (else 1), 1 one tap per phase with the next chunk's halo stored
 *   one piece per tap, 0 the same stored in one go;
 * "head_small" bf16 pyramid heads (Cout 4, C % 256 == 0): 1 (default) the wave-per-8-pixels head (GroupNorm fused)
 *   where the tiled head cannot take the image (H % 8 or W % 32 != 0), 2 also for up to 16384 output pixels, 0 never;
 * "head_part" tiled bf16 pyramid head with Cout 4: 1 (default) the halo's 36 tap partials as one 1x1 GEMM then their
 *   shifted sum (last_kernel 15), 0 nine tap GEMMs over the halo (last_kernel 10);
 * "gn_slice" snrse_gn_apply with statistics (no resampling): 1 (default) each block owns a 64-channel slice of its
 *   pixels and folds only that slice's statistics, 0 each block folds all channels (equal results; read from the
 *   process default context, as snrse_gn_apply takes none). */
int snrse_set_option(const char* name, int value);

/* Read back a switch (any name above) or: "halo_kernel" = generation of the halo conv kernel the current
 * setting dispatches a 3x3 conv to (5), "last_kernel" = generation of the most recent snrse_conv2d launch (1 v1, 2 v2,
 * 3 / 4 split-bf16 register-staged / halo, 5 halo, 10 pyramid head, 11 split-bf16 pyramid head, 14 small-image
 * pyramid head, 15 tap-partials pyramid head),
 * "last_ksplit" = K splits of the most recent v2 launch, "last_epi_nt" /
 * "last_chunks" = store flavour / image-range launches of the most recent halo conv, "last_tw" = its tile
 * width (32 / 64). */
int snrse_get_option(const char* name, int* value);

/* AttnBlockpp attention core (layerspp.py:84-88): qkv [B][L][3C] -> out [B][L][C],
 * softmax(q k^T / sqrt(C)) v, flash-style on MFMA.  C must be 256.  dtype SNRSE_BF16, SNRSE_F32 (exact fp32
 * MFMAs) or SNRSE_F32X3 (fp32 in / out, q, k, v and the probabilities split into bf16 hi + lo, hi.hi + hi.lo + lo.hi
 * products: the fp32x3 parity mode). */
int snrse_attention(const void* qkv, void* out, int B, int L, int C, int dtype, hipStream_t stream);

/* Time embedding (ncsnpp.py:256-275): temb[b] = W2 silu(W1 [sin, cos](2 pi log t W_gfp) + b1) + b2. */
int snrse_temb_mlp(const float* t, const float* Wg, const float* W1, const float* b1, const float* W2,
                   const float* b2, float* temb, int B, int nf, hipStream_t stream);
/* The same MLP as two row-parallel launches (the form the network executor runs; every weight row is read once
 * per launch, spread over the chip): snrse_temb_gfp_dense gives the pre-activation a[b] = W1 [sin, cos](2 pi log t
 * W_gfp) + b1 (out [B][4 nf]), then snrse_temb_dense(a, W2, b2) = W2 silu(a) + b2 = temb.  nf even, 4 nf <= 512
 * (nf <= 128: snrse_temb_dense takes D = 4 nf <= 512; NCSN++ uses nf = 128). */
int snrse_temb_gfp_dense(const float* t, const float* Wg, const float* W1, const float* b1, float* out, int B, int nf,
                         hipStream_t stream);
/* All ResBlock Dense_0 projections (layerspp.py:264-265): out[b][r] = W[r] . silu(temb[b]) + bias[r]. */
int snrse_temb_dense(const float* temb, const float* W, const float* bias, float* out, int B, int R, int D,
                     hipStream_t stream);

/* Fused input conv, 16-bit (ncsnpp.py:253-254, 282-285): complex x, y [B][H][W] -> out [B*H*W][128]
 * (dtype SNRSE_F16 or SNRSE_BF16) = conv3x3(cat(x.re, x.im, y.re, y.im), wgt) + bias, plus the f32 input pyramid
 * pyr [B*H*W][4] and out's GroupNorm statistics [B][SLOTS][128][2] (zeroed here unless option
 * stats_zeroed).  wgt: dtype [128][64], k = (ky * 3 + kx) * 4 + channel, k >= 36 zero.
 * Requires W % 64 == 0 and (H * W / 64) % 16 == 0 (else SNRSE_EINVAL: use snrse_input_pack). */
int snrse_input_conv(snrse_ctx* ctx, const void* x, const void* y, int B, int H, int W, const void* wgt, const float* bias,
                     void* out, float* pyr, double* stats, int dtype, hipStream_t stream);

/* The same input conv for the fp32x3 parity mode: wgt = ops.split_weight of the packed [128][64] weights ([128][128]
 * bf16: per 32-element K tile 32 hi then 32 lo), split-bf16 products (w_hi.x_hi + w_lo.x_hi + w_hi.x_lo), f32 out
 * [B*H*W][128]; the input rows staged in LDS (W % 64 == 0, W <= 1024, (H*W/64) % 16 == 0).  Replaces
 * snrse_input_pack + the split GEMM on its im2col. */
int snrse_input_conv_x3(snrse_ctx* ctx, const void* x, const void* y, int B, int H, int W, const void* wgt,
                        const float* bias, float* out, float* pyr, double* stats, hipStream_t stream);

/* Network input (ncsnpp.py:253-254, 282-285): complex x, y [B,F,T] -> im2col [B,F,T,64]
 * (tap-major 3x3 x {x.re, x.im, y.re, y.im}, zero padded) in dtype, and the f32 input
 * pyramid [B,F,T,4]. */
int snrse_input_pack(const void* x, const void* y, int B, int H, int W, void* col, float* pyr, int dtype,
                     hipStream_t stream);

/* Output head + preconditioning + SDE step (ncsnpp.py:398-404, model.py:481-541,
 * predictors.py:75-80, correctors.py:69-81).  pyr [B,F,T,4] (f32 if pyr_f32 else bf16),
 * t [B], score_mode 0 = -dnn ('bbed'), 1 = c_skip x + c_out dnn ('sebridge*').
 * coef [B][4] = {a, by, c, s}: x_mean = a x + by y + c score; x_out = x_mean + s z.
 * z = noise (complex64 tensor) or, if noise == NULL, Philox4x32-10(seed, offset + index)
 * complex normal with each part N(0, 1/2).  x_out == NULL: only score_out is written. */
int snrse_score_update(const void* pyr, int pyr_f32, const float* out_w, const float* out_b,
                       const float* t, int score_mode, int B, int HW, const void* x, const void* y,
                       const void* noise, uint64_t seed, uint64_t offset, const float* coef,
                       void* x_out, void* xmean_out, void* score_out, hipStream_t stream);

/* Same step for an arbitrary score tensor (generic score_fn). */
int snrse_sde_update(const void* x, const void* y, const void* score, const void* noise, uint64_t seed,
                     uint64_t offset, const float* coef, int B, int HW, void* x_out, void* xmean_out,
                     hipStream_t stream);

/* out = coef[b][0] x + coef[b][1] y + coef[b][3] z (prior sampling, sdes.py:225-232, 298-304). */
int snrse_axpby_noise(const void* x, const void* y, const void* noise, uint64_t seed, uint64_t offset,
                      const float* coef, int B, int HW, void* out, hipStream_t stream);

/* Row-seeded forms of the three entries above: the draw of element e of batch row b is
 * Philox4x32-10(row_seed[b], draw * HW + e), exactly what the entry above draws for a [1][HW] batch with
 * seed = row_seed[b], offset = draw * HW -- so an utterance's noise depends on its own seed and the draw index
 * only, not on the batch it shares or its row in it.  row_seed [B] on the device; noise != NULL overrides it. */
int snrse_score_update_rs(const void* pyr, int pyr_f32, const float* out_w, const float* out_b,
                          const float* t, int score_mode, int B, int HW, const void* x, const void* y,
                          const void* noise, const uint64_t* row_seed, uint64_t draw, const float* coef,
                          void* x_out, void* xmean_out, void* score_out, hipStream_t stream);
int snrse_sde_update_rs(const void* x, const void* y, const void* score, const void* noise,
                        const uint64_t* row_seed, uint64_t draw, const float* coef, int B, int HW, void* x_out,
                        void* xmean_out, hipStream_t stream);
int snrse_axpby_noise_rs(const void* x, const void* y, const void* noise, const uint64_t* row_seed,
                         uint64_t draw, const float* coef, int B, int HW, void* out, hipStream_t stream);

/* Evaluation metrics (eval.py:144-157 -> utils.py:10-35 energy_ratios, sgmse/util/other.py:71-75
 * si_sdr), batched: s_hat, s, n [B][L] f32 (n may be NULL) -> out [B][3] f64 = (SI-SDR, SI-SIR,
 * SI-SAR) in dB from six fp64 dot products per utterance; SI-SIR / SI-SAR are NaN without n. */
int snrse_energy_ratios(const float* s_hat, const float* s, const float* n, int B, int L, double* out,
                        hipStream_t stream);

/* norm_factor = max |y| per utterance (model.py:726): out[b] = max_i |sig[b][i]|.  +-inf gives inf.  A NaN sample
 * is skipped (the maximum is folded with fmaxf, which returns its other operand), where torch's abs().max()
 * returns NaN: a row's result is the maximum of its non-NaN samples, 0 for a row of NaN only. */
int snrse_absmax(const float* sig, int B, int L, float* out, hipStream_t stream);

/* Ragged batches: utterances of different lengths in one [B][Lstride] f32 buffer with lengths [B] int32 on the
 * device; row b is valid on [0, L_b) and nothing at or past L_b is read into a result.  The metrics' dot
 * products and the maximum run over [0, L_b).  The STFT reflects each row at its own L_b, writes its
 * T_b = 1 + L_b / 128 frames and zeroes frames [T_b, Tpad); the lengths live on the device, so the CALLER checks
 * 255 < L_b <= Lstride and T_b <= Tpad before the call (snrse.ops.stft raises for them). */
int snrse_energy_ratios_ragged(const float* s_hat, const float* s, const float* n, const int* lengths, int B,
                               int Lstride, double* out, hipStream_t stream);
int snrse_absmax_ragged(const float* sig, const int* lengths, int B, int Lstride, float* out, hipStream_t stream);
int snrse_stft_ragged(const float* sig, const int* lengths, int B, int Lstride, const float* in_div,
                      float in_scale, int Tpad, int mode, void* out, hipStream_t stream);

/* Sample-rate conversion in front of the network (csrc/audio_resample.hip): rational polyphase FIR resampling of a
 * ragged batch, x [B][stride_in] f32 with lengths [B] int32 on the device -> y [B][stride_out] f32.  The
 * arithmetic of scipy.signal.resample_poly(x, up, down, window=w, padtype='constant'): with half = (len(w) - 1) / 2,
 * h = up w and n_out_b = ceil(L_b up / down),
 *   y[b][m] = sum_n x[b][n] h[m down + half - n up]     0 <= n < L_b,  0 <= m down + half - n up <= 2 half.
 * up, down must be coprime.  taps: h phase-major, [up][K] f32 with K = ceil((2 half + 1) / up) and
 * taps[p][j] = h[p + j up] (0 where p + j up > 2 half); NULL is allowed for up == down == 1, which copies.
 * Nothing at or past L_b of a row is read, outputs [n_out_b, stride_out) are written as zero, L_b = 0 gives a row
 * of zeros; the CALLER sees to n_out_b <= stride_out (an output past the stride is not written).  Every output is
 * one fp32 fma chain over j ascending: no atomics, the same bits on every launch and for a row launched alone.
 * EINVAL when a block's input span, about 256 down / up + K samples, exceeds 64 KB of LDS (down / up above ~60).
 * snrse_resample_poly_block: outputs per block (the lengths at which the kernel changes path). */
int snrse_resample_poly(const float* x, const int* lengths, int B, long long stride_in, int up, int down, int half,
                        const float* taps, float* y, long long stride_out, hipStream_t stream);
int snrse_resample_poly_block(void);

/* The band above 8 kHz, kept at the recording's own rate (csrc/highband.hip).  The networks run at 16 kHz, so a
 * recording at R > 16000 comes back from them band-limited.  For one row let y be the recording at rate R (L
 * samples), u its 16 kHz version (L16 = ceil(L 16000 / R) samples, what the enhancers consume), x the enhanced
 * 16 kHz row (L16 samples), h the 16 k -> R filter in the resampler's phase-major layout with up / down = R / 16000
 * in lowest terms, and U(v)[n] = sum_j v[j] h[n down + half - j up], 0 <= n < L, the arithmetic above.  Then
 *   out[n] = U(x)[n] + g[n] (y[n] - U(u)[n]) = g[n] y[n] + sum_j h[.] (x[j] - g[n] u[j]).
 * y = U(u) + (y - U(u)) holds by construction: g = 1 with x = u returns y, g = 0 is the plain resampler, and
 * g < 1 blends the anti-alias filter's crossover smoothly instead of leaving a hole.
 *
 * The gain g[n]: a constant (gains NULL: gain_const), or linear interpolation between per-frame values g_s, frame
 * t centred at 16 kHz sample 128 t, in integer arithmetic: num = n 16000, den = R 128 (64-bit; n down and up 128
 * after the reduction, the same quotient and the same fraction), i = num / den, a = (num % den) / den,
 *   g[n] = (1 - a) g_s[min(i, T - 1)] + a g_s[min(i + 1, T - 1)],
 * exactly g_s[i] where den divides num.  gains [B][Tmax] f32 with frames [B] int32 (T_b, 1 <= T_b <= Tmax; T_b < 1
 * counts as g = 0), values >= 0; nothing at or past T_b of a row is read.
 *
 * snrse_resample_mix: x, u [B][stride16] f32 with len16 [B], y [B][strideR] f32 with lenR [B] -> out [B][strideR]
 * f32, all on the device.  One output per thread, the block's span of x and u staged in LDS with zeros outside
 * [0, L16_b); nothing at or past a row's length is read in any input, outputs [L_b, strideR) are written as zero.
 * One fp32 fma chain over j ascending per output: no atomics, the same bits on every launch and for a row launched
 * alone.  up > down, coprime; the definition covers L_b <= ceil(L16_b up / down), a recording no longer than its
 * 16 kHz version brought back up (snrse.ops.resample_mix refuses a longer one; past that length U is zero).
 * EINVAL when the staged span of x and u exceeds 64 KB of LDS.
 *
 * snrse_band_gain: the "follow" policy's g_s -- the high band is attenuated as much as the network attenuated the
 * top octave it saw.  With S the raw STFT (n_fft 510, hop 128, periodic Hann, centred, reflect at the row's own
 * L16, un-normalised) and T_b = 1 + L16_b / 128 frames:
 *   E_u[t], E_x[t] = sum over bins k = 128 .. 255 of |S[k, t]|^2 of u and of x,
 *   g_f[t] = 1 where E_u[t] == 0, else clamp(sqrt(E_x[t] / E_u[t]), floor_gain, 1), floor_gain = 10^(-floor_db / 20),
 *   g_s[t] = the mean of g_f over frames max(0, t - 2) .. min(T_b - 1, t + 2) (truncated, not zero-padded).
 * u, x [B][Lstride] f32 with lengths [B] int32 (the CALLER checks 255 < L_b <= Lstride and T_b <= Tmax);
 * energies: a workspace of B * 2 * Tmax doubles (E_u, E_x per row); gains [B][Tmax] f32, zero from T_b on.  The
 * DFT, the energies and the ratios are fp64 in a fixed order, the result is rounded to fp32 once; two launches on
 * the stream, no host synchronisation. */
int snrse_resample_mix(const float* x, const float* u, const int* len16, long long stride16, const float* y,
                       const int* lenR, long long strideR, int B, int up, int down, int half, const float* taps,
                       const float* gains, const int* frames, int Tmax, float gain_const, float* out,
                       hipStream_t stream);
int snrse_band_gain(const float* u, const float* x, const int* lengths, int B, int Lstride, int Tmax,
                    double floor_gain, double* energies, float* gains, hipStream_t stream);

/* Recordings of any length (csrc/window.hip, snrse/longform.py): a recording is cut into overlapping windows of W
 * samples, the windows run as rows of the batched enhancers, and their results are joined by a cross-fade over the
 * first V samples of every window of a recording but its first.
 *
 * snrse_window_gather: src [R][stride] f32 ragged with lengths [R] int32 on the device; table [nwin][3] int32 on the
 * device = (source row, start, length <= W) per window -> out [nwin][W] f32, out[j][i] = src[row_j][start_j + i]
 * for i < length_j and start_j + i < L_row, zero otherwise.  Nothing at or past a source row's length is read, and a
 * table entry that names no row of src gives a row of zeros.
 *
 * snrse_window_merge: win [nwin][W] f32, starts [nwin] int32 (sample at which each window begins in its recording),
 * silent [nwin] uint8, first [R + 1] int32 (recording r owns the windows first[r] .. first[r + 1] - 1, whose starts
 * ascend from 0), lengths [R] int32, fade [V] f32 = sin^2(pi (i + 1/2) / (2 V)), all on the device -> out
 * [R][stride_out] f32.  For sample n < L_r, with k the last window of r whose start s_k <= n and i = n - s_k:
 *   k is not r's first window and i < V:  out = fma(fade[i], x_k[i], (1 - fade[i]) * x_{k-1}[n - s_{k-1}])
 *   otherwise:                            out = x_k[i]
 * where x_j[.] is win[j][.], or 0 without reading it when silent[j] is set.  What a window holds past the next
 * one's fade is never read; samples [L_r, stride_out) are written as zero; a one-window recording is a copy.  One
 * thread per output sample and one fixed fp32 expression: no atomics, the same bits on every launch and for a
 * recording launched alone.  The CALLER sees to windows that cover their recording (each gap <= W - V); a sample
 * no window covers is written as zero.
 *
 * Both return hipErrorInvalidValue before any HIP call for a NULL pointer or a size <= 0; the merge also for
 * 4 V > W. */
int snrse_window_gather(const float* src, const int* lengths, int R, long long stride, const int* table, int nwin,
                        int W, float* out, hipStream_t stream);
int snrse_window_merge(const float* win, int nwin, int W, const int* starts, const unsigned char* silent,
                       const int* first, const int* lengths, int R, const float* fade, int V, float* out,
                       long long stride_out, hipStream_t stream);

/* ESTOI, the extended short-time objective intelligibility measure (Jensen & Taal 2016 with pystoi's conventions;
 * csrc/estoi.hip), of a ragged batch: x clean and y processed, [B][stride] f32 at 10 kHz, lengths [B] int32 on the
 * device (clamped to [0, stride]) -> out [B] f64 and info [B][2] int32 = (K, S).  For one row of length L, with the
 * window w[n] = 0.5 (1 - cos(2 pi (n + 1) / 257)), n = 0..255, and eps = 2^-52:
 *   1. frames i = 0..nf-1 start at 128 i for every i with 128 i < L - 256: nf = max(0, ceil((L - 256) / 128)), a
 *      frame that would end exactly at L is not taken.  e_i = 20 log10(|w x[128 i : 128 i + 256]|_2 + eps); frame i is
 *      kept iff e_i > max_i e_i - 40.  x alone decides, the same frames are kept in y: K frames f_0 < ... < f_{K-1}.
 *   2. the kept frames are windowed and overlap-added at hop 128 into x' of 128 (K - 1) + 256 samples, and x' is framed
 *      again by the rule of 1: M = K - 1 frames, X[:, j] = rfft(w x'[128 j : 128 j + 256], 512).  The same for y.
 *   3. M < 30: out = 1e-5, S = 0.
 *   4. 15 third-octave bands, centres 150 2^(k/3) Hz, edges the geometric means of neighbouring centres snapped to
 *      the nearest bin: [7,9) [9,11) [11,14) [14,17) [17,22) [22,27) [27,34) [34,43) [43,55) [55,69) [69,87) [87,109)
 *      [109,138) [138,174) [174,219).  Xb[k][j] = sqrt(sum over the bins of band k of |X[bin][j]|^2).
 *   5. segments m = 0..S-1, S = M - 29: the 15 x 30 block Xb[:, m : m + 30] has each row's mean (over its 30 frames)
 *      subtracted and is divided by (the row's L2 norm + eps), then each column's mean (over the 15 bands) subtracted
 *      and divided by (the column's L2 norm + eps); the same for Yb; out = sum over m, k, j of the products / (30 S).
 * The energies, the keep decision and step 5 are fp64; the spectra are fp32.  An all-zero row gives 0.0 with every
 * frame kept.  Nothing at or past L of a row is read into a result.  No floating-point atomics: a row's bits are the
 * same on every launch, launched alone, and under any permutation of the batch.  Five launches whatever B is, no
 * host synchronisation.  work: work_bytes >= the workspace size of (B, stride) bytes of device memory, 256-byte
 * aligned; snrse_estoi_workspace gives 0, no valid size, for B <= 0 or stride <= 0.  EINVAL, before any HIP call, for
 * B <= 0, stride <= 0, a NULL pointer or a short workspace.
 * snrse_estoi_block: re-framed frames per workgroup of the spectrum kernel (where the kernel changes block). */
int snrse_estoi(const float* x, const float* y, const int* lengths, int B, long long stride, void* work,
                size_t work_bytes, double* out, int* info, hipStream_t stream);
size_t snrse_estoi_workspace(int B, long long stride);
int snrse_estoi_block(void);

/* Programme loudness, ITU-R BS.1770-4 integrated loudness of ragged batches (csrc/loudness.hip, snrse/loudness.py).
 *
 * K-weighting for a sample rate fs: the standard's analog prototype re-discretised per rate (at 48 kHz the
 * standard's table to 1e-13).  With K = tan(pi f0 / fs) and a0 = 1 + K / Q + K^2:
 *   shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196,
 *              Vh = 10^(G / 20), Vb = Vh^0.4996667741545416,
 *              b = [(Vh + Vb K / Q + K^2) / a0, 2 (K^2 - Vh) / a0, (Vh - Vb K / Q + K^2) / a0]
 *              a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
 *   high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773,
 *              b = [1, -2, 1], a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
 * computed by the host in float64 (snrse.loudness.kweighting) and handed over as doubles.  z = HP(shelf(x)), both
 * biquads in transposed direct form II from a zero state; the samples are read as f32, everything after is f64.
 *
 * Blocks.  n100 = (fs + 5) / 10 samples (integer division).  Sub-block i of a row of length L is
 * s_i = sum of z[n]^2 over n in [i n100, (i + 1) n100), for i < nsub = L / n100; the tail of fewer than n100 samples
 * is not used.  Block j of a FILE (a set of rows: its channels) is
 *   e_j = sum over its rows of (s_j + s_{j+1} + s_{j+2} + s_{j+3}) / (4 n100),   j <= nsub - 4,
 * 400 ms at a hop of 100 ms, every channel with weight 1 (the files carry no channel layout; the standard's 1.41 for
 * surround channels is not applied).  l_j = -0.691 + 10 log10(e_j).
 * Gates.  Keep j with l_j > -70; Gamma = -0.691 + 10 log10(mean of e_j over the kept) - 10; the integrated loudness
 * I = -0.691 + 10 log10(mean of e_j over the kept with l_j > Gamma).  No block (nsub < 4) or none kept: I = -inf.
 *
 * snrse_kweight_sums: x [B][stride] f32 with lengths [B] int32 on the device; params [B][42] f64 per row = the ten
 * coefficients (shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2), then A^C and A^(C S) row-major 4 x 4, A the
 * zero-input transition of one sample on the state (shelf w1, w2, high-pass w1, w2), C = snrse_kweight_chunk()
 * and S = snrse_kweight_group(); n100 [B] int32 (rows of different rates share the launches; a row with
 * n100 < C has no sub-block) -> sums [B][Nmax] f64, s_i for i < min(nsub_b, Nmax) and 0 from there on.  A row is cut
 * into chunks of C samples: every chunk's zero-state final state, a scan s_{k+1} = A^C s_k + f_k over the row in
 * groups of S chunks, then every chunk again from its exact state -- the recurrence's own values, no run-in -- with
 * z^2 summed into the (at most two) sub-blocks it touches; one wave per sub-block adds the chunks' partials in a
 * fixed order.  The filtered signal is never stored.  snrse_kweight_block() chunks share a workgroup, which stages
 * their samples in LDS.  No floating-point atomics: a row's bits do not depend on the batch, the row's place in
 * it or the launch.  Nothing at or past L_b is read; L_b = 0 is allowed.  work: snrse_kweight_workspace(B, stride)
 * bytes of device memory, 256-byte aligned (0, no valid size, for B <= 0, stride <= 0 or stride >= 2^31).  Six
 * launches, no host synchronisation.  EINVAL before any HIP call for a NULL pointer, a size <= 0, x not 4-byte
 * aligned or a short workspace.
 *
 * snrse_loudness_gate: sums [B][Nmax], nsub [B] (clamped to [0, Nmax]), n100 [B], group [B] int32 = the file of
 * each row, in [0, G); the rows of a file are adjacent and share one rate, a file has the fewest sub-blocks of its
 * rows -> per file lufs [G] f64 = I, counts [G][3] int32 = blocks, blocks kept by the absolute gate, blocks kept by
 * the relative gate, margin [G] f64 = the smallest |l_j - gate| in LU over every comparison made (l_j with -70, and
 * the blocks above -70 with Gamma; +inf when no comparison was made), which shows a decision that rested on
 * rounding.  One workgroup per file, fp64, sums in a fixed order, no host synchronisation.
 *
 * snrse_peak_oversampled: out [B] f32 = max |y[m]| over m in [0, up L_b) of y = snrse_resample_poly(x, up, down = 1)
 * with the same taps layout ([up][K]) and the same fp32 fma chain over j ascending, so the value has the bits of the
 * maximum of that entry's output, which is never written here; 0 for L_b = 0.  A NaN output is skipped, by
 * snrse_absmax's rule.  The host calls it with up = 4 and the resampler's default 81-tap filter: a 4x oversampled
 * peak, NOT the 48-tap filter of BS.1770 Annex 2, hence no "dBTP".
 *
 * snrse_gain_to_pcm16: q [B][stride] int16 = clip(rint(fl32(fl32(gain[b]) x) 32768), -32768, 32767), rint to even:
 * what a 16-bit wav writer makes of the f32 product; f (may be NULL) [B][stride] f32 = that product.  gain [B] f64
 * on the device; both outputs are zero from L_b on. */
int snrse_kweight_sums(const float* x, const int* lengths, int B, long long stride, const double* params,
                       const int* n100, void* work, size_t work_bytes, double* sums, int Nmax, hipStream_t stream);
size_t snrse_kweight_workspace(int B, long long stride);
int snrse_kweight_chunk(void);
int snrse_kweight_block(void);
int snrse_kweight_group(void);
int snrse_loudness_gate(const double* sums, int Nmax, const int* nsub, const int* n100, const int* group, int B, int G,
                        double* lufs, int* counts, double* margin, hipStream_t stream);
int snrse_peak_oversampled(const float* x, const int* lengths, int B, long long stride, int up, int half,
                           const float* taps, float* out, hipStream_t stream);
int snrse_gain_to_pcm16(const float* x, const int* lengths, int B, long long stride, const double* gain, short* q,
                        float* f, hipStream_t stream);

/* Range statistics of a contiguous tensor [B][per] (dtype SNRSE_F32 / SNRSE_F16 / SNRSE_BF16; a complex64
 * spectrogram is 2*per floats): peak[b] = max |v| over the FINITE elements of row b (0 when there is none),
 * nonfinite[b] = number of inf / NaN elements of row b (saturating at INT_MAX).  accumulate == 0: overwrite
 * peak / nonfinite; != 0: fold into their contents (max / saturating add), so a series of tensors can be folded
 * into one slot without host work.  What the fp16 range guard (snrse/guard.py: one call per enhancement on the
 * returned spectrogram) and the range probe (NCSNppHIP.range_report: every stored tensor of one evaluation)
 * run; the GroupNorm statistics of the GEMM epilogues are taken before the 16-bit pack and stay finite when the
 * stored value is +-inf.  csrc/range.hip. */
int snrse_range_stats(const void* src, int B, long long per, int dtype, float* peak, int* nonfinite,
                      int accumulate, hipStream_t stream);

/* ---- Stage kernels of the per-row adaptive RK45 (snrse/ode.py rk45_solve_rows; csrc/ode.hip).  Every row of a
 * [B][n] float64 state (a complex128 state is n = 2 x elements doubles, pairs of reals) integrates with its own
 * step h[b]; the controller stays on the host.  fp64 arithmetic without fma contraction: each product and sum
 * rounds as numpy's and torch's do.  k / v: HOST arrays of ns <= 7 device pointers to stage tensors [B][n] of
 * kdtype SNRSE_F32 (promoted in the load) or SNRSE_F64, c: HOST array of their ns coefficients (the caller drops
 * zero coefficients; ns = 0 is a zero sum); both are copied into the launch.  Every tensor's base address must be
 * 16-B aligned.  The results are the same bits on every launch (no floating-point atomics). */

/* out[b][e] = y[b][e] + h[b] * (c_0 K_0[b][e] + c_1 K_1[b][e] + ...), summed in stage order; out32 (may be NULL):
 * the float32 cast of out.  h [B] float64 on the device. */
int snrse_rk45_combine(const double* y, const double* h, const void* const* k, const double* c, int ns, int kdtype,
                       int B, long long n, double* out, float* out32, hipStream_t stream);

/* out[b] = sqrt(mean_e |m[b] * sum_s c_s V_s[b][e]|^2 / (atol + rtol * max(|a[b][e]|, |b2[b][e]|))^2), |.| the
 * complex modulus over pairs when cplx (n even) -- the error norm of a step (V = K, c = E, m = h, a = y,
 * b2 = y_new) and the three norms of the initial step (b2 = a = y0, m NULL = 1).  Two passes: block partials
 * partial [B][snrse_rk45_rownorm_blocks(B, n)] float64, then a fold in block order. */
int snrse_rk45_rownorm(const void* const* v, const double* c, int ns, int vdtype, const double* m, const double* a,
                       const double* b2, double rtol, double atol, int cplx, int B, long long n, double* partial,
                       double* out, hipStream_t stream);
int snrse_rk45_rownorm_blocks(int B, long long n);

/* Rows with mask[b] != 0 (int32 [B], device): y[b] <- y_new[b] (ywords 32-bit words per row) and
 * f[b] <- f_new[b] (fwords); every other row keeps its bits. */
int snrse_rk45_accept(const int* mask, void* y, const void* y_new, long long ywords, void* f, const void* f_new,
                      long long fwords, int B, hipStream_t stream);

/* STFT (data_module.py:291-293 with spec_fwd 241-254 and pad_spec other.py:83-90):
 * sig [B][L] f32 -> out complex64 [B][256][Tpad], frames 1 + L/128 (the rest zero).
 * mode 0 raw, 1 exponent transform (|X|^0.5 e^{i angle X} * 0.15).  The signal is scaled by
 * in_scale / in_div[b] (in_div: per-utterance norm factors on the device, or NULL). */
int snrse_stft(const float* sig, int B, int L, const float* in_div, float in_scale, int Tpad, int mode,
               void* out, hipStream_t stream);

/* iSTFT (data_module.py:295-297 with spec_back 256-267): spec complex64 [B][256][T] -> out [B][L]
 * f32, times out_scale[b] (NULL = 1).  frames: workspace of B*T*510 floats. */
int snrse_istft(const void* spec, int B, int T, int L, int mode, const float* out_scale, float* frames,
                float* out, hipStream_t stream);

/* Exponent spectrogram transform on interleaved complex64 (data_module.py:241-267):
 * dir 0 = spec_fwd (|c|^0.5 e^{i angle c} * 0.15), dir 1 = spec_back (inverse).  In place allowed. */
int snrse_spec_transform(const void* in, void* out, long long n, int dir, hipStream_t stream);

/* SNR estimator SNRNet.forward (snrnet.py:47-97) on the raw complex STFT spec [B][256][T]
 * (T % 16 == 0): out[b] = sigmoid(...) in (0, 1).  Weights f32 in torch layouts (see
 * csrc/snrnet.hip); ws: workspace of snrse_snrnet_workspace(B, T) bytes. */
int snrse_snrnet(const void* spec, int B, int T, const float* w5, const float* b5, const float* w3,
                 const float* b3, const float* wt1, const float* wt2, const float* wt3, const float* wt4,
                 const float* bt1, const float* bt2, const float* bt3, const float* bt4, const float* wih,
                 const float* bsum, const float* whh, const float* fcw, const float* fcb, float* ws,
                 float* out, hipStream_t stream);
size_t snrse_snrnet_workspace(int B, int T);

/* ---- Training of the SNR estimator (snr_estimator.py:81-116 around SNRNet; csrc/snrnet_train.hip), f32.
 * T % 16 == 0 and T >= 32 (one chunk makes the unbiased std over the chunks, and the loss, NaN). */

/* Batch perturbation (snr_estimator.py:93-98) on interleaved complex64 [B][per]:
 * out = (x + (y - x) 0.56234 SNR) 2.040166 / sqrt(1 + SNR^2), SNR = gt[b] / (1 - gt[b]). */
int snrse_snr_perturb(const void* x, const void* y, const float* gt, int B, long long per, void* out,
                      hipStream_t stream);
/* snrse_snrnet that also saves what the backward needs (pool winners, LSTM gates and cell states, the head's
 * argmin / argmax) in tws, snrse_snrnet_train_workspace(B, T) bytes kept by the caller until the backward. */
int snrse_snrnet_train_fwd(const void* spec, int B, int T, const float* w5, const float* b5, const float* w3,
                           const float* b3, const float* wt1, const float* wt2, const float* wt3, const float* wt4,
                           const float* bt1, const float* bt2, const float* bt3, const float* bt4, const float* wih,
                           const float* bsum, const float* whh, const float* fcw, const float* fcb, void* tws,
                           float* out, hipStream_t stream);
size_t snrse_snrnet_train_workspace(int B, int T);
/* est [B]: the forward's output; dest [B]: d loss / d est.  Gradients in the layout of the packed weights
 * (dwih / dwhh [2][512][128]; dbsum [2][512] is the gradient of bias_ih and of bias_hh alike). */
int snrse_snrnet_backward(const void* spec, int B, int T, const float* est, const float* dest, const float* w3,
                          const float* wt1, const float* wt2, const float* wt3, const float* wt4, const float* wih,
                          const float* whh, const float* fcw, void* tws, float* dw5, float* db5, float* dw3,
                          float* db3, float* dwt1, float* dwt2, float* dwt3, float* dwt4, float* dbt1, float* dbt2,
                          float* dbt3, float* dbt4, float* dwih, float* dbsum, float* dwhh, float* dfcw, float* dfcb,
                          hipStream_t stream);

/* ---- Consistency-training step (ScoreModel._step, model.py:361-390, with the
 * backward pass PyTorch Lightning runs through loss.backward() and the Adam / torch_ema updates of
 * model.py:99-106).  All f32, NHWC activations; csrc/train.hip. */

/* dW[co][ky][kx][ci] += sum_p dY[p][co] X[p + (ky-1, kx-1)][ci] (ksize 3, pad 1) or the 1x1 form;
 * X is the channel concatenation of x0 [.., C0] and x1 [.., C1] (C0 > 0; C1 >= 0, x1 NULL only when C1 == 0).
 * dw [Cout][ksize*ksize][C0+C1] is accumulated into (+=, atomics): the caller zeroes it for a plain gradient.
 * Every entry of this section returns hipErrorInvalidValue, before any HIP call, for a NULL required pointer,
 * a count <= 0 (C1 < 0) or anything else its comment rules out (ksize other than 1 or 3 here). */
int snrse_conv_wgrad(const float* dy, int Cout, const float* x0, int C0, const float* x1, int C1, int B, int H,
                     int W, int ksize, float* dw, hipStream_t stream);
/* The same with split-bf16 products (fp32 in and out; dY and X split into bf16 hi / lo, three bf16 MFMA
 * products per block): the fp32x3 training mode.  Cout, C0, C1 multiples of 4 (16-byte vector loads of both
 * images; anything else is hipErrorInvalidValue). */
int snrse_conv_wgrad_x3(const float* dy, int Cout, const float* x0, int C0, const float* x1, int C1, int B, int H,
                        int W, int ksize, float* dw, hipStream_t stream);
/* scale * per-(b, c) sums over the HW pixels of x [B][HW][C] added into out_bc [B][C] and / or the
 * per-c total into out_c [C] (bias, Dense_0 and temb gradients).  Both outputs are added into (+=); at least
 * one of them is non-NULL. */
int snrse_chan_sum(const float* x, int B, int HW, int C, float* out_bc, float* out_c, float scale,
                   hipStream_t stream);
/* per-(b, group) mean and rstd = 1/sqrt(var + eps) from the slotted (sum, sumsq) statistics of the
 * forward GroupNorm (snrse_gn_stats) of one or two channel-concatenated sources: mean, rstd [B][groups]
 * (the variance is clamped at 0 before eps is added).  C0 > 0, C1 >= 0 (st1 NULL only when C1 == 0), HW > 0,
 * groups > 0 dividing C0 + C1, mean and rstd non-NULL. */
int snrse_gn_moments(const double* st0, int C0, const double* st1, int C1, int B, int HW, int groups, float eps,
                     float* mean, float* rstd, hipStream_t stream);
/* GroupNorm (+SiLU when act) backward (nn.GroupNorm layerspp.py:221,233; SiLU layers.py:38-39):
 * dy [B][HW][C0+C1] -> dx0 [B][HW][C0], dx1 [B][HW][C1]; dgamma / dbeta [C] accumulated (+=);
 * R: workspace of 2*B*(C0+C1) floats.  C0 > 0, C1 >= 0 (x1 and dx1 NULL only when C1 == 0), HW > 0, groups > 0
 * dividing C0 + C1; gamma, beta, mean, rstd non-NULL; dgamma and dbeta may each be NULL (not computed). */
int snrse_gn_backward(const float* x0, int C0, const float* x1, int C1, const float* dy, int B, int HW,
                      int groups, const float* gamma, const float* beta, const float* mean, const float* rstd,
                      int act, float* R, float* dx0, float* dx1, float* dgamma, float* dbeta, hipStream_t stream);
/* batched strided GEMM on MFMA: C[b](m,n) = alpha sum_k A[b](m,k) B[b](k,n) + beta C[b](m,n) (+ bias[n]),
 * element (i, j) of operand X at X + b*sXb + i*sX(row) + j*sX(col).  Any beta is supported; with beta == 0
 * C is written without being read (it may hold NaN).  bias may be NULL; it is added after alpha, not scaled by
 * it, and does not depend on beta.  The edges M, N % 64 and K % 16 are handled. */
int snrse_bgemm(const float* A, long long sAb, long long sAm, long long sAk, const float* Bm, long long sBb,
                long long sBk, long long sBn, float* C, long long sCb, long long sCm, long long sCn, const float* bias,
                int batch, int M, int N, int K, float alpha, float beta, hipStream_t stream);
/* row softmax P = softmax(scale S) and its backward dS = scale P (dP - <dP, P>_row), rows of L. */
int snrse_softmax_rows(const float* S, float* P, long long rows, int L, float scale, hipStream_t stream);
int snrse_softmax_bwd_rows(const float* P, const float* dP, float* dS, long long rows, int L, float scale,
                           hipStream_t stream);
/* elementwise: y = silu(x); dx (+)= dy silu'(x); y = a x + b y (b == 0: y is written without being read, so it
 * may be uninitialised; x may alias y); y = x * s[b] (recip: x / s[b]). */
int snrse_silu(const float* x, float* y, long long n, hipStream_t stream);
int snrse_silu_bwd(const float* x, const float* dy, float* dx, long long n, int accumulate, hipStream_t stream);
int snrse_axpby(const float* x, float* y, long long n, float a, float b, hipStream_t stream);
int snrse_scale_rows(const float* x, const float* s, float* y, int B, long long per, int recip, hipStream_t stream);
/* GaussianFourierProjection of log t (layerspp.py:32-43): out [B][2 nf] = [sin, cos](2 pi log t W). */
int snrse_gfp(const float* t, const float* Wg, int B, int nf, float* out, hipStream_t stream);
/* perturbation of the consistency step on complex64 [B][HW]: mu = H(H^-1(x)(1 - w_b) + H^-1(y) w_b),
 * x_t = mu + s_b z (H = exponent transform when transform != 0, model.py:304-312, 372-376); H(0) = 0. */
int snrse_ct_perturb(const void* x, const void* y, const void* z, const float* wmix, const float* nscale, int B,
                     int HW, int transform, void* mu, void* xt, hipStream_t stream);
/* sebridge_v3 outputs f_k = cs_k x_k + co_k dnn_k (coef [B][4] = cs1, co1, cs0, co0), the mse
 * (sqrt_loss = 0) or sqrt_mse (1) consistency loss per utterance into loss_b [B] (f64, the batch loss
 * is their mean), and its gradient w.r.t. dnn1 / dnn0 (complex64 [B][HW]; HW % 64 == 0, so that a wave never
 * spans two utterances: anything else is hipErrorInvalidValue).  sqrt_mse: where f_k is exactly 0 the
 * gradient through s(f_k) is taken as 0. */
int snrse_ct_loss(const void* dnn1, const void* dnn0, const void* x1, const void* x0, const float* coef, int B,
                  int HW, int sqrt_loss, double* loss_b, void* g1, void* g0, hipStream_t stream);
/* one torch.optim.Adam step (+ torch_ema update when a tensor's ema pointer is set) over a table of
 * device tensors {float* p, const float* g, float* m, float* v, float* ema, int64 n} (device memory),
 * split into chunks of 2048 elements (chunk_tensor / chunk_start, device arrays of nchunks). */
int snrse_adam_ema(const void* tensors, const int* chunk_tensor, const long long* chunk_start, int nchunks,
                   float lr, float beta1, float beta2, float eps, float bias_corr1, float bias_corr2_sqrt,
                   float ema_decay, hipStream_t stream);
/* The step with torch.nn.utils.clip_grad_norm_(norm_type = 2) and a gradient scale, without a host read-back:
 * snrse_grad_sumsq writes partial[chunk] = sum g^2 (f64) for the chunks of a tensor table (a NULL g counts 0);
 * snrse_grad_clip_coef folds npartials of them in a fixed order (bit-stable, no atomics) into
 * out[0] = total_norm = accum_scale sqrt(sum) and out[1] = gscale = accum_scale min(1, max_norm /
 * (total_norm + 1e-6)) (max_norm <= 0: no clipping, gscale = accum_scale); snrse_adam_ema_scaled is
 * snrse_adam_ema with every gradient element multiplied by *gscale (device memory) first. */
int snrse_grad_sumsq(const void* tensors, const int* chunk_tensor, const long long* chunk_start, int nchunks,
                     double* partial, hipStream_t stream);
int snrse_grad_clip_coef(const double* partial, int npartials, float max_norm, float accum_scale, float* out,
                         hipStream_t stream);
int snrse_adam_ema_scaled(const void* tensors, const int* chunk_tensor, const long long* chunk_start, int nchunks,
                          float lr, float beta1, float beta2, float eps, float bias_corr1, float bias_corr2_sqrt,
                          float ema_decay, const float* gscale, hipStream_t stream);
/* Multi-tensor gradient pack for the data-parallel all-reduce: over the same tensor table and chunk list,
 * flat[flat_off[t] + i] = g_t[i] * scale for every element of every tensor t, one launch, one block per chunk (a
 * NULL g writes zeros).  flat_off (device array, one entry per table row) holds each tensor's first element in
 * flat and must be a multiple of 4 elements with flat itself 16-B aligned; elements of flat between the tensors
 * are not written.  Stores are 16 B wide, loads too when the gradient's base is 16-B aligned; plain vector
 * stores, no atomics.  hipErrorInvalidValue before any HIP call for nchunks < 0, a scale that is not finite or
 * not > 0, or a NULL tensors / chunk_tensor / chunk_start / flat_off / flat with nchunks > 0; nchunks == 0 is a
 * no-op that returns success. */
int snrse_grad_pack(const void* tensors, const int* chunk_tensor, const long long* chunk_start, int nchunks,
                    const long long* flat_off, float scale, float* flat, hipStream_t stream);

/* ---- Fixed-SNR dataset preparation (snrse.snrize; csrc/snrize.hip): active-level analysis of a clean / noise
 * pair and its remix to a target active SNR.  Ragged batches: c, n [B][stride] f32 with lengths [B] (clamped to
 * [0, stride] on the device; nothing at or past a row's length is read).  Windows of W samples, non-overlapping
 * from sample 0, the last one possibly partial (its mean is over its true length); nWmax = ceil(stride / W).
 * Window k of a row is active iff sqrt(mean n_k^2) > 10^(-50/20) (max |n| + eps), eps = 2^-52: by the noise alone.
 * No f64 atomics and a fixed order of every sum: a row's results are the same bits whichever rows share its launch
 * and however its buffer is aligned.  Every entry returns hipErrorInvalidValue, before any HIP call, for a NULL
 * required pointer, B, stride or W <= 0, stride >= 2^31 or a float pointer that is not 4-B aligned. */

/* wsums [B][nWmax][2] f64 = (sum c^2, sum n^2) of every window a row has (the others are left unwritten);
 * partials [B][ceil(nWmax / P)][5] f64 = (sum c, sum n, sum c^2, sum n^2, sum c n) over each block's P windows,
 * P = snrse_active_windows_per_block(); nmax [B] f32 = max |n| of the row. */
int snrse_active_window_sums(const float* c, const float* n, const int* lengths, int B, long long stride, int W,
                             double* wsums, double* partials, float* nmax, hipStream_t stream);
int snrse_active_windows_per_block(void);
/* From those three: out [B][5] f64 = clean_rms, noise_rms (sqrt of the sum over the active windows / their sample
 * count, windows in ascending order; both eps when no window is active), the number of active windows, the Pearson
 * coefficient of c and n over the whole row (0 when either has no variance) and the gain
 * g = clean_rms / noise_rms * 10^(-snr_db[b] / 20) that brings the pair to snr_db[b] dB active SNR. */
int snrse_active_finalize(const double* wsums, const double* partials, const float* nmax, const int* lengths, int B,
                          long long stride, int W, const double* snr_db, double* out, hipStream_t stream);
/* n_out = gf n and y_out = fma(gf, n, c) with gf = (float)gain[b * gain_stride] (y_out is the once-rounded
 * gf n + c, not c + n_out rounded again), both [B][stride] f32 and zero from the row's length on;
 * ymax [B] f32 = max |y_out| of the row. */
int snrse_snr_mix(const float* c, const float* n, const int* lengths, int B, long long stride, const double* gain,
                  int gain_stride, float* n_out, float* y_out, float* ymax, hipStream_t stream);
/* Clip guard and 16-bit output: scale[b] = ymax[b] > 0.99 ? (0.99 - eps) / ymax[b] : 1 (f64, computed on the
 * device); each of c, n1, y times (float)scale[b] into c_f, n_f, y_f (f32; may alias their inputs) and, of those
 * products x, clip(round_half_even(32768 x), -32768, 32767) into c_q, n_q, y_q (int16).  Any of the six outputs
 * may be NULL; all are [B][stride] and zero from the row's length on. */
int snrse_scale_to_pcm16(const float* c, const float* n1, const float* y, const int* lengths, int B, long long stride,
                         const float* ymax, float* c_f, float* n_f, float* y_f, short* c_q, short* n_q, short* y_q,
                         double* scale, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SNRSE_H_ */
