/* C-ABI of libditsep_hip.so -- MI355X (gfx950) latent-diffusion separation engine.
 *
 * Drop-in boundary for the hot path of eduardburlacu/DiTSep:
 *   LatentDiffSep.separate()            reference src/diffsep_latent.py:471-487
 *   LatentDiffSep.get_pc_sampler()      reference src/diffsep_latent.py:406-469
 *     -> sdes.get_pc_sampler()          reference src/sdes/__init__.py:133-193
 *   LatentDiffSep.forward (score net)   reference src/diffsep_latent.py:147-148
 *   LatentDiffSep.encode / decode       reference src/diffsep_latent.py:107-128
 *
 * Conventions: plain pointers and sizes only; every data pointer is a DEVICE
 * pointer owned by the caller (fp32, contiguous, the reference's own tensor
 * layouts) unless a parameter says host; `stream` is a hipStream_t passed as
 * void* (NULL = default stream).  Functions return 0 on success, a negative
 * DSN_E* code on failure (message via dsn_last_error); no exceptions cross the
 * boundary.  One context per device; a context is not re-entrant.
 */
#ifndef DITSEP_HIP_H
#define DITSEP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSN_OK 0
#define DSN_EINVAL (-1)   /* bad argument / shape                                  */
#define DSN_EHIP (-2)     /* HIP runtime error                                     */
#define DSN_ESTATE (-3)   /* weights missing / not finalized                       */
#define DSN_ENOMEM (-4)
#define DSN_ESOLVER (-5)  /* dsn_ode_sample: step size underflow or attempt limit      */

#define DSN_PREC_BF16 1    /* bf16 MFMA operands, fp32 accumulate                  */
#define DSN_PREC_BF16X3 2  /* split-bf16 (hi,lo) operands: 3 bf16 MFMAs per product */
#define DSN_PREC_FP16 3    /* fp16 MFMA operands (11-bit mantissa), fp32 accumulate */
#define DSN_PREC_FP16X3 4  /* split-fp16 (hi,lo) operands: 3 fp16 MFMAs per product */
#define DSN_PREC_FP8 5     /* BASELINE config 5: the DiT layer GEMMs (to_qkv, to_out, FF in/out) on fp8 e4m3 operands
                              with E8M0 block scales per 32 K-elements (v_mfma_scale_f32_16x16x128_f8f6f4, fp32
                              accumulate); everything else as DSN_PREC_FP16.  A throughput mode: e4m3 operand rounding
                              (2^-4) cannot meet the 1e-3 waveform bound, its deviation is reported, not hidden. */

#define DSN_SCORE_NONE 0
#define DSN_SCORE_DIT 1    /* reference src/stable_audio_tools/models/dit.py:12-244  */
#define DSN_SCORE_NCSNPP 2 /* reference src/models/diffsep/score_models.py:140-186   */

#define DSN_MAX_VAE_BLOCKS 8

typedef struct dsn_ctx dsn_ctx;

typedef struct dsn_config {
  int32_t device;
  int32_t precision;   /* DSN_PREC_*                                               */
  int32_t n_src;       /* config.model.n_speakers                                  */
  int32_t latent_dim;  /* VAE latent channels (64)                                 */
  /* score network */
  int32_t score_kind;  /* DSN_SCORE_*                                              */
  int32_t dit_embed_dim, dit_depth, dit_heads;
  /* NCSN++ latent score network (config.model.score_model.backbone_args, default.yaml:16-28) */
  int32_t ncsn_nf, ncsn_n_levels;
  int32_t ncsn_ch_mult[4];
  int32_t ncsn_num_res_blocks, ncsn_attn_resolution, ncsn_image_size, ncsn_max_latent_length;
  /* Oobleck VAE (oobleck_finetune.json keys) */
  int32_t vae_channels;
  int32_t vae_n_blocks;                       /* len(c_mults) == len(strides)      */
  int32_t vae_c_mults[DSN_MAX_VAE_BLOCKS];
  int32_t vae_strides[DSN_MAX_VAE_BLOCKS];
  int32_t vae_enc_latent_dim;                 /* encoder out channels (2*latent)   */
  int32_t vae_use_snake, vae_final_tanh;
  int32_t vae_has_encoder, vae_has_decoder;
  /* OUVE SDE (config.model.sde) */
  float sde_theta, sde_sigma_min, sde_sigma_max;
} dsn_config;

/* lifecycle */
dsn_ctx* dsn_create(const dsn_config* cfg);
void dsn_destroy(dsn_ctx* ctx);
const char* dsn_last_error(const dsn_ctx* ctx);   /* ctx may be NULL after a failed dsn_create */

/* Weights: one call per state_dict entry, reference key names and layouts
 * (Lightning checkpoint `state_dict`: `score_model.*`, `vae.decoder.*`,
 * `vae.encoder.*`; old-style weight norm `weight_g` / `weight_v`;
 * reference src/diffsep_latent.py:341-392).  `data` is fp32; is_device != 0 when it
 * is a device pointer.  dsn_finalize_weights folds weight norm, transposes to the
 * K-major packed MFMA layout and splits into bf16 planes, on the GPU. */
int dsn_load_tensor(dsn_ctx* ctx, const char* name, const float* data, const int64_t* shape, int ndim,
                    int is_device);
int dsn_finalize_weights(dsn_ctx* ctx);
/* strict != 0 (what dsn_finalize_weights does): besides a missing tensor, any loaded tensor the configured network
 * does not consume is an error (DSN_ESTATE, the names in dsn_last_error) -- nn.Module.load_state_dict(strict=True)
 * semantics; known module buffers (`*.inv_freq`, `*.num_batches_tracked`) are ignored.  strict == 0 drops them. */
int dsn_finalize_weights_ex(dsn_ctx* ctx, int strict);

/* score = score_model(xt, time_cond, mix)      (LatentDiffSep.forward)
 * xt [B,n_src,D,T], t [B], mix [B,1,D,T] -> out [B,n_src,D,T] */
int dsn_score(dsn_ctx* ctx, const float* xt, const float* t, const float* mix, float* out, int B, int T,
              void* stream);

/* OUVE schedule scalars exactly as the sampler uses them (host arrays of N floats each;
 * any output pointer may be NULL).  timesteps = linspace(1, t_eps, N). */
int dsn_ouve_schedule(const dsn_ctx* ctx, int N, float t_eps, float snr, float* timesteps, float* std,
                      float* corr_step, float* corr_gain, float* G, float* std_T);

/* pc_sampler() of sdes.get_pc_sampler("reverse_diffusion", "ald", ...):
 * y [B,1,D,T] -> x_out [B,n_src,D,T]; nfe_out (host) = N*(corrector_steps+1).
 * noise: [1 + N*(corrector_steps+1), B, n_src, D, T] standard normals in the reference's
 * draw order (prior, then per step corrector draws, predictor draw), or NULL to draw
 * on-device (Philox4x32-10, `seed`). */
int dsn_pc_sample(dsn_ctx* ctx, const float* y, const float* noise, uint64_t seed, float* x_out, int B, int T,
                  int N, int corrector_steps, float snr, float t_eps, int denoise, int* nfe_out, void* stream);

/* pc_sampler() of sdes.get_pc_scheduled_sampler (src/sdes/__init__.py:49-130): as dsn_pc_sample with
 * caller-provided timesteps (host array, N entries used: the first N of the reference's N+1-point
 * linear / log / revlog grid).  State shape is [B,n_src,D,T] (the reference samples y.shape there). */
int dsn_pc_sample_sched(dsn_ctx* ctx, const float* y, const float* noise, uint64_t seed, float* x_out, int B, int T,
                        int N, const float* timesteps_host, int corrector_steps, float snr, int denoise, int* nfe_out,
                        void* stream);

/* The other registered predictors / correctors of the reference's sampler library, same loop:
 *   predictor  DSN_PRED_REVERSE_DIFFUSION (predictors.py:55-66) | DSN_PRED_EULER_MARUYAMA (:39-52) |
 *              DSN_PRED_NONE (:69-77, no score call, no draw)
 *   corrector  DSN_CORR_ALD (correctors.py:58-84) | DSN_CORR_LANGEVIN (:35-55: one step size per corrector step from
 *              the batch means of the per-item score / noise norms -- it couples the items of a batch)
 * noise (or the on-device draw) holds 1 + N*(corrector_steps + (predictor != NONE)) tensors in consumption order.
 * timesteps: host array of N floats or NULL (= linspace(1, t_eps, N)).  prior_mean: optional [B,n_src,D,T] device
 * tensor the prior is drawn around instead of y (`true_mean`, sdes/__init__.py:175-176).  intermediates: optional
 * [N][2][B,n_src,D,T] device buffer receiving (x, x_mean) after each step's corrector (`intermediate=True`).
 * nfe_out = N*(corrector_steps+1) whatever the predictor, as the reference reports it (__init__.py:186). */
enum { DSN_PRED_REVERSE_DIFFUSION = 0, DSN_PRED_EULER_MARUYAMA = 1, DSN_PRED_NONE = 2 };
enum { DSN_CORR_ALD = 0, DSN_CORR_LANGEVIN = 1 };
typedef struct dsn_sampler_opts {
  int predictor, corrector, corrector_steps;
  float snr, t_eps;
  int denoise;
  const float* timesteps;
  const float* prior_mean;
  float* intermediates;
} dsn_sampler_opts;
int dsn_pc_sample_ex(dsn_ctx* ctx, const float* y, const float* noise, uint64_t seed, float* x_out, int B, int T,
                     int N, const dsn_sampler_opts* opts, int* nfe_out, void* stream);

/* Ragged batches (DiT score network only): B mixtures of different lengths in tensors padded to the longest, T frames.
 * frames [B] (HOST int32): item b's latent frame count, 1 <= frames[b] <= T; its valid frames are the prefix
 * [..., :frames[b]].  Every DiT operation but self-attention acts per token, and attention masks each item's keys at
 * its own 1 + frames[b] tokens (the timestep token first), so item b's result over its valid frames is what the item
 * gets in a call of its own with T = frames[b].  The padded region of y / xt may hold anything finite.
 *   dsn_score_ragged      as dsn_score; out[b, :, :, frames[b]:] is unspecified (finite for finite inputs).
 *   dsn_pc_sample_ragged  as dsn_pc_sample_ex (OUVE; all three predictors, DSN_CORR_ALD, caller timesteps, prior_mean,
 *                         intermediates -- whose padded region is unspecified).  y and noise keep their padded shapes
 *                         [B,1,D,T] and [draws,B,n_src,D,T]: item b consumes noise[..., :frames[b]].
 *                         x_out[b, :, :, frames[b]:] is written as zero.  nfe_out as in dsn_pc_sample_ex.
 *                         With the on-device RNG (noise == NULL) an item's draws are indexed by its position in the
 *                         padded tensor: the result is a valid sample, but NOT the sample the item alone would draw
 *                         for that seed.
 * DSN_EINVAL, by name and before any launch: a score network other than the DiT (NCSN++ convolves across time, so
 * padding changes an item's result); a frame count outside [1, T]; DSN_CORR_LANGEVIN (its per-item norms would run
 * over the padding).  The Mix / PriorMix, Schroedinger-bridge and ODE samplers have no ragged form: each reduces over
 * the latent or couples the batch.  The score-matching loss has one, dsn_score_loss_ragged (declared with
 * dsn_score_loss), whose reductions run over each item's own frames.  The codec's ragged form is the block below.  Under
 * dsn_enable_graphs the lengths are data of the captured graph, not part of its key: one graph per (B, T, options)
 * serves every set of lengths. */
int dsn_score_ragged(dsn_ctx* ctx, const float* xt, const float* t, const float* mix, const int32_t* frames, float* out,
                     int B, int T, void* stream);
int dsn_pc_sample_ragged(dsn_ctx* ctx, const float* y, const int32_t* frames, const float* noise, uint64_t seed,
                         float* x_out, int B, int T, int N, const dsn_sampler_opts* opts, int* nfe_out, void* stream);

/* Ragged batches through the codec (either score network, or none): B items of different lengths in tensors padded to
 * the longest, T latent frames, coded in ONE pass.  frames [B] (HOST int32) as above.  The codec's convolutions reach
 * across time, so between two layers the engine writes every item's rows past its own end as zero (one small launch
 * per layer, call site "vae.ragged_tail_zero"): each convolution then reads past an item's end what it reads for the
 * item alone, its zero padding, and item b's result over its valid range is what the item gets in a call of its own
 * with T = frames[b], up to the summation order of a split-K layer.  No convolution kernel knows about lengths; the
 * padded rows are computed and discarded.
 *   dsn_decode_ragged    est [B,n_src,D,T] -> wav [B,n_src,hop*T].  The padded region of est may hold anything finite.
 *                        wav[b, :, hop*frames[b]:] is written as zero; cropping to each item's sample count stays with
 *                        the caller.
 *   dsn_encode_ragged    mix [B,1,hop*T] -> y [B,1,D,T].  Item b's samples must be ZERO past its own length (the caller
 *                        zero-extends every item to hop*T samples) and frames[b] = dsn_latent_frames of that length.
 *                        vae_noise [B,D,T] or NULL: item b consumes vae_noise[b, :, :frames[b]].  y[b, :, :, frames[b]:]
 *                        is written as zero.  With the on-device RNG (vae_noise == NULL) an item's draws are indexed by
 *                        its position in the padded tensor: the result is a valid sample, but NOT the sample the item
 *                        alone would draw for that seed.
 *   dsn_separate_ragged  dsn_encode_ragged (seed), dsn_pc_sample_ragged (seed + 1, as dsn_separate), dsn_decode_ragged in
 *                        one call: mix [B,1,hop*T] -> wav [B,n_src,hop*T].  DiT only, with dsn_pc_sample_ragged's
 *                        refusals.
 * DSN_EINVAL / DSN_ESTATE, by name and before any launch or workspace growth: a frame count outside [1, T]; a missing
 * encoder or decoder; a hop length (decode) or latent width that is not a multiple of 8 (the tail launch stores 16
 * bytes per lane).  Under dsn_enable_graphs dsn_decode_ragged is captured once per (B, T), as dsn_decode is; the
 * lengths are data of the graph.  The encoder runs eagerly, as in dsn_encode. */
int dsn_decode_ragged(dsn_ctx* ctx, const float* est, const int32_t* frames, float* wav, int B, int T, void* stream);
int dsn_encode_ragged(dsn_ctx* ctx, const float* mix, const int32_t* frames, const float* vae_noise, uint64_t seed,
                      float* y, int B, int T, void* stream);
int dsn_separate_ragged(dsn_ctx* ctx, const float* mix, const int32_t* frames, const float* vae_noise, const float* noise,
                        uint64_t seed, float* wav, int B, int T, int N, const dsn_sampler_opts* opts, int* nfe_out,
                        void* stream);

/* Long recordings as ONE latent each, with a window-blended DiT score (the MultiDiffusion / DiffCollage construction
 * applied to the score).  R recordings of frames[r] latent frames (HOST int32, 1 <= frames[r] <= T) in tensors padded
 * to T frames.  The sampler state is the whole [R,n_src,D,T] latent -- one trajectory, one prior draw, one noise
 * stream; only the score call is windowed:
 *   plan    a recording of F <= Tw frames is one window [0, F).  Otherwise hop = Tw - To, W = 1 + ceil((F - Tw) / hop)
 *           windows of Tw frames, window w starting at min(w hop, F - Tw): the last one is shifted back into the
 *           recording, never zero-extended.  Seam j is the To frames [(j+1) hop, (j+1) hop + To), the last To frames of
 *           window j; left of it a frame takes window j, right of it window j+1, inside it
 *           fall[k] s_j + rise[k] s_{j+1} with the fade tables of dsn_window_stitch.  The plan is two tables, which
 *           the device follows (the kernels know nothing about hops): wtab [Wtot][3] = (recording, start, length), the
 *           windows of all recordings in order, and ftab [R T][4] = (window0, offset0, window1, offset1) with
 *           fw [R T][2] = (fall, rise); window1 = -1 outside seams, window0 = -1 past a recording's end.
 *   score   every evaluation gathers the windows from the long state straight into the DiT's operand planes
 *           (call site of launch_win_pack_tokens), runs exactly the dense DiT call at (B = windows, T = Tw') at most
 *           `batch` windows at a time (batch <= 0: all at once) -- Tw' = Tw, or the longest recording when none is
 *           longer than a window; windows shorter than Tw' run the length-aware attention kernels, as a ragged batch
 *           does -- and blends the window scores back into [R T][n_src D] in one gather launch
 *           ("score.win_blend"): a copy outside seams, fmaf(rise, s1, fall * s0) inside, zero past a recording's end.
 *           The blended score is a DEFINITION: it is not the score of any trained model.
 *   dsn_score_windowed      xt [R,n_src,D,T], t [R], mix [R,1,D,T] -> out [R,n_src,D,T]
 *   dsn_pc_sample_windowed  dsn_pc_sample_ex on the long state with that score: nfe = N (corrector_steps + 1), every
 *                           evaluation shared by the whole pool.  x_out[r, :, :, frames[r]:] is zero.
 *   dsn_separate_windowed   dsn_encode_ragged (seed) -> dsn_pc_sample_windowed (seed + 1) -> dsn_decode_ragged in one
 *                           call: mix [R,1,hop*T] -> wav [R,n_src,hop*T], with their conventions.
 * The tables are uploaded per call into fixed workspace buffers, outside any capture: under dsn_enable_graphs the
 * sampler's graph key carries R, T, Wtot, Tw, To, batch and the short-window flag, not the table contents.
 * DSN_EINVAL by name, before any launch: a score network other than the DiT; Tw < 1, To < 0, 2 To > Tw (a frame may lie
 * in at most two windows); a frame count outside [1, T]; an unknown fade; n_src D not a multiple of 4; the langevin
 * corrector when the frame counts differ; opts->prior_mean / intermediates / timesteps are not supported.
 * dsn_score_window_plan is the plan alone (needs no context and no GPU): Wtot and Tw' always, the tables into any
 * non-null HOST array ([Wtot][3], [R T][4], [R T][2]). */
int dsn_score_window_plan(const int32_t* frames, int R, int T, int Tw, int To, int fade, int32_t* wtab, int32_t* ftab,
                          float* fw, int* Wtot, int* Twin);
int dsn_score_windowed(dsn_ctx* ctx, const float* xt, const float* t, const float* mix, const int32_t* frames, float* out,
                       int R, int T, int Tw, int To, int fade, int batch, void* stream);
int dsn_pc_sample_windowed(dsn_ctx* ctx, const float* y, const int32_t* frames, const float* noise, uint64_t seed,
                           float* x_out, int R, int T, int N, int Tw, int To, int fade, int batch,
                           const dsn_sampler_opts* opts, int* nfe_out, void* stream);
int dsn_separate_windowed(dsn_ctx* ctx, const float* mix, const int32_t* frames, const float* vae_noise,
                          const float* noise, uint64_t seed, float* wav, int R, int T, int N, int Tw, int To, int fade,
                          int batch, const dsn_sampler_opts* opts, int* nfe_out, void* stream);

/* The secondary SDE family of the reference's sampler package on the latent state read as [B, n_src, D*T]:
 * MixSDE (sdes.py:182-352) / PriorMixSDE (:355-593; diffusion scaled by the running RMS of the mixture over `avg_len`
 * flattened latent samples) through the same predictor-corrector loop, predictors as above, corrector
 * DSN_MIXCORR_ALD2 (AnnealedLangevinDynamics2, correctors.py:87-121) or DSN_MIXCORR_NONE.  noise: [1 + N*(corrector_steps
 * + (predictor != NONE)), B, n_src, D, T] in consumption order, or NULL (device RNG).  MixSDE's prior is written for
 * 2 sources (reference :347).  nfe_out = N*(corrector_steps+1). */
enum { DSN_MIXCORR_ALD2 = 0, DSN_MIXCORR_NONE = 1 };
typedef struct dsn_mix_opts {
  int prior_mix;                      /* 0 MixSDE, 1 PriorMixSDE */
  float d_lambda, sigma_min, sigma_max;
  int avg_len;                        /* PriorMixSDE only */
  int predictor, corrector, corrector_steps;
  float snr, t_eps;
  int denoise;
} dsn_mix_opts;
int dsn_pc_sample_mix(dsn_ctx* ctx, const float* y, const float* noise, uint64_t seed, float* x_out, int B, int T, int N,
                      const dsn_mix_opts* opts, int* nfe_out, void* stream);

/* get_sb_sampler (src/sdes/__init__.py:284-389) with SBVESDE(k, c, eps = sb_eps) (sdes.py:701-779): the state starts
 * as y repeated over the sources; N first-order Schroedinger-bridge steps over linspace(1, t_eps, N + 1), the score
 * network's output taken as the data estimate.  sampler_type DSN_SB_SDE consumes noise [N, B, n_src, D, T] (or the
 * device RNG), DSN_SB_ODE none. */
enum { DSN_SB_SDE = 0, DSN_SB_ODE = 1 };
int dsn_sb_sample(dsn_ctx* ctx, const float* y, const float* noise, uint64_t seed, float* x_out, int B, int T, int N, float k,
                  float c, float sb_eps, float t_eps, int sampler_type, void* stream);

/* ode_sampler() of sdes.get_ode_sampler (src/sdes/__init__.py:196-281): the probability-flow ODE
 *   dx/dt = theta (y - x) - 1/2 g(t)^2 score(x, t, y)
 * integrated from t = 1 down to t_eps by an explicit embedded Runge-Kutta pair with the step control of
 * scipy 1.15's solve_ivp(method = "RK45" | "RK23", rtol, atol, first_step, max_step): one step size for the whole
 * batch (the RMS error norm runs over the flattened [B,n_src,D,T] state), one score call per stage.  The state and the
 * stages are fp64, the score network reads their fp32 cast.  The prior is y broadcast over the n_src sources plus
 * std(1) z -- z = noise [B,n_src,D,T] or draw 0 of the on-device stream for `seed` -- drawn by dsn_pc_sample's own
 * prior kernel, so the same noise or seed gives bit for bit the x_T dsn_pc_sample starts from.  denoise != 0: one
 * noise-free reverse-diffusion step at t_eps with dt = 1/N, the PC sampler's predictor kernel with zero noise (not
 * counted in nfev, as in the reference).  Deviations from the reference, stated: the state is real (not complex64) and has n_src sources (the
 * reference draws the prior in y's one-source shape); where solve_ivp would return success=False (step size below
 * 10 ulp of t) this call fails with DSN_ESOLVER, and so it does after max_attempts step attempts.  Either failure is
 * reported by this call after it synchronised its stream; stats (may be NULL) are filled in every case.
 * first_step == 0: scipy's select_initial_step (one extra evaluation); max_step <= 0 or inf: unbounded.  Under
 * dsn_enable_graphs one step attempt is captured once per (B, T, method) and replayed. */
enum { DSN_ODE_RK45 = 0, DSN_ODE_RK23 = 1 };
enum { DSN_ODE_FINISHED = 0, DSN_ODE_STEP_TOO_SMALL = 1, DSN_ODE_TOO_MANY_ATTEMPTS = 2 };
typedef struct DsnOdeOpts {
  int method;                         /* DSN_ODE_RK45 | DSN_ODE_RK23 */
  double rtol, atol;
  double t_eps;                       /* the ODE runs from 1 to t_eps; the denoising step uses (float)t_eps */
  int denoise;
  int N;                              /* sde.N: dt = 1/N of the denoising step */
  double first_step;                  /* 0 = automatic, else in (0, 1 - t_eps] */
  double max_step;                    /* <= 0 or inf = unbounded */
  int max_attempts;                   /* > 0 */
} DsnOdeOpts;
typedef struct DsnOdeStats {
  int nfev;                           /* scipy's count: 1 + (1 if first_step is automatic) + stages x attempts */
  int n_accepted, n_rejected;
  double t_final;
  int status;                         /* DSN_ODE_* */
} DsnOdeStats;
int dsn_ode_sample(dsn_ctx* ctx, const float* y, const float* noise, uint64_t seed, float* x_out, int B, int T,
                   const DsnOdeOpts* o, DsnOdeStats* stats, void* stream);

/* Denoising score-matching loss of a checkpoint on (mixture, target) latent pairs with ONE score call: the forward
 * half of the reference's validation_step (src/diffsep_latent.py:130-187).  y [B,1,D,T], x0 [B,n_src,D,T].
 *   DSN_LOSS_DSM       sample_prior + compute_score_loss: t_b ~ U(t_eps, 1), x_t = (e x0 + (1 - e) y) + sigma(t) z with
 *                      e = exp(-theta t), sigma = OUVESDE._std(t); loss[b,s] = mean over (D,T) of (sigma score + z)^2.
 *                      perm [B,n_src] int32 (device, may be NULL = identity): slot s of item b holds source perm[b,s]
 *                      of x0 (utils.shuffle_sources).
 *   DSN_LOSS_INIT_PIT  compute_score_loss_init_hack_pit: t = 1, x_t = y + sigma z0 and, per (item, slot), the minimum
 *                      over the source j placed in the slot of mean (sigma score + z0 + (y - mean(x0[j])) / sigma)^2 --
 *                      the reference's per-slot minimum over all n! permutations, which it evaluates with n! network
 *                      calls on identical inputs.  t and perm must be NULL.
 * reduction: DSN_LOSS_REDUCE_NONE -> loss_out [B,n_src] (what MSELoss(reduction="none") followed by the reference's
 * mean over the last two axes leaves), DSN_LOSS_REDUCE_MEAN -> loss_out [1] (MSELoss()).
 * t [B] (device, may be NULL): injected times in (0, 1]; else t_b = t_eps + (1 - t_eps) u_b with u_b word 0 of the
 * Philox4x32-10 block of counter b under key seed ^ 0x9E3779B97F4A7C15 (same 24-bit mapping as the normals).
 * noise [B,n_src,D,T] (device, may be NULL): z; else draw 0 of the samplers' normal stream under key `seed` (the z a
 * sampler's prior would use for that seed).  Optional outputs (device, may be NULL): xt_out [B,n_src,D,T], t_out [B],
 * sigma_out [B], z_out [B,n_src,D,T].  loss_out == NULL: perturb only (sample_prior), no score call.
 * sigma and e are evaluated in fp64 per item and rounded once to fp32; x_t is fp32 in the reference's order; the
 * loss terms are formed and summed in fp64 in a fixed order (bit-identical between runs), then rounded to fp32.
 * Injected t / perm are checked on the host before any launch (this synchronises the stream); n_src <= 4.  Under
 * dsn_enable_graphs the sequence perturb, score call, reduce, combine is captured once per (B, T, mode, reduction). */
enum { DSN_LOSS_DSM = 0, DSN_LOSS_INIT_PIT = 1 };
enum { DSN_LOSS_REDUCE_NONE = 0, DSN_LOSS_REDUCE_MEAN = 1 };
typedef struct DsnLossOpts {
  int mode;                           /* DSN_LOSS_DSM | DSN_LOSS_INIT_PIT */
  int reduction;                      /* DSN_LOSS_REDUCE_NONE | DSN_LOSS_REDUCE_MEAN */
  float t_eps;                        /* lower end of the time draw, in (0, 1) */
} DsnLossOpts;
int dsn_score_loss(dsn_ctx* ctx, const float* y, const float* x0, const float* t, const float* noise,
                   const int32_t* perm, uint64_t seed, float* loss_out, float* xt_out, float* t_out, float* sigma_out,
                   float* z_out, int B, int T, const DsnLossOpts* opts, void* stream);
/* The same loss on a ragged batch (DiT only; NCSN++ is refused by name as in dsn_score_ragged): y, x0, noise and the
 * outputs keep their padded shapes, frames [B] (HOST int32, 1 <= frames[b] <= T) as in the ragged block above.
 *   perturb  x_t[b, :, :, :frames[b]] is exactly dsn_score_loss's value (same fp32 order, sigma and e rounded once from
 *            fp64); x_t is written as zero past the item's end, and x0 and noise are not read there (they may hold
 *            anything, NaN included).  y's padding is only handed on to the score call and must be finite.
 *   score    one dsn_score_ragged-path call on (x_t, t, y, frames), also for DSN_LOSS_INIT_PIT.
 *   reduce   loss[b, s] = mean over the D * frames[b] valid elements of (sigma score + z)^2 (INIT_PIT: the per-slot
 *            minimum over j of the table entry), fp64 terms summed in a fixed order that depends on the item's own
 *            length only.  DSN_LOSS_REDUCE_MEAN is the mean of the B * n_src row means.  This is a DEFINITION: the
 *            reference has no mixed-length form; for equal lengths it equals MSELoss().
 * RNG: t_b comes from counter b as in the dense call.  With noise == NULL the normals are indexed by position in the
 * padded tensor: a valid draw, but NOT the draw the item alone would make for that seed (dsn_pc_sample_ragged's
 * caveat).  Injected noise: item b uses noise[b, ..., :frames[b]].  z_out hands the padded z back as it was used.
 * Under dsn_enable_graphs the lengths are data of the captured graph: one graph per (B, T, mode, reduction). */
int dsn_score_loss_ragged(dsn_ctx* ctx, const float* y, const float* x0, const int32_t* frames, const float* t,
                          const float* noise, const int32_t* perm, uint64_t seed, float* loss_out, float* xt_out,
                          float* t_out, float* sigma_out, float* z_out, int B, int T, const DsnLossOpts* opts,
                          void* stream);

/* LatentDiffSep.decode: est [B,n_src,D,T] -> wav [B,n_src,target_len] (crop of hop*T;
 * target_len <= 0 means hop*T). */
int dsn_decode(dsn_ctx* ctx, const float* est, float* wav, int B, int T, int target_len, void* stream);

/* AudioAutoencoder.decode_audio(latents, chunked=True, overlap, chunk_size) (reference
 * src/stable_audio_tools/models/autoencoders.py:665-731): long-form decode as independent chunks of `chunk_size`
 * latent frames every chunk_size-overlap frames (plus a final chunk flush with the end), pasted with overlap/2
 * frames dropped at each interior edge.  Bounds activation memory by the chunk, not the utterance.
 * T < chunk_size is an error (the reference fails there too). */
int dsn_decode_chunked(dsn_ctx* ctx, const float* est, float* wav, int B, int T, int target_len, int chunk_size,
                       int overlap, void* stream);

/* AudioAutoencoder.encode_audio(audio, chunked=True, ...) (autoencoders.py:596-663) behind LatentDiffSep.encode's
 * padding: the encoder output (mean ++ scale) is stitched by the same rule, then sampled once with vae_noise
 * [B,D,T] (the reference samples every chunk with its own draw before stitching: the same distribution). */
int dsn_encode_chunked(dsn_ctx* ctx, const float* mix, const float* vae_noise, uint64_t seed, float* y, int B, int L,
                       int chunk_size, int overlap, void* stream);

/* LatentDiffSep.encode (mixture branch): mix [B,1,L] -> y [B,1,D,T], T = (L + pad)/hop with
 * the reference's pad rule (a full extra hop when L % hop == 0).  vae_noise [B,D,T] or NULL
 * (on-device draw with `seed`). */
int dsn_encode(dsn_ctx* ctx, const float* mix, const float* vae_noise, uint64_t seed, float* y, int B, int L,
               void* stream);
int dsn_latent_frames(const dsn_ctx* ctx, int L);   /* T for an L-sample mixture */
int dsn_hop_length(const dsn_ctx* ctx);

/* LatentDiffSep.separate(mix, target_dim, latent=False): encode -> sample -> decode.
 * noise / vae_noise as above (both NULL = on-device RNG). */
int dsn_separate(dsn_ctx* ctx, const float* mix, const float* vae_noise, const float* noise, uint64_t seed,
                 float* wav, int B, int L, int target_len, int N, int corrector_steps, float snr, float t_eps,
                 int denoise, int* nfe_out, void* stream);

/* SI-SDR with permutation-invariant assignment: ref, est [B,n,L] (device) -> si_sdr [B,n] and perm [B,n]
 * (host; est source perm[b][i] is matched to ref source i).  Replaces the fast_bss_eval call of
 * src/evaluate_latent.py:118-136 (compute_permutation=True, zero_mean=False); n <= 4. */
int dsn_si_sdr_pit(dsn_ctx* ctx, const float* ref, const float* est, int B, int n, int L, float* si_sdr_out,
                   int* perm_out, void* stream);

/* SI-SDR, SI-SIR and SI-SAR with the permutation solved: what evaluate_latent.py:118-136 gets from
 * fast_bss_eval.si_bss_eval_sources(ref, est, zero_mean=False, compute_permutation=True, clamp_db=100).
 * ref, est [B,n,L] (device) -> si_sdr / si_sir / si_sar [B,n] and perm [B,n] (host; any may be NULL).
 * perm_by: 0 = permutation with the best mean SI-SDR, 1 = best mean SI-SIR (bss_eval's convention).
 * clamp_db <= 0: no clamping.  n <= 4. */
int dsn_si_bss_eval(dsn_ctx* ctx, const float* ref, const float* est, int B, int n, int L, int perm_by, float clamp_db,
                    float* si_sdr_out, float* si_sir_out, float* si_sar_out, int* perm_out, void* stream);

/* STOI (extended = 0) or ESTOI (extended = 1) of est against ref as pystoi.stoi(ref, est, fs, extended)
 * defines it (restated in tests/; parity with the pystoi package unpinned).  ref, est [B,n,L] fp32 (device),
 * fs the signal rate.  perm [B*n] host, may be NULL: est source perm[b*n+i] is scored against ref source i
 * (the dsn_si_bss_eval convention).  out [B*n] host.  frames_out [B*n] host, may be NULL: STFT frames left
 * after silent-frame removal (< 30 -> out = 1e-5).  n <= 4; a signal rate whose resampling filter to 10 kHz
 * would exceed 65536 taps is refused (10000/fs must reduce to a small ratio, as it does for 8, 16, 44.1, 48 kHz). */
int dsn_stoi(dsn_ctx* ctx, const float* ref, const float* est, int B, int n, int L, int fs, int extended,
             const int* perm, float* out, int* frames_out, void* stream);

/* The objective measures behind the Hu & Loizou composite scores, as the reference's src/evaluate/evaluate_covl.py
 * computes them per utterance (restated in tests/composite_restatement.py and pinned to the reference's own functions
 * by tests/golden/composite.npz): the log-likelihood ratio of the LPC models (llr) and the weighted spectral slope
 * (wss), each the mean of the round(0.95 F) smallest of the F per-frame values, the segmental SNR (segsnr, mean over
 * the frames of the value clamped to [-10, 35] dB) and the overall SNR (snr), both on the mean-removed signals with
 * the estimate rescaled to the reference's peak.  ref, est [B,n,L] fp32 (device); fs 8000 or 16000.  perm [B*n] host,
 * may be NULL: est source perm[b*n+i] is scored against ref source i.  Every array of `out` is a host array of B*n
 * entries and may be NULL; frames receives F.  With pesq [B*n] (host; PESQ itself is not computed here) the call
 * also fills
 *   csig = 3.093 - 1.029 llr + 0.603 pesq - 0.009 wss
 *   cbak = 1.634 + 0.478 pesq - 0.007 wss + 0.063 segsnr
 *   covl = 1.594 + 0.805 pesq - 0.512 llr - 0.007 wss
 * each clipped to [1, 5]; asking for one of them without pesq is DSN_EINVAL.  Also DSN_EINVAL, before any launch:
 * n > 4, a perm entry outside [0, n), another fs, L shorter than one frame plus one hop (F < 1).
 * A constant estimate (all zeros included) has no peak to rescale to: the conditioning divides by max|est - mean| = 0
 * as the reference does, and segsnr, snr and cbak are NaN; llr and wss read the raw signals and stay defined. */
typedef struct DsnCompositeOut {
  float *llr, *wss, *segsnr, *snr, *csig, *cbak, *covl;
  int* frames;
} DsnCompositeOut;
int dsn_composite(dsn_ctx* ctx, const float* ref, const float* est, int B, int n, int L, int fs, const int* perm,
                  const float* pesq, const DsnCompositeOut* out, void* stream);

/* The three metric calls above on a batch of differently long items, one call (one device-to-host copy, one
 * synchronise) whatever B is.  ref, est stay [B,n,L] fp32 (device) with L the padded length Lmax; lens [B] (host, like
 * `frames` of the ragged calls above) holds the sample count of item b, shared by its n sources.  Item b gets exactly
 * what the dense call gives for ref[b, :, :lens[b]], est[b, :, :lens[b]] alone, bit for bit: every sum runs in the
 * order the item's own length fixes.  Nothing past lens[b] is read, so the padding may hold anything (NaN included).
 * All other arguments are those of the dense call.
 *   dsn_si_bss_eval_ragged  the permutation is solved per item.
 *   dsn_stoi_ragged         an item shorter than one 10 kHz frame (256 samples at 10 kHz) scores 1e-5 with 0 frames,
 *                           as the dense call does for a batch that short; fewer than 30 frames -> 1e-5, as there.
 *   dsn_composite_ragged    out->frames receives every item's own F = lens[b] / hop - win / hop, and its trimmed means
 *                           take round(0.95 F) of them.
 * DSN_EINVAL by name, before anything is allocated or launched: lens null; lens[b] outside [1, L]; for
 * dsn_composite_ragged an item shorter than one frame plus one hop (the message names the item and the samples needed);
 * and whatever the dense call refuses. */
int dsn_si_bss_eval_ragged(dsn_ctx* ctx, const float* ref, const float* est, int B, int n, int L, const int32_t* lens,
                           int perm_by, float clamp_db, float* si_sdr_out, float* si_sir_out, float* si_sar_out,
                           int* perm_out, void* stream);
int dsn_stoi_ragged(dsn_ctx* ctx, const float* ref, const float* est, int B, int n, int L, const int32_t* lens, int fs,
                    int extended, const int* perm, float* out, int* frames_out, void* stream);
int dsn_composite_ragged(dsn_ctx* ctx, const float* ref, const float* est, int B, int n, int L, const int32_t* lens,
                         int fs, const int* perm, const float* pesq, const DsnCompositeOut* out, void* stream);

/* Classic bss_eval SDR, SIR and SAR (Vincent et al. 2006): the decomposition dsn_si_bss_eval makes with one tap, made
 * with a distortion filter of filter_length = F taps (1 <= F <= 512) -- what fast_bss_eval.bss_eval_sources
 * reports, and with sir_sar = 0 fast_bss_eval.sdr (restated in float64 in tests/bss_eval_restatement.py; parity with
 * the fast_bss_eval and mir_eval packages unpinned).  ref, est [B,n,L] fp32 (device), all signals zero-extended,
 * reference i scaled by s_i = 1 / |ref_i| (0 for an all-zero reference; the norm in fp64 over exact products):
 *   c_ij[k] = s_i s_j sum_t ref_i[t] ref_j[t+k], |k| < F;   G[(i,p),(j,q)] = c_ij[p-q] + load_diag [i = j and p = q]
 *   d_ij[p] = s_i sum_t ref_i[t-p] est_j[t], 0 <= p < F;    ee_j = sum_t est_j[t]^2
 *   pt_ij = d_ij^T G_ii^-1 d_ij (G_ii: the F x F Toeplitz block of reference i),  pall_j = d_j^T G^-1 d_j (M = n F)
 *   SDR_ij = 10 log10(pt_ij / (ee_j - pt_ij)),  SIR_ij = 10 log10(pt_ij / (pall_j - pt_ij)),
 *   SAR_j = 10 log10(pall_j / (ee_j - pall_j))
 * numerators and denominators clamped below at 1e-300, the dB value then to +-clamp_db when clamp_db > 0.  With F = 1
 * this is the SI-BSS decomposition.  Device: fp64 correlations (exact products, fixed order), an fp64 Cholesky of G
 * and of every G_ii with the right-hand sides carried as extra rows (only the quadratic forms are formed, never the
 * filters), the ratios and the permutation.  The permutation: `perm` [B*n] (host, may be NULL) is used as is (est
 * source perm[b*n+i] against ref source i); otherwise all n! candidates in lexicographic order, the key the sum of
 * SIR (perm_by = 1, bss_eval's convention) or of SDR (perm_by = 0), replaced only by a strictly greater key.
 * Outputs (host, float64, any may be NULL): sdr, sir, sar [B*n] on the chosen pairs (sar of the assigned estimate),
 * sdr_pairs, sir_pairs [B*n*n] ([b][i][j]: est_j against ref_i), perm_out [B*n], status [B].
 * sir_sar = 0: the M x M system is skipped, sir, sar and sir_pairs are NaN and perm_by = 0 is forced; sdr is bit for
 * bit that of the full call.
 * lens [B] (host, may be NULL: every item has L samples): item b holds lens[b] samples and gets bit for bit what the
 * dense call gives for ref[b, :, :lens[b]], est[b, :, :lens[b]] alone; nothing past its end is read.  Two calls give
 * the same bits (no atomics; every sum's order is fixed by the item's own length, n and F).
 * Breakdown: a pivot that is <= 0 or not finite (an all-zero reference without load_diag; references so band-limited
 * that G is numerically singular) sets status[b] = 1 and every value of item b to NaN (its perm_out: `perm`, or the
 * identity); the call still returns DSN_OK.  load_diag > 0 regularises.
 * Workspace: the items are taken in chunks whose correlation partials, lag tables and systems stay within
 * workspace_budget bytes (0 = 512 MiB); the chunking changes no bit of any item.  dsn_bss_eval_plan (no context, no
 * GPU) returns the time tiles of the longest item, M, the items per chunk and the bytes of one chunk.
 * There is no zero_mean option (the caller subtracts the means) and no conjugate-gradient solver.
 * DSN_EINVAL by name, before anything is allocated or launched: ref or est null; n outside [1, 4]; filter_length outside
 * [1, 512]; load_diag < 0 (or NaN); lens[b] outside [1, L]; a perm entry outside [0, n); perm_by outside {0, 1}; a
 * budget smaller than one item. */
typedef struct DsnBssEvalOpts {
  int filter_length, perm_by;
  double clamp_db, load_diag;
  int sir_sar;
  int64_t workspace_budget;
} DsnBssEvalOpts;
typedef struct DsnBssEvalOut {
  double *sdr, *sir, *sar;        /* [B*n] host */
  double *sdr_pairs, *sir_pairs;  /* [B*n*n] host */
  int* perm_out;                  /* [B*n] */
  int* status;                    /* [B] */
} DsnBssEvalOut;
int dsn_bss_eval(dsn_ctx* ctx, const float* ref, const float* est, int B, int n, int L, const int32_t* lens,
                 const int* perm, const DsnBssEvalOpts* opts, const DsnBssEvalOut* out, void* stream);
int dsn_bss_eval_plan(int B, int n, int L, int F, int64_t budget, int* tiles, int* M, int* items_per_chunk,
                      int64_t* workspace_bytes);

/* Put the separated windows of one long recording back together: chunks [W][n][Lw] fp32 (device), window w covering
 * samples [w hop, w hop + Lw) with hop = Lw - overlap -> out [n][L] fp32 (device), with the speakers in window 0's
 * order.  Needs no score network and no codec.  Three stages, all on the device:
 *   Gram         G[w][i][j] = sum_k chunks[w][i][hop + k] chunks[w+1][j][k] over the overlap k in [0, overlap), for
 *                every boundary w < W - 1: exact fp64 products summed in fp64 in an order the shape alone fixes (no
 *                atomics: two calls give identical bits).
 *   permutations sigma_w maximises sum_i G[w][i][sigma(i)] -- the assignment of least squared difference on the
 *                overlap; a source silent there drops out of the decision.  All n! candidates in lexicographic order
 *                of (sigma(0) .. sigma(n-1)), a candidate replacing the best only when strictly greater: ties (an
 *                all-zero overlap, overlap = 0) go to the identity.  P_0 = id, P_{w+1}(i) = sigma_w(P_w(i)).
 *                align == 0: the Gram stage is skipped and every P_w is the identity.
 *   cross-fade   for t in [0, L), w = min(t / hop, W - 1), k = t - w hop: with w >= 1 and k < overlap
 *                out[i][t] = fall[k] chunks[w-1][P_{w-1}(i)][hop + k] + rise[k] chunks[w][P_w(i)][k] (two fp32 products
 *                and their fp32 sum, not contracted), else out[i][t] = chunks[w][P_w(i)][k], bit for bit.
 *                rise[k] = sin^2(pi (k + 1/2) / (2 overlap)) (fade = 0, Hann) or (k + 1/2) / overlap (fade = 1,
 *                linear), fall[k] = 1 - rise[k]: fp64 on the host, rounded once to fp32.
 * perm_out [W][n] and gram_out [W-1][n][n] are host arrays and may be NULL: with either the call synchronises the
 * stream and fills them (gram_out with zeros when align == 0); with both NULL it only enqueues.
 * DSN_EINVAL by name, before anything is allocated or launched: chunks or out null; n outside [1, 4]; W < 1; Lw < 1;
 * overlap < 0; 2 overlap > Lw (an output sample is covered by at most two windows: the cross-fade is a gather);
 * a fade other than 0 | 1; L outside ((W-1) hop + overlap, (W-1) hop + Lw] for W > 1 or outside [1, Lw] for W = 1
 * (the last window starts inside the recording and is zero-extended past its end, and its overlap holds real samples). */
enum { DSN_FADE_HANN = 0, DSN_FADE_LINEAR = 1 };
int dsn_window_stitch(dsn_ctx* ctx, const float* chunks, int W, int n, int Lw, int overlap, int L, int fade, int align,
                      float* out, int32_t* perm_out, double* gram_out, void* stream);

/* Sinc resampling on the device: audio at any sample rate to the model's rate and back.  The filter is the default of
 * torchaudio.transforms.Resample (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), which the reference applies
 * in AudioAutoencoder.preprocess_audio_list_for_encoder (autoencoders.py:553-594); restated in float64 in
 * tests/resample_restatement.py.  With g = gcd(fs_in, fs_out), orig = fs_in / g, new = fs_out / g,
 * base = min(orig, new) 0.99, width = ceil(6 orig / base), K = 2 width + orig, for phase p < new and tap k < K
 *   t = clamp((-p / new + (k - width) / orig) base, -6, 6),  h[p][k] = float32(sinc(pi t) cos^2(pi t / 12) base / orig)
 * (float64, rounded once), and a row of L samples gives ceil(new L / orig) samples
 *   out[m new + p] = sum_k h[p][k] xz[m orig + k - width]        (xz: x extended by zeros on both sides).
 * Content above 0.495 of the lower rate is removed.  In float32 all taps of a phase but one short run are exactly 0:
 * the plan keeps, per phase, the first tap k0[p] that is not and `support` taps from there (the longest such run over
 * the phases, zero-filled on the right).  A tap is dropped only when it equals 0.0f, so the compact sum is the dense sum.
 *   dsn_resample_plan    the plan alone (no context, no GPU): orig, new, width, support always; k0 [new] and taps
 *                        [new][support] into any non-null HOST array.  DSN_EINVAL for a non-positive rate.
 *   dsn_resample_length  ceil(new L / orig); -1 for a non-positive rate or L < 0.
 *   dsn_resample         x [B][C][L] fp32 (device) -> out [B][C or 1][Lout] fp32 (device) in one launch.  lens (HOST,
 *                        [B], or NULL: every item has L samples) are the valid samples per item, shared by its channels:
 *                        item b gets ceil(new lens[b] / orig) samples, the rest of its rows is written as zero, and
 *                        nothing at or past lens[b] is read (the padding may hold NaN).  downmix != 0: the channels are
 *                        averaged in fp32 before the filter, (x_0 + .. + x_{C-1}) / C in that order, and out has one
 *                        channel.  Each output is one fp32 product and support - 1 fused multiply-adds in tap order; no
 *                        atomics: two calls give identical bits.  fs_in == fs_out is a copy (with lens, zero past each
 *                        item).  Needs no score network and no codec.  The tables are uploaded once per (orig, new) and
 *                        kept by the context; the call synchronises the stream when it uploads tables or new lens, so
 *                        it must not be captured into a graph.
 * DSN_EINVAL by name, before anything is allocated or launched: x or out null; a non-positive rate; C < 1, L < 1, B < 1,
 * B C > 65535; lens[b] outside [1, L]; Lout < ceil(new L / orig); a plan whose table, first taps and tile span do not fit
 * the LDS budget the kernel declares (csrc/resample.hip).  All pairs between {8000, 16000} and {8000, 11025, 16000,
 * 22050, 24000, 32000, 44100, 48000} fit (support <= 73, tables <= 32.5 KB). */
int dsn_resample_plan(int fs_in, int fs_out, int* orig, int* new_, int* width, int* support, int32_t* k0, float* taps);
int dsn_resample_length(int fs_in, int fs_out, int L);
int dsn_resample(dsn_ctx* ctx, const float* x, int B, int C, int L, const int32_t* lens, int fs_in, int fs_out,
                 int downmix, float* out, int Lout, void* stream);

/* Mixture-consistent STFT masks: a refinement of separated estimates against the mixture they came from (Wiener-style
 * post-filtering; csrc/maskrefine.hip, restated in float64 in tests/mask_refine_restatement.py).  It is a definition, not
 * a trained step, and nothing calls it unless asked to.  Per item, with mixture m [L], estimates s_i [L] (i < n):
 *   padding    Lp = hop ceil(L / hop); every signal is zero-extended to Lp
 *   analysis   torch.stft(center = True, pad_mode = "reflect") with the periodic Hann window of n_fft samples, computed
 *              in fp64 and rounded once to fp32: F = 1 + Lp / hop frames, bins 0 .. n_fft / 2
 *   masks      a_i = |S_i|^power,  M_i = (a_i + eps) / (sum_j a_j + n eps): they sum to 1, also where every estimate is
 *              silent (there M_i = 1 / n)
 *   synthesis  Y_i = M_i X (X: the mixture's STFT), y_i = the overlap-add of the windowed inverse frames divided, per
 *              sample, by the sum of w^2 over the frames that cover it; cropped to L
 * Every output carries the mixture's phase and sum_i y_i = m up to rounding.  mix [B][Lmax], est and out [B][n][Lmax]
 * fp32 (device), one launch, no workspace.  lens (HOST, [B], or NULL: every item is Lmax long): item b has its own
 * L_b = lens[b], Lp_b and F_b and is reflected at its own end; nothing at or past lens[b] is read from mix or est (the
 * padding may hold NaN) and out is written as zero there.  All arithmetic is fp32 in a fixed order with no atomics: an
 * item's result does not depend on its position in the batch, on the other items or on how the samples are divided among
 * workgroups, and two calls give identical bits.  With n = 1 the mask is exactly 1; silent estimates with n = 2 or 4
 * give the n = 1 result scaled by 1 / n to the bit.  Needs no score network and no codec.  The window and the twiddles
 * are formed on the device; the call uploads `lens` when it is given and differs from the last upload, and then
 * synchronises the stream, so with lens it must not be captured into a graph.
 * DSN_EINVAL by name, before anything is allocated or launched: mix, est or out null; B < 1 or B > 65535; n outside
 * [1, 4]; n_fft not a power of two in [64, 2048]; n_fft / hop not in {2, 4, 8}; power not 1 or 2; eps not finite or <= 0;
 * Lmax > 2^30; lens[b] (or Lmax without lens) outside [n_fft / 2 + 1, Lmax] -- one reflection must reach the item, the
 * message names the item and the samples needed; out overlapping mix or est (neighbouring workgroups read the samples
 * around a span). */
int dsn_mask_refine(dsn_ctx* ctx, const float* mix, const float* est, int B, int n, int Lmax, const int32_t* lens,
                    int n_fft, int hop, int power, float eps, float* out, void* stream);

/* Multichannel stems from mono estimates: the mixture's C channels filtered with what the mono estimates say about the
 * sources, so every source comes back with the mixture's channels and spatial image (the last step of Open-Unmix /
 * norbert; Duong, Vincent, Gribonval 2010; csrc/maskrefine.hip, restated in float64 in tests/stems_restatement.py).  A
 * definition, not a trained step; nothing calls it unless asked to.  mix [B][C][Lmax], est [B][n][Lmax] (mono), out
 * [B][n][C][Lmax] fp32 (device).  lens and channels (HOST, [B], or NULL: Lmax and C for every item): item b has
 * lens[b] samples and uses its first channels[b] channels; its other output channels and everything at or past lens[b]
 * are written as zero, and nothing there is read from mix or est (it may hold NaN).  Padding, analysis, window,
 * reflection, masks M_i and synthesis are dsn_mask_refine's (above), X_c the STFT of channel c, S_i of estimate i.
 *   DSN_STEMS_MASK    Y_i,c = M_i X_c: one launch, no workspace, C <= 8.  out[b][i][c] has, bit for bit, what
 *                     dsn_mask_refine returns for mix = channel c.
 *   DSN_STEMS_WIENER  one expectation-maximisation pass of the multichannel Wiener filter, C = channels[b] <= 2.  With
 *                     the fp32 spectra and masks widened to fp64 (bin f, frame t):
 *                       v_i(f,t) = M_i^2 (1/C) sum_c |X_c|^2
 *                       N_i(f) = sum_t M_i^2 X X^H (C x C, Hermitian),  d_i(f) = sum_t v_i
 *                       R_i(f) = N_i / d_i, the identity where d_i = 0
 *                       Sigma(f,t) = sum_j v_j R_j,  lambda(f,t) = reg tr(Sigma) / C + eps
 *                       z = (Sigma + lambda I)^-1 X  (the closed-form 2 x 2 adjugate),
 *                       Y_i = v_i R_i z + (lambda / n) z
 *                     so sum_i Y_i = X in exact arithmetic: the regularisation's remainder is handed out equally and
 *                     every channel of the stems adds up to that channel of the mixture.  N, d, R and the per-bin
 *                     solve are fp64 (two identical channels make Sigma singular: only lambda inverts it); Y is
 *                     rounded once to fp32 before the inverse transform.  Three launches: every frame is owned by
 *                     exactly one workgroup of the statistics launch (frames [c S / hop, (c + 1) S / hop), S = 2048,
 *                     4096 for n_fft = 2048), which adds its frames in increasing order; a reduce launch adds the
 *                     partials in workgroup order; the filter launch reads R from global memory.  No floating-point
 *                     atomics: the order depends on the item's length and the parameters alone.
 * An item has the same bits alone, at any batch position and under any padding, and two calls give identical bits.
 * Silent estimates give n outputs that are equal to the bit.  info_R ([B][n][n_fft / 2 + 1][C][C] complex as double
 * pairs; zero outside an item's own channels) and info_den ([B][n][n_fft / 2 + 1]) are HOST arrays or NULL: R_i and
 * d_i of the Wiener mode (zeros in mask mode); with either the stream is synchronised.  The partials and R live in a
 * workspace the context keeps and grows.  The call uploads lens and channels when given and then synchronises the
 * stream, so with them it must not be captured into a graph.  Needs no score network and no codec.
 * DSN_EINVAL by name, before anything is allocated or launched: what dsn_mask_refine refuses; an unknown mode; C outside
 * [1, 8] (mask) or [1, 2] (wiener); channels[b] outside [1, C]; reg not finite or < 0; out overlapping mix or est. */
enum { DSN_STEMS_MASK = 0, DSN_STEMS_WIENER = 1 };
int dsn_stems(dsn_ctx* ctx, const float* mix, const float* est, int B, int C, int n, int Lmax, const int32_t* lens,
              const int32_t* channels, int mode, int n_fft, int hop, int power, float eps, float reg, float* out,
              double* info_R, double* info_den, void* stream);

/* Mask-based MVDR beamforming: a microphone-array recording and the mono estimates of its sources -> one mono signal per
 * source, a linear time-invariant filter of the microphones that passes the source undistorted at the reference
 * microphone and places spatial nulls on the other sources (Souden, Benesty, Affes 2010; Heymann et al. / Erdogan et
 * al. 2016; csrc/beamform.hip, restated in float64 in tests/beamform_restatement.py).  A definition, not a trained
 * step; nothing calls it unless asked to.  mix [B][C][Lmax], est and out [B][n][Lmax] fp32 (device), C <= 8, n <= 4.
 * lens and channels (HOST, [B], or NULL: Lmax and C for every item): item b has lens[b] samples and C_b = channels[b]
 * channels; nothing at or past lens[b] and no channel >= channels[b] is read (they may hold NaN), and out is zero at or
 * past lens[b].  `ref` < C_b is the reference channel.  Padding, window, reflection, frame count F, the spectra
 * X_c(f,t), S_i(f,t) and the fp32 masks M_i(f,t) are dsn_mask_refine's (above), with the bits they have there; spectra
 * and masks are widened to fp64.  Per item, source i and bin f:
 *   statistics    N_i(f) = sum_t M_i X X^H, C_b x C_b Hermitian, the upper triangle stored; products in fp64.  Every
 *                 frame has, per source, exactly one owning workgroup, which adds its frames in increasing order
 *                 (bins below 256 over all its frames in registers; bins 256 and up a group of 2048 / n_fft frames in
 *                 registers, then into its partial); the owners' partials are added in owner order.  An owner takes whole spans of S / hop frames (S = 2048, 4096 for n_fft = 2048): one span, or
 *                 ceil(spans / 16) where the item has more than 16 spans -- a function of the item's length and the
 *                 parameters alone.
 *   interference  Q_i(f) = sum_{j != i} N_j, added in increasing j; the zero matrix for n = 1
 *   loading       lambda_i(f) = reg tr(Q_i) / C_b + eps,  A = Q_i + lambda I
 *   solve         A = L L^H by fp64 Cholesky,  Z = A^-1 N_i (all C_b columns),  tau = sum_c Re Z_cc in channel order
 *   weights       w_i(f) = Z[:, ref] / tau where tau is finite and > 0, otherwise the unit vector e_ref (tau = 0 only
 *                 where the mixture is zero in that bin on every frame)
 *   apply         Y_i(f,t) = sum_c conj(w_i,c) X_c in fp64 and in channel order, rounded once to fp32; with
 *                 DSN_BEAMFORM_POST_MASK then Y_i <- (M_i Re Y_i, M_i Im Y_i), the two fp32 products of the mask mode
 *   synthesis     dsn_mask_refine's inverse transform, overlap-add and envelope division; cropped to L
 * The scale of N_i cancels in w, so nothing is normalised by sum_t M.  With C_b = 1, w = Z / Z = 1.0 exactly: the output
 * of every source equals dsn_mask_refine with n = 1, and with DSN_BEAMFORM_POST_MASK dsn_mask_refine itself.  Silent
 * estimates give n outputs that are equal to the bit.  No floating-point atomics: an item has the same bits alone, at
 * any batch position, under any padding, from a base pointer of any 4-byte alignment, under any workspace budget and
 * in a second call.  The partials and N ((owners + 1) n C (C + 1) (n_fft / 2 + 1) doubles per item, owners =
 * min(16, spans of Lmax)) live in a workspace the context keeps; the batch is processed in chunks of as many items as
 * fit `workspace_budget` bytes (0: 512 MiB); the weights (B n (n_fft / 2 + 1) C complex doubles) are kept for the whole
 * batch outside that budget.  info_w (HOST, [B][n][n_fft / 2 + 1][C] complex as double pairs, or NULL): the weights,
 * zero in channels an item does not have; with it the stream is synchronised.  The call uploads lens and channels
 * when given and then synchronises the stream, so with them it must not be captured into a graph.  Needs no score
 * network and no codec.  It computes one filter per recording (dsn_beamform_track, below, follows moving sources);
 * dual-mono input has no spatial information and gives the channel average; its effect on separation quality is
 * unmeasured.
 * DSN_EINVAL by name, before anything is allocated or launched: what dsn_mask_refine refuses; C outside [1, 8];
 * channels[b] outside [1, C]; ref outside [0, channels[b]) for any item (the message names the item); reg not finite or
 * < 0; an unknown post-filter; a negative budget or one too small for one item (the message names the bytes needed);
 * out overlapping mix or est. */
enum { DSN_BEAMFORM_POST_NONE = 0, DSN_BEAMFORM_POST_MASK = 1 };
int dsn_beamform(dsn_ctx* ctx, const float* mix, const float* est, int B, int C, int n, int Lmax, const int32_t* lens,
                 const int32_t* channels, int ref, int n_fft, int hop, int power, float eps, float reg, int postfilter,
                 int64_t workspace_budget, float* out, double* info_w, void* stream);

/* dsn_beamform on spatially refined masks: between the estimates' masks and the MVDR filter a complex angular central
 * Gaussian mixture model (cACGMM; Ito, Araki, Nakatani 2016) learns where every source sits, with the estimates' masks
 * as time-frequency priors (Nakatani et al. 2017; Drude & Haeb-Umbach 2017: "guided source separation"), and its
 * posteriors gamma replace the masks in the statistics (csrc/spatial.hip, restated in float64 in
 * tests/spatial_restatement.py).  A definition, not a trained step; nothing calls it unless asked to.  mix, est, out,
 * lens, channels, ref, n_fft, hop, power, eps and reg are dsn_beamform's; the spectra X_c(f,t) and the fp32 masks M_k
 * are dsn_mask_refine's, with the bits they have there, widened to fp64.  Per item (C_b channels) and bin f, in fp64:
 *   setup       p(t) = sum_c |X_c|^2 in channel order; a frame is live where p > 0 (false for NaN);
 *               z(t) = X(t) / sqrt(p(t)).  Classes: K = n + 1 if noise > 0, otherwise n.  Priors
 *               a_k = (1 - noise) ((1 - floor) M_k + floor / n) for k < n, a_n = noise.  B_k = I.
 *   `iterations` times
 *     E-step    B_k = L L^H by Cholesky, q_k(t) = z^H B_k^-1 z = sum_c |y_c|^2 with L y = z, l_k = 2 sum_c log L_cc,
 *               log gamma_k(t) = log a_k - l_k - C_b log q_k, normalised over the classes in class order with the
 *               maximum subtracted
 *     M-step    over the live frames in increasing t whatever the tiling:
 *               B_k = C_b sum_t (gamma_k / q_k) z z^H / sum_t gamma_k, the identity where sum_t gamma_k is zero (a
 *               class whose prior is zero everywhere); then B_k += (mask_reg tr(B_k) / C_b + mask_eps) I.
 *               A Cholesky pivot of any B_k that is not finite and positive makes every B_k of that bin the identity
 *               from then on (gamma is then the normalised prior); the bin is flagged in info_fail.
 *   after the last M-step one more E-step gives gamma; dead frames take gamma = a.  gamma stays fp64 and is never
 *   rounded before use.  An item with one channel skips the model and takes gamma = a, and so does every item with
 *   iterations = 0: nothing has been learned, every class has B_k = I, and the posterior is the prior.
 *   statistics  N_k(f) = sum_t gamma_k X X^H for all K classes in increasing t, the upper triangle, on the
 *               unnormalised spectra as in dsn_beamform
 *   then dsn_beamform's interference, loading, solve and weights with Q_i = sum_{j != i, j < K} N_j -- the noise class
 *   enters every Q_i and gets no filter --, its apply without post-filter and its synthesis.
 * With iterations = 0, noise = 0, floor = 0, gamma is M and the call is dsn_beamform up to the order of its sums (the
 * fp32 masks of a frame sum to 1 only up to fp32 rounding, which a normalisation would move into the weights).  A NaN in an estimate makes the priors of the frames it touches NaN, every bin
 * fails its first pivot, N is NaN and w = e_ref: the reference channel is handed back.  A NaN in the mixture makes the
 * frames it touches dead; N is NaN as well and w = e_ref, with no bin flagged.  No floating-point atomics: an item has
 * the same bits alone, at any batch position, under any padding, from a base pointer of any 4-byte alignment, under
 * any workspace budget and in a second call.  The statistics, spectra, masks and flags of a chunk of items live in a
 * workspace the context keeps, (n_fft / 2 + 1) (8 (n + 1) C (C + 1) + Fs (8 C + 4 n) + 4) bytes per item with
 * Fs = 1 + ceil(Lmax / hop); the batch is processed in chunks of as many items as fit `workspace_budget` bytes
 * (0: 512 MiB); the weights are kept for the whole batch outside that budget.  info_w (HOST, as dsn_beamform's),
 * info_gamma (HOST, [B][K][n_fft / 2 + 1][Fs] doubles: gamma as the statistics used it, zero in frames an item does
 * not have) and info_fail (HOST, [B][n_fft / 2 + 1] int32: 1 where the bin failed a pivot) or NULL; with any of them the
 * stream is synchronised.  The call uploads lens and channels when given and then synchronises the stream, so with
 * them it must not be captured into a graph.  Needs no score network and no codec.  Not trained and not tuned; its
 * effect on separation quality is unmeasured; time-frequency priors only (no activity-only guidance); no gamma
 * post-filter.
 * DSN_EINVAL by name, before anything is allocated or launched: what dsn_beamform refuses (it has no post-filter);
 * iterations outside [0, 16]; noise outside [0, 0.9]; floor outside [0, 1]; mask_reg not finite or < 0; mask_eps not
 * finite or <= 0. */
int dsn_beamform_spatial(dsn_ctx* ctx, const float* mix, const float* est, int B, int C, int n, int Lmax,
                         const int32_t* lens, const int32_t* channels, int ref, int n_fft, int hop, int power, float eps,
                         float reg, int iterations, float noise, float floor, float mask_reg, float mask_eps,
                         int64_t workspace_budget, float* out, double* info_w, double* info_gamma, int32_t* info_fail,
                         void* stream);

/* dsn_beamform with block-adaptive weights: the recording is cut into blocks of `block_frames` frames, every block gets
 * the MVDR filter of the statistics of a context window of blocks around it, and every frame is filtered with the
 * weights interpolated between the centres of the two nearest blocks, so the filter follows a source that moves
 * (the per-segment beamformer of the guided-source-separation recipes since CHiME-5; csrc/beamform_track.hip, restated in
 * float64 in tests/beamform_track_restatement.py).  A definition, not a trained step; nothing calls it unless asked to.
 * mix, est, out, lens, channels, ref, n_fft, hop, power, eps, reg and postfilter are dsn_beamform's, and so is
 * everything up to the statistics: the frames, the spectra X_c(f,t), the fp32 masks M_i, F = 1 + ceil(L_b / hop), the
 * widening to fp64.  With Tb = block_frames, per item, source i and bin f:
 *   blocks         block k holds the frames [k Tb, min(F, (k + 1) Tb)); K = ceil(F / Tb) from the item's own length; the
 *                  last block is as short as it falls
 *   partials       P_i^(k) = sum_{t in block k} M_i X X^H in increasing t whatever the tiling, the upper triangle,
 *                  products in fp64; every block has exactly one owning workgroup per source (bins below 256 over all
 *                  the block's frames in registers; bins 256 and up a group of 2048 / n_fft frames in registers, then
 *                  into the partial)
 *   context        N_i^(k) = sum_{j = max(0, k - context)}^{min(K - 1, k + context)} P_i^(j), added in increasing j
 *   weights        w_i^(k)(f): dsn_beamform's interference, loading, Cholesky solve, tau and e_ref fallback on N^(k)
 *   frame weights  in integers: num = 2 t + 1 - Tb; num <= 0: k0 = 0, alpha = 0; otherwise k0 = num div 2 Tb and
 *                  alpha = (double)(num mod 2 Tb) / (double)(2 Tb); k0 >= K - 1: k0 = K - 1, alpha = 0 (the first and the
 *                  last half block hold their block's weights).  With interpolate = 0: k0 = t div Tb, alpha = 0.
 *                  w(t) = w^(k0) + alpha (w^(k0+1) - w^(k0)) per real and imaginary part in fp64, not contracted; where
 *                  alpha = 0, w(t) = w^(k0) and block k0 + 1 is not read.  Equal neighbours give exactly that weight.
 *   apply          Y_i(f,t) = sum_c conj(w_i,c(t)) X_c in fp64 and in channel order, rounded once to fp32; post-filter and
 *                  synthesis are dsn_beamform's
 * One block (Tb >= F) is dsn_beamform up to the order of its sums.  With C_b = 1 every w is 1.0 exactly and the output
 * is dsn_mask_refine's as in dsn_beamform; silent estimates give n equal outputs; context >= K - 1 gives every block
 * the same weights and interpolate = 1 the bits of interpolate = 0.  No floating-point atomics: an item has the same
 * bits alone, at any batch position, under any padding, from a base pointer of any 4-byte alignment, under any
 * workspace budget and in a second call.  With Kmax = ceil((1 + ceil(Lmax / hop)) / Tb), the partials, their context
 * sums, the weights (they scale with Kmax) and the blocks' channel counts live in a workspace the context keeps,
 * Kmax (8 n (n_fft / 2 + 1) (2 C (C + 1) + 2 C) + 4) bytes per item; the batch is processed in chunks of as many items
 * as fit `workspace_budget` bytes (0: 512 MiB); an item that does not fit is refused, not split.  info_w (HOST,
 * [B][Kmax][n][n_fft / 2 + 1][C] complex as double pairs, or NULL): the blocks' weights, zero in blocks and channels an
 * item does not have; with it the stream is synchronised.  The call uploads lens and channels when given and then
 * synchronises the stream, so with them it must not be captured into a graph.  Needs no score network and no codec.
 * Blocks of fixed length, not speaker-activity segments; no recursive or online form; no combination with
 * dsn_beamform_spatial; its effect on separation quality is unmeasured.
 * DSN_EINVAL by name, before anything is allocated or launched: what dsn_beamform refuses; block_frames outside
 * [4, 2^20]; context outside [0, 64]; interpolate not 0 or 1; Kmax above 4096. */
int dsn_beamform_track(dsn_ctx* ctx, const float* mix, const float* est, int B, int C, int n, int Lmax,
                       const int32_t* lens, const int32_t* channels, int ref, int n_fft, int hop, int power, float eps,
                       float reg, int postfilter, int block_frames, int context, int interpolate,
                       int64_t workspace_budget, float* out, double* info_w, void* stream);

/* The design of the beamforming weights: what dsn_beamform, dsn_beamform_spatial and dsn_beamform_track do with the
 * statistics of a bin once A is factored (csrc/beamform_design.hip, restated in float64 in
 * tests/beamform_design_restatement.py).  Everything up to and including A = Q_i + lambda I = L L^H is dsn_beamform's: the
 * statistics N_k, the interference Q_i over all classes j != i, the loading lambda = reg tr(Q_i) / C_b + eps, the identity
 * block for the channels an item does not have.  Then, per (item, source, bin), in fp64:
 *   whitening   G = L^-1 N_i L^-H by two forward solves per column (Y = L^-1 N_i, then G = L^-1 Y^H); Hermitian and
 *               positive semidefinite; the diagonal is taken as real
 *   eigenpair   (mu, u), the principal eigenpair of G, by a cyclic-by-row two-sided complex Jacobi iteration: `sweeps`
 *               sweeps (1 .. 30) over the pairs (p, q), p < q, row by row.  A pair with G_pq = 0 exactly is skipped.
 *               Otherwise theta = (G_qq - G_pp) / (2 |G_pq|), t = sign(theta) / (|theta| + sqrt(1 + theta^2)) (sign(0) = 1;
 *               t = 1 / (2 theta) where |theta| > 1e150), c = 1 / sqrt(1 + t^2), s = t c, e = G_pq / |G_pq|,
 *               J = [[c, s e], [-s conj(e), c]] on (p, q); G <- G J, V <- V J, then G <- J^H G (V starts as I; nothing
 *               is set to zero by hand).  After the last sweep mu is the largest diagonal entry of G (ties: the lowest
 *               index m) and u = V[:, m], a unit vector.
 *   steering    v = L^-H u and h = L u = A v, the steering estimate; v^H A v = 1
 *   weights     DSN_BEAMFORM_DESIGN_SOUDEN: dsn_beamform's solve and weights, none of the above.
 *               DSN_BEAMFORM_DESIGN_RANK1:  w = v conj(h_ref), the MVDR filter A^-1 h / (h^H A^-1 h) conj(h_ref) of the
 *               rank-one model N_i ~ h h^H; it does not depend on the phase of u.
 *               DSN_BEAMFORM_DESIGN_GEV:    w = (v p) |h| / sqrt(C_b) with p = conj(h_ref) / |h_ref| (1 where |h_ref| = 0)
 *               and |h|^2 summed over the item's channels in channel order: the max-SNR filter (Warsitz & Haeb-Umbach
 *               2007; Heymann et al. 2016) with blind analytic normalisation on the loaded A, its phase fixed at the
 *               reference microphone.  Not distortionless.
 *   fallbacks   w = e_ref where a Cholesky pivot or mu is not finite and positive (silent estimates: mu = 0; a NaN
 *               estimate); an item with C_b = 1 takes w = 1.0 exactly for every design; channels an item does not have
 *               get zero weight.
 * The apply step, the post-filter, dsn_beamform_track's blocks and interpolation and dsn_beamform_spatial's noise class
 * (it enters Q_i; the first n classes get a filter) are untouched, and so are the invariants: no floating-point atomics,
 * an item has the same bits alone, at any batch position, under any padding, under any workspace budget and in a second
 * call.  The three _design calls take the arguments of their namesakes with `design, sweeps` after `reg`; with
 * DSN_BEAMFORM_DESIGN_SOUDEN they are their namesakes to the bit (sweeps is still checked).  Not trained, not tuned;
 * no eigenvalue-based rank selection, no MPDR, no LCMV; the effect on real recordings is unmeasured.
 * DSN_EINVAL by name: what the namesake refuses; an unknown design; sweeps outside [1, 30].
 *
 * dsn_beamform_solve is the weights launch alone, for callers with their own covariances: N (DEVICE,
 * [items][classes][C (C + 1)][bins] doubles: per class the upper triangle of a Hermitian C x C matrix row after row,
 * every entry a plane of real parts followed by a plane of imaginary parts, [bins] each), classes = n or n + 1 (all
 * classes enter Q_i, the first n get a filter), channels (HOST, [items], or NULL: C each), ref, bins in [1, 1025], reg
 * and eps as above -> w (DEVICE, [items][n][bins][C] complex as double pairs, info_w's layout).  Entries of channels an
 * item does not have are not read.  One launch on `stream`, nothing is synchronised unless channels is given (it is
 * uploaded, as above).  DSN_EINVAL by name: N or w null; items outside [1, 2^24]; items n bins above 2^31; C, n,
 * classes, bins, reg, eps, channels[b], ref, design or sweeps out of range. */
enum { DSN_BEAMFORM_DESIGN_SOUDEN = 0, DSN_BEAMFORM_DESIGN_RANK1 = 1, DSN_BEAMFORM_DESIGN_GEV = 2 };
int dsn_beamform_design(dsn_ctx* ctx, const float* mix, const float* est, int B, int C, int n, int Lmax,
                        const int32_t* lens, const int32_t* channels, int ref, int n_fft, int hop, int power, float eps,
                        float reg, int design, int sweeps, int postfilter, int64_t workspace_budget, float* out,
                        double* info_w, void* stream);
int dsn_beamform_spatial_design(dsn_ctx* ctx, const float* mix, const float* est, int B, int C, int n, int Lmax,
                                const int32_t* lens, const int32_t* channels, int ref, int n_fft, int hop, int power,
                                float eps, float reg, int design, int sweeps, int iterations, float noise, float floor,
                                float mask_reg, float mask_eps, int64_t workspace_budget, float* out, double* info_w,
                                double* info_gamma, int32_t* info_fail, void* stream);
int dsn_beamform_track_design(dsn_ctx* ctx, const float* mix, const float* est, int B, int C, int n, int Lmax,
                              const int32_t* lens, const int32_t* channels, int ref, int n_fft, int hop, int power,
                              float eps, float reg, int design, int sweeps, int postfilter, int block_frames, int context,
                              int interpolate, int64_t workspace_budget, float* out, double* info_w, void* stream);
int dsn_beamform_solve(dsn_ctx* ctx, const double* N, const int32_t* channels, int ref, int items, int C, int n,
                       int classes, int bins, float reg, float eps, int design, int sweeps, double* w, void* stream);

/* Weighted prediction error (WPE) dereverberation: the channels of a reverberant recording in, the same channels with
 * the late reverberation predicted from their own delayed past and subtracted out (Nakatani et al. 2010; Yoshioka &
 * Nakatani 2012; the offline recipe; csrc/dereverb.hip, restated in float64 in tests/dereverb_restatement.py).  A
 * definition, not a trained step; nothing calls it unless asked to.  mix and out [B][C][Lmax] fp32 (device), C <= 8,
 * taps K in [1, 16], delay D in [1, 8], C K <= 80, iterations I in [1, 8].  lens and channels (HOST, [B], or NULL: Lmax
 * and C for every item): item b has L_b = lens[b] samples and C_b = channels[b] channels; nothing at or past lens[b]
 * and no channel >= channels[b] is read (they may hold NaN), and out is zero there.  Padding, window, reflection, frame
 * count F and the spectra Y_c(f,t) are dsn_mask_refine's (above), with the bits they have there, widened to fp64.  Per
 * item and bin f, all in fp64:
 *   stacked past  y~(t) in C^(C_b K), entry k C_b + c = Y_c(f, t - D - k), zero where t - D - k < 0
 *   start         X = Y
 *   I times       lambda(t) = (1 / C_b) sum_c |X_c(t)|^2 in channel order;  m = max_t lambda(t), taken as an integer
 *                 maximum on the bits (exact in any order);  lambda(t) <- max(lambda(t), 1e-10 m);  where m == 0 the bin
 *                 passes through (G = 0).
 *                 R = sum_t y~ y~^H / lambda(t) (Hermitian, one triangle kept),  P = sum_t y~ Y(t)^H / lambda(t)
 *                 (C_b K x C_b), both added in increasing t whatever the tiling: y~_i / lambda(t) is formed first (a
 *                 multiplication with the quotient 1 / lambda(t)), then the product.
 *                 delta = reg tr(R) / (C_b K) + eps,  A = R + delta I = L L^H by Cholesky,  G = A^-1 P.  A pivot that is
 *                 not finite and positive sets G = 0 for this and the remaining iterations of that bin; the bin is
 *                 counted.
 *                 X_c(t) = Y_c(t) - sum_j conj(G[j][c]) y~_j(t) in index order
 *   after the last iteration X is rounded once to fp32; synthesis is dsn_mask_refine's: the inverse transform, the
 *   overlap-add, the envelope division, cropped to L_b.
 * Consequences.  No floating-point atomics: an item has the same bits alone, at any batch position, under any padding,
 * from a base pointer of any 4-byte alignment, under any workspace budget and in a second call.  An item with F <= D
 * has P = 0 exactly, so G = 0 and X = Y: every channel comes back as dsn_mask_refine of that channel with n = 1, bit
 * for bit; so does a silent item.  Scaling the input by a power of two scales lambda by its square and leaves R, P,
 * delta and G bit-identical: dereverb(2^k x) = 2^k dereverb(x) to the bit, away from under- and overflow.
 * The spectra, X, lambda, G and the per-bin flags of a chunk of items live in a workspace the context keeps,
 * (n_fft / 2 + 1) (8 (2 C^2 K + Fs + 2 C Fs) + 4) bytes per item with Fs = 1 + ceil(Lmax / hop); the batch is processed
 * in chunks of as many items as fit `workspace_budget` bytes (0: 512 MiB).  info_G (HOST, [B][n_fft / 2 + 1][C K][C]
 * complex as double pairs, or NULL): the last iteration's filter, row k C_b + c of the item's own system, zero outside
 * it.  info_fail (HOST, [B] int32, or NULL): the bins of the item that passed through because of a failed pivot.  With
 * either one the stream is synchronised.  The call uploads lens and channels when given and then synchronises the
 * stream, so with them it must not be captured into a graph.  Needs no score network and no codec.  Offline: one
 * filter per recording, no PSD context, no recursive form; its effect on separation quality is unmeasured.
 * DSN_EINVAL by name, before anything is allocated or launched: what dsn_mask_refine refuses; C, taps, delay, C taps or
 * iterations outside the limits above; channels[b] outside [1, C]; reg not finite or < 0; eps not finite or <= 0; a
 * negative budget or one too small for one item (the message names the bytes needed); out overlapping mix. */
int dsn_dereverb(dsn_ctx* ctx, const float* mix, int B, int C, int Lmax, const int32_t* lens, const int32_t* channels,
                 int n_fft, int hop, int taps, int delay, int iterations, float reg, float eps, int64_t workspace_budget,
                 float* out, double* info_G, int32_t* info_fail, void* stream);

/* Ensemble combine: K candidate separations of the same mixtures (K draws of the diffusion sampler) -> one separation
 * (csrc/ensemble.hip, restated in float64 in tests/ensemble_restatement.py).  A definition, not a trained step; nothing
 * calls it unless asked to.  cands [B][K][n][Lmax], mix [B][Lmax] or NULL, out [B][n][Lmax] fp32 (device),
 * 1 <= K <= 16, 1 <= n <= 4.  lens (HOST, [B], or NULL: every item is Lmax long): item b has L_b = lens[b] samples;
 * nothing at or past lens[b] is read (the padding may hold NaN) and out is written as zero there.  Per item:
 *   Gram       the K n candidate rows, row (k, i) = k n + i, plus the mixture's row m = K n when mix is given (R rows):
 *              G[p][q] = sum_{t < L_b} x_p[t] x_q[t].  fp32 x fp32 products are exact in fp64 and are summed in fp64 in a
 *              fixed order over tiles of 2048 samples counted from the item's own start: per thread in stride order, a
 *              fixed tree, the tile partials in index order; plain stores, no atomics.  An item has the same bits alone,
 *              at any batch position and under any padding.  |G - exact| <= L_b 2^-53 sum_t |x_p[t]| |x_q[t]|.
 *   alignment  S[a][k] = max over the n! permutations pi of sum_i G[(a, i)][(k, pi(i))] (raw inner products, the window
 *              stitch's rule; ties go to the lexicographically first permutation).  S is symmetric: it is formed for
 *              a < k and used for (k, a) as well, so with K = 2 the two totals are one number.  The anchor a* = argmax_a
 *              sum_{k != a} S[a][k] (k ascending; ties to the lowest index; 0 for K = 1, 2).  perm[k] is the maximiser for
 *              (a*, k) and perm[a*] the identity: slot i of candidate k is its source perm[k][i].
 *   info       E_k = (G[m][m] - 2 sum_i G[m][(k, i)]) + sum_i sum_j G[(k, i)][(k, j)] (m the mixture's row; i, then j,
 *              ascending) is |mix - sum_i cand_k,i|^2 and resid_db[k] = 10 log10(max(E_k, 0) / G[m][m]); best = argmin_k
 *              E_k, ties to the lowest index.  E_k is a difference of sums of size |mix|^2: a relative residual energy
 *              below about L_b 2^-53 (-111 dB at 64000 samples) is rounding, not signal -- a candidate that sums exactly to
 *              the mixture reports -inf or a figure below that floor.  A silent mixture gives NaN.  Without mix best is
 *              -1 and resid_db NaN.  agree_db[k][i] is the SI-SDR of row c = (k, perm[k][i]) against the anchor's row
 *              a = (a*, i): 10 log10(g^2 / max(G[a][a] G[c][c] - g^2, 0)) with g = G[a][c]; NaN when either energy is 0,
 *              otherwise +inf for k = a*.
 *   combine    one gather launch over the aligned rows c_k,i = cands[k][perm[k][i]], fp32, contraction off:
 *              DSN_ENSEMBLE_MEAN    s = ((c_0,i + c_1,i) + ...) + c_K-1,i in candidate order, every addition's rounding
 *                                   error (Knuth's two-sum, six fp32 operations, exact) added into e in the same
 *                                   order; then (s + e) / float(K), s / float(K) where e is 0 (K = 1: a copy).  The bare sequential sum does
 *                                   not return x from 8 or 16 copies of x (5 x, 6 x, 7 x each round); this one
 *                                   does for K = 2, 4, 8, 16: e is exact there and s + e = K x.  A sum that
 *                                   overflows gives NaN, not inf.
 *              DSN_ENSEMBLE_MEDIAN  the middle of the K values per sample (stable order); even K: (lo + hi) * 0.5f of
 *                                   the two middle values
 *              DSN_ENSEMBLE_BEST    c_best,i (refused without mix)
 *              DSN_ENSEMBLE_MEDOID  c_a*,i
 * 16-byte loads and stores where Lmax is a multiple of 4 and the bases are aligned, scalar ones otherwise, with the
 * same bits.  Every *_out is a HOST array or NULL: perm_out [B][K][n], anchor_out / best_out [B], resid_db_out [B][K],
 * agree_db_out [B][K][n], gram_out [B][R][R]; with any of them the stream is synchronised.  The call uploads `lens` when
 * it is given and differs from the last upload, and then synchronises the stream.  Needs no score network and no codec;
 * two calls give identical bits.
 * DSN_EINVAL by name, before anything is allocated or launched: cands or out null; B outside [1, 65535]; K outside
 * [1, 16]; n outside [1, 4]; Lmax outside [1, 2^30]; an unknown mode; DSN_ENSEMBLE_BEST without mix; lens[b] outside
 * [1, Lmax]; out overlapping cands. */
enum { DSN_ENSEMBLE_MEAN = 0, DSN_ENSEMBLE_MEDIAN = 1, DSN_ENSEMBLE_BEST = 2, DSN_ENSEMBLE_MEDOID = 3 };
int dsn_ensemble_combine(dsn_ctx* ctx, const float* cands, const float* mix, int B, int K, int n, int Lmax,
                         const int32_t* lens, int mode, float* out, int32_t* perm_out, int32_t* anchor_out,
                         int32_t* best_out, double* resid_db_out, double* agree_db_out, double* gram_out, void* stream);

/* The first and the last step of separating audio files, on the device: the `data` payloads of WAV files to fp32 and
 * fp32 back to payloads, and the reference's output gain (src/inference/separate.py:73-78).  Restated in numpy in
 * tests/pcm_restatement.py.  All three need no score network and no codec.  Every per-item table (offset, frames,
 * channels, encoding, lens) is a HOST array, like `lens` of the resampling call: the call uploads it and synchronises
 * the stream, so it must not be captured into a graph.  Samples are little-endian; a payload interleaves its channels.
 *   decode   bytes [nbytes] (device, any alignment) holds the payloads of B files back to back: item b is frames[b]
 *            frames of channels[b] samples of encoding[b] from byte offset[b] (any alignment).  -> out [B][Cout][Lmax]
 *            fp32 (device) in one launch, whatever mix of encodings and channel counts the batch holds.  The
 *            conversions are those of torchaudio.load(normalize=True):
 *              U8  (v - 128) / 128        S16  v / 2^15        S24  v / 2^23 (three bytes, sign-extended)
 *              S32 float32(v) 2^-31, v rounded once to nearest even        F32  the bits, NaN payloads included
 *              F64 rounded once to fp32 (nearest even, overflow to +-inf, every NaN to the quiet NaN 0x7fc00000)
 *            -- all exact but S32 and F64, all defined to the bit.  downmix != 0: Cout must be 1 and a frame becomes
 *            (x_0 + .. + x_{C-1}) / C in fp32 in that order, the expression of the resampling call (a one-channel item
 *            is not divided: its bits pass).  downmix == 0: channel c < channels[b] goes to out[b][c], the channels
 *            past an item's own count are written as zero.  Samples at or past frames[b] are written as zero.  No byte
 *            outside [0, nbytes) is loaded, and none outside an item's own range takes part in its result.
 *   encode   x [R][Lmax] fp32 (device), one row per (file, speaker), lens[r] samples each -> R mono payloads in bytes
 *            [nbytes] (device), row r at byte offset[r].  encoding is S16, S24 or F32.  An integer encoding of b bits:
 *            q = rint(x 2^(b-1)) (ties to even; the product is exact), clamped to [-2^(b-1), 2^(b-1) - 1], NaN -> 0.
 *            clipped [R] (HOST, may be NULL) counts, per row, the samples whose rounded value lay outside that range
 *            or was not finite (integer atomics: the count does not depend on their order); F32 copies the bits and
 *            counts nothing.  Only the lens[r] bytes-per-sample bytes of a row are written: whatever lies between and
 *            after the rows stays as it was.  Two calls give identical bytes.
 *   encode_frames  the same for multichannel payloads: x [R][C][Lmax], row r is lens[r] frames of its first channels[r]
 *            channels (lens, channels: HOST, or NULL: Lmax and C each), interleaved sample by sample at byte
 *            offset[r].  Quantisation, clamping and NaN handling are encode's; clipped[r] is summed over the row's
 *            channels.  With C = 1 the bytes are encode's.  Only a row's own bytes are written.
 *   scale    mix [B][Lmax], sep [B][n][Lmax] fp32 (device) -> out [B][n][Lmax]:
 *              alpha[b][i] = sum_t mix[b][t] sep[b][i][t] / sum_t (sep[b][i][t]^2 + 1e-10)  over t < lens[b],
 *            both sums in fp64 over exact fp64 products, in an order a row's own length fixes (per thread in stride
 *            order, a fixed tree, the tile sums in index order; no floating-point atomics: a row gives the bits it
 *            gives alone, and so does a second call); alpha is rounded once to fp32 and out = alpha sep is one fp32
 *            product.  An all-zero estimate gives alpha = 0 and a zero row.  lens (HOST, or NULL: Lmax each); nothing
 *            at or past lens[b] is read, and out is written as zero there.  alpha_out [B][n] (HOST, may be NULL: the
 *            call then only enqueues once lens is on the device).
 * DSN_EINVAL by name, before anything is allocated or launched: a null pointer; B, R, n or Lmax < 1; B or R > 65535;
 * an encoding outside the list (decode) or other than S16, S24, F32 (encode); frames[b] outside [1, Lmax];
 * channels[b] < 1; a frame of more than DSN_PCM_MAX_FRAME_BYTES bytes; downmix with Cout != 1; without downmix
 * channels[b] > Cout; an item whose bytes leave [0, nbytes); lens[r] outside [1, Lmax]; rows of the encoder whose
 * payloads overlap or leave the buffer; (encode_frames) C < 1 or channels[r] outside [1, C]. */
enum { DSN_PCM_U8 = 0, DSN_PCM_S16 = 1, DSN_PCM_S24 = 2, DSN_PCM_S32 = 3, DSN_PCM_F32 = 4, DSN_PCM_F64 = 5 };
#define DSN_PCM_MAX_FRAME_BYTES 48
int dsn_pcm_decode(dsn_ctx* ctx, const void* bytes, int64_t nbytes, int B, const int64_t* offset, const int32_t* frames,
                   const int32_t* channels, const int32_t* encoding, int downmix, float* out, int Cout, int Lmax,
                   void* stream);
int dsn_pcm_encode(dsn_ctx* ctx, const float* x, int R, int Lmax, const int32_t* lens, int encoding, void* bytes,
                   int64_t nbytes, const int64_t* offset, int64_t* clipped, void* stream);
int dsn_pcm_encode_frames(dsn_ctx* ctx, const float* x, int R, int C, int Lmax, const int32_t* lens,
                          const int32_t* channels, int encoding, void* bytes, int64_t nbytes, const int64_t* offset,
                          int64_t* clipped, void* stream);
int dsn_scale_output(dsn_ctx* ctx, const float* mix, const float* sep, int B, int n, int Lmax, const int32_t* lens,
                     float* out, float* alpha_out, void* stream);

/* Programme loudness, true peak and one gain on the device: the level step in front of dsn_pcm_encode* (ITU-R BS.1770-4 /
 * EBU R 128 integrated loudness; csrc/loudness.hip, restated in float64 in tests/loudness_restatement.py).  A
 * measurement and a single gain, not a limiter; nothing calls it unless asked to.  x [B][C][Lmax] fp32 (device), C <= 2.
 * Item b has channels[b] <= C channels, lens[b] samples and its own rate rates[b] in Hz, any integer in [8000, 192000];
 * every channel has weight 1.
 *   K-weighting  two biquads in cascade, formed on the host in fp64 from the rate fs (the libebur128 / pyloudnorm
 *                formulation).  Shelf: f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196,
 *                K = tan(pi f0 / fs), Vh = 10^(G / 20), Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2,
 *                b = [Vh + Vb K / Q + K^2, 2 (K^2 - Vh), Vh - Vb K / Q + K^2] / a0, a = [1, 2 (K^2 - 1) / a0,
 *                (1 - K / Q + K^2) / a0].  High-pass: f0 = 38.13547087602444, Q = 0.5003270373238773, K, a0 and a by
 *                the same expressions, b = [1, -2, 1] (not divided by a0).  At 48 kHz these are the standard's table.
 *                dsn_kweight_coeffs(fs, out): out = shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2 (no context, no
 *                GPU); DSN_EINVAL for a rate outside [8000, 192000] or a null out.
 *   blocks       h = (fs + 5) / 10 by integer division (11025 Hz gives 1103).  Block j covers samples [j h, j h + 4 h)
 *                of the filtered signal y, which starts from zero state at sample 0; only complete blocks count:
 *                J = (L - 4 h) / h + 1 when L >= 4 h, else 0.  z_j = sum_c mean(y_c^2) over the block,
 *                l_j = -0.691 + 10 log10(z_j).
 *   gates        absolute: l_j > -70.  Gamma = -0.691 + 10 log10(mean of z_j over the absolute-gated blocks) - 10.
 *                I = -0.691 + 10 log10(mean of z_j over the blocks with l_j > -70 and l_j > Gamma); -inf when no
 *                block passes.
 *   true peak    the maximum of |.| over all channels of the item interpolated to four times its rate by this
 *                library's resampler at the ratio 1 -> 4 (dsn_resample_plan(1, 4): 4 phases of 13 taps, zero beyond an
 *                item's own ends), each value one fp32 product and support - 1 fused multiply-adds in tap order.  The
 *                sample peak is max |x|.  Both are exact maxima: they do not depend on the order of reduction.  A
 *                non-finite sample makes both peaks NaN and is counted.  Without want_true_peak the true peak is NaN.
 * The recursion runs in fp64 over chunks of 256 samples counted from the item's own start: a first launch filters
 * every chunk from zero state and keeps its final state (four doubles), one thread per (item, channel) carries the
 * true state across the chunks with the 4 x 4 zero-input transition matrix raised to the chunk length (formed on the
 * host in fp64 per distinct rate), a second launch filters every chunk again from its true state and adds y^2 in fp64
 * in sample order into the two h-sample segments the chunk touches; a block is four consecutive segments, a segment
 * the sum of its chunks' parts in chunk order, and one pass per item forms z_j, the gates and I in fp64 in index
 * order.  The peaks are one more launch that stages a tile and its halo in LDS (16-byte loads where a quad is aligned
 * and whole) and writes no interpolated signal.  No floating-point atomics (the maxima and the count are integer
 * atomics, which no order changes): an item has the same bits alone, at any batch position, under any padding, from a
 * base pointer of any 4-byte alignment and in a second call -- they depend on its own samples, length, rate and
 * channel count alone.  Nothing at or past lens[b], or in a channel an item does not have, is read (it may hold NaN).
 *   dsn_loudness    stats_host [B][6] doubles (HOST): I (LUFS), true peak (linear), sample peak (linear), J, the number
 *                   of blocks passing both gates, the count of non-finite samples.  lens, channels and rates are HOST
 *                   arrays; lens and channels may be NULL (Lmax and C for every item).  The call uploads its tables and
 *                   synchronises the stream: it must not be captured into a graph.  The workspace lives in the context
 *                   and grows.  Needs no score network and no codec.
 *   dsn_apply_gain  x [R][C][Lmax] -> out [R][C][Lmax]: out = gain[r] x as one fp32 product per sample; zero at or past
 *                   lens[r] and in the channels past channels[r], where nothing is read.  gain [R] is a HOST fp32 array.
 *                   16-byte loads and stores where the rows are aligned, scalar ones otherwise, with the same bits.
 *                   out may be x itself (any other overlap is refused).
 * The gain that reaches a target is the caller's to form from the statistics (ditsep_amd.native.loudness_gain:
 * g_dB = target - I_src, at most ceiling - 20 log10(TP) with a true-peak ceiling, 0 dB for I_src = -inf; 10^(g_dB / 20)
 * rounded once to fp32).
 * DSN_EINVAL by name, before anything is allocated or launched: a null pointer (x, rates, stats_host; x, gain, out);
 * B or R < 1 or > 65535; C outside [1, 2]; channels[b] outside [1, C]; lens[b] outside [1, Lmax]; a rate outside
 * [8000, 192000]; Lmax < 1 or > 2^30. */
int dsn_kweight_coeffs(int fs, double* out);
int dsn_loudness(dsn_ctx* ctx, const float* x, int B, int C, int Lmax, const int32_t* lens, const int32_t* channels,
                 const int32_t* rates, int want_true_peak, double* stats_host, void* stream);
int dsn_apply_gain(dsn_ctx* ctx, const float* x, int R, int C, int Lmax, const int32_t* lens, const int32_t* channels,
                   const float* gain, float* out, void* stream);

/* True-peak look-ahead limiter: a time-varying gain that lowers only the neighbourhood of the peaks, so that the rest of
 * a programme can rise to a loudness target its true-peak ceiling would otherwise forbid (csrc/limiter.hip, restated in
 * float64 in tests/limiter_restatement.py).  Nothing calls it unless asked to.  x [R][C][Lmax] fp32 (device), C <= 2;
 * row r has channels[r] <= C channels, lens[r] samples and the rate rates[r] in [8000, 192000] Hz.  A group is the set
 * of rows that share one gain curve: group [R] holds 0 .. G - 1 in non-decreasing order, and the rows of a group share
 * one length and one rate.  All arithmetic is fp32 without contraction, except where an fma is written.  For group q
 * with the pre-gain G_q = pregain[q], the ceiling c (linear) and the half-window
 * W = max(1, floor(lookahead_ms fs / 1000 + 1/2)), 1 <= W <= 1024:
 *   1 pre-gain   y = G_q x, one product per sample (the bits of dsn_apply_gain).
 *   2 envelope   p[t] = max over the group's rows and channels of max(|y[t]|, |u[4 t]|, .., |u[4 t + 3]|), u the row
 *                interpolated 1 -> 4 as dsn_loudness forms its true peak (dsn_resample_plan(1, 4): one product and
 *                support - 1 fmas in tap order, zero beyond the item's own ends).  A non-finite y is counted and makes
 *                the group's whole curve NaN.
 *   3 required   r[t] = min(1, c / p[t]) by a correctly rounded division, 1 where p = 0; and where the fp32 product
 *                r[t] p[t] rounds above c (the quotient was rounded up), r[t] is the next float below.  With that step
 *                fl(g[t] p[t]) <= c holds for every sample whatever the rounding does, since g <= r below.
 *   4 hold       m[t] = min over |s - t| <= W of r[s], with r = 1 outside [0, len).
 *   5 smoothing  g[t] = max(0, min(r[t], 1 - a[t])), a[t] = sum_{k = -W .. W} w[k] (1 - m[t + k]) accumulated from 0 by
 *                fma in increasing k, w[k] = (1/2 + 1/2 cos(pi k / (W + 1))) / (W + 1) formed on the host in fp64 and
 *                rounded once (the exact sum is 1).  It is written on the deficit 1 - m: where no sample within 2 W needs
 *                reducing every term is +0, g is exactly 1.0f and out is y bit for bit -- and a tile or a sample that
 *                skips the sum there has the bits of the sum.
 *   6 output     out = y g[t] = (G_q x) g[t], two products, for every row of the group.
 * Two launches over tiles of 2048 samples counted from the group's own start: the envelope (every row of the group
 * through LDS with the interpolator's halo, 16-byte loads where a quad is aligned and whole) writes r to a workspace in
 * the context; the second stages r over the tile and 2 W on either side, forms the hold by doubling minima (a minimum
 * does not depend on its order), then a and g.  No floating-point atomics: a group's curve has the same bits alone, at
 * any batch position, under any padding, from a base pointer of any 4-byte alignment and in a second call.  Symmetric
 * (zero-phase, release = attack), offline; no soft knee, no clipper.  The true peak of out as dsn_loudness measures it
 * is NOT bounded by c by theorem (interpolating g y is not g times the interpolation): a caller that promises a ceiling
 * measures again and trims (ditsep_amd.native.Engine.loudness_normalize does).
 *   dsn_limiter_curve  curve [G][Lmax] fp32 (device): g over [0, len), 1.0f at and past len.  envelope: NULL, or
 *                      [G][Lmax] fp32 (device) that receives p over [0, len) (not written elsewhere).  stats_host
 *                      [G][3] doubles (HOST): the smallest g (NaN with non-finite samples), the number of samples with
 *                      g < 1, the count of non-finite samples.  lens, channels, rates, group and pregain are HOST arrays;
 *                      lens and channels may be NULL.  Uploads its tables and synchronises the stream: not for capture.
 *   dsn_apply_curve    x [R][C][Lmax] -> out [R][C][Lmax]: out = (pregain[group[r]] x) curve[group[r]][t]; zero at or
 *                      past lens[r] and in the channels past channels[r], where nothing is read.  Any rows: group[r] in
 *                      [0, G) in any order, so the curve of the stems can be applied to their mixture.  curve is
 *                      [G][Lmax] with this call's Lmax.  out may be x itself (any other overlap is refused).
 * DSN_EINVAL by name, before anything is allocated or launched: what dsn_loudness refuses; a null group, pregain or
 * curve; G < 1 or (curve) > R; a group label outside [0, G) or (curve) out of order; rows of a group that disagree on
 * length or rate; W outside [1, 1024] or a look-ahead that is negative or not finite; a ceiling that is not finite and
 * positive; a pre-gain that is not finite. */
int dsn_limiter_curve(dsn_ctx* ctx, const float* x, int R, int C, int Lmax, const int32_t* lens, const int32_t* channels,
                      const int32_t* rates, const int32_t* group, int G, const float* pregain, float ceiling,
                      double lookahead_ms, float* curve, float* envelope, double* stats_host, void* stream);
int dsn_apply_curve(dsn_ctx* ctx, const float* x, int R, int C, int Lmax, const int32_t* lens, const int32_t* channels,
                    const int32_t* group, int G, const float* pregain, const float* curve, float* out, void* stream);

/* Speaker activity of separated stems: per item, source and STFT frame the decision "this stem carries its speaker
 * here", and a gate that makes the other stretches digital silence (csrc/activity.hip, restated in float64 in
 * tests/activity_restatement.py).  A decision rule on separated estimates -- a level floor relative to the recording
 * plus a dominance test between the stems, with hysteresis and minimum durations --, not a trained voice-activity
 * detector, and nothing calls it unless asked to.  Per item, with L = lens[b] and estimates s_i [L] (i < n):
 *   frames     dsn_mask_refine's (above): periodic Hann, centred, reflected at the item's own end, F = 1 + ceil(L / hop)
 *              frames, fp32 spectra S_i(j, t) with the bits they have there
 *   energy     E_i(t) = sum_{j = j_lo .. j_hi} (re^2 + im^2), every term and the sum in fp64 from the fp32 spectrum, in
 *              increasing j.  The caller turns a band in Hz into bins: j_lo = ceil(f_lo n_fft / fs), j_hi =
 *              min(n_fft / 2, floor(f_hi n_fft / fs)).
 *   level      lev_i(t) = (sum_{u = max(0, t - h)}^{min(F - 1, t + h)} E_i(u)) / count, in increasing u, one division
 *              (h = half_width)
 *   peak, top  P = max_{i,t} lev_i(t), top(t) = max_i lev_i(t).  A NaN compares false everywhere: its frame is inactive
 *              and P and top pass it over.  P = 0 makes the item inactive throughout.
 *   on, stay   on_i(t) = lev >= P c_r and lev >= top(t) c_d; stay_i(t) the same with c_r_stay, c_d_stay.  The caller
 *              passes the four factors as doubles (c_r = 10^(-range_db / 10), c_d = 10^(-dominance_db / 10), the stay
 *              factors with hysteresis_db added to both); the device multiplies and compares, contraction off.
 *   hysteresis a_i(t) = on_i(t) or (a_i(t - 1) and stay_i(t)), a_i(-1) = 0
 *   run rules  in this order: an off-run between two on-runs that is shorter than min_off frames becomes on (the
 *              stretches before the first and after the last on-run never do); an on-run shorter than min_on frames is
 *              cleared; every remaining run [s, e) becomes [max(0, s - pad), min(F, e + pad)) and runs that touch merge.
 * act [B][n][Fmax] bytes (device, Fmax = 1 + ceil(Lmax / hop)) is the result, 0 for the frames an item does not have;
 * frames_on [B][n] int32 (device) its sum per row; energy and level [B][n][Fmax] fp64 (device) are E and lev, 0 for the
 * frames an item does not have.  Frame t owns the samples [t hop - hop / 2, (t + 1) hop - hop / 2) of [0, L): a run
 * [s, e) is the sample segment [max(0, s hop - hop / 2), min(L, e hop - hop / 2)).  The device writes no segment table.
 * Two launches: the band energies (workgroup per group of frames and item), then everything else with one workgroup
 * per item: hysteresis and the run rules are chunked scans over the workgroup, so no thread walks more than
 * ceil(F / 256) frames.  No floating-point atomics: an item has the same bits alone, at any batch position, under any
 * padding (nothing at or past lens[b] is read; it may hold NaN), from a base pointer of any 4-byte alignment and in a
 * second call.  Uploads lens and synchronises the stream when lens is given: not for capture.
 * DSN_EINVAL by name, before anything is allocated or launched: a null pointer; B outside [1, 65535]; n outside [1, 4];
 * what dsn_mask_refine refuses of n_fft, hop, Lmax and lens; a band that is empty or outside [0, n_fft / 2]; half_width
 * outside [0, 1024]; a factor outside [0, 1] or a stay factor above its on factor; min_on or min_off < 1; pad < 0; more
 * than 2^22 frames per item.
 *
 * dsn_activity_gate: x [B][n][Lmax] -> out [B][n][Lmax] with act [B][n][Fa] bytes.  Sample m < L of a row lies in a
 * segment iff act[(m + hop / 2) / hop] is set; there out = x bit for bit (NaN and -0 included).  Elsewhere d >= 1 is the
 * distance in samples to the nearest sample inside a segment of the same row: out = +0 for d > fade whatever x holds,
 * else ramp[d - 1] x, one fp32 multiply.  ramp [fade] (HOST) is float(0.5 + 0.5 cos(pi d / (fade + 1))), d = 1 .. fade,
 * formed by the caller in fp64 and rounded once: the device evaluates no cosine.  Where two ramps overlap the nearer
 * segment rules; fade = 0 is a hard gate.  Samples at or past lens[b] are written +0 and nothing there is read.  out may
 * be x itself.  Uploads its tables and synchronises the stream: not for capture.
 * DSN_EINVAL by name: a null pointer; B, n as above; Lmax outside [1, 2^30]; hop outside [8, 65536]; fade outside
 * [0, 4096]; a ramp value outside [0, 1]; lens[b] outside [1, Lmax]; Fa smaller than the frames Lmax needs; out
 * overlapping x without being x. */
int dsn_activity(dsn_ctx* ctx, const float* est, int B, int n, int Lmax, const int32_t* lens, int n_fft, int hop, int j_lo,
                 int j_hi, int half_width, double c_r, double c_d, double c_r_stay, double c_d_stay, int min_on,
                 int min_off, int pad, uint8_t* act, int32_t* frames_on, double* energy, double* level, void* stream);
int dsn_activity_gate(dsn_ctx* ctx, const float* x, const uint8_t* act, int B, int n, int Lmax, int Fa,
                      const int32_t* lens, int hop, int fade, const float* ramp, float* out, void* stream);

/* The pair tables behind the generator objective of the reference's src/ldm.py (LDM.losses_gen, forward value only):
 * the multi-resolution STFT loss of stable_audio_tools/training/losses/auraloss.py (MultiResolutionSTFTLoss, optionally
 * A-weighted) and the L1 / MSE waveform losses of training/losses/losses.py, each wrapped in PITLoss there (restated in
 * tests/mrstft_restatement.py and pinned to the reference's own modules by tests/golden/mrstft.npz).  The reference
 * evaluates a loss once per source permutation; every term of every permutation is a mean of the values below, so this
 * call forms each spectrum once.  reals, decoded [B,n,L] fp32 (device), n <= 4.  For item b, reference source i and
 * estimate source j, with mag = sqrt(max(re^2 + im^2, 1e-8)) of torch.stft(x, fft, hop, win, hann_window(win)) (its
 * defaults: center, reflect padding, 1 + L / hop frames, no normalisation) of the signals, which are first filtered
 * with `taps` (conv1d with padding n_taps / 2, i.e. cross-correlation) when taps is non-null:
 *   sc      [R,B,n,n] = |mag_d_j - mag_r_i|_F / |mag_d_j|_F    (the reference hands (reals, decoded) to auraloss as
 *                                                               (input, target): the norm below is the estimate's)
 *   log_mag [R,B,n,n] = mean |log mag_r_i - log mag_d_j|
 *   lin_mag [R,B,n,n] = mean |mag_r_i - mag_d_j|
 *   l1, l2  [B,n,n]   = mean |r_i - d_j|, mean (r_i - d_j)^2 of the unfiltered signals
 * all fp64 host arrays; each may be NULL.  A table whose weight (w_sc, w_log_mag, w_lin_mag) is zero is filled with
 * zeros: the reference does not evaluate that term.  Every sum has a fixed order: two calls give identical bits.
 * DSN_EINVAL, before any launch: n > 4; more than 16 resolutions; an FFT size that is not a power of two from 32 to
 * 2048; win outside [1, fft]; hop < 1; L <= max(fft) / 2 (reflect padding undefined); an even tap count or more
 * than 127 taps. */
typedef struct DsnMrstftConfig {
  int n_res;
  const int *fft, *hop, *win;      /* host arrays [n_res] */
  float w_sc, w_log_mag, w_lin_mag;
  const float* taps;               /* host [n_taps]; NULL: no prefilter */
  int n_taps;
} DsnMrstftConfig;
typedef struct DsnMrstftOut {
  double *sc, *log_mag, *lin_mag, *l1, *l2;
} DsnMrstftOut;
int dsn_mrstft_loss(dsn_ctx* ctx, const float* reals, const float* decoded, int B, int n, int L,
                    const DsnMrstftConfig* cfg, const DsnMrstftOut* out, void* stream);
/* The same tables for a ragged batch: reals, decoded [B,n,L] padded to the longest item, lens [B] (HOST int32): item b
 * holds lens[b] samples.  Item b's rows of every table are those of dsn_mrstft_loss on the item alone with L = lens[b]:
 * 1 + lens[b] / hop frames per resolution, centred and reflected at the item's own end; the prefilter reads zero past
 * that end; l1 / l2 divide by lens[b], log_mag / lin_mag by bins * frames_b.  Nothing at or past lens[b] is read (the
 * padding may hold NaN).  An item's sums are cut into workgroup partials by its own length and the resolution alone
 * (the dense call's partition at B = 1), so its tables have the same bits alone, at any batch position, under any
 * amount of padding and in a second call.  DSN_EINVAL, before any launch, beside the dense call's refusals: lens[b]
 * outside [1, L]; lens[b] <= max(fft) / 2. */
int dsn_mrstft_loss_ragged(dsn_ctx* ctx, const float* reals, const float* decoded, const int32_t* lens, int B, int n,
                           int L, const DsnMrstftConfig* cfg, const DsnMrstftOut* out, void* stream);

/* introspection for benchmarks / tests */
int dsn_enable_graphs(dsn_ctx* ctx, int enable);          /* hipGraph replay of sample/decode */
int64_t dsn_workspace_bytes(const dsn_ctx* ctx);
/* Per-launch HIP-event timing of the dominant (implicit-GEMM MFMA) kernel: between begin and
 * end every launch is bracketed by events on the launch stream (graphs are bypassed).
 * Returns summed kernel time, summed ALGORITHMIC flops (2*M*N*K of each contraction, the
 * 3x split-bf16 passes not counted) and the launch count. */
int dsn_profile_begin(dsn_ctx* ctx);
int dsn_profile_end(dsn_ctx* ctx, double* gemm_ms, double* gemm_flops, int64_t* gemm_launches);
/* of the region closed by the last dsn_profile_end: the HBM-bound fused ResidualUnit launches alone (they are
 * also part of the totals above) -- summed kernel time, ALGORITHMIC bytes (operand planes in, fp32 residual in,
 * fp32 and planes out), launch count */
int dsn_profile_hbm(dsn_ctx* ctx, double* ms, double* bytes, int64_t* launches);
/* of the same region, per call site ("dit.qkv", "dit.ff_in", "dit.residual_norm", "vae.residual_unit_fused", ...):
 * summed event time, algorithmic flops and algorithmic HBM bytes (0 where not stated), launch count.  `names` is
 * max_rows x DSN_PROFILE_NAME_LEN chars.  Returns the number of rows available (may exceed max_rows). */
#define DSN_PROFILE_NAME_LEN 48
int dsn_profile_rows(dsn_ctx* ctx, int max_rows, char* names, double* ms, double* flops, double* bytes,
                     int64_t* launches);

/* ---- NOT PART OF THE ABI ------------------------------------------------------------------------------------
 * dsn_test_gemm, dsn_test_kernel, dsn_dit_plan, dsn_debug_read and dsn_bench_igemm below are hooks for this repository's own tests,
 * repro scripts and kernel sweeps.  They name internal workspace buffers and kernel variants, change without notice, and a binding of
 * the reference-facing interface must not use them. */
/* Test hook: run ONE chosen kernel of the implicit-GEMM family (ditsep_amd/csrc/igemm.h) on a descriptor built from
 * caller-owned fp32 device tensors, with any subset of the epilogue features.  Operands are rounded to the engine's
 * operand planes first.  A launcher that refuses the descriptor fails the call by name: there is no fall-back to another
 * kernel.  Every descriptor built here is bounds-audited when DSN_AUDIT is set (the test suite sets it). */
enum { DSN_TG_AUTO = 0, DSN_TG_TILE = 1, DSN_TG_V1 = 2, DSN_TG_PANEL = 3, DSN_TG_SKINNY = 4, DSN_TG_HALO = 5,
       DSN_TG_SPLITK = 6 };
typedef struct DsnTestGemm {
  int kernel;                 /* DSN_TG_* */
  int bm, bn, nst, bk;        /* TILE: igemm2 instantiation; PANEL: nst / bk pick the 8-wave ring (0 = any) */
  int panel_rows, panel_bn, panel_wm;  /* PANEL */
  int ksplit;                 /* SKINNY (slabs in out_f32, slab_stride apart) and SPLITK (slabs in `slabs`) */
  /* geometry: out[b][j][n] = sum_{tap,ci} w[n][tap*Cin+ci] a[b*in_bstride + (j*in_stride + tap*tap_dil - in_pad) *
   * in_row_elems + a_off + ci]; 2-D 3x3 mode when img_w > 0.  Zero in_row_elems / in_bstride / out_* = dense. */
  int B, Lin, Cin, N, taps, in_stride, tap_dil, in_pad, rows_per_b;
  int M;                      /* GEMM rows; 0 = B * rows_per_b (fewer: the last item is short) */
  int in_row_elems, a_off;
  int64_t in_bstride;
  int img_h, img_w;
  int64_t out_bstride;
  int out_row_elems, out_off;
  int64_t out_limit;
  const float* a;             /* input, a_numel floats (a multiple of 4) */
  int64_t a_numel;
  const float* w;             /* [N][taps*Cin] */
  /* epilogue operands (null = off) */
  const float* bias;
  int bias_mod;
  const float* bbias;
  int bbias_stride;
  const float* resid;
  int64_t resid_bstride;
  int resid_row_elems, resid_off;
  float out_scale;
  int f32_op;                 /* DSN_F32_* of the kernels: 1 = tanh */
  int act;                    /* 1 = ELU, 2 = Snake, 3 = SiLU (operand-plane output only) */
  const float* act_a;
  const float* act_b;
  int act_mod;
  int swiglu;
  float* gn_stats;
  float* gn_stats2;
  int gn_nq2, gn_qoff2;
  const float* sc_a;          /* halo 1x1 shortcut input [B][rows_per_b][sc_row_elems], sc_a_numel floats */
  int64_t sc_a_numel;
  const float* sc_w;          /* [N][sc_Cin] */
  const float* sc_bias;
  int sc_Cin, sc_row_elems;
  /* outputs */
  float* out_f32;
  int16_t* out_planes;        /* P planes of out_ps elements each, raw 16-bit operand bits */
  int64_t out_ps;
  float* slabs;               /* SPLITK: ksplit slabs, slab_stride floats apart */
  int64_t slab_stride;
} DsnTestGemm;
int dsn_test_gemm(dsn_ctx* ctx, const DsnTestGemm* t, void* stream);

/* Test hook: run ONE launch wrapper of the non-GEMM kernels (ditsep_amd/csrc/kernels.h, qkv_attention_launch,
 * ru_fused_launch) with the caller's arguments on caller-owned device tensors -- the sampler update, prior, noise and
 * VAE-sample kernels included, see the end of the struct.  Which kernel runs is the wrapper's own
 * dispatch.  `a` (and `w` of QKV_ATTENTION, `w` / `w2` of RU_FUSED) are fp32 tensors rounded to the engine's operand planes
 * first; every other tensor is passed through.
 * Outputs land in caller-owned buffers.  An argument the wrapper does not support fails the call by name. */
enum { DSN_TK_ATTENTION = 1, DSN_TK_QKV_ATTENTION = 2, DSN_TK_RESIDUAL_NORM = 3, DSN_TK_GN_STATS = 4,
       DSN_TK_GN_APPLY = 5, DSN_TK_FIR2D = 6, DSN_TK_CONV_OUT1 = 7, DSN_TK_CONV_IN1 = 8, DSN_TK_RU_FUSED = 9,
       DSN_TK_PC_PRIOR = 10, DSN_TK_PC_CORRECTOR = 11, DSN_TK_PC_ITEM_NORMS = 12, DSN_TK_PC_PREDICTOR = 13,
       DSN_TK_SIGMA_MIX = 14, DSN_TK_MIX_PRIOR = 15, DSN_TK_MIX_CORRECTOR = 16, DSN_TK_MIX_PREDICTOR = 17,
       DSN_TK_SB_UPDATE = 18, DSN_TK_REPEAT_SOURCES = 19, DSN_TK_VAE_SAMPLE = 20, DSN_TK_RANDN = 21,
       DSN_TK_RAND_UNIFORM = 22, DSN_TK_CODEC_TAIL_ZERO = 23,
       DSN_TK_WN_SCALE = 24, DSN_TK_PACK_WEIGHT = 25, DSN_TK_PACK_BIAS_SWIGLU = 26, DSN_TK_PACK_WEIGHT_FP8 = 27,
       DSN_TK_PACKED_ROW_SUM = 28, DSN_TK_FP8_ROW_SUM = 29, DSN_TK_BIAS_PLUS_WBETA = 30, DSN_TK_SNAKE_PARAMS = 31,
       DSN_TK_PACK_TOKENS = 32, DSN_TK_UNPACK_TOKENS = 33, DSN_TK_COPY_ROWS = 34, DSN_TK_TO_PLANES = 35,
       DSN_TK_ZERO_TAIL = 36, DSN_TK_VAE_SAMPLE_RAGGED = 37, DSN_TK_TIMESTEP_FEATURES = 38, DSN_TK_ROPE_TABLES = 39,
       DSN_TK_NCSN_PACK = 40, DSN_TK_NCSN_FOURIER = 41, DSN_TK_NCSN_OUTPUT = 42, DSN_TK_WIN_PACK_TOKENS = 43,
       DSN_TK_WIN_BLEND_TOKENS = 44 };
/* `mode` of DSN_TK_PACK_WEIGHT (the PACK_* index maps of ditsep_amd/csrc/kernels.h); DSN_TK_PACK_WEIGHT_FP8 takes the
 * first two */
enum { DSN_PACK_LINEAR = 0, DSN_PACK_LINEAR_SWIGLU = 1, DSN_PACK_CONV = 2, DSN_PACK_CONVT = 3, DSN_PACK_CONV2D = 4,
       DSN_PACK_NIN = 5 };
typedef struct DsnTestKernel {
  int kind;                   /* DSN_TK_* */
  /* ATTENTION: a = q | k | v [B*S][3*H*dh] -> out_planes [B*S][H*dh] (or out_fp8 + out_fp8_scale)
   * QKV_ATTENTION: a = LayerNorm output [B*S][D], w = to_qkv [3*D][D], bias [3*D] (optional), rope_cos / rope_sin
   *   [S][32] caller-owned buffers that launch_rope_tables fills here, ipp items per panel; q scale 1/8
   * both: `lens` (device int32 [B], 1 <= lens[b] <= S, checked here) runs the length-aware variant */
  int B, S, H, dh, D, ipp;
  /* RESIDUAL_NORM: x [rows][D] (updated in place), slabs nslab x slab_stride, bias / gamma / beta [D] */
  int rows, nslab, do_norm;
  float eps;
  int64_t slab_stride;
  /* GN_STATS / GN_APPLY / FIR2D: view x + b*bstride + row*rstride + channel of B items, HW rows (FIR2D: img_h x img_w),
   * C channels.  GN_STATS -> out_f32 = stats; GN_APPLY reads `stats`; FIR2D: `up`, `add` (optional, output shape) */
  int C, HW, rstride, img_h, img_w, up, silu;
  int64_t bstride;
  /* CONV_OUT1: a = input [B*L][C] (planes), w [ktaps][C] fp32 -> out_f32 [B*L].  CONV_IN1: x = wav [B][L], w [C][ktaps],
   * bias [C] -> out_f32 / out_planes [B*L][C], act (0 none, 1 ELU, 2 Snake with act_a / act_b [C]) */
  int L, ktaps, apply_tanh, act;
  /* RU_FUSED: a = activated input [B][L][128] (planes), w = k7 weight [128][7*128] (k = tap*128 + cin) and w2 = 1x1
   * weight [128][128] (planes), bias / bias2 [128], x = fp32 residual stream [B][L][128], dilation dil, act / act_a /
   * act_b after the k7 conv, act_out / out_act_a / out_act_b on the output planes -> out_f32 (may be null, may be x)
   * and / or out_planes, both [B][L][128] */
  int dil, act_out;
  const float* a;
  int64_t a_numel;            /* a multiple of 4 */
  const float* w;
  int64_t w_numel;
  const float* w2;
  int64_t w2_numel;
  float* x;
  const float* slabs;
  const float* bias;
  const float* bias2;
  const float* gamma;
  const float* beta;
  const float* stats;
  const float* add;
  const float* act_a;
  const float* act_b;
  const float* out_act_a;
  const float* out_act_b;
  float* rope_cos;
  float* rope_sin;
  /* outputs */
  float* out_f32;
  int16_t* out_planes;        /* P planes of out_ps elements each, raw 16-bit operand bits */
  int64_t out_ps;
  uint8_t* out_fp8;           /* e4m3 bytes instead of planes, with out_fp8_scale (E8M0, one per 32 columns) */
  uint8_t* out_fp8_scale;
  /* The sampler's kernels between two score calls (fp32 only, nothing is rounded to planes).  State x [B,n,D,T]
   * (updated in place, or the output of the priors and REPEAT_SOURCES), y [B,1,D,T], score [B*T][n*D] token-major,
   * z [B,n,D,T], smix [B][D*T] (null = 1), xmean [B,n,D,T]:
   *   PC_PRIOR       x = mean + stdT z; mean = y broadcast over the sources, or y itself [B,n,D,T] with mean_full
   *   PC_CORRECTOR   x, xmean (may be null), score, z; step and gain, or norms [2 B] (|score| then |z| per item) and snr
   *   PC_ITEM_NORMS  x = a [B][count] -> out_f32 [B]
   *   PC_PREDICTOR   x, xmean, y, score, z; theta, dt, G, g, em
   *   SIGMA_MIX      y [B][L], avg_len -> out_f32 [B][L]
   *   MIX_PRIOR      y, z, smix -> x; s1, s2
   *   MIX_CORRECTOR  x, xmean (may be null), score, z, smix; s1, s2 (square roots of the two eigenvalues), snr
   *   MIX_PREDICTOR  x, xmean, score, z, smix; lam, dt, g, sqdt, em
   *   SB_UPDATE      x = w_prev x + w_est score + w3 (third_is_y ? y : z); that tensor null: no third term
   *   REPEAT_SOURCES y -> x
   *   VAE_SAMPLE     x = encoder output [B][T][2 D] (mean ++ scale), z = noise [B,D,T] -> out_f32 [B,D,T]
   *   RANDN, RAND_UNIFORM  count values of the stream (seed, offset) -> out_f32; RAND_UNIFORM: lo, hi
   *   CODEC_TAIL_ZERO  launch_codec_tail_zero on B items of L rows of C channels: lens = frames (device int32
   *                  [ceil(B / rep)], 0 <= frames * mul <= L checked here), rep, mul; destinations out_planes (the engine's
   *                  plane count, out_ps apart), x (the fp32 stream) and out_f32, each [B][L][C], any of them null
   * Refused by name before any launch: a missing tensor, a non-positive B, n, D, T, L or count, avg_len < 1, and
   * n > 4 for the three MIX_* kernels (they hold the sources of a position in four-element arrays). */
  int n, T, avg_len, em, mean_full, third_is_y;
  float stdT, step, gain, snr, theta, dt, G, g, s1, s2, lam, sqdt, w_prev, w_est, w3, lo, hi;
  uint64_t seed, offset;
  int64_t count;
  const float* y;
  const float* score;
  const float* z;
  const float* smix;
  const float* norms;
  float* xmean;
  const int32_t* lens;        /* ATTENTION / QKV_ATTENTION: valid tokens per item (null: dense); CODEC_TAIL_ZERO: frames */
  int rep, mul;               /* CODEC_TAIL_ZERO */
  /* Load-time weight preparation and the per-call movers and feature kernels: every tensor is passed through to the
   * wrapper (nothing is rounded to planes first), fp32 unless said otherwise.
   *   WN_SCALE         x = v [rows][count], gamma = g [rows] -> out_f32 [rows] = g / |v row|
   *   PACK_WEIGHT      x = the source weight of `count` floats, which must be what `mode` addresses:
   *                      LINEAR, LINEAR_SWIGLU  [N][K], colscale [K] optional          (SWIGLU: N % 32 == 0)
   *                      CONV    [Cout][Cin][kw], scale [Cout] optional; N = Cout, K = kw Cin
   *                      CONVT   [Cin][Cout][kw], scale [Cin] optional;  kw = 2 stride, N = stride Cout, K = 2 Cin
   *                      CONV2D  [Cout][Cin][kw];  stride = the padded Cin >= Cin, N >= Cout, K = kw stride
   *                      NIN     [K][N]
   *                    -> out_planes [N][K] (out_ps >= N K); a scale / colscale the mode does not read is refused
   *   PACK_BIAS_SWIGLU x = bias [N] -> out_f32 [N] in PACK_LINEAR_SWIGLU row order (N % 32 == 0)
   *   PACK_WEIGHT_FP8  x = [N][K], K % 32 == 0, mode LINEAR or LINEAR_SWIGLU (N % 32 == 0), colscale [K] optional
   *                    -> out_fp8 [N][K] e4m3 bytes, out_fp8_scale [N][K / 32] E8M0 bytes
   *   PACKED_ROW_SUM   in_planes (the engine's plane count, in_ps >= N K apart) [N][K] -> out_f32 [N]
   *   FP8_ROW_SUM      in_fp8 [N][K], in_fp8_scale [N][K / 32], K % 32 == 0 -> out_f32 [N]
   *   BIAS_PLUS_WBETA  x = W [N][K], beta [K], bias [N] optional -> out_f32 [N]
   *   SNAKE_PARAMS     act_a = alpha, act_b = beta [C] -> out_f32 = exp(alpha), out2_f32 = 1 / (exp(beta) + 1e-9)
   *   PACK_TOKENS      x = src0 [B][C0][T], y = src1 [B][C1][T] (null exactly when C1 == 0) -> out_f32 and / or
   *                    out_planes [B T][C0 + C1]
   *   UNPACK_TOKENS    x = [B T][C] -> out_f32 [B][C][T]
   *   COPY_ROWS        x = [rows][C] -> out_f32, rows dst_stride floats apart; C, dst_stride multiples of 4, dst_stride >= C
   *   TO_PLANES        x = [count] -> out_planes; count a multiple of 4, out_ps >= count and a multiple of 4
   *   ZERO_TAIL        x [B,n,D,T] in place, lens (device int32 [B], counts the timestep token): t >= lens[b] - 1 zeroed
   *   VAE_SAMPLE_RAGGED  VAE_SAMPLE with lens = frames (device int32 [B]): out_f32[b, :, t] = 0 for t >= frames[b]
   *   TIMESTEP_FEATURES  x = t [B], w [half] -> out_planes [B][2 half] = cos | sin
   *   ROPE_TABLES      S positions, dh = the rotary width (even) -> rope_cos, rope_sin [S][dh]
   *   NCSN_PACK        x = xt [B,n,H,T], y = mix [B,1,H,T] -> out_f32 and / or out_planes [B][H][Wp][Cp];
   *                    Wp >= T, Cp >= n + 1
   *   NCSN_FOURIER     x = t [B], w [half] -> out_planes [B][2 half] = sin | cos of 2 pi log(t) w
   *   NCSN_OUTPUT      x = pyr [B][H][Wp][Cp], y = t [B], w [n][cin], bias [n] -> out_f32 [B T][n H]; Wp >= T, Cp >= cin
   *   WIN_PACK_TOKENS  PACK_TOKENS with the window gather: x = src0 [R][C0][Tsrc], y = src1 [R][C1][Tsrc], wtab (device
   *                    int32 [B][3] = recording, start, length; checked here against R, Tsrc and T) -> out_f32
   *                    and / or out_planes [B T][C0 + C1]; rows t >= length of a window are written as zero
   *   WIN_BLEND_TOKENS x = window tokens [B][T][C], ftab (device int32 [rows][4] = window0, offset0, window1, offset1;
   *                    checked here against B and T), fw (device fp32 [rows][2] = fall, rise) -> out_f32 [rows][C];
   *                    C a multiple of 4
   * Refused by name before any launch: a missing tensor, a non-positive size, and each condition listed above. */
  int mode, N, K, Cin, Cout, kw, stride;
  const float* scale;
  const float* colscale;
  const int16_t* in_planes;
  int64_t in_ps;
  const uint8_t* in_fp8;
  const uint8_t* in_fp8_scale;
  int C0, C1;
  int64_t dst_stride;
  int Wp, Cp, cin, half;
  float* out2_f32;
  const int32_t* wtab;        /* WIN_PACK_TOKENS */
  const int32_t* ftab;        /* WIN_BLEND_TOKENS */
  const float* fw;
  int Tsrc, R;                /* WIN_PACK_TOKENS: the sources' frames per recording, and the recordings */
} DsnTestKernel;
int dsn_test_kernel(dsn_ctx* ctx, const DsnTestKernel* t, void* stream);

/* Test hook: what one DiT score call of B mixtures x T frames would run under `cfg` (its precision included) and the
 * DSN_* switches of the environment -- the plan dit_forward launches from (ditsep_amd/csrc/dit_plan.h).  Needs no
 * context and no GPU.  A `*_rows` of 0 means that GEMM runs no row-panel kernel. */
typedef struct DsnDitPlan {
  int M, S;                   /* token rows B * S, tokens per item S = T + 1 */
  int skinny;                 /* the layer GEMMs run the weight-streaming skinny kernel */
  int fold_rows;              /* > 0: ff_norm folded into FF-in; to_out in panels of this many rows, no split-K */
  int qa_ipp;                 /* > 0: fused to_qkv + attention with this many items per panel */
  int qkv_rows;
  int attn_out_ksplit, attn_out_rows;
  int ff_in_rows;
  int ff_out_ksplit, ff_out_rows;
  int project_out_rows;
} DsnDitPlan;
int dsn_dit_plan(const dsn_config* cfg, int B, int T, DsnDitPlan* out);

/* Development hook: copy `count` floats of a named workspace buffer to host memory. */
int dsn_debug_read(dsn_ctx* ctx, const char* name, float* host, int64_t count);
/* Development hook: average milliseconds of `iters` launches of the implicit-GEMM kernel on random
 * operands of the given contraction (variant 1 = register-staged core, 2 = glds-ring core). */
int dsn_bench_igemm(dsn_ctx* ctx, int B, int Lin, int Cin, int N, int taps, int tap_dil, int in_pad, int ksplit,
                    int variant, int iters, double* ms_out);

#ifdef __cplusplus
}
#endif
#endif /* DITSEP_HIP_H */
