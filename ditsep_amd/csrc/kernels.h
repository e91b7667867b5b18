// Launch wrappers for the non-GEMM kernels of the separation path (kernels.hip).
#pragma once
#include "common.h"

// ---- layout transforms -----------------------------------------------------
// src0 [B][C0][T] (+ src1 [B][C1][T]) channel-major fp32 -> token-major
// dst[(b*T + t)*(C0+C1) + c] as fp32 (optional) and as operand planes (optional).
void launch_pack_tokens(const float* src0, int C0, const float* src1, int C1, int B, int T,
                        float* dst_f32, op16_t* dst_planes, long ps, int planes, hipStream_t s);
// the same with a window gather (the window-blended score call): item w of dst is window w of wtab [W][3] = (recording,
// start, length; device) of sources [R][C][Tsrc], Tw rows per window, rows past a window's length written as zero
void launch_win_pack_tokens(const float* src0, int C0, const float* src1, int C1, const int* wtab, int W, int Tw,
                            int Tsrc, float* dst_f32, op16_t* dst_planes, long ps, int planes, hipStream_t s);
// tw[w] = t[wtab[3 w]]: the recordings' times replicated to their windows
void launch_win_times(const float* t, const int* wtab, int W, float* tw, hipStream_t s);
// window tokens [W][Tw][C] -> out [rows][C] by the frame table ftab [rows][4] = (window0, offset0, window1, offset1),
// fw [rows][2] = (fall, rise): zero (window0 < 0), a copy (window1 < 0) or fmaf(rise, s1, fall s0).  C % 4 == 0.
void launch_win_blend_tokens(const float* src, const int* ftab, const float* fw, float* out, long rows, int C, int Tw,
                             hipStream_t s);
// rows of `width` floats (multiple of 4) into rows `dst_stride` floats apart
void launch_copy_rows(const float* src, float* dst, int rows, int width, long dst_stride, hipStream_t s);
// token-major fp32 [B*T][C] -> channel-major [B][C][T]
void launch_unpack_tokens(const float* src, float* dst, int B, int C, int T, hipStream_t s);
// fp32 [n] -> operand planes, optional activation
void launch_to_planes(const float* src, op16_t* dst, long ps, int planes, long n, hipStream_t s);

// ---- predictor-corrector sampler (OUVE; reference layout x[B,n,D,T], y[B,1,D,T]) ----
// score is token-major [B*T][n*D].
// mean: y [B,1,D,T] (mean_full = 0) or a full prior mean [B,n,D,T] (mean_full = 1)
void launch_pc_prior(const float* mean, int mean_full, const float* z, float* x, float stdT, int B, int n, int D,
                     int T, hipStream_t s);
// norms == null: host scalars (ALD); else [2][B] per-item norms of score and noise (Langevin corrector)
void launch_pc_corrector(float* x, float* x_mean /*nullable*/, const float* score_tok, const float* z, float step,
                         float noise_gain, const float* norms, float snr, int B, int n, int D, int T, hipStream_t s);
void launch_pc_item_norms(const float* a, long per_item, int B, float* out, hipStream_t s);
// em = 0 reverse diffusion, 1 Euler-Maruyama; G = g sqrt(dt)
void launch_pc_predictor(float* x, float* x_mean, const float* y, const float* score_tok, const float* z,
                         float theta, float dt, float G, float g, int em, int B, int n, int D, int T, hipStream_t s);

// ---- secondary sampler family (MixSDE / PriorMixSDE + ald2, Schroedinger bridge) on x [B,n,D,T] ----
// smix [B][D*T] = PriorMixSDE._std_sigma_mix of the flattened mixture latent (null: MixSDE, factor 1)
void launch_sigma_mix(const float* y, float* smix, int B, int L, int avg_len, hipStream_t s);
// x = 0.5 y + (s1 A + s2 Pn) z * smix
void launch_mix_prior(const float* y, const float* z, float* x, const float* smix, float s1, float s2, int B, int n, int D,
                      int T, hipStream_t s);
// ald2 step with L = (sq1 A + sq2 Pn) smix (x_mean may be null)
void launch_mix_corrector(float* x, float* x_mean, const float* score_tok, const float* z, const float* smix, float sq1,
                          float sq2, float snr, int B, int n, int D, int T, hipStream_t s);
// em = 0 reverse diffusion, 1 Euler-Maruyama; g = diffusion scalar, sqdt = sqrt(dt)
void launch_mix_predictor(float* x, float* x_mean, const float* score_tok, const float* z, const float* smix,
                          float lambda, float dt, float g, float sqdt, int em, int B, int n, int D, int T, hipStream_t s);
// x = w_prev x + w_est est + w3 (third_is_y ? y[B,1,D,T] : z[B,n,D,T]); third may be null
void launch_sb_update(float* x, const float* est_tok, const float* third, float w_prev, float w_est, float w3,
                      int third_is_y, int B, int n, int D, int T, hipStream_t s);
void launch_repeat_sources(const float* y, float* x, int B, int n, int D, int T, hipStream_t s);
// ragged batches: x [B,n,D,T], x[b, :, :, t] = 0 for t >= lens[b] - 1; lens (device, [B]) counts an item's tokens
// including the DiT's timestep token, as the attention kernels take it
void launch_zero_tail(float* x, const int* lens, int B, int n, int D, int T, hipStream_t s);

// ---- DiT pieces ---------------------------------------------------------------
// x += bias + sum(split-K slabs) (written back when nslab > 0), then LayerNorm (do_norm) or a
// plain copy to operand planes.  D <= 4096, D % 4 == 0, nslab <= RESIDUAL_NORM_MAX_SLABS.
// out_fp8_scale != null: `out` receives fp8 (e4m3) bytes [rows][D] and out_fp8_scale E8M0 scales [rows][D/32].
constexpr int RESIDUAL_NORM_MAX_SLABS = 8;
void launch_residual_norm(float* x, const float* slabs, int nslab, long slab_stride, const float* bias,
                          const float* gamma, const float* beta, op16_t* out, long ps, int planes, int rows, int D,
                          float eps, int do_norm, hipStream_t s, unsigned char* out_fp8_scale = nullptr);
// FourierFeatures: t[B], w[half] -> planes [B][2*half] = [cos(2 pi t w), sin(2 pi t w)]
void launch_timestep_features(const float* t, const float* w, int B, int half, op16_t* out, long ps,
                              int planes, hipStream_t s);
// MFMA attention over operand planes q|k|v [B*S][3*H*dh] written by the fused QKV epilogue (attention.hip): whole
// sequences of up to 256 keys in registers where their V fits in LDS, blocked keys with an online softmax otherwise.
// out_fp8_scale != null: `out` receives fp8 (e4m3) bytes [B*S][H*dh] and out_fp8_scale the E8M0 block scales
// [B*S][H*dh/32] (MX operand of the fp8 out-projection) instead of 16-bit planes.
// dh in {64,128,256} (hipErrorNotSupported otherwise); returns the launch status
// lens != null (device, int [B], 1 <= lens[b] <= S; the caller validates): ragged batch of items padded to S tokens --
// the length-aware instantiations mask keys >= lens[b] and skip key tiles wholly past it; same kernel choice and grid
// as the dense launch for (B, S, H).  Query rows >= lens[b] are still computed over the item's valid keys.
hipError_t launch_attention_mfma(const op16_t* qkv, long ps, op16_t* out, long out_ps, int pl, int B, int S, int H,
                                 int dh, hipStream_t s, unsigned char* out_fp8_scale = nullptr,
                                 const int* lens = nullptr);
void launch_rope_tables(float* cos_t, float* sin_t, int S, int rot, hipStream_t s);

// ---- Oobleck edges -------------------------------------------------------------
// final decoder conv: planes [S*L][C] (already activated), w fp32 [7][C] -> tanh(sum) fp32 [S*L]
void launch_conv_out1(const op16_t* a, long ps, int planes, const float* w, float* out, int S, int L, int C,
                      int ktaps, int apply_tanh, hipStream_t s);
// first encoder conv: wav fp32 [S][L] (Cin = 1), w [Cout][K], bias -> fp32 x [S*L][Cout] + act planes
void launch_conv_in1(const float* wav, const float* w, const float* bias, int S, int L, int Cout, int ktaps,
                     float* out_f32, op16_t* out_planes, long ps, int planes, int act, const float* act_a,
                     const float* act_b, hipStream_t s);
// VAE bottleneck sample: enc fp32 token-major [S*T][2*D] (mean | scale) + noise [S][D][T] -> y [S][D][T]
void launch_vae_sample(const float* enc_tok, const float* noise, float* y, int S, int D, int T, hipStream_t s);

// ---- ragged batches through the codec (codec_ragged.hip) -------------------------------------------
// Item s of S items padded to L rows of C channels ([S][L][C] row-major) has frames[s / rep] * mul valid rows: frames
// (device, int [ceil(S / rep)]) counts latent frames, rep items share an entry (the n_src sources of a mixture on the
// decoder side, 1 on the encoder side), mul is the level's rows per latent frame.  Rows [valid, L) of the item are
// written as zero in each of the n_planes operand planes (plane stride ps), in the fp32 stream xf and in the plain fp32
// output `out`; any of the three may be null.  Only tail rows are touched: an item with valid == L is left alone.  The
// grid depends on (S, L, C) alone, so a captured launch serves every set of lengths.  16-byte stores: C % 8 == 0 and
// 16-byte aligned destinations.  Returns null, or the reason the arguments were refused (nothing was launched).
const char* launch_codec_tail_zero(op16_t* planes, long ps, int n_planes, float* xf, float* out, int S, int L, int C,
                                   const int* frames, int rep, int mul, hipStream_t s);
// launch_vae_sample with y[s, :, t] = 0 for t >= frames[s] (device, int [S])
void launch_vae_sample_ragged(const float* enc_tok, const float* noise, const int* frames, float* y, int S, int D, int T,
                              hipStream_t s);

// ---- RNG ------------------------------------------------------------------------
// Philox4x32-10 + Box-Muller standard normals
void launch_randn(float* out, long n, unsigned long long seed, unsigned long long offset, hipStream_t s);

// ---- weight packing ---------------------------------------------------------------
enum { PACK_LINEAR = 0, PACK_LINEAR_SWIGLU = 1, PACK_CONV = 2, PACK_CONVT = 3, PACK_CONV2D = 4, PACK_NIN = 5 };
// PACK_CONV2D: src [Cout][Cin][taps] (taps = kw: 9 for 3x3 row-major (ky,kx), 1 for 1x1) -> dst [N][taps*Cin_pad],
//   Cin_pad = `stride`, zero where ci >= Cin or n >= Cout.   PACK_NIN: src [Cin][Cout] -> dst [Cout][Cin].
// per-row scale g / ||v|| for old-style weight norm (norm over all dims but 0); v [R][inner]
void launch_wn_scale(const float* v, const float* g, float* scale, int R, long inner, hipStream_t s);
// generic gather into packed [N][K] planes; see kernels.hip for the index maps
// colscale (PACK_LINEAR / PACK_LINEAR_SWIGLU only): per input column factor, W[n][k] * colscale[k] (LayerNorm gamma
// folded into the consuming Linear)
void launch_pack_weight(const float* src, const float* scale, op16_t* dst, long ps, int planes, int mode,
                        int N, int K, int Cin, int Cout, int kw, int stride, hipStream_t s,
                        const float* colscale = nullptr);
// out[n] = sum_k packed[n][k] (the rounded operand values; both planes in the split modes)
void launch_packed_row_sum(const op16_t* w, long ps, int planes, int N, int K, float* out, hipStream_t s);
// out[n] = (bias ? bias[n] : 0) + sum_k W[n][k] beta[k]
void launch_bias_plus_wbeta(const float* W, const float* beta, const float* bias, int N, int K, float* out,
                            hipStream_t s);
void launch_pack_bias_swiglu(const float* src, float* dst, int N, hipStream_t s);
// Linear weight [N][K] fp32 (swiglu: rows interleaved as PACK_LINEAR_SWIGLU) -> fp8 e4m3 bytes [N][K] + E8M0 block
// scales [N][K/32] (one per 32 consecutive K-elements); K % 32 == 0.  colscale [K] (optional) is multiplied in before
// quantisation (a LayerNorm gamma folded into the weight).
void launch_pack_weight_fp8(const float* src, unsigned char* dst, unsigned char* scales, int N, int K, int swiglu,
                            hipStream_t s, const float* colscale = nullptr);
// out[n] = sum_k of the dequantised fp8 (MX) row n: the folded LayerNorm's mean * colsum term for fp8 weights
void launch_fp8_row_sum(const unsigned char* w, const unsigned char* scales, int N, int K, float* out, hipStream_t s);
// snake parameters: alpha -> exp(alpha), beta -> 1/(exp(beta)+1e-9)
void launch_snake_params(const float* alpha, const float* beta, float* a_out, float* ib_out, int C,
                         hipStream_t s);

// ---- NCSN++ (ncsn_kernels.hip): channels-last images, row = (item, y, x) -------------------------
// Views: x + item*bstride + row*rstride + channel (rstride >= C lets a kernel read a channel slice
// of a wider concat buffer).
void launch_ncsn_pack(const float* xt, const float* mix, int B, int n, int H, int T, int Wp, int Cp, float* of,
                      op16_t* op, long ps, int planes, hipStream_t s);
void launch_gn_stats(const float* x, long bstride, int rstride, int C, int B, int HW, float* stats,
                     hipStream_t s);   // stats [B][ceil(HW/64)][C/4][2] = (mean, M2) per 64-row slice and channel quad
void launch_gn_apply(const float* x, long bstride, int rstride, int C, int B, int HW, const float* stats,
                     const float* gamma, const float* beta, float eps, int silu, float* of, op16_t* op, long ps,
                     int planes, hipStream_t s);
void launch_fir2d(const float* x, long bstride, int rstride, int C, int B, int H, int W, int up, const float* add,
                  float* of, op16_t* op, long ps, int planes, hipStream_t s);
void launch_ncsn_fourier(const float* t, const float* w, int B, int nf, op16_t* out, long ps, int planes,
                         hipStream_t s);
void launch_ncsn_output(const float* pyr, int Cp, const float* t, const float* w, const float* bias, int cin, int n,
                        int B, int H, int T, int Wp, float* score, hipStream_t s);

// ---- metrics -----------------------------------------------------------------------------------------
// out[(b*n + i)*n + j][3] = (<ref_i, est_j>, |ref_i|^2, |est_j|^2) in fp64.  Rows are L apart; lens [B] (device,
// nullable): item b sums its first lens[b] samples only and reads nothing past them
void launch_sisdr_dots(const float* ref, const float* est, int B, int n, int L, const int* lens, double* out,
                       hipStream_t s);

// ---- STOI / ESTOI (stoi.hip) ----------------------------------------------------------------------------
// one-third-octave band b covers the 512-point FFT bins [lo[b], hi[b])
struct StoiBands {
  int lo[15], hi[15];
};
// polyphase resampling of ref and est [items][n_in] (est row ymap[item], or item when ymap is null) to
// out [2][items][n_out] with fp64 taps [ntaps] already scaled by `up` (scipy.signal.resample_poly's alignment).
// lens [items / n] (device, nullable): the items of batch entry b hold lens[b] <= n_in samples and get
// ceil(lens[b] up / down) <= n_out outputs; the rest of their output rows is left as it was
void launch_stoi_resample(const float* ref, const float* est, const int* ymap, int items, int n_in, const int* lens,
                          int n, const double* taps, int ntaps, int up, int down, int n_pre_pad, int n_pre_remove,
                          int n_out, float* out, hipStream_t s);
// the rest of STOI (extended = 0) or ESTOI (1) on 10 kHz signals x = xs + item*stride, y = ys + ymap[item]*stride
// (ymap nullable) with F = (len - 256)/128 + 1 frames each; with Fb [items / n] (device, nullable) the items of batch
// entry b have Fb[b] <= F frames (0: no frame, score 1e-5) and F sizes the buffers and grids.  Work buffers:
// en [items*F] f64, idx [items*F], Kc [items], tob [items*2*15*max(F-1,1)] f64, part [items*max(F-30,1)] f64.  -> score [items] f64 and the STFT
// frame count left after silent-frame removal, frames [items].
void launch_stoi_frames(const float* xs, const float* ys, long stride, const int* ymap, int items, int F,
                        const int* Fb, int n, StoiBands bands, int extended, double* en, int* idx, int* Kc,
                        double* tob, double* part, double* score, int* frames, hipStream_t s);

// ---- LLR / WSS / segmental SNR of the composite measures (composite.hip) ----------------------------------
#define COMPOSITE_BANDS 25
#define COMPOSITE_COND 4   // doubles per item of the condition stage: mean(ref), mean(est), scale, overall SNR (dB)
// frame geometry of a signal rate
struct CompositeShape {
  int win, hop, nfft, order;
};
// false when no kernel is instantiated for fs (8000 and 16000 are)
bool composite_shape(int fs, CompositeShape* s);
// critical-band filter b weighs the FFT bins [start[b], start[b] + len[b]) (all below nfft / 2) by
// bweights[off[b] ..]: the reference's Gaussian filters with the entries at or below the -30 dB factor left out
struct CompositeBands {
  int start[COMPOSITE_BANDS], len[COMPOSITE_BANDS], off[COMPOSITE_BANDS];
};
// ref, est [items][L] (est row ymap[item], or item when ymap is null), F >= 1 frames per item, win [shape.win] the
// fp64 window, k = round(0.95 F).  Work buffers: cond [items*COMPOSITE_COND], llr / wss / ssnr [items*F] (the
// per-frame values).  -> out [items][3] = LLR, WSS (means of the k smallest frames), segmental SNR (mean); the
// overall SNR is cond[item][3].  All fp64.  lens, Fb, kb [items / n] (device, all null or none): the items of batch
// entry b hold lens[b] <= L samples, Fb[b] in [1, F] frames and k = kb[b]; rows stay L and F apart.
void launch_composite(int fs, const float* ref, const float* est, const int* ymap, int items, int L, int F, int k,
                      const int* lens, const int* Fb, const int* kb, int n, const double* win,
                      const CompositeBands& bands, const double* bweights, double* cond, double* llr, double* wss, double* ssnr, double* out, hipStream_t s);

// ---- bss_eval SDR / SIR / SAR with F-tap distortion filters (bss_eval.hip) ----------------------------------
#define BSS_MAX_SRC 4
#define BSS_MAX_TAPS 512
#define BSS_TILE 4096                        // samples of an item one workgroup of the correlation launch takes
#define BSS_DEFAULT_BUDGET (512LL << 20)     // bytes of per-chunk workspace when the caller gives 0
// What a call on (B, n, L, F) under a workspace budget does: time tiles of the longest item, M = n F unknowns,
// correlation jobs per item (2 n^2 + n), items per chunk, and the doubles one item takes of the tile partials
// [jobs][tiles][F], the lag tables [jobs][F] and the systems (one of M and n - 1 of F unknowns: the lower triangle of
// the factor, m (m + 1) / 2 entries, then the n right-hand sides of m each); per_item = the bytes of all three.
struct BssPlan {
  int tiles, M, jobs, items_per_chunk;
  long part, tab, mat_full, mat_block, mats;
  int64_t per_item;
};
// false where dsn_bss_eval_plan refuses: B, L < 1, n outside [1, 4], F outside [1, 512], budget < 0 or below one item
inline bool bss_eval_plan(int B, int n, int L, int F, int64_t budget, BssPlan* p) {
  if (B < 1 || L < 1 || n < 1 || n > BSS_MAX_SRC || F < 1 || F > BSS_MAX_TAPS || budget < 0) return false;
  p->tiles = (int)(((long)L + BSS_TILE - 1) / BSS_TILE);
  p->M = n * F;
  p->jobs = 2 * n * n + n;
  p->part = (long)p->jobs * p->tiles * F;
  p->tab = (long)p->jobs * F;
  p->mat_full = (long)p->M * (p->M + 1) / 2 + (long)n * p->M;
  p->mat_block = (long)F * (F + 1) / 2 + (long)n * F;
  p->mats = p->mat_full + (long)(n - 1) * p->mat_block;
  p->per_item = (int64_t)sizeof(double) * (p->part + p->tab + p->mats);
  const int64_t fit = (budget ? budget : BSS_DEFAULT_BUDGET) / p->per_item;
  if (fit < 1) return false;
  p->items_per_chunk = (int)(fit < B ? fit : B);
  if (p->items_per_chunk > 65535) p->items_per_chunk = 65535;   // (a grid dimension)
  return true;
}
// items [item0, item0 + items) of ref, est [B][n][L] (lens [B] device, nullable: item b holds lens[b] <= L samples and
// nothing past them is read) -> part, tab (chunk-local, sized by the plan) and ee [B][n] = sum est_j^2
void launch_bss_corr(const float* ref, const float* est, int n, int L, const int* lens, int F, int item0, int items,
                     const BssPlan& plan, double* part, double* tab, double* ee, hipStream_t s);
// the chunk's lag tables -> Q [B][2][4][4] (Q[0][j][i]: the share of reference i's rows in pall_j; Q[1][i][j] = pt_ij)
// and status [B] (zeroed by the caller; 1 where a pivot was <= 0 or not finite).  full == 0: only the pt_ij.
// mats: the chunk's systems, plan.mats doubles per item
void launch_bss_solve(const double* tab, int n, int F, int full, double load_diag, int item0, int items,
                      const BssPlan& plan, double* mats, double* Q, int* status, hipStream_t s);
// -> sdr, sir, sar [B][n] on the chosen pairs, the pair tables [B][n][n] ([i][j]: est_j against ref_i) and perm_out
// [B][n]; perm [B][n] (device, nullable: searched, key = sum of SIR when perm_by && full, else of SDR).  Items with
// status != 0 are NaN throughout (their permutation is the caller's, or the identity)
void launch_bss_finish(const double* Q, const double* ee, const int* status, const int* perm, int B, int n, int full,
                       int perm_by, double clamp_db, double* sdr, double* sir, double* sar, double* sdr_pairs,
                       double* sir_pairs, int* perm_out, hipStream_t s);

// ---- multi-resolution STFT and time-domain reconstruction losses (mrstft.hip) -------------------------------
#define MRSTFT_MAX_SRC 4
#define MRSTFT_MAX_RES 16
#define MRSTFT_MAX_TAPS 127   // prefilter taps (odd)
#define MRSTFT_TCHUNK 1024    // samples of an item one workgroup of the time stage takes
#define MRSTFT_TACC (MRSTFT_MAX_SRC * MRSTFT_MAX_SRC * 2)                    // doubles per time-stage partial
#define MRSTFT_SACC (MRSTFT_MAX_SRC * MRSTFT_MAX_SRC * 3 + MRSTFT_MAX_SRC)   // doubles per spectral partial
// per resolution r < R: FFT length, hop, frames 1 + L / hop, frame groups per workgroup, workgroups per item and the
// offset (in doubles) of its partials [B][wgs][MRSTFT_SACC] in the partials buffer
struct MrstftPlan {
  int R;
  int fft[MRSTFT_MAX_RES], hop[MRSTFT_MAX_RES], frames[MRSTFT_MAX_RES], gpw[MRSTFT_MAX_RES], wgs[MRSTFT_MAX_RES];
  long off[MRSTFT_MAX_RES];
};
bool mrstft_fft_ok(int fft);   // a power of two in [32, 2048]
__host__ __device__ inline int mrstft_time_chunks(int L) { return (L + MRSTFT_TCHUNK - 1) / MRSTFT_TCHUNK; }
// The spectral stage's partition of one item's F = 1 + L / hop frames: groups of 2048 / fft consecutive frames, gpw
// groups per workgroup, wgs workgroups -- about 1024 workgroups per launch over the B items that share the plan.
// The dense call plans once with its B and L; a ragged call plans every item as a batch of one with its own length
// (on the host for the grid, in the kernels for the item), so an item's partition never depends on its neighbours.
struct MrstftSplit {
  int F, gpw, wgs;
};
__host__ __device__ inline MrstftSplit mrstft_split(int fft, int hop, int B, int L) {
  const int F = 1 + L / hop, fpg = 2048 / fft, groups = (F + fpg - 1) / fpg;
  const int cap = (1024 + B - 1) / B, lim = groups < cap ? groups : cap, want = lim > 1 ? lim : 1;
  const int gpw = (groups + want - 1) / want;
  return {F, gpw, (groups + gpw - 1) / gpw};
}
// fills entry r (entries 0 .. r-1 must be filled: off accumulates).  lens (host [B], nullable): the ragged plan --
// wgs[r] is the largest count any item needs (the launch grid and the stride of the partials); frames / gpw are unused
void mrstft_plan_resolution(MrstftPlan* plan, int r, int fft, int hop, int B, int L, const int* lens = nullptr);
// The three launches below take lens [B] (device, nullable): item b holds lens[b] <= L samples in its rows of stride
// L.  Its frames reflect at its own end, the prefilter reads zero past it, nothing at or past lens[b] is read or
// written, and its partials are those of mrstft_split(fft, hop, 1, lens[b]) and of the time chunks below lens[b];
// the workgroups past them leave at once and finish does not read their slots.
// x = reals, y = decoded [B][n][L] -> tpart [B][chunks][MRSTFT_TACC] (sum |r_i - d_j|, sum (r_i - d_j)^2) and, with
// taps [ntaps] (device, fp32, ntaps odd <= MRSTFT_MAX_TAPS), xf / yf [B][n][L] = conv1d(., taps, padding = ntaps / 2)
// in fp64
void launch_mrstft_time(const float* x, const float* y, int B, int n, int L, const float* taps, int ntaps, double* xf,
                        double* yf, double* tpart, hipStream_t s, const int* lens = nullptr);
// resolution r: the signals [B][n][L] are xr64 / xd64 (the prefiltered ones) or, when those are null, xr / xd;
// win [fft] the window zero-padded to the FFT length -> part + plan.off[r]
void launch_mrstft_spec(const MrstftPlan& plan, int r, const float* xr, const float* xd, const double* xr64,
                        const double* xd64, const float* win, int B, int n, int L, double* part, hipStream_t s,
                        const int* lens = nullptr);
// partials -> sc / lg / lin [R][B][n][n], l1 / l2 [B][n][n] (fp64, device)
void launch_mrstft_finish(const MrstftPlan& plan, const double* part, const double* tpart, int B, int n, int L,
                          double* sc, double* lg, double* lin, double* l1, double* l2, hipStream_t s,
                          const int* lens = nullptr);

// ---- probability-flow ODE sampler (ode.hip) ---------------------------------------------------------------
// Explicit embedded Runge-Kutta pair with scipy 1.15's solve_ivp step control on the fp64 state y [B,n,D,T].
// Stages: K[0] = f(t, y), K[1 .. stages-1] the intermediate stages, K[stages] = f(t + h, y_new) (FSAL); K holds
// stages + 1 rows of `total` doubles.
#define DSN_ODE_MAX_ROWS 7
struct OdeTableau {
  int stages;                                          // 6 (RK45), 3 (RK23)
  int err_order;                                       // error-estimator order: 4 (RK45), 2 (RK23)
  double a[DSN_ODE_MAX_ROWS][DSN_ODE_MAX_ROWS];        // a[i][j], j < i < stages
  double b[DSN_ODE_MAX_ROWS];                          // [stages]
  double c[DSN_ODE_MAX_ROWS];                          // [stages]
  double e[DSN_ODE_MAX_ROWS];                          // [stages + 1]
};
// OUVE parameters of the drift theta (y - x) - 1/2 g(t)^2 s, g(t)^2 = (sigma_min ratio^t)^2 2 log(ratio)
struct OdeSde {
  double theta, sigma_min, ratio, logratio;
};
// solver state in device memory (written by the one-thread controller kernels only)
struct OdeCtl {
  double t, t_new, h, h_abs, min_step, t_bound, direction, max_step, first_step, rtol, atol, h0, d1;
  int step_rejected, accept_pending, done, status;     // status: DSN_ODE_* (include/ditsep_hip.h), -1 running
  int nfev, accepted, rejected, attempts, max_attempts;
};
int ode_grid(long total);   // workgroups of the grid kernels = number of error-norm partials
// prior x_T = y + stdT z by launch_pc_prior itself -> xs32 (score input), widened to y64 (fp64 state); tv [B] = 1
void launch_ode_prior(const float* ymix, const float* z, double* y, float* xs32, float* tv, float stdT, int B, int n,
                      int D, int T, hipStream_t s);
// select_initial_step (scipy common.py): f0 -> K0 and the d0 / d1 partials; h0; y1 = y0 + h0 dir f0; f1 partials; h1
void launch_ode_init_f0(const OdeSde& q, const OdeCtl* ctl, const float* ymix, const float* sc, const double* y,
                        double* K0, double* part, int B, int n, int D, int T, hipStream_t s);
void launch_ode_init_h0(OdeCtl* ctl, const double* part, long total, hipStream_t s);
void launch_ode_init_y1(const OdeCtl* ctl, const double* y, const double* K0, double* xs64, float* xs32, float* tv,
                        int B, long total, hipStream_t s);
void launch_ode_init_f1(const OdeSde& q, const OdeCtl* ctl, const float* ymix, const float* sc, const double* y,
                        const double* K0, const double* xs64, double* part, int B, int n, int D, int T, hipStream_t s);
void launch_ode_init_h1(OdeCtl* ctl, const double* part, long total, int err_order, hipStream_t s);
// one attempt: prep (apply the last acceptance, first stage point), then per stage `st` = 1 .. stages the score call
// on xs32 / tv followed by launch_ode_stage(st), then launch_ode_control.  Every kernel is a no-op once ctl->done.
void launch_ode_prep(const OdeTableau& tab, const OdeCtl* ctl, double* y, const double* yn, double* K, double* xs64,
                     float* xs32, float* tv, int B, long total, hipStream_t s);
void launch_ode_stage(const OdeTableau& tab, const OdeSde& q, const OdeCtl* ctl, int stage, const float* ymix,
                      const float* sc, const double* y, double* yn, double* K, double* xs64, float* xs32, float* tv,
                      double* part, int B, int n, int D, int T, hipStream_t s);
void launch_ode_control(OdeCtl* ctl, const double* part, long total, int stages, int err_order, hipStream_t s);
// final state as fp32 -> out; tv = t_eps (the denoising step is launch_pc_predictor with zero noise: its x_mean)
void launch_ode_emit(const OdeCtl* ctl, const double* y, const double* yn, float* out, float* tv, float t_eps, int B,
                     long total, hipStream_t s);

// ---- denoising score-matching loss (loss.hip) ---------------------------------------------------------------
// out[b] = lo + (hi - lo) u_b, clamped to hi; u_b = ((w >> 8) + 0.5) / 2^24 with w word 0 of the Philox4x32-10 block
// of counter b + offset under key `seed` (randn_kernel's generator, kernels.hip)
void launch_rand_uniform(float* out, long n, unsigned long long seed, unsigned long long offset, float lo, float hi,
                         hipStream_t s);
// OUVE marginal of x(t): mean = e x0 + (1 - e) y, e = exp(-theta t); sigma = OUVESDE._std(t)
struct LossSde {
  double theta, sigma_min, logsig;
};
#define DSN_LOSS_CHUNK 2048   // elements of one (item, source) row a workgroup sums
__host__ __device__ inline int loss_chunks(int D, int T) { return (int)(((long)D * T + DSN_LOSS_CHUNK - 1) / DSN_LOSS_CHUNK); }
// perturb, one launch over [B,n,D,T]:  pit = 0: x_t = (e x0[b, perm[b,s]] + (1 - e) y) + sigma(t_b) z  (perm nullable:
// identity);  pit = 1: x_t = y + sigma(t_b) z.  Also writes tv [B] = t (the score call's time vector) and sigma [B].
// t_in nullable: every item at t_const (pit mode: T = 1).
// The three launches take tok [B] (device, nullable): the ragged form, tok[b] = 1 + frames[b], the token counts the
// length-aware attention kernels read.  perturb then writes x_t[b, :, :, frames[b]:] as zero and reads neither x0, z
// nor y there; reduce and combine walk the D frames[b] valid elements of a row in (channel, frame) order, cut into
// chunks of DSN_LOSS_CHUNK from the row's start, so an item's sums depend on its own length alone.
void launch_loss_perturb(const LossSde& q, const float* y, const float* x0, const float* z, const float* t_in,
                         float t_const, const int* perm, int pit, float* xt, float* tv, float* sigma, int B, int n,
                         int D, int T, hipStream_t s, const int* tok = nullptr);
// reduce: part[((b n + s) nj + j) chunks + c] = fp64 sum over chunk c of row (b, s) of (sigma s_theta + z_j)^2 with
// score token-major [B*T][n*D].  pit = 0: nj = 1, z_0 = z.  pit = 1: nj = n, z_j = z + (y - mean(x0[b, j])) / sigma.
void launch_loss_reduce(const LossSde& q, const float* score_tok, const float* z, const float* y, const float* x0,
                        const float* tv, const float* sigma, int pit, double* part, int B, int n, int D, int T,
                        hipStream_t s, const int* tok = nullptr);
// combine (one workgroup, fixed order): row[b n + s] = min_j (sum_c part) / (D T); mean_reduction = 0: out [B n] =
// (float)row, else out [1] = (float)(sum row / (B n)).  rows [B n] fp64 is scratch.  chunks is the stride of part
// (loss_chunks(D, T)); with tok a row sums its own loss_chunks(D, frames[b]) chunks and divides by D frames[b].
void launch_loss_combine(const double* part, double* rows, float* out, int B, int n, int nj, int chunks, int D, int T,
                         int mean_reduction, hipStream_t s, const int* tok = nullptr);

// ---- sinc resampling (resample.hip) -------------------------------------------------------------------------
// x [B][C][L] -> out [B][C or 1][Lout] by the compact polyphase table of resample_plan.h: taps [n][stride] (row p holds
// c[p][0 .. S), stride >= S), k0 [n], both on the device; kmin = min k0, kspan = max k0 + S - kmin.  lens [B] (device,
// or null: every item has L samples): item b's first ceil(n lens[b] / o) outputs are formed, the rest of its row is
// written as zero, and nothing at or past lens[b] is read.  downmix: the C channels are averaged while the input is
// staged and out has one channel.  resample_lds_refusal: nullptr, or why the plan does not fit the kernel's LDS.
long resample_lds_words(int o, int n, int stride, int kspan);
const char* resample_lds_refusal(int o, int n, int stride, int kspan, char* buf, size_t bufsz);
void launch_resample(const float* x, const int* lens, const float* taps, const int* k0, float* out, int B, int C,
                     int L, int Lout, int o, int n, int width, int S, int stride, int kmin, int kspan, int downmix,
                     hipStream_t s);

// ---- WAV payloads and the output gain (pcm.hip) -------------------------------------------------------------
struct PcmItem {      // one item of a decode call, or one row of an encode call
  long offset;        // its first byte in the byte buffer
  int frames;         // frames
  int channels, enc;  // enc: (decode only) DSN_PCM_*
  int pad;
};
// bytes per sample of DSN_PCM_U8 .. DSN_PCM_F64; 0 for anything else
__host__ __device__ inline int pcm_sample_bytes(int enc) {
  return enc == 0 ? 1 : enc == 1 ? 2 : enc == 2 ? 3 : enc == 3 || enc == 4 ? 4 : enc == 5 ? 8 : 0;   // (by code 0 .. 5)
}
long scale_output_tiles(int L);   // tiles the gain's sum launch cuts a row of L samples into
// bytes [nbytes] -> out [B][Cout][Lmax] by items [B] (device); max_frame_bytes: the widest frame among them (LDS)
void launch_pcm_decode(const unsigned char* bytes, long nbytes, const PcmItem* items, int B, int downmix, float* out,
                       int Cout, int Lmax, int max_frame_bytes, hipStream_t s);
// x [R][C][Lmax] -> row r's items[r].frames frames of its first items[r].channels channels, interleaved, as `enc` from
// bytes + items[r].offset; clipped [R] (device, zeroed by the caller) is added to with integer atomics
void launch_pcm_encode(const float* x, const PcmItem* items, int R, int C, int Lmax, int enc, unsigned char* bytes,
                       unsigned long long* clipped, hipStream_t s);
// part [B n][tiles][2] = the fp64 sums over tile c of mix sep and sep^2 + 1e-10 (t < lens[b]; tiles past it untouched);
// alpha [B n] = float(sum_c part[.][c][0] / sum_c part[.][c][1]) over the row's own ceil(lens[b] / tile) tiles;
// out = alpha sep for t < lens[b], zero past it.  lens [B] (device, or null: Lmax each)
void launch_scale_output(const float* mix, const float* sep, const int* lens, int B, int n, int Lmax, double* part,
                         float* alpha, float* out, hipStream_t s);

// ---- window stitch (stitch.hip) -----------------------------------------------------------------------------
// chunks [W][n][Lw]: window w covers samples [w hop, w hop + Lw) of a recording, hop = Lw - O, 2 O <= Lw, n <= 4.
#define DSN_STITCH_TILE 4096   // overlap positions one workgroup of the Gram launch sums
inline int stitch_tiles(int O) { return (O + DSN_STITCH_TILE - 1) / DSN_STITCH_TILE; }
// part[((w tiles + c) n + i) n + j] = fp64 sum over tile c of chunks[w][i][hop + k] * chunks[w + 1][j][k]
// (w < W - 1; exact fp64 products, per-thread strided accumulation, then a fixed tree: no atomics)
void launch_stitch_gram(const float* chunks, int W, int n, int Lw, int O, double* part, hipStream_t s);
// one workgroup.  align != 0: gram[w][i][j] = sum_c part in index order; sigma_w = the permutation with the largest
// sum_i gram[w][i][sigma(i)], candidates in lexicographic order, replaced only by a strictly greater score (ties go
// to the identity); perm [W][n]: P_0 = id, P_{w+1}(i) = sigma_w(P_w(i)).  align == 0: every P_w = id, part and gram
// are not touched.
void launch_stitch_perm(const double* part, double* gram, int* perm, int W, int n, int tiles, int align,
                        hipStream_t s);
// out [n][L]: t in the first O samples of window w >= 1 -> fall[k] chunks[w-1][P_{w-1}(i)][hop + k] +
// rise[k] chunks[w][P_w(i)][k], k = t - w hop; every other t a plain copy of chunks[w][P_w(i)][k], w = min(t / hop,
// W - 1).  fall, rise [O] fp32 (device).
void launch_stitch_gather(const float* chunks, const int* perm, const float* fall, const float* rise, float* out, int W,
                          int n, int Lw, int O, int L, hipStream_t s);

// ---- mixture-consistent STFT masks (maskrefine.hip) -----------------------------------------------------------
// mix [B][Lmax], est / out [B][n][Lmax] fp32, lens [B] (device) or null, n <= MASK_REFINE_MAX_SRC, nfft a power of two
// mask_refine_fft_ok accepts, nfft / hop in {2, 4, 8}: one launch, a workgroup per (span of output samples, item).
#define MASK_REFINE_MAX_SRC 4
bool mask_refine_fft_ok(int nfft);
void launch_mask_refine(const float* mix, const float* est, const int* lens, float* out, int B, int n, int Lmax,
                        int nfft, int hop, int power, float eps, hipStream_t s);
// Multichannel stems (dsn_stems): mix [B][C][Lmax], est [B][n][Lmax], out [B][n][C][Lmax], lens / chans [B] (device) or
// null.  wiener == 0: the launch above with a grid dimension over the channel, C <= STEMS_MASK_MAX_CH; part, R and den
// are not touched.  wiener != 0 (C <= STEMS_WIENER_MAX_CH), three launches: fp64 partials part [B][stems_stat_spans]
// [n][5][bins] over the frames each workgroup owns, R [B][n][bins][C][C] complex and den [B][n][bins] from them in
// workgroup order, and the per-bin solve inside the filter launch.  bins = nfft / 2 + 1.
#define STEMS_MASK_MAX_CH 8
#define STEMS_WIENER_MAX_CH 2
int stems_stat_spans(int nfft, int hop, int Lmax);
void launch_stems(const float* mix, const float* est, const int* lens, const int* chans, float* out, double* part,
                  double* R, double* den, int B, int C, int n, int Lmax, int wiener, int nfft, int hop, int power,
                  float eps, float reg, hipStream_t s);

// ---- mask-based MVDR beamforming (beamform.hip) --------------------------------------------------------------------
// mix [items][C][Lmax], est / out [items][n][Lmax] fp32, lens / chans [items] (device) or null, C <= BEAMFORM_MAX_CH.
// launch_beamform_weights, three launches: fp64 partials part [items][beamform_owners][n][C (C + 1)][bins] over the
// frames each owner takes (grid (owners, items, n): every frame has one owner per source; an item has at most
// BEAMFORM_MAX_OWNERS of them, each taking whole spans, more than one on long items), N [items][n][C (C + 1)][bins] from them in owner order, and the per-bin
// Cholesky solve that writes w [items][n][bins][C] complex doubles.  launch_beamform_apply: one launch, a workgroup
// per (span, item, source), w read from global memory.  bins = nfft / 2 + 1.
#define BEAMFORM_MAX_CH 8
#define BEAMFORM_MAX_OWNERS 16
#define BEAMFORM_DEFAULT_BUDGET (512L << 20)
#define BEAMFORM_MAX_SWEEPS 30
#define BEAMFORM_DEFAULT_SWEEPS 10
int beamform_owners(int nfft, int hop, int Lmax);
size_t beamform_item_doubles(int nfft, int hop, int Lmax, int C, int n);   // part and N of one item
void launch_beamform_weights(const float* mix, const float* est, const int* lens, const int* chans, int ref,
                             double* part, double* N, double* w, int items, int C, int n, int Lmax, int nfft, int hop,
                             int power, float eps, float reg, int design, int sweeps, hipStream_t s);
// the weights launch alone, on given statistics N [items][classes][C (C + 1)][bins]: the first n <= classes of the
// classes get a filter, all of them enter the interference (dsn_beamform: classes = n).  `design`
// (DSN_BEAMFORM_DESIGN_*) picks the launch: Souden's filter is beamform.hip's kernel, the rank-one MVDR and the GEV
// filter are launch_beamform_design (beamform_design.hip: `sweeps` Jacobi sweeps on the whitened N_i).
void launch_beamform_solve(const double* N, const int* chans, int ref, double* w, int items, int C, int n, int classes,
                           int bins, double reg, double eps, int design, int sweeps, hipStream_t s);
void launch_beamform_design(const double* N, const int* chans, int ref, double* w, int items, int C, int n, int classes,
                            int bins, double reg, double eps, int design, int sweeps, hipStream_t s);
void launch_beamform_apply(const float* mix, const float* est, const int* lens, const int* chans, const double* w,
                           float* out, int items, int C, int n, int Lmax, int nfft, int hop, int power, float eps,
                           int post, hipStream_t s);

// ---- block-adaptive MVDR weights (beamform_track.hip) ---------------------------------------------------------------
// dsn_beamform_track: blocks of Tb frames, Kmax = track_blocks(hop, Lmax, Tb) per item.  launch_track_weights, three
// launches: fp64 partials part [items][Kmax][n][C (C + 1)][bins] (grid (block, item, source): a block has one owner per
// source), their sums over the blocks within `context` of each block N [items][Kmax][n][C (C + 1)][bins] together with
// blockch [items][Kmax], the item's channel count for the blocks it has and 0 for the others (the solve then writes
// zero weights there), and launch_beamform_solve with (item, block) as its item: w [items][Kmax][n][bins][C] complex
// doubles.  launch_track_apply: launch_beamform_apply's layout with the weights of frame t interpolated between the
// blocks k0 and k0 + 1 (track_frame_weight).  track_item_bytes: part, N, w and blockch of one item.
#define TRACK_MIN_BLOCK 4
#define TRACK_MAX_BLOCK (1 << 20)
#define TRACK_MAX_CONTEXT 64
#define TRACK_MAX_BLOCKS 4096
#define TRACK_DEFAULT_BUDGET (512L << 20)
int track_blocks(int hop, int Lmax, int Tb);
size_t track_item_bytes(int nfft, int hop, int Lmax, int C, int n, int Tb);
void launch_track_weights(const float* mix, const float* est, const int* lens, const int* chans, int ref, double* part,
                          double* N, double* w, int* blockch, int items, int C, int n, int Lmax, int nfft, int hop,
                          int power, float eps, float reg, int Tb, int context, int design, int sweeps, hipStream_t s);
void launch_track_apply(const float* mix, const float* est, const int* lens, const int* chans, const double* w,
                        float* out, int items, int C, int n, int Lmax, int nfft, int hop, int power, float eps, int post,
                        int Tb, int interpolate, hipStream_t s);

// ---- spatial mask refinement for the beamformer (spatial.hip) --------------------------------------------------------
// mix [items][C][Lmax], est [items][n][Lmax] fp32, lens / chans [items] (device) or null.  Two launches: the transforms
// of the channels and the estimates, spectra and fp32 masks bin-major into the workspace, and one workgroup per
// (bin, item) that runs all iterations of the guided cACGMM in fp64 on-die and writes the statistics of its `classes`
// (n, or n + 1 with the noise class) in the layout launch_beamform_solve reads.  `workspace` holds spatial_item_bytes
// per item: N [n + 1][C (C + 1)][bins] doubles | X [bins][C][Fs] complex floats | M [bins][n][Fs] floats | failed [bins]
// int32, each array for all items in turn (N with `classes` per item); Fs = spatial_frames, bins = nfft / 2 + 1.
// gamma [items][classes][bins][Fs] doubles (device) or null.
#define SPATIAL_MAX_ITER 16
#define SPATIAL_DEFAULT_BUDGET (512L << 20)
int spatial_frames(int hop, int Lmax);
size_t spatial_item_bytes(int nfft, int hop, int Lmax, int C, int n);
void launch_spatial_statistics(const float* mix, const float* est, const int* lens, const int* chans, void* workspace,
                               double* gamma, int items, int C, int n, int classes, int Lmax, int nfft, int hop,
                               int power, float eps, int iterations, double noise, double floor, double mask_reg,
                               double mask_eps, hipStream_t s);

// ---- weighted prediction error dereverberation (dereverb.hip) ------------------------------------------------------
// mix / out [items][C][Lmax] fp32, lens / chans [items] (device) or null.  Three launches: the frames' transforms
// bin-major into the workspace, one workgroup per (bin, item) that runs all iterations of the K-tap, D-delay filter
// estimate in fp64 on-die (dynamic LDS dereverb_lds_bytes of the call's own C K), and the synthesis.  `workspace` holds
// dereverb_item_bytes per item: G [bins][C K][C] complex doubles | lambda [bins][Fs] doubles | Y, X [bins][C][Fs]
// complex floats | failed [bins] int32, each array for all items in turn; Fs = dereverb_frames, bins = nfft / 2 + 1.
#define DEREVERB_MAX_CH 8
#define DEREVERB_MAX_TAPS 16
#define DEREVERB_MAX_DELAY 8
#define DEREVERB_MAX_UNKNOWNS 80
#define DEREVERB_MAX_ITER 8
#define DEREVERB_DEFAULT_BUDGET (512L << 20)
int dereverb_frames(int hop, int Lmax);
size_t dereverb_lds_bytes(int C, int K, int D);
size_t dereverb_item_bytes(int nfft, int hop, int Lmax, int C, int K);
void launch_dereverb(const float* mix, const int* lens, const int* chans, void* workspace, float* out, int items, int C,
                     int Lmax, int nfft, int hop, int K, int D, int I, double reg, double eps, hipStream_t s);

// ---- ensemble combine (ensemble.hip) -----------------------------------------------------------------------------
// cands [B][K][n][Lmax], mix [B][Lmax] or null, out [B][n][Lmax] fp32, lens [B] (device) or null, K <= ENSEMBLE_MAX_K,
// n <= ENSEMBLE_MAX_SRC.  Three launches: Gram partials part [B][tiles][NB][16] (4 x 4 blocks of row pairs on and above
// the diagonal of the R = K n (+ 1) rows; ensemble_gram_plan gives NB), one workgroup per item for gram [B][R][R],
// perm [B][K][n], anchor / best [B], resid_db [B][K], agree_db [B][K][n], and the gather.
#define ENSEMBLE_MAX_K 16
#define ENSEMBLE_MAX_SRC 4
#define ENS_TILE 2048   // samples one workgroup of the Gram launch sums, counted from the item's own start
inline int ensemble_tiles(int Lmax) { return (Lmax + ENS_TILE - 1) / ENS_TILE; }
void ensemble_gram_plan(int R, int* RB, int* NB, int* S, int* SUBQ);
void launch_ensemble_gram(const float* cands, const float* mix, const int* lens, double* part, int B, int K, int n,
                          int Lmax, hipStream_t s);
void launch_ensemble_solve(const int* lens, const double* part, double* gram, int* perm, int* anchor, int* best,
                           double* resid_db, double* agree_db, int B, int K, int n, int Lmax, int has_mix,
                           hipStream_t s);
void launch_ensemble_gather(const float* cands, const int* lens, const int* perm, const int* anchor, const int* best,
                            float* out, int B, int K, int n, int Lmax, int mode, hipStream_t s);

// ---- loudness, true peak and the gain (loudness.hip) -----------------------------------------------------------
// x [B][C][Lmax] fp32, C <= LOUD_MAX_CH.  items [B] and rates [distinct rates] are device tables: an item's samples,
// channels, segment length h = (fs + 5) / 10 and the row of `rates` with its K-weighting coefficients (kweight_coeffs'
// ten) and the zero-input transition of the cascade's four state variables over LOUD_CHUNK samples (row-major).
// Four launches: the chunks' final states from zero state into state [B][C][chunks][4]; one thread per (item, channel)
// turning them into the chunks' initial states in place; the chunks again from those, their y^2 sums into part
// [B][C][chunks][2] (the segment the chunk starts in, and the next); one workgroup per item for seg [B][C][segs],
// z [B][segs] and stats [B][6].  want_tp and the sample peak: one launch that stages tiles of LOUD_PEAK_TILE samples and
// their halo, peaks [B][2] (true, sample; the bits of non-negative floats under an integer maximum) and bad [B] zeroed
// by the caller.  taps [4][stride], k0 [4]: the (1, 4) resampling tables on the device.
#define LOUD_MAX_CH 2
#define LOUD_CHUNK 256
#define LOUD_MIN_RATE 8000
#define LOUD_MAX_RATE 192000
#define LOUD_PEAK_TILE 2048
struct LoudRate {
  double c[10];
  double P[16];
};
struct LoudItem {
  int len, ch, h, rate;
};
void kweight_coeffs(int fs, double out[10]);
void kweight_chunk_transition(const double c[10], double P[16]);
inline long loudness_chunks(int Lmax) { return ((long)Lmax + LOUD_CHUNK - 1) / LOUD_CHUNK; }
inline long loudness_segments(int Lmax) { return (long)Lmax / ((LOUD_MIN_RATE + 5) / 10) + 1; }
void launch_loudness(const float* x, const LoudItem* items, const LoudRate* rates, int B, int C, int Lmax, double* state,
                     double* part, double* seg, double* z, unsigned* peaks, unsigned long long* bad, double* stats,
                     const float* taps, const int* k0, int S, int stride, int kmin, int kspan, int width, int want_tp,
                     hipStream_t s);
// out = gain[r] x over a row's own samples and channels (rows [R]: len, ch), zero elsewhere; out may be x
void launch_apply_gain(const float* x, const LoudItem* rows, const float* gain, float* out, int R, int C, int Lmax,
                       hipStream_t s);

// ---- true-peak look-ahead limiter (limiter.hip) ------------------------------------------------------------------
// x [R][C][Lmax] fp32.  rows [R] and groups [G] are device tables: a row's samples, channels and group; a group's rows
// [row0, row1), their common length, the half-window W, the row of `window` ([distinct W][2 LIM_MAX_W + 1], w[-W .. W]
// from column 0) and the pre-gain.  Two launches over tiles of LIM_TILE samples: the required gain r into req
// [G][Lmax] (and the envelope p into env [G][Lmax] unless null) with bad [G] counting non-finite samples, then the
// curve [G][Lmax] with reduced [G] (samples with g < 1) and deepest [G] (0x3f800000 minus the bits of the smallest g,
// under an integer maximum); bad, reduced and deepest zeroed by the caller.  taps [4][stride], k0 [4]: the (1, 4)
// resampling tables on the device.
#define LIM_TILE 2048
#define LIM_MAX_W 1024
struct LimRow {
  int len, ch, group, pad;
};
struct LimGroup {
  int row0, row1, len, W, wofs;
  float pregain;
};
size_t limiter_curve_lds(int Wmax);
void launch_limiter_curve(const float* x, const LimRow* rows, const LimGroup* groups, int G, int C, int Lmax, int Wmax,
                          float ceiling, const float* window, const float* taps, const int* k0, int S, int stride,
                          int kmin, int kspan, int width, float* req, float* env, float* curve, unsigned long long* bad,
                          unsigned long long* reduced, unsigned* deepest, hipStream_t s);
// out = (pregain[group] x) curve[group][t] over a row's own samples and channels, zero elsewhere; out may be x
void launch_apply_curve(const float* x, const LimRow* rows, const float* pregain, const float* curve, float* out, int R,
                        int C, int Lmax, hipStream_t s);

// ---- speaker activity of separated stems (activity.hip) ----------------------------------------------------------
// est [B][n][Lmax] fp32, lens [B] (device) or null; energy, level [B][n][Fmax] fp64, act [B][n][Fmax] bytes, frames_on
// [B][n], Fmax = activity_frames(hop, Lmax).  Two launches: the band energies (workgroup per frame group and item), then
// level, thresholds, hysteresis and run rules (workgroup per item, chunked scans).  The band [j_lo, j_hi] and the four
// threshold factors come from the host.
#define ACTIVITY_MAX_FRAMES (1 << 22)
#define ACTIVITY_MAX_HALF_WIDTH 1024
#define ACTIVITY_MAX_FADE 4096
#define ACTIVITY_MIN_HOP 8   // the smallest hop of the STFT; bounds the frames a gate span stages
#define ACTIVITY_MAX_HOP 65536
int activity_frames(int hop, int Lmax);
void launch_activity(const float* est, const int* lens, int B, int n, int Lmax, int nfft, int hop, int j_lo, int j_hi,
                     int half_width, double c_r, double c_d, double c_rs, double c_ds, int min_on, int min_off, int pad,
                     double* energy, double* level, uint8_t* act, int* frames_on, hipStream_t s);
// out = x inside the segments act marks (frame (m + hop / 2) / hop owns sample m), ramp[d - 1] x at distance d <= fade
// from the nearest segment sample, +0 further away and past the item's end.  act [B][n][Fa] bytes, ramp [fade]; out may
// be x.
void launch_activity_gate(const float* x, const uint8_t* act, const int* lens, const float* ramp, float* out, int B, int n,
                          int Lmax, int Fa, int hop, int fade, hipStream_t s);
