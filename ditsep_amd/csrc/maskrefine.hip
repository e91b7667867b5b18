// Mixture-consistent STFT masks (dsn_mask_refine; the definition is in include/ditsep_hip.h, restated in float64 in
// tests/mask_refine_restatement.py): soft masks from the magnitudes of the estimates, applied to the mixture's STFT
// and transformed back, so every output carries the mixture's phase and the outputs add up to the mixture.
//
// One launch, no frame workspace.  Workgroup (c, b) owns the output samples [c SPAN, (c + 1) SPAN) of item b, SPAN a
// multiple of every hop, and forms all SPAN / hop + n_fft / hop - 1 frames that touch them itself: the frames it
// shares with its neighbours are recomputed, not exchanged.  Frames go through LDS in groups of 2048 / n_fft:
//   load      the n + 1 signals of a frame (mixture, estimates) from global memory, reflected at the item's own padded
//             end Lp_b and zero at or past lens[b] (never read there), times the window
//   forward   every real frame alone as ONE complex transform of half the length: z[t] = x[2t] + i x[2t + 1] packs its
//             even and odd samples, a Stockham radix-2 in LDS (fp32; twiddles from sincospi in double, rounded once)
//             transforms it, and the conjugate-symmetry split E[k] = (Z[k] + conj Z[H - k]) / 2, O[k] = (Z[k] -
//             conj Z[H - k]) / 2i, X[k] = E[k] + w^k O[k], X[H - k] = conj(E[k] - w^k O[k]) gives bins 0 .. n_fft / 2
//   masks     per bin a_i = |S_i|^power, M_i = (a_i + eps) / (((a_0 + a_1) + ..) + n eps), Y_i = M_i X -- and at once
//             the inverse of the split, so the n spectra are again half-length complex transforms in place
//   inverse   the same Stockham with conjugated twiddles; Re and Im are the even and odd samples of the frame
//   add       y w / n_fft added into the workgroup's SPAN samples in LDS, frame after frame in frame order
// and at the end every sample is divided by the sum of w^2 over the frames of the item that cover it (in frame order)
// and stored, 16 bytes at a time where the rows allow; at or past lens[b] the row is written as zero.
//
// A pair of signals is NOT packed into one full-length transform: there the rounding of one signal's spectrum depends
// on its partner, and the contract's exact cases (n = 1 hands the mixture's own transform back whatever the estimate
// holds; silent estimates give the n = 1 bits scaled by 1 / n) would not hold.  Packing a signal's own even and odd
// samples costs no more butterflies (2 x H/2 log2 H against H log2 2H for a pair) and leaves no odd source over.
//
// Bit identity: a frame's values depend on the item's samples and the frame index alone -- the same code with floating
// point contraction off and the fused multiply-adds written out, whichever workgroup and frame slot computes it --,
// every sample adds its frames in increasing frame order starting from +0, and there are no atomics.  So the result
// does not depend on SPAN, on the batch position or on the other items, and two calls give identical bits.
//
// dsn_stems (multichannel stems from mono estimates) runs the same kernel in three modes:
//   MR_MASK    the launch above with a grid dimension over the mixture's channels: workgroup (c, b, ch) filters channel
//              ch of item b with the masks of the mono estimates and writes out[b][i][ch].  The mono call is C = 1.
//   MR_STATS   workgroup (c, b) owns the frames [c SPAN / hop, (c + 1) SPAN / hop) of item b -- every frame has exactly
//              one owner --, transforms its C channels and n estimates and sums, per bin, M_i^2 X X^H and v_i in fp64
//              over its frames in increasing order: the thread that owns a bin adds one group of frames in registers
//              and then adds that to the workgroup's own partial in global memory (plain loads and stores).
//   (reduce)   one thread per (item, source, bin) adds the partials in workgroup order and writes R = N / d and d.
//   MR_WIENER  as MR_MASK, but all C channels are transformed and, in place of Y = M X, the per-bin solve of the
//              multichannel Wiener filter runs in fp64 with R read from global memory; only channel ch of the n
//              outputs is formed, rounded once to fp32, and transformed back.
// In every mode a frame goes through the same functions of maskrefine_dev.h -- mr_tables, mr_load, mr_fft, mr_split and
// mr_masks, then mr_merge, mr_add and mr_finish --, which beamform.hip and dereverb.hip call too, so X, S, M and the
// output samples have the same bits wherever they are formed.
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

#include "maskrefine_dev.h"   // the frame pipeline: shared with beamform.hip and dereverb.hip

// tests/test_gpu_mask_refine.py reads the spans from the text of this file, so they are stated here as well.  Every
// kernel and launch uses maskrefine_dev.h's mr_span(nfft); the assertion keeps this statement equal to it.
template <int NFFT>
constexpr int mr_span() { return NFFT >= 2048 ? 4096 : 2048; }
static_assert(mr_span<64>() == mr_span(64) && mr_span<128>() == mr_span(128) && mr_span<256>() == mr_span(256) &&
                  mr_span<512>() == mr_span(512) && mr_span<1024>() == mr_span(1024) &&
                  mr_span<2048>() == mr_span(2048),
              "the spans stated in maskrefine.hip are not those of maskrefine_dev.h");

constexpr int MR_BF = (MR_MAX_SRC + 1) * (MR_POINTS / 2) / MRT;   // butterflies per thread and stage at n = 4
constexpr int MR_BF_STEMS = (STEMS_WIENER_MAX_CH + MR_MAX_SRC) * (MR_POINTS / 2) / MRT;   // .. with C = 2 channels
enum { MR_MASK = 0, MR_STATS = 1, MR_WIENER = 2 };
constexpr int MR_STAT = 5;   // fp64 sums per (source, bin): N00, N11, Re N01, Im N01, d

// One bin of the multichannel Wiener filter in fp64 (include/ditsep_hip.h, dsn_stems): X [Cb] the mixture's channels,
// M [n] the masks, R -> R_0 of this bin ([C][C] complex as double pairs, source stride rs doubles); Y [n] = channel
// `co` of the n outputs, rounded once.  Cb is 1 or 2; Cb = 1 reads R[0] only.
__device__ __forceinline__ void mr_wiener_bin(const MaskRefineShape& q, int Cb, int co, const float2* X, const float* M,
                                              const double* __restrict__ R, long rs, float2* Y) {
  const int n = q.n, C = q.C;
  const double x0r = X[0].x, x0i = X[0].y, x1r = Cb > 1 ? (double)X[1].x : 0.0, x1i = Cb > 1 ? (double)X[1].y : 0.0;
  const double p = ((x0r * x0r + x0i * x0i) + (x1r * x1r + x1i * x1i)) / (double)Cb;
  double v[MR_MAX_SRC], s00 = 0.0, s11 = 0.0, s01r = 0.0, s01i = 0.0;
#pragma unroll
  for (int i = 0; i < MR_MAX_SRC; ++i)
    if (i < n) {
      const double* Ri = R + i * rs;
      v[i] = ((double)M[i] * (double)M[i]) * p;
      s00 += v[i] * Ri[0];
      if (Cb > 1) {
        s11 += v[i] * Ri[2 * (C + 1)];
        s01r += v[i] * Ri[2];
        s01i += v[i] * Ri[3];
      }
    }
  const double lam = (double)q.reg * ((s00 + s11) / (double)Cb) + (double)q.eps;
  const double a00 = s00 + lam, a11 = s11 + lam;
  double z0r, z0i, z1r = 0.0, z1i = 0.0;
  if (Cb > 1) {   // z = adj(A) X / det A, A = [[a00, s01], [conj s01, a11]]
    const double det = a00 * a11 - (s01r * s01r + s01i * s01i);
    z0r = (a11 * x0r - (s01r * x1r - s01i * x1i)) / det;
    z0i = (a11 * x0i - (s01r * x1i + s01i * x1r)) / det;
    z1r = (a00 * x1r - (s01r * x0r + s01i * x0i)) / det;
    z1i = (a00 * x1i - (s01r * x0i - s01i * x0r)) / det;
  } else {
    z0r = x0r / a00;
    z0i = x0i / a00;
  }
  const double share = lam / (double)n, zr = co == 0 ? z0r : z1r, zi = co == 0 ? z0i : z1i;
#pragma unroll
  for (int i = 0; i < MR_MAX_SRC; ++i)
    if (i < n) {
      const double* Rc = R + i * rs + 2 * co * C;   // row `co` of R_i
      double yr = Rc[0] * z0r - Rc[1] * z0i, yi = Rc[0] * z0i + Rc[1] * z0r;
      if (Cb > 1) {
        yr += Rc[2] * z1r - Rc[3] * z1i;
        yi += Rc[2] * z1i + Rc[3] * z1r;
      }
      Y[i] = make_float2((float)(v[i] * yr + share * zr), (float)(v[i] * yi + share * zi));
    }
}

// mix [B][C][Lmax], est [B][n][Lmax], out [B][n][C][Lmax], lens / chans [B] or null (Lmax / C each).
// MR_MASK, MR_WIENER: grid (ceil(Lmax / SPAN), B, C); MR_STATS: grid (frame spans, B), part [B][spans][n][MR_STAT][H + 1].
// Rg [B][n][H + 1][C][C][2] (MR_WIENER).
// Dynamic LDS: float2 tw[H] | float2 buf[NX + n][G][H] | float win[NFFT] | float ola[n][SPAN] (not MR_STATS), NX = 1
// (MR_MASK) or C mixture channels
template <int NFFT, int MODE>
__global__ __launch_bounds__(MRT) void mask_refine_kernel(const MaskRefineShape q, const float* __restrict__ mix,
                                                          const float* __restrict__ est,
                                                          const int* __restrict__ lens, const int* __restrict__ chans,
                                                          float* __restrict__ out, const double* __restrict__ Rg,
                                                          double* __restrict__ part) {
  static_assert(NFFT >= 64 && NFFT <= 2 * MR_POINTS && (NFFT & (NFFT - 1)) == 0, "FFT size");
  constexpr int H = NFFT / 2, G = MR_POINTS / H, NP = H / 2 + 1, SPAN = mr_span(NFFT);
  constexpr int BF = MODE == MR_MASK ? MR_BF : MR_BF_STEMS;
  extern __shared__ __attribute__((aligned(16))) float2 mr_lds[];
  const int n = q.n, hop = q.hop, tid = threadIdx.x;
  const int b = blockIdx.y, co = blockIdx.z, s0 = blockIdx.x * SPAN;
  const int Cb = chans ? chans[b] : q.C;
  const int nx = MODE == MR_MASK ? 1 : Cb;          // mixture channels in LDS: slots 0 .. nx - 1, then the estimates
  const int cx = MODE == MR_MASK ? co : 0;          // .. the first of them
  float2* tw = mr_lds;
  float2* buf = tw + H;
  float* win = reinterpret_cast<float*>(buf + ((MODE == MR_MASK ? 1 : q.C) + n) * MR_POINTS);
  float* ola = win + NFFT;
  const MrItem it = mr_item(lens, b, q.Lmax, hop);
  const float* mixb = mix + ((long)b * q.C + cx) * q.Lmax;
  const float* estb = est + (long)b * n * q.Lmax;
  float* outb = out + ((long)b * n * q.C + co) * q.Lmax;   // source i: + i C Lmax
  const long orow = (long)q.C * q.Lmax;

  if (MODE != MR_STATS && (s0 >= it.L || co >= Cb)) {   // (uniform) past the item's end, or a channel it does not have
    mr_zero<H>(outb, orow, n, s0, q.Lmax, q.vec, tid);
    return;
  }
  const int fps = SPAN / hop;   // MR_STATS: the frames one workgroup owns
  if (MODE == MR_STATS && (int)blockIdx.x * fps >= it.F) return;   // (uniform)

  mr_tables<H>(tw, win, tid);
  if (MODE != MR_STATS)
    for (int e = tid; e < n * SPAN; e += MRT) ola[e] = 0.f;

  const MrFrames fr = mr_frames<H>(it, s0, hop);
  const int pend = fr.pend;
  const int f_first = MODE == MR_STATS ? (int)blockIdx.x * fps : fr.f_first;
  const int f_last = MODE == MR_STATS ? min(it.F, f_first + fps) - 1 : fr.f_last;
  const long rs = 2L * (H + 1) * q.C * q.C;   // doubles between R_i and R_{i+1} of an item
  double* partw = MODE == MR_STATS ? part + ((long)b * gridDim.x + blockIdx.x) * n * MR_STAT * (H + 1) : nullptr;

  for (int f0 = f_first; f0 <= f_last; f0 += G) {
    __syncthreads();   // the tables are in; the previous group's frames have been added
    mr_load<H>(buf, win, mixb, estb, q.Lmax, it, hop, nx, n, f0, f_last, tid);
    __syncthreads();
    mr_fft<H, false, BF>(buf, tw, (nx + n) * (MR_POINTS / 2), tid);
    if (MODE == MR_STATS) {
      // ---- statistics: a thread owns bin j for the whole launch and adds this group's frames in frame order
      for (int j = tid; j <= H; j += MRT) {
        const bool lower = 2 * j <= H;
        const int k = lower ? j : H - j, km = (H - k) & (H - 1);
        const float2 t = tw[k];
        double acc[MR_MAX_SRC][MR_STAT];
#pragma unroll
        for (int i = 0; i < MR_MAX_SRC; ++i)
#pragma unroll
          for (int u = 0; u < MR_STAT; ++u) acc[i][u] = 0.0;
        for (int fg = 0; fg < G && f0 + fg <= f_last; ++fg) {
          float2 xk, xm;
          float mk[MR_MAX_SRC], mm[MR_MAX_SRC];
          const float2* a = buf + fg * H;
          mr_split(a[k], a[km], t, xk, xm);
          const float2 x0 = lower ? xk : xm;
          float2 x1 = make_float2(0.f, 0.f);
          if (nx > 1) {
            mr_split(a[MR_POINTS + k], a[MR_POINTS + km], t, xk, xm);
            x1 = lower ? xk : xm;
          }
          mr_masks(q, buf + nx * MR_POINTS + fg * H, k, km, t, mk, mm);
          const double x0r = x0.x, x0i = x0.y, x1r = x1.x, x1i = x1.y;
          const double p00 = x0r * x0r + x0i * x0i, p11 = x1r * x1r + x1i * x1i;
          const double p01r = x0r * x1r + x0i * x1i, p01i = x0i * x1r - x0r * x1i;   // X_0 conj X_1
          const double pm = (p00 + p11) / (double)nx;
#pragma unroll
          for (int i = 0; i < MR_MAX_SRC; ++i)
            if (i < n) {
              const double m = lower ? mk[i] : mm[i], m2 = m * m;
              acc[i][0] += m2 * p00;
              acc[i][1] += m2 * p11;
              acc[i][2] += m2 * p01r;
              acc[i][3] += m2 * p01i;
              acc[i][4] += m2 * pm;
            }
        }
#pragma unroll
        for (int i = 0; i < MR_MAX_SRC; ++i)
          if (i < n) {
#pragma unroll
            for (int u = 0; u < MR_STAT; ++u) {
              double* d = partw + ((long)i * MR_STAT + u) * (H + 1) + j;
              *d = f0 == f_first ? acc[i][u] : *d + acc[i][u];
            }
          }
      }
      continue;
    }
    // ---- masks: one thread per (frame, pair of bins k and H - k); the estimates' slots become Y_i, packed again
    for (int e = tid; e < G * NP; e += MRT) {
      const int fg = e / NP, k = e - fg * NP, km = (H - k) & (H - 1);
      if (f0 + fg > f_last) continue;
      const float2 t = tw[k];
      float2 xk[STEMS_WIENER_MAX_CH], xm[STEMS_WIENER_MAX_CH], yk[MR_MAX_SRC], ym[MR_MAX_SRC];
      float mk[MR_MAX_SRC], mm[MR_MAX_SRC];
      const float2* a = buf + fg * H;
      mr_split(a[k], a[km], t, xk[0], xm[0]);
      if (MODE == MR_WIENER && nx > 1) mr_split(a[MR_POINTS + k], a[MR_POINTS + km], t, xk[1], xm[1]);
      mr_masks(q, buf + nx * MR_POINTS + fg * H, k, km, t, mk, mm);
      if (MODE == MR_WIENER) {
        const double* Rb = Rg + (long)b * n * rs;
        mr_wiener_bin(q, Cb, co, xk, mk, Rb + 2L * k * q.C * q.C, rs, yk);
        mr_wiener_bin(q, Cb, co, xm, mm, Rb + 2L * (H - k) * q.C * q.C, rs, ym);
      } else {
#pragma unroll
        for (int i = 0; i < MR_MAX_SRC; ++i)
          if (i < n) {
            yk[i] = make_float2(mk[i] * xk[0].x, mk[i] * xk[0].y);
            ym[i] = make_float2(mm[i] * xm[0].x, mm[i] * xm[0].y);
          }
      }
#pragma unroll
      for (int i = 0; i < MR_MAX_SRC; ++i)
        if (i < n) {
          float2 zk, zm;
          mr_merge(yk[i], ym[i], t, zk, zm);
          float2* o = buf + ((nx + i) * G + fg) * H;
          o[k] = zk;
          if (km != k) o[km] = zm;
        }
    }
    __syncthreads();
    mr_fft<H, true, BF>(buf + nx * MR_POINTS, tw, n * (MR_POINTS / 2), tid);
    for (int i = 0; i < n; ++i)
      mr_add<H>(ola + i * SPAN, buf + (nx + i) * MR_POINTS, win, s0, pend, hop, f0, min(f0 + G - 1, f_last), tid);
  }
  if (MODE != MR_STATS) mr_finish<H>(ola, win, outb, orow, n, it, s0, pend, hop, q.Lmax, q.vec, tid);
}

// R [B][n][H + 1][C][C] complex and den [B][n][H + 1] from part [B][spans][n][MR_STAT][H + 1]: one thread per (item,
// source, bin) adds the item's own ceil(F / fps) partials in workgroup order; R = N / d, the identity where d = 0,
// zero outside the item's own channels.
__global__ __launch_bounds__(MRT) void stems_reduce_kernel(const double* __restrict__ part, const int* __restrict__ lens,
                                                           const int* __restrict__ chans, int B, int n, int C, int Lmax,
                                                           int bins, int hop, int fps, int spans,
                                                           double* __restrict__ R, double* __restrict__ den) {
  const long e = (long)blockIdx.x * MRT + threadIdx.x;
  if (e >= (long)B * n * bins) return;
  const int j = (int)(e % bins), i = (int)(e / bins % n), b = (int)(e / bins / n);
  const int L = lens ? lens[b] : Lmax, Cb = chans ? chans[b] : C;
  const int F = 1 + (L + hop - 1) / hop, ns = (F + fps - 1) / fps;
  double s[MR_STAT] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int c = 0; c < ns; ++c)
#pragma unroll
    for (int u = 0; u < MR_STAT; ++u)
      s[u] += part[((((long)b * spans + c) * n + i) * MR_STAT + u) * bins + j];
  const double d = s[4];
  double* Re = R + 2 * e * C * C;
  for (int u = 0; u < 2 * C * C; ++u) Re[u] = 0.0;
  Re[0] = d == 0.0 ? 1.0 : s[0] / d;
  if (Cb > 1) {
    Re[2 * (C + 1)] = d == 0.0 ? 1.0 : s[1] / d;
    if (d != 0.0) {
      Re[2] = s[2] / d, Re[3] = s[3] / d;
      Re[2 * C] = s[2] / d, Re[2 * C + 1] = -(s[3] / d);
    }
  }
  den[e] = d;
}

struct MrArgs {
  const float *mix, *est;
  const int *lens, *chans;
  float* out;
  double *R, *den, *part;
  int B;
};

template <int NFFT, int MODE>
void mr_launch(const MaskRefineShape& q, const MrArgs& a, dim3 grid, hipStream_t st) {
  const int nxmax = MODE == MR_MASK ? 1 : STEMS_WIENER_MAX_CH, nx = MODE == MR_MASK ? 1 : q.C;
  const bool ola = MODE != MR_STATS;
  dsn_allow_lds<mask_refine_kernel<NFFT, MODE>>((int)mr_lds_bytes(NFFT, nxmax + MR_MAX_SRC, ola ? MR_MAX_SRC : 0));
  hipLaunchKernelGGL((mask_refine_kernel<NFFT, MODE>), grid, dim3(MRT), mr_lds_bytes(NFFT, nx + q.n, ola ? q.n : 0), st,
                     q, a.mix, a.est, a.lens, a.chans, a.out, a.R, a.part);
}

template <int NFFT>
void mr_run(int wiener, const MaskRefineShape& q, const MrArgs& a, hipStream_t st) {
  constexpr int SPAN = mr_span(NFFT);
  const dim3 grid((unsigned)((q.Lmax + SPAN - 1) / SPAN), (unsigned)a.B, (unsigned)q.C);
  if (!wiener) {
    mr_launch<NFFT, MR_MASK>(q, a, grid, st);
    return;
  }
  const int spans = stems_stat_spans(NFFT, q.hop, q.Lmax), bins = NFFT / 2 + 1;
  mr_launch<NFFT, MR_STATS>(q, a, dim3((unsigned)spans, (unsigned)a.B), st);
  const long rows = (long)a.B * q.n * bins;
  hipLaunchKernelGGL(stems_reduce_kernel, dim3((unsigned)((rows + MRT - 1) / MRT)), dim3(MRT), 0, st, a.part, a.lens,
                     a.chans, a.B, q.n, q.C, q.Lmax, bins, q.hop, SPAN / q.hop, spans, a.R, a.den);
  mr_launch<NFFT, MR_WIENER>(q, a, grid, st);
}

void mr_dispatch(int nfft, int wiener, const MaskRefineShape& q, const MrArgs& a, hipStream_t st) {
  mr_for_nfft(nfft, [&](auto N) { mr_run<decltype(N)::value>(wiener, q, a, st); });
}

}  // namespace

bool mask_refine_fft_ok(int nfft) { return nfft >= 64 && nfft <= 2 * MR_POINTS && (nfft & (nfft - 1)) == 0; }

void launch_mask_refine(const float* mix, const float* est, const int* lens, float* out, int B, int n, int Lmax,
                        int nfft, int hop, int power, float eps, hipStream_t st) {
  const MaskRefineShape q{n, Lmax, hop, power, eps, ((uintptr_t)out & 15) == 0 && Lmax % 4 == 0 ? 1 : 0, 1, 0.f};
  mr_dispatch(nfft, 0, q, MrArgs{mix, est, lens, nullptr, out, nullptr, nullptr, nullptr, B}, st);
}

int stems_stat_spans(int nfft, int hop, int Lmax) {
  const int F = 1 + (Lmax + hop - 1) / hop, fps = mr_span(nfft) / hop;
  return (F + fps - 1) / fps;
}

void launch_stems(const float* mix, const float* est, const int* lens, const int* chans, float* out, double* part,
                  double* R, double* den, int B, int C, int n, int Lmax, int wiener, int nfft, int hop, int power,
                  float eps, float reg, hipStream_t st) {
  const MaskRefineShape q{n, Lmax, hop, power, eps, ((uintptr_t)out & 15) == 0 && Lmax % 4 == 0 ? 1 : 0, C, reg};
  mr_dispatch(nfft, wiener, q, MrArgs{mix, est, lens, chans, out, R, den, part, B}, st);
}
