// Pair tables of the multi-resolution STFT loss and the time-domain L1 / L2 losses of the reference's LDM objective
// (stable_audio_tools/training/losses/auraloss.py::MultiResolutionSTFTLoss under losses.py::PITLoss; restated in
// float64 in tests/mrstft_restatement.py, pinned to the reference's own modules by tests/golden/mrstft.npz).
// The reference evaluates the whole loss once per source permutation; every term of every permutation is a mean of
// values of one (item b, reference source i, estimate source j) pair, so each spectrum is formed once.
// Stages:
//   time     per (b, chunk of samples): the pair partials sum |r_i - d_j| and sum (r_i - d_j)^2 on the raw signals and,
//            with taps, the zero-padded "same" FIR (cross-correlation, fp64 accumulation) of all 2 n signals of the
//            item into an fp64 workspace
//   spectral per resolution and (b, block of frames): torch.stft's frames (center = True, reflect padding, window
//            zero-padded to the FFT length); source i's reference and estimate frames are the real and imaginary part
//            of one complex FFT (Stockham radix-2 in LDS, fp64) and are separated by conjugate symmetry; per bin
//            mag = sqrt(max(re^2 + im^2, 1e-8)) and the pair partials sum (mag_d - mag_r)^2, sum |log mag_r -
//            log mag_d|, sum |mag_r - mag_d| and, per estimate, sum mag_d^2 in fp64.  No magnitude goes to memory.
//   finish   the workgroup partials summed in index order in fp64 -> the pair tables
// Every reduction has a fixed order (no atomics): two calls on the same input give bit-identical results.
// Ragged batches (lens non-null in all three kernels): item b holds lens[b] samples in rows of stride L.  Its frames,
// its reflection, the zero past the end that the prefilter reads and the divisors are those of its own length, and
// its partition into workgroup partials is the one the item gets as a batch of one (mrstft_split(fft, hop, 1,
// lens[b]); time chunks from the item's start), so its tables have the same bits alone, at any batch position and
// under any padding.  Workgroups an item does not need leave before their first barrier and write nothing; finish
// sums the item's own partials only.
// The filtered signals, the windowed frames and the transforms are fp64: the A-weighted spectra span more than 80 dB,
// the log-magnitude term weighs every bin alike, and on a single resolution with few frames the float32 rounding of
// the filtered signal alone moves that term by up to 1.2e-6 (the fp32 FFT by 1.6e-6, measured), past the 1e-6 the
// tests allow.
#include "kernels.h"

namespace {

constexpr int kThreads = 256;      // time and finish stages
constexpr int kSpecThreads = 512;  // spectral stage
constexpr int kMaxSrc = MRSTFT_MAX_SRC;
constexpr int kPoints = 2048;  // complex points per source a workgroup transforms together: 2048 / NFFT frames

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// workgroup sum of v in a fixed order (WAVES waves).  red: WAVES doubles of LDS.
template <int WAVES>
__device__ inline double block_sum(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();  // red may still be read by the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) s += red[w];
  return s;
}

// ---- time-domain partials and the prefilter ---------------------------------------------------------------
// x = reals, y = decoded, [B][n][L].  Workgroup (chunk c, item b): samples [c * MRSTFT_TCHUNK, ...).
// tpart[(b * chunks + c) * MRSTFT_TACC + (i * 4 + j) * 2 + {0: sum |r_i - d_j|, 1: sum (r_i - d_j)^2}].
// FILTER: xf / yf [B][n][L] = conv1d(x, taps, padding = ntaps / 2) (cross-correlation), ntaps odd and <= MRSTFT_MAX_TAPS.
template <bool FILTER>
__global__ __launch_bounds__(kThreads) void mrstft_time_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                               int n, int L, const float* __restrict__ taps, int ntaps,
                                                               double* __restrict__ xf, double* __restrict__ yf,
                                                               double* __restrict__ tpart,
                                                               const int* __restrict__ lens) {
  constexpr int kHalo = MRSTFT_MAX_TAPS - 1;
  __shared__ float sig[FILTER ? 2 * kMaxSrc : 1][FILTER ? MRSTFT_TCHUNK + kHalo : 1];
  __shared__ double tp[FILTER ? MRSTFT_MAX_TAPS : 1];
  __shared__ double red[4];
  const int b = blockIdx.y, c = blockIdx.x, chunks = gridDim.x;
  const int Lb = lens ? lens[b] : L;  // the item's samples; the rows keep the stride L
  const int t0 = c * MRSTFT_TCHUNK, tn = min(MRSTFT_TCHUNK, Lb - t0);
  if (tn <= 0) return;  // uniform: a chunk past the item's end
  const float* xb = x + (long)b * n * L;
  const float* yb = y + (long)b * n * L;
  double a1[kMaxSrc][kMaxSrc], a2[kMaxSrc][kMaxSrc];
#pragma unroll
  for (int i = 0; i < kMaxSrc; ++i)
#pragma unroll
    for (int j = 0; j < kMaxSrc; ++j) a1[i][j] = a2[i][j] = 0.0;
  for (int t = threadIdx.x; t < tn; t += kThreads) {
    double r[kMaxSrc], d[kMaxSrc];
#pragma unroll
    for (int i = 0; i < kMaxSrc; ++i) {
      r[i] = i < n ? (double)xb[(long)i * L + t0 + t] : 0.0;
      d[i] = i < n ? (double)yb[(long)i * L + t0 + t] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < kMaxSrc; ++i)
#pragma unroll
      for (int j = 0; j < kMaxSrc; ++j) {
        const double e = r[i] - d[j];
        a1[i][j] += fabs(e);
        a2[i][j] += e * e;
      }
  }
  double* out = tpart + ((long)b * chunks + c) * MRSTFT_TACC;
#pragma unroll
  for (int i = 0; i < kMaxSrc; ++i)
#pragma unroll
    for (int j = 0; j < kMaxSrc; ++j) {
      if (i < n && j < n) {  // uniform
        const double s1 = block_sum<kThreads / 64>(a1[i][j], red), s2 = block_sum<kThreads / 64>(a2[i][j], red);
        if (threadIdx.x == 0) {
          out[(i * kMaxSrc + j) * 2] = s1;
          out[(i * kMaxSrc + j) * 2 + 1] = s2;
        }
      }
    }
  if constexpr (FILTER) {
    const int half = ntaps / 2, span = tn + ntaps - 1;
    for (int k = threadIdx.x; k < ntaps; k += kThreads) tp[k] = (double)taps[k];
    for (int s = 0; s < 2 * n; ++s) {
      const float* src = (s < n ? xb : yb) + (long)(s < n ? s : s - n) * L;
      for (int q = threadIdx.x; q < span; q += kThreads) {
        const int t = t0 - half + q;
        sig[s][q] = (t >= 0 && t < Lb) ? src[t] : 0.f;
      }
    }
    __syncthreads();
    for (int s = 0; s < 2 * n; ++s) {
      double* dst = (s < n ? xf : yf) + ((long)b * n + (s < n ? s : s - n)) * L + t0;
      for (int t = threadIdx.x; t < tn; t += kThreads) {
        double acc = 0.0;
        for (int k = 0; k < ntaps; ++k) acc += tp[k] * (double)sig[s][t + k];
        dst[t] = acc;
      }
    }
  }
}

// ---- spectral partials ---------------------------------------------------------------------------------------
// The references and estimates [B][n][L]: the prefiltered fp64 signals xr64 / xd64 or, when those are null, the raw
// fp32 signals xr / xd; win [NFFT] the zero-padded float32 window.  Workgroup
// (w, b) takes the frame groups [w * gpw, (w + 1) * gpw) of item b, a group being 2048 / NFFT consecutive frames.
// part[(b * gridDim.x + w) * MRSTFT_SACC + a]: a = (i * 4 + j) * 3 + {0: sum (mag_d_j - mag_r_i)^2, 1: sum |log mag_r_i
// - log mag_d_j|, 2: sum |mag_r_i - mag_d_j|}, a = 48 + j: sum mag_d_j^2.
// Dynamic LDS: double2 tw[NFFT / 2] | double2 buf[2048 / NFFT frames][n][NFFT].
template <int NFFT>
__global__ __launch_bounds__(kSpecThreads) void mrstft_spec_kernel(const float* __restrict__ xr,
                                                                   const float* __restrict__ xd,
                                                                   const double* __restrict__ xr64,
                                                                   const double* __restrict__ xd64,
                                                                   const float* __restrict__ win, int n, int L,
                                                                   int hop, int F, int gpw,
                                                                   double* __restrict__ part,
                                                                   const int* __restrict__ lens) {
  constexpr int kThreads = kSpecThreads;
  static_assert(NFFT >= 32 && NFFT <= kPoints && (NFFT & (NFFT - 1)) == 0, "FFT size");
  constexpr int FPG = kPoints / NFFT, LOG = __builtin_ctz(NFFT), NB = NFFT / 2 + 1, HALF = NFFT / 2;
  constexpr int kBf = kMaxSrc * (kPoints / 2) / kThreads;  // butterflies per thread and stage at n = kMaxSrc
  extern __shared__ __attribute__((aligned(16))) double2 smem[];
  __shared__ double red[kThreads / 64];
  double2* tw = smem;
  double2* buf = smem + HALF;
  const int b = blockIdx.y, w = blockIdx.x, tid = threadIdx.x;
  const int rowL = L;  // stride of a signal's row
  if (lens) {          // the item's own length and its own partition (uniform)
    L = lens[b];
    const MrstftSplit sp = mrstft_split(NFFT, hop, 1, L);
    F = sp.F;
    gpw = sp.gpw;
    if (w >= sp.wgs) return;
  }
  for (int t = tid; t < HALF; t += kThreads) {
    double s, c;
    sincospi((double)t / HALF, &s, &c);  // exp(-2 pi i t / NFFT)
    tw[t] = make_double2(c, -s);
  }
  const long boff = (long)b * n * rowL;
  const bool wide = xr64 != nullptr;  // uniform
  const int groups = (F + FPG - 1) / FPG;
  const int g1 = min(groups, (w + 1) * gpw);
  const int nbf = n * (kPoints / 2);  // butterflies per stage

  double acc[kMaxSrc][kMaxSrc][3], den[kMaxSrc];
#pragma unroll
  for (int i = 0; i < kMaxSrc; ++i) {
    den[i] = 0.0;
#pragma unroll
    for (int j = 0; j < kMaxSrc; ++j) acc[i][j][0] = acc[i][j][1] = acc[i][j][2] = 0.0;
  }

  for (int g = w * gpw; g < g1; ++g) {
    const int f0 = g * FPG;
    __syncthreads();  // the previous group's spectra are read; tw is written
    // ---- frames: source i's windowed reference frame in .x, its estimate frame in .y
    for (int e = tid; e < kPoints; e += kThreads) {
      const int fg = e >> LOG, t = e & (NFFT - 1), f = f0 + fg;
      int idx = f * hop - HALF + t;  // f * hop <= L: no overflow
      idx = idx < 0 ? -idx : idx;
      idx = idx >= L ? 2 * (L - 1) - idx : idx;  // L > NFFT / 2: one reflection reaches [0, L)
      const bool valid = f < F;
      idx = valid ? idx : 0;
      const double wv = (double)win[t];
#pragma unroll
      for (int i = 0; i < kMaxSrc; ++i)
        if (i < n) {
          const long at = boff + (long)i * rowL + idx;
          double r = 0.0, d = 0.0;
          if (valid) {
            r = wide ? xr64[at] : (double)xr[at];
            d = wide ? xd64[at] : (double)xd[at];
          }
          buf[(fg * n + i) * NFFT + t] = make_double2(r * wv, d * wv);
        }
    }
    __syncthreads();
    // ---- Stockham radix-2, natural order in and out: a stage reads x[j], x[j + NFFT / 2] of every transform into
    // registers and, after a barrier, writes the butterfly to ((j - k) << 1) + k and that + Ns, k = j mod Ns
    for (int ls = 0; ls < LOG; ++ls) {
      const int Ns = 1 << ls;
      double2 u[kBf], v[kBf];
#pragma unroll
      for (int q = 0; q < kBf; ++q) {
        const int bf = tid + q * kThreads;
        if (bf < nbf) {
          const double2* a = buf + (bf >> (LOG - 1)) * NFFT;
          const int j = bf & (HALF - 1), k = j & (Ns - 1);
          const double2 tf = tw[k << (LOG - 1 - ls)], z = a[j + HALF];
          u[q] = a[j];
          v[q] = make_double2(tf.x * z.x - tf.y * z.y, tf.x * z.y + tf.y * z.x);
        }
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < kBf; ++q) {
        const int bf = tid + q * kThreads;
        if (bf < nbf) {
          double2* a = buf + (bf >> (LOG - 1)) * NFFT;
          const int j = bf & (HALF - 1), k = j & (Ns - 1), j0 = ((j - k) << 1) + k;
          a[j0] = make_double2(u[q].x + v[q].x, u[q].y + v[q].y);
          a[j0 + Ns] = make_double2(u[q].x - v[q].x, u[q].y - v[q].y);
        }
      }
      __syncthreads();
    }
    // ---- bins 0 .. NFFT / 2 of every valid frame: Z = R + i D with R, D the spectra of real signals, so
    // R[k] = (Z[k] + conj Z[N - k]) / 2 and D[k] = (Z[k] - conj Z[N - k]) / (2 i)
    for (int e = tid; e < FPG * NB; e += kThreads) {
      const int fg = e / NB, k = e - fg * NB;
      if (f0 + fg >= F) continue;
      double mr[kMaxSrc], md[kMaxSrc], lr[kMaxSrc], ld[kMaxSrc];
#pragma unroll
      for (int i = 0; i < kMaxSrc; ++i) {
        mr[i] = md[i] = lr[i] = ld[i] = 0.0;
        if (i < n) {
          const double2* a = buf + (fg * n + i) * NFFT;
          const double2 z1 = a[k], z2 = a[(NFFT - k) & (NFFT - 1)];
          const double rx = 0.5 * (z1.x + z2.x), ry = 0.5 * (z1.y - z2.y);
          const double dx = 0.5 * (z1.y + z2.y), dy = 0.5 * (z2.x - z1.x);
          const double pr = fmax(rx * rx + ry * ry, 1e-8), pd = fmax(dx * dx + dy * dy, 1e-8);
          mr[i] = sqrt(pr);
          md[i] = sqrt(pd);
          lr[i] = 0.5 * log(pr);
          ld[i] = 0.5 * log(pd);
          den[i] += pd;
        }
      }
#pragma unroll
      for (int i = 0; i < kMaxSrc; ++i)
#pragma unroll
        for (int j = 0; j < kMaxSrc; ++j) {
          const double dm = md[j] - mr[i];
          acc[i][j][0] += dm * dm;
          acc[i][j][1] += fabs(lr[i] - ld[j]);
          acc[i][j][2] += fabs(dm);
        }
    }
  }

  double* out = part + ((long)b * gridDim.x + w) * MRSTFT_SACC;
#pragma unroll
  for (int i = 0; i < kMaxSrc; ++i) {
    if (i >= n) continue;  // uniform
#pragma unroll
    for (int j = 0; j < kMaxSrc; ++j) {
      if (j >= n) continue;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const double s = block_sum<kThreads / 64>(acc[i][j][q], red);
        if (tid == 0) out[(i * kMaxSrc + j) * 3 + q] = s;
      }
    }
    const double s = block_sum<kThreads / 64>(den[i], red);
    if (tid == 0) out[kMaxSrc * kMaxSrc * 3 + i] = s;
  }
}

// ---- finish --------------------------------------------------------------------------------------------------
// One thread per (table row, b, i, j); rows 0 .. R-1 are the resolutions, row R the time-domain losses.
//   sc[r][b][i][j] = sqrt(sum (mag_d_j - mag_r_i)^2) / sqrt(sum mag_d_j^2)
//   log_mag / lin_mag [r][b][i][j] = sum / (bins * frames);  l1 / l2 [b][i][j] = sum / L
__global__ __launch_bounds__(kThreads) void mrstft_finish_kernel(MrstftPlan plan, const double* __restrict__ part,
                                                                 const double* __restrict__ tpart, int B, int n, int L,
                                                                 int tchunks, double* __restrict__ sc,
                                                                 double* __restrict__ lg, double* __restrict__ lin,
                                                                 double* __restrict__ l1, double* __restrict__ l2,
                                                                 const int* __restrict__ lens) {
  const long per = (long)B * n * n, e = (long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= per * (plan.R + 1)) return;
  const int r = (int)(e / per);
  const long o = e - (long)r * per;
  const int j = (int)(o % n), i = (int)((o / n) % n), b = (int)(o / ((long)n * n));
  const int Lb = lens ? lens[b] : L;
  if (r == plan.R) {
    double s1 = 0.0, s2 = 0.0;
    const int own = lens ? mrstft_time_chunks(Lb) : tchunks;  // tchunks stays the stride
    for (int c = 0; c < own; ++c) {
      const double* p = tpart + ((long)b * tchunks + c) * MRSTFT_TACC + (i * kMaxSrc + j) * 2;
      s1 += p[0];
      s2 += p[1];
    }
    l1[o] = s1 / Lb;
    l2[o] = s2 / Lb;
    return;
  }
  const int W = plan.wgs[r];  // the stride; a ragged item sums its own workgroups
  const MrstftSplit sp = lens ? mrstft_split(plan.fft[r], plan.hop[r], 1, Lb) : MrstftSplit{plan.frames[r], 0, W};
  const double* base = part + plan.off[r] + (long)b * W * MRSTFT_SACC;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, sd = 0.0;
  for (int w = 0; w < sp.wgs; ++w) {
    const double* p = base + (long)w * MRSTFT_SACC;
    s0 += p[(i * kMaxSrc + j) * 3];
    s1 += p[(i * kMaxSrc + j) * 3 + 1];
    s2 += p[(i * kMaxSrc + j) * 3 + 2];
    sd += p[kMaxSrc * kMaxSrc * 3 + j];
  }
  const double cnt = (double)(plan.fft[r] / 2 + 1) * sp.F;
  sc[(long)r * per + o] = sqrt(s0) / sqrt(sd);
  lg[(long)r * per + o] = s1 / cnt;
  lin[(long)r * per + o] = s2 / cnt;
}

template <int NFFT>
void launch_spec(const float* xr, const float* xd, const double* xr64, const double* xd64, const float* win, int B,
                 int n, int L, int hop, int F, int wgs, int gpw, double* part, hipStream_t st, const int* lens) {
  const size_t smem = ((size_t)NFFT / 2 + (size_t)n * kPoints) * sizeof(double2);
  dsn_allow_lds<mrstft_spec_kernel<NFFT>>((int)((NFFT / 2 + kMaxSrc * kPoints) * sizeof(double2)));
  hipLaunchKernelGGL((mrstft_spec_kernel<NFFT>), dim3(wgs, B), dim3(kSpecThreads), smem, st, xr, xd, xr64, xd64, win, n,
                     L, hop, F, gpw, part, lens);
}

}  // namespace

bool mrstft_fft_ok(int fft) { return fft >= 32 && fft <= kPoints && (fft & (fft - 1)) == 0; }

void mrstft_plan_resolution(MrstftPlan* plan, int r, int fft, int hop, int B, int L, const int* lens) {
  static_assert(kPoints == 2048, "mrstft_split groups 2048 / fft frames");
  MrstftSplit sp = mrstft_split(fft, hop, B, L);
  if (lens) {
    sp = {0, 0, 0};
    for (int b = 0; b < B; ++b) sp.wgs = std::max(sp.wgs, mrstft_split(fft, hop, 1, lens[b]).wgs);
  }
  plan->fft[r] = fft;
  plan->hop[r] = hop;
  plan->frames[r] = sp.F;
  plan->gpw[r] = sp.gpw;
  plan->wgs[r] = sp.wgs;
  plan->off[r] = r == 0 ? 0 : plan->off[r - 1] + (long)B * plan->wgs[r - 1] * MRSTFT_SACC;
}

void launch_mrstft_time(const float* x, const float* y, int B, int n, int L, const float* taps, int ntaps, double* xf,
                        double* yf, double* tpart, hipStream_t st, const int* lens) {
  const dim3 grid(mrstft_time_chunks(L), B);
  if (taps)
    hipLaunchKernelGGL(mrstft_time_kernel<true>, grid, dim3(kThreads), 0, st, x, y, n, L, taps, ntaps, xf, yf, tpart, lens);
  else
    hipLaunchKernelGGL(mrstft_time_kernel<false>, grid, dim3(kThreads), 0, st, x, y, n, L, taps, ntaps, xf, yf, tpart, lens);
}

void launch_mrstft_spec(const MrstftPlan& plan, int r, const float* xr, const float* xd, const double* xr64,
                        const double* xd64, const float* win, int B, int n, int L, double* part, hipStream_t st,
                        const int* lens) {
  double* p = part + plan.off[r];
  const int hop = plan.hop[r], F = plan.frames[r], wgs = plan.wgs[r], gpw = plan.gpw[r];
  switch (plan.fft[r]) {
    case 32: launch_spec<32>(xr, xd, xr64, xd64, win, B, n, L, hop, F, wgs, gpw, p, st, lens); break;
    case 64: launch_spec<64>(xr, xd, xr64, xd64, win, B, n, L, hop, F, wgs, gpw, p, st, lens); break;
    case 128: launch_spec<128>(xr, xd, xr64, xd64, win, B, n, L, hop, F, wgs, gpw, p, st, lens); break;
    case 256: launch_spec<256>(xr, xd, xr64, xd64, win, B, n, L, hop, F, wgs, gpw, p, st, lens); break;
    case 512: launch_spec<512>(xr, xd, xr64, xd64, win, B, n, L, hop, F, wgs, gpw, p, st, lens); break;
    case 1024: launch_spec<1024>(xr, xd, xr64, xd64, win, B, n, L, hop, F, wgs, gpw, p, st, lens); break;
    default: launch_spec<2048>(xr, xd, xr64, xd64, win, B, n, L, hop, F, wgs, gpw, p, st, lens); break;
  }
}

void launch_mrstft_finish(const MrstftPlan& plan, const double* part, const double* tpart, int B, int n, int L,
                          double* sc, double* lg, double* lin, double* l1, double* l2, hipStream_t st, const int* lens) {
  const long total = (long)B * n * n * (plan.R + 1);
  hipLaunchKernelGGL(mrstft_finish_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                     plan, part, tpart, B, n, L, mrstft_time_chunks(L), sc, lg, lin, l1, l2, lens);
}
