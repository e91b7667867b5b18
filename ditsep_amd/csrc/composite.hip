// The objective measures behind the Hu & Loizou (2008) composite scores CSIG / CBAK / COVL: the log-likelihood
// ratio of the LPC models (LLR, Quackenbush et al.), the weighted spectral slope (WSS, Klatt 1982) and the
// segmental SNR, as the reference's src/evaluate/evaluate_covl.py defines them (restated in float64 in
// tests/composite_restatement.py, pinned to the reference's own functions by tests/golden/composite.npz).
// Items are the (b, source) pairs of a [B, n, L] batch; ref is the clean signal, est the estimate.  Frames are
// `win` = 30 ms long, `hop` = win / 4 apart, under the window 0.5 (1 - cos(2 pi k / (win + 1))), k = 1 .. win.
// Stages:
//   condition  per item, for the segmental SNR only: the means, the scale max|ref - mean| / max|est - mean| and the
//              overall SNR of the conditioned signals; LLR and WSS read the raw signals
//   frame      one wave per frame: segmental SNR of the conditioned frames; autocorrelation lags 0 .. P of both
//              windowed frames in fp64, Levinson-Durbin, LLR; zero-padded FFT of both frames in LDS (fp32
//              butterflies), 25 Gaussian critical-band energies (fp64 sums over a sparse table built by the host),
//              slopes, nearest-peak search, Klatt weights, WSS
//   finish     per item and measure: the mean of the k smallest per-frame values (LLR, WSS; k from the host) chosen
//              by rank over LDS tiles, any frame count; the plain mean (segmental SNR)
// Every reduction has a fixed order (no atomics): two calls on the same input give bit-identical results.
// Ragged batches (dsn_composite_ragged): rows stay Lmax apart and batch entry b = item / n brings its own sample
// count lens[b], frame count Fb[b] and trimmed count kb[b], all from the host (null arrays: every item is full
// length).  Buffers and grids are sized by the longest item; a workgroup wholly past an item's frames leaves at once,
// a wave past them inside a live workgroup still walks every barrier with zeros.  Nothing past lens[b] is read, and
// every sum runs in the order the item's own length fixes: an item gets the same bits in a padded batch as alone.
#include "kernels.h"

namespace {

constexpr int kBands = COMPOSITE_BANDS;
constexpr int kCondThreads = 1024;
constexpr int kTile = 1024;  // frames per LDS tile of the rank selection

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// cond[item][COMPOSITE_COND]: mean(ref), mean(est), max|ref - mean| / max|est - mean|, overall SNR in dB.
// A constant (or all-zero) estimate has max|est - mean| = 0: the scale is inf (or NaN), and so are the results.
__global__ __launch_bounds__(kCondThreads) void composite_condition_kernel(const float* __restrict__ ref,
                                                                            const float* __restrict__ est,
                                                                            const int* __restrict__ ymap, int L,
                                                                            const int* __restrict__ lens, int n,
                                                                            double* __restrict__ cond) {
  constexpr int kWaves = kCondThreads / 64;
  __shared__ double red[6][kWaves];
  __shared__ double par[3];
  const int item = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* r = ref + (long)item * L;
  const float* e = est + (long)(ymap ? ymap[item] : item) * L;
  const int len = lens ? lens[item / n] : L;  // rows are L apart; the item's own samples
  double sr = 0.0, se = 0.0, xr = -INFINITY, xe = -INFINITY, nr = -INFINITY, ne = -INFINITY;  // n*: max of -x
  for (int t = threadIdx.x; t < len; t += kCondThreads) {
    const double a = r[t], b = e[t];
    sr += a;
    se += b;
    xr = fmax(xr, a);
    nr = fmax(nr, -a);
    xe = fmax(xe, b);
    ne = fmax(ne, -b);
  }
  sr = wave_sum(sr);
  se = wave_sum(se);
  xr = wave_max(xr);
  nr = wave_max(nr);
  xe = wave_max(xe);
  ne = wave_max(ne);
  if (lane == 0) {
    red[0][wave] = sr;
    red[1][wave] = se;
    red[2][wave] = xr;
    red[3][wave] = nr;
    red[4][wave] = xe;
    red[5][wave] = ne;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s0 = 0.0, s1 = 0.0, m2 = -INFINITY, m3 = -INFINITY, m4 = -INFINITY, m5 = -INFINITY;
    for (int w = 0; w < kWaves; ++w) {
      s0 += red[0][w];
      s1 += red[1][w];
      m2 = fmax(m2, red[2][w]);
      m3 = fmax(m3, red[3][w]);
      m4 = fmax(m4, red[4][w]);
      m5 = fmax(m5, red[5][w]);
    }
    const double mr = s0 / len, me = s1 / len;
    // max |x - mean| is reached at the largest or the smallest sample (rounding is monotone)
    const double ar = fmax(m2 - mr, m3 + mr), ae = fmax(m4 - me, m5 + me);
    par[0] = mr;
    par[1] = me;
    par[2] = ar / ae;
  }
  __syncthreads();
  const double mr = par[0], me = par[1], sc = par[2];
  double S = 0.0, N = 0.0;
  for (int t = threadIdx.x; t < len; t += kCondThreads) {
    const double c = (double)r[t] - mr, p = ((double)e[t] - me) * sc, d = c - p;
    S += c * c;
    N += d * d;
  }
  S = wave_sum(S);
  N = wave_sum(N);
  __syncthreads();  // red is reused
  if (lane == 0) {
    red[0][wave] = S;
    red[1][wave] = N;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s0 = 0.0, s1 = 0.0;
    for (int w = 0; w < kWaves; ++w) {
      s0 += red[0][w];
      s1 += red[1][w];
    }
    double* o = cond + (long)item * COMPOSITE_COND;
    o[0] = mr;
    o[1] = me;
    o[2] = sc;
    o[3] = 10.0 * log10(s0 / (s1 + 1e-19));
  }
}

// LPC coefficients a[0 .. P) of the autocorrelation lags R[0 .. P] by Levinson-Durbin (the prediction polynomial is
// 1 - sum a_j z^-(j+1)), the prediction error floored at 1e-15 in the division as the reference does
template <int P>
__device__ inline void levinson(const double (&R)[P + 1], double (&a)[P]) {
  double E = R[0];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < i; ++j) s += a[j] * R[i - j];
    const double rc = (R[i + 1] - s) / fmax(1e-15, E);
    double prev[P];
#pragma unroll
    for (int j = 0; j < i; ++j) prev[j] = a[j];
#pragma unroll
    for (int j = 0; j < i; ++j) a[j] = prev[j] - rc * prev[i - 1 - j];
    a[i] = rc;
    E = (1.0 - rc * rc) * E;
  }
}

// [1, -a] R [1, -a]^T with R the Toeplitz matrix of the lags
template <int P>
__device__ inline double lpc_form(const double (&a)[P], const double (&R)[P + 1]) {
  double c[P + 1];
  c[0] = 1.0;
#pragma unroll
  for (int j = 0; j < P; ++j) c[j + 1] = -a[j];
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i <= P; ++i) {
    double row = 0.0;
#pragma unroll
    for (int j = 0; j <= P; ++j) row += c[j] * R[i > j ? i - j : j - i];
    acc += c[i] * row;
  }
  return acc;
}

// radix-2 decimation in time on bit-reversed input, NFFT / 2 butterflies per stage, one wave per buffer; every wave
// of the workgroup runs it together (the barriers are workgroup-wide)
template <int NFFT>
__device__ inline void lds_fft(float2* a, const float2* tw, int lane) {
  for (int half = 1; half < NFFT; half <<= 1) {
    const int tstep = (NFFT / 2) / half;
#pragma unroll
    for (int j = 0; j < NFFT / 128; ++j) {
      const int b = lane + 64 * j;
      const int jj = b & (half - 1);
      const int i0 = ((b - jj) << 1) + jj, i1 = i0 + half;
      const float2 w = tw[jj * tstep], u = a[i0], z = a[i1];
      const float2 t = make_float2(w.x * z.x - w.y * z.y, w.x * z.y + w.y * z.x);
      a[i0] = make_float2(u.x + t.x, u.y + t.y);
      a[i1] = make_float2(u.x - t.x, u.y - t.y);
    }
    __syncthreads();
  }
}

// the band energy the slope at band n leads to: to the right while the slope stays positive, to the left while it
// does not, with the reference's end points (E[n - 1] after the last positive slope, E[n + 1] before the first)
__device__ inline double nearest_peak(const double* E, int i) {
  int n = i;
  if (E[i + 1] - E[i] > 0.0) {
    while (n < kBands - 1 && E[n + 1] - E[n] > 0.0) ++n;
    return E[n - 1];
  }
  while (n >= 0 && E[n + 1] - E[n] <= 0.0) --n;
  return E[n + 1];
}

// Frame f of item blockIdx.y: llr / wss / ssnr [item][F].  One wave per frame, four frames per workgroup.
// W = window length, NFFT = 2^ceil(log2(2 W)), P = LPC order; 2 (W + P) <= NFFT, so that both windowed fp64 frames
// (each followed by P zeros) fit the wave's FFT buffer.
template <int W, int NFFT, int P>
__global__ __launch_bounds__(256) void composite_frame_kernel(const float* __restrict__ ref,
                                                              const float* __restrict__ est,
                                                              const int* __restrict__ ymap, int L, int F,
                                                              const int* __restrict__ Fb, int n,
                                                              const double* __restrict__ win, CompositeBands bands,
                                                              const double* __restrict__ bweights,
                                                              const double* __restrict__ cond,
                                                              double* __restrict__ llr, double* __restrict__ wss,
                                                              double* __restrict__ ssnr) {
  static_assert(2 * (W + P) <= NFFT && NFFT % 128 == 0 && W % 4 == 0, "frame geometry");
  constexpr int kHop = W / 4, WP = W + P, NJ = (W + 63) / 64, LOG = __builtin_ctz(NFFT);
  __shared__ double raw[4][NFFT];  // per wave: the fp64 frames, then the float2 FFT buffer
  __shared__ float2 tw[NFFT / 2];
  __shared__ double wn[W];
  __shared__ double edb[4][2][kBands];
  const int item = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int Fi = Fb ? Fb[item / n] : F;  // the item's frames; F stays the row stride of llr / wss / ssnr
  if ((int)blockIdx.x * 4 >= Fi) return;  // uniform over the workgroup
  for (int t = threadIdx.x; t < NFFT / 2; t += 256) {
    double s, c;
    sincospi((double)t / (NFFT / 2), &s, &c);  // exp(-2 pi i t / NFFT)
    tw[t] = make_float2((float)c, (float)-s);
  }
  for (int t = threadIdx.x; t < W; t += 256) wn[t] = win[t];
  const int f = blockIdx.x * 4 + wave;
  const bool valid = f < Fi;
  const double* cd = cond + (long)item * COMPOSITE_COND;
  const double mr = cd[0], me = cd[1], sc = cd[2];
  const float* r = ref + (long)item * L + (long)(valid ? f : 0) * kHop;
  const float* e = est + (long)(ymap ? ymap[item] : item) * L + (long)(valid ? f : 0) * kHop;
  double* fr = raw[wave];
  double* fe = fr + WP;
  __syncthreads();

  // ---- load, window; segmental SNR of the conditioned frames
  float xr[NJ], xe[NJ];
  double sig = 0.0, noi = 0.0;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int t = lane + 64 * j;
    xr[j] = xe[j] = 0.f;
    if (t < W) {
      const double w = wn[t];
      const double a = valid ? (double)r[t] : 0.0, b = valid ? (double)e[t] : 0.0;
      const double wa = w * a, wb = w * b;
      fr[t] = wa;
      fe[t] = wb;
      xr[j] = (float)wa;
      xe[j] = (float)wb;
      const double c = w * (a - mr), d = c - w * ((b - me) * sc);
      sig += c * c;
      noi += d * d;
    }
  }
  if (lane < P) fr[W + lane] = fe[W + lane] = 0.0;
  sig = wave_sum(sig);
  noi = wave_sum(noi);
  if (valid && lane == 0) {
    double v = 10.0 * log10(sig / (noi + 1e-10) + 1e-10);
    v = v < -10.0 ? -10.0 : v;  // a NaN stays a NaN
    v = v > 35.0 ? 35.0 : v;
    ssnr[(long)item * F + f] = v;
  }
  __syncthreads();

  // ---- LLR
  {
    double Rr[P + 1], Re[P + 1];
#pragma unroll
    for (int k = 0; k <= P; ++k) Rr[k] = Re[k] = 0.0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int t = lane + 64 * j;
      if (t < W) {
        const double a = fr[t], b = fe[t];
#pragma unroll
        for (int k = 0; k <= P; ++k) {
          Rr[k] += a * fr[t + k];
          Re[k] += b * fe[t + k];
        }
      }
    }
#pragma unroll
    for (int k = 0; k <= P; ++k) {
      Rr[k] = wave_sum(Rr[k]);
      Re[k] = wave_sum(Re[k]);
    }
    double ar[P], ae[P];
    levinson<P>(Rr, ar);
    levinson<P>(Re, ae);
    const double num = fmax(1e-10, lpc_form<P>(ae, Rr)), den = fmax(1e-10, lpc_form<P>(ar, Rr));
    double v = log(num / den);
    if (isnan(v)) v = 0.0;  // numpy.nan_to_num
    else if (isinf(v)) v = v > 0.0 ? 1.7976931348623157e308 : -1.7976931348623157e308;
    if (valid && lane == 0) llr[(long)item * F + f] = v;
  }
  __syncthreads();  // the frames are read; their storage becomes the FFT buffer

  // ---- WSS: band energies in dB of both spectra
  float2* a = reinterpret_cast<float2*>(raw[wave]);
  for (int sgn = 0; sgn < 2; ++sgn) {
#pragma unroll
    for (int j = 0; j < NFFT / 64; ++j) {
      const int p = lane + 64 * j;
      constexpr int jc = NJ - 1;  // xr / xe are zero beyond the window already; beyond NJ chunks comes the padding
      const float v = j < NJ ? (sgn == 0 ? xr[j < NJ ? j : jc] : xe[j < NJ ? j : jc]) : 0.f;
      a[__brev((unsigned)p) >> (32 - LOG)] = make_float2(v, 0.f);
    }
    __syncthreads();
    lds_fft<NFFT>(a, tw, lane);
    if (lane < kBands) {
      const double* bw = bweights + bands.off[lane];
      const int s0 = bands.start[lane], n = bands.len[lane];
      double acc = 0.0;
      for (int i = 0; i < n; ++i) {
        const float2 z = a[s0 + i];
        acc += ((double)z.x * z.x + (double)z.y * z.y) * bw[i];
      }
      edb[wave][sgn][lane] = 10.0 * log10(fmax(acc, 1e-10));
    }
    __syncthreads();  // the buffer is rewritten for est; edb is read below
  }

  // ---- slopes, nearest peaks, Klatt weights (Kmax = 20, Klocmax = 1), normalised weighted slope distance
  const double* Ec = edb[wave][0];
  const double* Ep = edb[wave][1];
  double num = 0.0, den = 0.0;
  if (lane < kBands - 1) {
    double mc = Ec[0], mp = Ep[0];
    for (int i = 1; i < kBands; ++i) {
      mc = fmax(mc, Ec[i]);
      mp = fmax(mp, Ep[i]);
    }
    const double sc_ = Ec[lane + 1] - Ec[lane], sp_ = Ep[lane + 1] - Ep[lane];
    const double wc = (20.0 / (20.0 + mc - Ec[lane])) * (1.0 / (1.0 + nearest_peak(Ec, lane) - Ec[lane]));
    const double wp = (20.0 / (20.0 + mp - Ep[lane])) * (1.0 / (1.0 + nearest_peak(Ep, lane) - Ep[lane]));
    den = (wc + wp) / 2.0;
    num = den * (sc_ - sp_) * (sc_ - sp_);
  }
  num = wave_sum(num);
  den = wave_sum(den);
  if (valid && lane == 0) wss[(long)item * F + f] = num / den;
}

// out[item][measure]: measure 0 / 1 = mean of the k smallest per-frame LLR / WSS values, 2 = mean segmental SNR.
// Frame i is among the k smallest when fewer than k frames precede it in (value, index) order.
__global__ __launch_bounds__(256) void composite_finish_kernel(const double* __restrict__ llr,
                                                               const double* __restrict__ wss,
                                                               const double* __restrict__ ssnr, int F, int k,
                                                               const int* __restrict__ Fb,
                                                               const int* __restrict__ kb, int n,
                                                               double* __restrict__ out) {
  __shared__ double tile[kTile];
  __shared__ double red[4];
  const int item = blockIdx.x, m = blockIdx.y;  // m is uniform over the workgroup
  const double* v = (m == 0 ? llr : m == 1 ? wss : ssnr) + (long)item * F;
  if (Fb) {  // the item's own frame and trimmed counts; the rows stay F apart
    F = Fb[item / n];
    k = kb[item / n];
  }
  double acc = 0.0;
  if (m == 2) {
    for (int i = threadIdx.x; i < F; i += 256) acc += v[i];
  } else {
    for (int i0 = 0; i0 < F; i0 += 256) {
      const int i = i0 + threadIdx.x;
      const double vi = i < F ? v[i] : 0.0;
      int rank = 0;
      for (int j0 = 0; j0 < F; j0 += kTile) {
        const int jn = min(kTile, F - j0);
        __syncthreads();
        for (int q = threadIdx.x; q < jn; q += 256) tile[q] = v[j0 + q];
        __syncthreads();
        for (int j = 0; j < jn; ++j) {
          const double x = tile[j];
          rank += (x < vi || (x == vi && j0 + j < i)) ? 1 : 0;
        }
      }
      if (i < F && rank < k) acc += vi;
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[(long)item * 3 + m] = ((red[0] + red[1]) + (red[2] + red[3])) / (m == 2 ? F : k);
}

}  // namespace

bool composite_shape(int fs, CompositeShape* s) {
  // instantiated signal rates: window = round(30 fs / 1000), hop = window / 4, FFT = 2^ceil(log2(2 window)),
  // LPC order 16 at fs >= 10 kHz, else 10
  if (fs == 16000) *s = CompositeShape{480, 120, 1024, 16};
  else if (fs == 8000) *s = CompositeShape{240, 60, 512, 10};
  else return false;
  return true;
}

void launch_composite(int fs, const float* ref, const float* est, const int* ymap, int items, int L, int F, int k,
                      const int* lens, const int* Fb, const int* kb, int n, const double* win,
                      const CompositeBands& bands, const double* bweights, double* cond,
                      double* llr, double* wss, double* ssnr, double* out, hipStream_t st) {
  hipLaunchKernelGGL(composite_condition_kernel, dim3(items), dim3(kCondThreads), 0, st, ref, est, ymap, L, lens, n,
                     cond);
  const dim3 grid((F + 3) / 4, items);
  if (fs == 16000)
    hipLaunchKernelGGL((composite_frame_kernel<480, 1024, 16>), grid, dim3(256), 0, st, ref, est, ymap, L, F, Fb, n,
                       win, bands, bweights, cond, llr, wss, ssnr);
  else
    hipLaunchKernelGGL((composite_frame_kernel<240, 512, 10>), grid, dim3(256), 0, st, ref, est, ymap, L, F, Fb, n,
                       win, bands, bweights, cond, llr, wss, ssnr);
  hipLaunchKernelGGL(composite_finish_kernel, dim3(items, 3), dim3(256), 0, st, llr, wss, ssnr, F, k, Fb, kb,
                     n, out);
}
