// STOI / extended STOI (Taal et al. 2011, Jensen & Taal 2016) as pystoi.stoi(x, y, fs, extended) defines it
// (restated in float64 in tests/stoi_restatement.py; parity with the pystoi package unpinned).  Items are the
// (b, source) pairs of a [B, n, L] batch; x is the clean reference, y the estimate.  Stages:
//   resample   polyphase FIR to 10 kHz (scipy.signal.resample_poly alignment), fp64 accumulation
//   energy     20 log10(|w * frame| + eps) of every 256-sample frame of x that fits (hop 128)
//   mask       per item: frames within 40 dB of the loudest kept, compacted frame list and its count K
//   envelope   overlap-add of the kept frames as a gather (at most two frames per sample), windowed 512-point FFT
//              in LDS, one-third-octave band magnitudes: tob [item][x|y][15][frame], K - 1 STFT frames
//   segment    per 30-frame segment: the STOI band correlations or the ESTOI row/column-normalised inner product
//   finish     per item: fixed-order fp64 sum over the segments; 1e-5 when fewer than 30 STFT frames remain
// Every reduction has a fixed order (no atomics): two calls on the same input give bit-identical scores.
// Ragged batches (dsn_stoi_ragged): rows stay Lmax apart and batch entry b = item / n brings its own sample count
// lens[b] and frame count Fb[b] (null arrays: every item is full length).  The resampler stops its taps at
// lens[b] - 1, energy and mask run over Fb[b] frames, and the later stages follow the kept-frame list, so nothing
// past an item's end is read; buffers and grids are sized by the longest item.  Every sum runs in the order the
// item's own length fixes: an item scores the same bits in a padded batch as alone.
#include "kernels.h"

namespace {

constexpr int kFrame = 256, kHop = 128, kFft = 512, kBands = 15, kSeg = 30;
constexpr double kEps = 2.220446049250313e-16;  // float64 machine epsilon, pystoi's EPS
constexpr double kDynRange = 40.0;

// floor / ceil division for a possibly negative numerator and a positive divisor
__device__ inline long floordiv(long a, long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// numpy.hanning(258)[1:-1]: the 256-point Hann window without its zero end points
__device__ inline float hann(int t) { return (float)(0.5 - 0.5 * cos(2.0 * M_PI * (t + 1) / 257.0)); }

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// out[sig][item][i], sig 0 = ref, 1 = est (est row ymap[item], or item when ymap is null).
// y[i] = sum_m x[m] h[c - m up], c = (i + n_pre_remove) down - n_pre_pad, 0 <= c - m up < ntaps: scipy's
// upfirdn on the zero-padded filter, the pre-padding removed.
// Rows are n_in apart; an item of batch entry b = item / n holds lens[b] samples (n_in when lens is null) and gives
// ceil(lens[b] up / down) outputs of its n_out-long output row: no tap reaches past lens[b] - 1.
__global__ __launch_bounds__(256) void stoi_resample_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                            const int* __restrict__ ymap, int n_in,
                                                            const int* __restrict__ lens, int n,
                                                            const double* __restrict__ taps, int ntaps, int up,
                                                            int down, int n_pre_pad, int n_pre_remove, int n_out,
                                                            int items, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int item = blockIdx.y, sig = blockIdx.z;
  const int len = lens ? lens[item / n] : n_in;
  if (i >= (lens ? (int)(((long)len * up + down - 1) / down) : n_out)) return;
  const float* x = sig == 0 ? ref + (long)item * n_in : est + (long)(ymap ? ymap[item] : item) * n_in;
  const long c = (long)(i + n_pre_remove) * down - n_pre_pad;
  const long mhi = min(floordiv(c, up), (long)len - 1);
  const long mlo = max(-floordiv(-(c - ntaps + 1), up), 0L);
  double acc = 0.0;
  for (long m = mlo; m <= mhi; ++m) acc += (double)x[m] * taps[c - m * up];
  out[((long)sig * items + item) * n_out + i] = (float)acc;
}

// Frames of an item: Fb[item / n] when the batch is ragged (Fb non-null), else F.  F stays the row stride of the
// per-frame buffers.
__device__ inline int item_frames(const int* __restrict__ Fb, int n, int item, int F) {
  return Fb ? Fb[item / n] : F;
}

// en[item][f] = 20 log10(|w * x[128 f : 128 f + 256]| + eps); one wave per frame
__global__ __launch_bounds__(256) void stoi_energy_kernel(const float* __restrict__ xs, long stride, int F,
                                                          const int* __restrict__ Fb, int n,
                                                          double* __restrict__ en) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= item_frames(Fb, n, blockIdx.y, F)) return;
  const float* x = xs + (long)blockIdx.y * stride + (long)f * kHop;
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int t = lane + 64 * j;
    const double v = (double)hann(t) * (double)x[t];
    acc += v * v;
  }
  acc = wave_sum(acc);
  if (lane == 0) en[(long)blockIdx.y * F + f] = 20.0 * log10(sqrt(acc) + kEps);
}

// per item: keep frame f iff max - 40 - en[f] < 0; idx[item][0..K) = kept frame indices in order, Kc[item] = K
// (K = 0 for an item without a frame)
__global__ __launch_bounds__(256) void stoi_mask_kernel(const double* __restrict__ en, int F,
                                                        const int* __restrict__ Fb, int n, int* __restrict__ idx,
                                                        int* __restrict__ Kc) {
  __shared__ double wmax[4];
  __shared__ int wcnt[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double* e = en + (long)blockIdx.x * F;
  const int Fi = item_frames(Fb, n, blockIdx.x, F);  // uniform over the workgroup
  double mx = -INFINITY;
  for (int f = threadIdx.x; f < Fi; f += 256) mx = fmax(mx, e[f]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) wmax[wave] = mx;
  __syncthreads();
  mx = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
  int* out = idx + (long)blockIdx.x * F;
  int base = 0;
  for (int f0 = 0; f0 < Fi; f0 += 256) {
    const int f = f0 + threadIdx.x;
    const bool keep = f < Fi && (mx - kDynRange - e[f]) < 0.0;
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += wcnt[w];
    if (keep) out[off + __popcll(bal & ((1ull << lane) - 1ull))] = f;
    base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) Kc[blockIdx.x] = base;
}

__device__ inline int brev9(int v) { return (int)(__brev((unsigned)v) >> 23); }

// STFT frame k (0 <= k < K - 1) of the silence-removed x and y, band magnitudes into
// tob[((item * 2 + sig) * 15 + band) * Fs + k].  One wave per frame, four frames per workgroup.
__global__ __launch_bounds__(256) void stoi_envelope_kernel(const float* __restrict__ xs,
                                                            const float* __restrict__ ys, long stride,
                                                            const int* __restrict__ ymap, int F,
                                                            const int* __restrict__ idx, const int* __restrict__ Kc,
                                                            StoiBands bands, int Fs, double* __restrict__ tob) {
  __shared__ float2 buf[4][kFft];
  __shared__ float2 tw[kFft / 2];
  __shared__ float win[kFrame];
  const int item = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  {
    const int t = threadIdx.x;
    double s, c;
    sincospi((double)t / (kFft / 2), &s, &c);  // exp(-2 pi i t / 512)
    tw[t] = make_float2((float)c, (float)-s);
    win[t] = hann(t);
  }
  const int Fr = Kc[item] - 1;
  const int k0 = blockIdx.x * 4;
  if (k0 >= Fr) return;  // uniform over the workgroup
  const int k = k0 + wave;
  const bool valid = k < Fr;
  const int* kept = idx + (long)item * F;
  __syncthreads();
  float2* a = buf[wave];
  for (int sig = 0; sig < 2; ++sig) {
    const float* s = sig == 0 ? xs + (long)item * stride : ys + (long)(ymap ? ymap[item] : item) * stride;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = lane + 64 * j;
      float v = 0.f;
      if (valid) {
        // overlap-added sample 128 k + p = 128 q + r: kept frame q at offset r plus kept frame q - 1 at r + 128
        const int q = k + (p >> 7), r = p & 127;
        v = win[r] * s[(long)kept[q] * kHop + r];
        if (q >= 1) v += win[r + kHop] * s[(long)kept[q - 1] * kHop + r + kHop];
        v *= win[p];
      }
      a[brev9(p)] = make_float2(v, 0.f);
      a[brev9(p + kFrame)] = make_float2(0.f, 0.f);
    }
    __syncthreads();
    // radix-2 decimation in time, 256 butterflies per stage, four per lane
    for (int half = 1; half < kFft; half <<= 1) {
      const int tstep = (kFft / 2) / half;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
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
    if (valid && lane < kBands) {
      double acc = 0.0;
      for (int f = bands.lo[lane]; f < bands.hi[lane]; ++f) {
        const float2 z = a[f];
        acc += (double)z.x * z.x + (double)z.y * z.y;
      }
      tob[(((long)item * 2 + sig) * kBands + lane) * Fs + k] = sqrt(acc);
    }
    __syncthreads();  // the buffer is rewritten for y
  }
}

// part[item][j]: segment j (STFT frames j .. j + 29) -- STOI: sum over bands of the clipped-estimate correlation;
// ESTOI: inner product of the row- then column-normalised segments over 30.  One thread per segment.
__global__ __launch_bounds__(64) void stoi_segment_kernel(const double* __restrict__ tob, int Fs,
                                                          const int* __restrict__ Kc, int extended, int Jmax,
                                                          double* __restrict__ part) {
  const int item = blockIdx.y;
  const int J = Kc[item] - 1 - (kSeg - 1);
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= J) return;
  const double* X = tob + (long)item * 2 * kBands * Fs + j;
  const double* Y = X + (long)kBands * Fs;
  double acc = 0.0;
  if (!extended) {
    const double clip = 1.0 + pow(10.0, 15.0 / 20.0);  // 1 + 10^(-BETA/20)
    for (int r = 0; r < kBands; ++r) {
      const double* x = X + (long)r * Fs;
      const double* y = Y + (long)r * Fs;
      double sxx = 0.0, syy = 0.0;
      for (int c = 0; c < kSeg; ++c) {
        sxx += x[c] * x[c];
        syy += y[c] * y[c];
      }
      const double alpha = sqrt(sxx) / (sqrt(syy) + kEps);
      double mx = 0.0, my = 0.0;
      for (int c = 0; c < kSeg; ++c) {
        mx += x[c];
        my += fmin(y[c] * alpha, x[c] * clip);
      }
      mx /= kSeg;
      my /= kSeg;
      double dxx = 0.0, dyy = 0.0, dxy = 0.0;
      for (int c = 0; c < kSeg; ++c) {
        const double dx = x[c] - mx, dy = fmin(y[c] * alpha, x[c] * clip) - my;
        dxx += dx * dx;
        dyy += dy * dy;
        dxy += dx * dy;
      }
      acc += dxy / ((sqrt(dxx) + kEps) * (sqrt(dyy) + kEps));
    }
  } else {
    // pystoi adds eps-scaled noise before each normalisation; here a zero-norm row or column normalises to 0
    double mx[kBands], ix[kBands], my[kBands], iy[kBands];
#pragma unroll
    for (int r = 0; r < kBands; ++r) {
      const double* x = X + (long)r * Fs;
      const double* y = Y + (long)r * Fs;
      double sx = 0.0, sy = 0.0;
      for (int c = 0; c < kSeg; ++c) {
        sx += x[c];
        sy += y[c];
      }
      mx[r] = sx / kSeg;
      my[r] = sy / kSeg;
      double qx = 0.0, qy = 0.0;
      for (int c = 0; c < kSeg; ++c) {
        qx += (x[c] - mx[r]) * (x[c] - mx[r]);
        qy += (y[c] - my[r]) * (y[c] - my[r]);
      }
      ix[r] = qx > 0.0 ? 1.0 / sqrt(qx) : 0.0;
      iy[r] = qy > 0.0 ? 1.0 / sqrt(qy) : 0.0;
    }
    for (int c = 0; c < kSeg; ++c) {
      double a[kBands], b[kBands], ma = 0.0, mb = 0.0;
#pragma unroll
      for (int r = 0; r < kBands; ++r) {
        a[r] = (X[(long)r * Fs + c] - mx[r]) * ix[r];
        b[r] = (Y[(long)r * Fs + c] - my[r]) * iy[r];
        ma += a[r];
        mb += b[r];
      }
      ma /= kBands;
      mb /= kBands;
      double saa = 0.0, sbb = 0.0, sab = 0.0;
#pragma unroll
      for (int r = 0; r < kBands; ++r) {
        const double da = a[r] - ma, db = b[r] - mb;
        saa += da * da;
        sbb += db * db;
        sab += da * db;
      }
      acc += sab * (saa > 0.0 ? 1.0 / sqrt(saa) : 0.0) * (sbb > 0.0 ? 1.0 / sqrt(sbb) : 0.0);
    }
    acc /= kSeg;
  }
  part[(long)item * Jmax + j] = acc;
}

// score[item] = sum_j part / (J * 15) (STOI) or / J (ESTOI), 1e-5 when J <= 0; frames[item] = K - 1
__global__ __launch_bounds__(256) void stoi_finish_kernel(const double* __restrict__ part, int Jmax,
                                                          const int* __restrict__ Kc, int extended,
                                                          double* __restrict__ score, int* __restrict__ frames) {
  __shared__ double red[4];
  const int item = blockIdx.x;
  const int K = Kc[item];
  const int Fr = K > 0 ? K - 1 : 0;
  const int J = Fr - (kSeg - 1);
  if (J <= 0) {
    if (threadIdx.x == 0) {
      score[item] = 1e-5;
      frames[item] = Fr;
    }
    return;
  }
  double acc = 0.0;
  for (int j = threadIdx.x; j < J; j += 256) acc += part[(long)item * Jmax + j];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    score[item] = ((red[0] + red[1]) + (red[2] + red[3])) / ((double)J * (extended ? 1 : kBands));
    frames[item] = Fr;
  }
}

}  // namespace

void launch_stoi_resample(const float* ref, const float* est, const int* ymap, int items, int n_in, const int* lens,
                          int n, const double* taps, int ntaps, int up, int down, int n_pre_pad, int n_pre_remove,
                          int n_out, float* out, hipStream_t st) {
  hipLaunchKernelGGL(stoi_resample_kernel, dim3((n_out + 255) / 256, items, 2), dim3(256), 0, st, ref, est, ymap,
                     n_in, lens, n, taps, ntaps, up, down, n_pre_pad, n_pre_remove, n_out, items, out);
}

void launch_stoi_frames(const float* xs, const float* ys, long stride, const int* ymap, int items, int F,
                        const int* Fb, int n, StoiBands bands, int extended, double* en, int* idx, int* Kc,
                        double* tob, double* part, double* score, int* frames, hipStream_t st) {
  const int Fs = max(F - 1, 1), Jmax = max(F - kSeg, 1);
  hipLaunchKernelGGL(stoi_energy_kernel, dim3((F + 3) / 4, items), dim3(256), 0, st, xs, stride, F, Fb, n, en);
  hipLaunchKernelGGL(stoi_mask_kernel, dim3(items), dim3(256), 0, st, en, F, Fb, n, idx, Kc);
  hipLaunchKernelGGL(stoi_envelope_kernel, dim3((Fs + 3) / 4, items), dim3(256), 0, st, xs, ys, stride, ymap, F, idx,
                     Kc, bands, Fs, tob);
  hipLaunchKernelGGL(stoi_segment_kernel, dim3((Jmax + 63) / 64, items), dim3(64), 0, st, tob, Fs, Kc, extended, Jmax,
                     part);
  hipLaunchKernelGGL(stoi_finish_kernel, dim3(items), dim3(256), 0, st, part, Jmax, Kc, extended, score, frames);
}
