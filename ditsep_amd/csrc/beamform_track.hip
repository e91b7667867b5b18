// Block-adaptive MVDR weights (dsn_beamform_track; the definition is in include/ditsep_hip.h, restated in float64 in
// tests/beamform_track_restatement.py): dsn_beamform with one filter per block of Tb frames, solved on the statistics
// of the blocks within `context` of it, and every frame filtered with the weights interpolated between the centres of
// its two nearest blocks.  Frames, spectra, masks and output samples are maskrefine_dev.h's, the statistics of a range
// of frames and the channel contraction beamform_dev.h's, so they have the bits they have in dsn_beamform.  Four
// launches per chunk of items:
//   stats    workgroup (k, b, i) owns block k of item b for source i -- the frames [k Tb, min(F, (k + 1) Tb)) -- and
//            writes P^(k) = sum_t M_i X X^H in frame order (bf_stats_frames: bins below 256 in registers over the whole
//            block, bins 256 and up a frame group at a time into the partial).
//   context  one thread per (item, block, source, entry, bin) adds the partials of the item's own blocks k - context ..
//            k + context in block order; zero for blocks and channels the item does not have.  The thread of entry 0,
//            bin 0, source 0 also writes the block's channel count for the solve: the item's, or 0 for a block the
//            item does not have.
//   weights  launch_beamform_solve (beamform.hip), unchanged, with (item, block) as its item and the blocks' channel
//            counts as its table: a block with 0 channels gets zero weights.
//   apply    workgroup (span, item, source), beamform_apply_kernel's layout; the thread of (frame t, bin pair) forms
//            k0 and alpha in integers (track_frame_weight) and w(t) = w0 + alpha (w1 - w0) in fp64 before it contracts
//            the channels; w1 is not read where alpha = 0.
// No atomics; nothing depends on the batch position, the padding or the chunking, so an item has the same bits alone.
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

#include "maskrefine_dev.h"

#include "beamform_dev.h"

// Frame t of an item of K blocks of Tb frames -> the block k0 whose weights it takes and alpha in [0, 1), the share of
// block k0 + 1's: centre to centre, in integers; the first and the last half block hold.  (t <= 2^30, Tb <= 2^20)
__host__ __device__ inline void track_frame_weight(int t, int Tb, int K, int interpolate, int& k0, double& alpha) {
  alpha = 0.0;
  if (!interpolate) {
    k0 = t / Tb;
    return;
  }
  const long num = 2L * t + 1 - Tb;
  k0 = 0;
  if (num <= 0) return;
  k0 = (int)(num / (2L * Tb));
  if (k0 >= K - 1) {
    k0 = K - 1;
    return;
  }
  alpha = (double)(num % (2L * Tb)) / (double)(2L * Tb);
}

// grid (Kmax, items, n).  part [items][Kmax][n][2 tri(C)][H + 1]: block blockIdx.x of the item, where it has one.
template <int NFFT>
__global__ __launch_bounds__(MRT) void track_stats_kernel(const MaskRefineShape q, int Tb, const float* __restrict__ mix,
                                                          const float* __restrict__ est, const int* __restrict__ lens,
                                                          const int* __restrict__ chans, double* __restrict__ part) {
  constexpr int H = NFFT / 2;
  const int n = q.n, b = blockIdx.y, src = blockIdx.z;
  const int Cb = chans ? chans[b] : q.C;
  const MrItem it = mr_item(lens, b, q.Lmax, q.hop);
  if ((long)blockIdx.x * Tb >= it.F) return;   // (uniform)
  const int f_first = blockIdx.x * Tb, f_last = (int)min((long)it.F, (long)f_first + Tb) - 1;
  const int T2 = 2 * bf_tri(q.C);
  bf_stats_frames<NFFT>(q, mix + (long)b * q.C * q.Lmax, est + (long)b * n * q.Lmax, it, Cb, src, f_first, f_last,
                        part + (((long)b * gridDim.x + blockIdx.x) * n + src) * T2 * (H + 1));
}

// N [items][Kmax][n][2 tri(C)][bins] from part of the same shape: block k's sum over the item's own blocks
// max(0, k - context) .. min(K - 1, k + context) in block order; zero in blocks and channels the item does not have.
// blockch [items][Kmax]: the item's channel count, 0 for a block it does not have.
__global__ __launch_bounds__(MRT) void track_context_kernel(const double* __restrict__ part, const int* __restrict__ lens,
                                                            const int* __restrict__ chans, int items, int Kmax, int n,
                                                            int C, int Lmax, int bins, int hop, int Tb, int context,
                                                            double* __restrict__ N, int* __restrict__ blockch) {
  const int T2 = 2 * bf_tri(C);
  const long e = (long)blockIdx.x * MRT + threadIdx.x;
  if (e >= (long)items * Kmax * n * T2 * bins) return;
  const int j = (int)(e % bins), u = (int)(e / bins % T2), i = (int)(e / bins / T2 % n);
  const int k = (int)(e / bins / T2 / n % Kmax), b = (int)(e / bins / T2 / n / Kmax);
  const int L = lens ? lens[b] : Lmax, Cb = chans ? chans[b] : C;
  const int F = 1 + (L + hop - 1) / hop, K = (F + Tb - 1) / Tb;
  if (j == 0 && u == 0 && i == 0) blockch[(long)b * Kmax + k] = k < K ? Cb : 0;
  // entry u / 2 is (c1, c2): it exists for the item where c2 < Cb
  int c1 = 0, rest = u / 2;
  while (rest >= C - c1) rest -= C - c1, ++c1;
  const int c2 = c1 + rest;
  double s = 0.0;
  if (c2 < Cb && k < K) {
    const long stride = (long)n * T2 * bins;
    const double* p = part + (long)b * Kmax * stride + ((long)i * T2 + u) * bins + j;
    for (int m = max(0, k - context); m <= min(K - 1, k + context); ++m) s += p[m * stride];
  }
  N[e] = s;
}

// grid (ceil(Lmax / SPAN), items, n).  w [items][Kmax][n][H + 1][C] complex doubles, out [items][n][Lmax].
// Dynamic LDS: float2 tw[H] | float2 buf[C + (post ? n : 0)][G][H] | float win[NFFT] | float ola[SPAN]
template <int NFFT>
__global__ __launch_bounds__(MRT) void track_apply_kernel(const MaskRefineShape q, int post, int Tb, int Kmax,
                                                          int interpolate, const float* __restrict__ mix,
                                                          const float* __restrict__ est, const int* __restrict__ lens,
                                                          const int* __restrict__ chans, const double* __restrict__ w,
                                                          float* __restrict__ out) {
  constexpr int H = NFFT / 2, G = MR_POINTS / H, NP = H / 2 + 1, SPAN = mr_span(NFFT);
  extern __shared__ __attribute__((aligned(16))) float2 bf_lds[];
  const int n = q.n, hop = q.hop, tid = threadIdx.x;
  const int b = blockIdx.y, src = blockIdx.z, s0 = blockIdx.x * SPAN;
  const int Cb = chans ? chans[b] : q.C;
  const int ne = post ? n : 0;
  float2* tw = bf_lds;
  float2* buf = tw + H;
  float* win = reinterpret_cast<float*>(buf + (q.C + ne) * MR_POINTS);
  float* ola = win + NFFT;
  const MrItem it = mr_item(lens, b, q.Lmax, hop);
  const float* mixb = mix + (long)b * q.C * q.Lmax;
  const float* estb = est + (long)b * n * q.Lmax;
  float* outb = out + ((long)b * n + src) * q.Lmax;

  if (s0 >= it.L) {   // (uniform) past the item's end
    mr_zero<H>(outb, 0, 1, s0, q.Lmax, q.vec, tid);
    return;
  }
  mr_tables<H>(tw, win, tid);
  for (int e = tid; e < SPAN; e += MRT) ola[e] = 0.f;

  const MrFrames fr = mr_frames<H>(it, s0, hop);
  const int f_first = fr.f_first, f_last = fr.f_last;
  const int K = (it.F + Tb - 1) / Tb;
  const long wstride = 2L * n * (H + 1) * q.C;                          // doubles from a block's weights to the next's
  const double* wb = w + (long)b * Kmax * wstride + 2L * src * (H + 1) * q.C;   // block k, bin j, channel c: wb[k wstride + 2 (j C + c)]

  for (int f0 = f_first; f0 <= f_last; f0 += G) {
    __syncthreads();   // the tables are in; the previous group's frames have been added
    mr_load<H>(buf, win, mixb, estb, q.Lmax, it, hop, Cb, ne, f0, f_last, tid);
    __syncthreads();
    mr_fft<H, false, BF_BF>(buf, tw, (Cb + ne) * (MR_POINTS / 2), tid);
    // ---- contract: one thread per (frame, pair of bins k and H - k); channel 0's slot becomes Y, packed again
    for (int e = tid; e < G * NP; e += MRT) {
      const int fg = e / NP, k = e - fg * NP;
      if (f0 + fg > f_last) continue;
      int k0;
      double alpha;
      track_frame_weight(f0 + fg, Tb, K, interpolate, k0, alpha);
      const double* w0 = wb + k0 * wstride;
      bf_contract<H>(q, post, buf, tw, Cb, src, fg, k, [&](int j, int c, double& re, double& im) {
        const double* a = w0 + 2L * (j * q.C + c);
        re = a[0];
        im = a[1];
        if (alpha != 0.0) {   // (alpha > 0 only where k0 + 1 < K)
          re = re + alpha * (a[wstride] - re);
          im = im + alpha * (a[wstride + 1] - im);
        }
      });
    }
    __syncthreads();
    mr_fft<H, true, BF_BF>(buf, tw, MR_POINTS / 2, tid);
    mr_add<H>(ola, buf, win, s0, fr.pend, hop, f0, min(f0 + G - 1, f_last), tid);
  }
  mr_finish<H>(ola, win, outb, 0, 1, it, s0, fr.pend, hop, q.Lmax, q.vec, tid);
}

}  // namespace

int track_blocks(int hop, int Lmax, int Tb) {
  const long F = 1 + ((long)Lmax + hop - 1) / hop;
  return (int)((F + Tb - 1) / Tb);
}

size_t track_item_bytes(int nfft, int hop, int Lmax, int C, int n, int Tb) {
  const size_t bins = (size_t)nfft / 2 + 1;
  return (size_t)track_blocks(hop, Lmax, Tb) * (8 * (size_t)n * bins * (2 * (size_t)C * (C + 1) + 2 * (size_t)C) + 4);
}

void launch_track_weights(const float* mix, const float* est, const int* lens, const int* chans, int ref, double* part,
                          double* N, double* w, int* blockch, int items, int C, int n, int Lmax, int nfft, int hop,
                          int power, float eps, float reg, int Tb, int context, int design, int sweeps,
                          hipStream_t st) {
  const MaskRefineShape q{n, Lmax, hop, power, eps, 0, C, reg};
  const int Kmax = track_blocks(hop, Lmax, Tb), bins = nfft / 2 + 1;
  mr_for_nfft(nfft, [&](auto NF) {
    constexpr int NFFT = decltype(NF)::value;
    dsn_allow_lds<track_stats_kernel<NFFT>>((int)mr_lds_bytes(NFFT, BF_MAX_CH + MR_MAX_SRC, 0));
    hipLaunchKernelGGL((track_stats_kernel<NFFT>), dim3((unsigned)Kmax, (unsigned)items, (unsigned)n), dim3(MRT),
                       mr_lds_bytes(NFFT, C + n, 0), st, q, Tb, mix, est, lens, chans, part);
  });
  const long rows = (long)items * Kmax * n * 2 * bf_tri(C) * bins;
  hipLaunchKernelGGL(track_context_kernel, dim3((unsigned)((rows + MRT - 1) / MRT)), dim3(MRT), 0, st, part, lens, chans,
                     items, Kmax, n, C, Lmax, bins, hop, Tb, context, N, blockch);
  launch_beamform_solve(N, blockch, ref, w, items * Kmax, C, n, n, bins, (double)reg, (double)eps, design, sweeps, st);
}

void launch_track_apply(const float* mix, const float* est, const int* lens, const int* chans, const double* w,
                        float* out, int items, int C, int n, int Lmax, int nfft, int hop, int power, float eps, int post,
                        int Tb, int interpolate, hipStream_t st) {
  const MaskRefineShape q{n, Lmax, hop, power, eps, ((uintptr_t)out & 15) == 0 && Lmax % 4 == 0 ? 1 : 0, C, 0.f};
  const int Kmax = track_blocks(hop, Lmax, Tb);
  mr_for_nfft(nfft, [&](auto NF) {
    constexpr int NFFT = decltype(NF)::value, SPAN = mr_span(NFFT);
    dsn_allow_lds<track_apply_kernel<NFFT>>((int)mr_lds_bytes(NFFT, BF_MAX_CH + MR_MAX_SRC, 1));
    hipLaunchKernelGGL((track_apply_kernel<NFFT>), dim3((unsigned)((Lmax + SPAN - 1) / SPAN), (unsigned)items, (unsigned)n),
                       dim3(MRT), mr_lds_bytes(NFFT, C + (post ? n : 0), 1), st, q, post, Tb, Kmax, interpolate, mix, est,
                       lens, chans, w, out);
  });
}
