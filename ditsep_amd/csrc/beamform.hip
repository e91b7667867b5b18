// Mask-based MVDR beamforming (dsn_beamform; the definition is in include/ditsep_hip.h, restated in float64 in
// tests/beamform_restatement.py): the masks of the mono estimates give one spatial covariance per source and bin from
// the mixture's own channels, and a minimum-variance distortionless-response filter (Souden, Benesty, Affes 2010)
// returns one mono signal per source.  Frames, spectra, masks and output samples are formed by the functions of
// maskrefine_dev.h that maskrefine.hip calls (mr_tables, mr_load, mr_fft, mr_split, mr_masks, mr_merge, mr_add,
// mr_finish), so they have the bits they have there; the statistics of a range of frames and the channel contraction are
// beamform_dev.h's (bf_stats_frames, bf_contract), which beamform_track.hip calls as well.  Three launches per chunk of
// items, then one for the batch:
//   stats    workgroup (o, b, i) owns the frames [o fpo, (o + 1) fpo) of item b for source i -- every frame has exactly
//            one owner per source; fpo is a whole number of spans, more than one where the item has more than
//            BEAMFORM_MAX_OWNERS spans --, transforms the item's C_b channels and n estimates in groups of
//            2048 / n_fft frames and, per bin, sums M_i X X^H (upper triangle, fp64 products) in frame order: the
//            thread that owns a bin below 256 keeps the sums of all the owner's frames in registers and stores them
//            once; bins 256 and up are summed over a group in registers and then added to the owner's partial in
//            global memory with plain loads and stores.
//   reduce   one thread per (item, source, entry, bin) adds the item's partials in owner order.
//   weights  eight lanes per (item, source, bin): every lane forms A = Q_i + lambda I and its Cholesky factor itself
//            (channels the item does not have are an identity block, which leaves the other entries' arithmetic as it
//            is) and solves column `lane` of Z = A^-1 N_i; the diagonal of Z goes through LDS, tau is added in channel
//            order by the lane of the reference channel, which writes w = Z[:, ref] / tau.  The launch also runs alone
//            on given statistics of `classes` >= n classes (launch_beamform_solve; spatial.hip's noise class): all
//            classes enter Q_i, the first n get a filter.  This is Souden's filter, DSN_BEAMFORM_DESIGN_SOUDEN; for the
//            other designs launch_beamform_solve launches beamform_design.hip's kernel in its place.
//   apply    workgroup (span, item, source), the mask kernel's layout: transforms the C_b channels (and the n
//            estimates only where the post-filter needs the masks), contracts the channels with w in fp64 in channel
//            order, rounds once, writes Y_i over channel 0's slot, inverse-transforms that slot and overlap-adds.
// No atomics; nothing depends on the batch position, the padding or the chunking, so an item has the same bits alone.
#include "../../include/ditsep_hip.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

#include "maskrefine_dev.h"

#include "beamform_dev.h"

constexpr int BF_LANES = 8, BF_GROUPS = MRT / BF_LANES;                          // weights launch: lanes per system

// frames one owner takes of an item of F frames: whole spans of `base` frames, as few as keep the owners within the cap
__host__ __device__ inline int bf_owner_frames(int F, int base) {
  const int spans = (F + base - 1) / base;
  return base * ((spans + BEAMFORM_MAX_OWNERS - 1) / BEAMFORM_MAX_OWNERS);
}

// grid (owners, items, n).  part [items][gridDim.x][n][2 tri(C)][H + 1]; the owner's frames go through bf_stats_frames.
template <int NFFT>
__global__ __launch_bounds__(MRT) void beamform_stats_kernel(const MaskRefineShape q, const float* __restrict__ mix,
                                                             const float* __restrict__ est,
                                                             const int* __restrict__ lens, const int* __restrict__ chans,
                                                             double* __restrict__ part) {
  constexpr int H = NFFT / 2, SPAN = mr_span(NFFT);
  const int n = q.n, hop = q.hop, b = blockIdx.y, src = blockIdx.z;
  const int Cb = chans ? chans[b] : q.C;
  const MrItem it = mr_item(lens, b, q.Lmax, hop);
  const int F = it.F;
  const int fpo = bf_owner_frames(F, SPAN / hop);
  if ((long)blockIdx.x * fpo >= F) return;   // (uniform)
  const int f_first = blockIdx.x * fpo, f_last = min(F, f_first + fpo) - 1;
  const int T2 = 2 * bf_tri(q.C);
  bf_stats_frames<NFFT>(q, mix + (long)b * q.C * q.Lmax, est + (long)b * n * q.Lmax, it, Cb, src, f_first, f_last,
                        part + (((long)b * gridDim.x + blockIdx.x) * n + src) * T2 * (H + 1));
}

// N [items][n][2 tri(C)][bins] from part [items][OW][n][2 tri(C)][bins]: the item's own owners, in owner order.  Entries
// of channels the item does not have are written as zero.
__global__ __launch_bounds__(MRT) void beamform_reduce_kernel(const double* __restrict__ part,
                                                              const int* __restrict__ lens,
                                                              const int* __restrict__ chans, int items, int n, int C,
                                                              int Lmax, int bins, int hop, int base, int OW,
                                                              double* __restrict__ N) {
  const int T2 = 2 * bf_tri(C);
  const long e = (long)blockIdx.x * MRT + threadIdx.x;
  if (e >= (long)items * n * T2 * bins) return;
  const int j = (int)(e % bins), u = (int)(e / bins % T2), i = (int)(e / bins / T2 % n);
  const int b = (int)(e / bins / T2 / n);
  const int L = lens ? lens[b] : Lmax, Cb = chans ? chans[b] : C;
  const int F = 1 + (L + hop - 1) / hop, fpo = bf_owner_frames(F, base), owners = (F + fpo - 1) / fpo;
  // entry u / 2 is (c1, c2): it exists for the item where c2 < Cb
  int c1 = 0, rest = u / 2;
  while (rest >= C - c1) rest -= C - c1, ++c1;
  const int c2 = c1 + rest;
  double s = 0.0;
  if (c2 < Cb)
    for (int o = 0; o < owners; ++o) s += part[((((long)b * OW + o) * n + i) * T2 + u) * bins + j];
  N[e] = s;
}

// N [items][classes][2 tri(C)][bins] -> w [items][n][bins][C] complex doubles: the first n of the classes >= n get a
// filter, all of them enter the interference.  Thread (g, lane) of a workgroup: system blockIdx.x BF_GROUPS + g =
// (item, source, bin), right-hand side `lane`.
__global__ __launch_bounds__(MRT) void beamform_weights_kernel(const double* __restrict__ N,
                                                               const int* __restrict__ chans, int ref, int items,
                                                               int n, int classes, int C, int bins, double reg,
                                                               double eps, double* __restrict__ w) {
  __shared__ double zd[BF_GROUPS][BF_LANES];
  const int lane = threadIdx.x % BF_LANES, g = threadIdx.x / BF_LANES;
  const long sys = (long)blockIdx.x * BF_GROUPS + g, total = (long)items * n * bins;
  const bool live = sys < total;
  const long e = live ? sys : total - 1;
  const int j = (int)(e % bins), i = (int)(e / bins % n), b = (int)(e / bins / n);
  const int Cb = chans ? chans[b] : C;
  const int T2 = 2 * bf_tri(C);
  const double* Nb = N + (long)b * classes * T2 * bins + j;   // entry u of class s: Nb[(s T2 + u) bins]

  // A = Q_i + lambda I and its Cholesky factor (bf_factor, beamform_dev.h): a[r (r + 1) / 2 + c] = L[r][c], c <= r
  double ar[BF_TRI], ai[BF_TRI];
  bf_factor(Nb, i, classes, C, Cb, bins, reg, eps, ar, ai);
  // column `lane` of N_i: N[r][lane] = upper(r, lane) for r <= lane, conj upper(lane, r) below
  double zr[BF_MAX_CH], zi[BF_MAX_CH];
#pragma unroll
  for (int r = 0; r < BF_MAX_CH; ++r) {
    zr[r] = zi[r] = 0.0;
    if (r < Cb && lane < Cb) {
      const int lo = min(r, lane), hi = max(r, lane);
      const long at = ((long)i * T2 + 2L * bf_idx(C, lo, hi)) * bins;
      zr[r] = Nb[at];
      zi[r] = r <= lane ? Nb[at + bins] : -Nb[at + bins];
    }
  }
  // L y = b, then L^H z = y
  bf_forward(ar, ai, zr, zi);
  bf_backward(ar, ai, zr, zi);
  double own = 0.0;
#pragma unroll
  for (int r = 0; r < BF_MAX_CH; ++r)
    if (r == lane) own = zr[r];
  zd[g][lane] = own;
  __syncthreads();
  if (!live || lane != ref) return;
  double tau = 0.0;
  for (int c = 0; c < Cb; ++c) tau = c == 0 ? zd[g][0] : tau + zd[g][c];
  const bool ok = tau > 0.0 && tau <= 1.7976931348623157e308;   // finite and positive (false for NaN)
  double* wo = w + 2L * e * C;
#pragma unroll
  for (int c = 0; c < BF_MAX_CH; ++c)
    if (c < C) {
      double vr = 0.0, vi = 0.0;
      if (c < Cb) {
        vr = ok ? zr[c] / tau : (c == ref ? 1.0 : 0.0);
        vi = ok ? zi[c] / tau : 0.0;
      }
      wo[2 * c] = vr;
      wo[2 * c + 1] = vi;
    }
}

// grid (ceil(Lmax / SPAN), items, n).  w [items][n][H + 1][C] complex doubles, out [items][n][Lmax].
// Dynamic LDS: float2 tw[H] | float2 buf[C + (post ? n : 0)][G][H] | float win[NFFT] | float ola[SPAN]
template <int NFFT>
__global__ __launch_bounds__(MRT) void beamform_apply_kernel(const MaskRefineShape q, int post,
                                                             const float* __restrict__ mix,
                                                             const float* __restrict__ est,
                                                             const int* __restrict__ lens, const int* __restrict__ chans,
                                                             const double* __restrict__ w, float* __restrict__ out) {
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
  const double* wb = w + 2L * ((long)b * n + src) * (H + 1) * q.C;   // bin j, channel c: wb[2 (j C + c)]

  for (int f0 = f_first; f0 <= f_last; f0 += G) {
    __syncthreads();   // the tables are in; the previous group's frames have been added
    mr_load<H>(buf, win, mixb, estb, q.Lmax, it, hop, Cb, ne, f0, f_last, tid);
    __syncthreads();
    mr_fft<H, false, BF_BF>(buf, tw, (Cb + ne) * (MR_POINTS / 2), tid);
    // ---- contract: one thread per (frame, pair of bins k and H - k); channel 0's slot becomes Y, packed again
    for (int e = tid; e < G * NP; e += MRT) {
      const int fg = e / NP, k = e - fg * NP;
      if (f0 + fg > f_last) continue;
      bf_contract<H>(q, post, buf, tw, Cb, src, fg, k, [&](int j, int c, double& re, double& im) {
        const double* wj = wb + 2L * j * q.C;
        re = wj[2 * c];
        im = wj[2 * c + 1];
      });
    }
    __syncthreads();
    mr_fft<H, true, BF_BF>(buf, tw, MR_POINTS / 2, tid);
    mr_add<H>(ola, buf, win, s0, fr.pend, hop, f0, min(f0 + G - 1, f_last), tid);
  }
  mr_finish<H>(ola, win, outb, 0, 1, it, s0, fr.pend, hop, q.Lmax, q.vec, tid);
}

struct BfArgs {
  const float *mix, *est;
  const int *lens, *chans;
  int ref;
  double *part, *N, *w;
  float* out;
  int items, post;
  double reg, eps;
  int design, sweeps;
};

template <int NFFT>
void bf_run(int stage, const MaskRefineShape& q, const BfArgs& a, hipStream_t st) {
  constexpr int SPAN = mr_span(NFFT);
  const int bins = NFFT / 2 + 1, T2 = 2 * bf_tri(q.C), OW = beamform_owners(NFFT, q.hop, q.Lmax);
  if (stage == 0) {
    dsn_allow_lds<beamform_stats_kernel<NFFT>>((int)mr_lds_bytes(NFFT, BF_MAX_CH + MR_MAX_SRC, 0));
    hipLaunchKernelGGL((beamform_stats_kernel<NFFT>), dim3((unsigned)OW, (unsigned)a.items, (unsigned)q.n), dim3(MRT),
                       mr_lds_bytes(NFFT, q.C + q.n, 0), st, q, a.mix, a.est, a.lens, a.chans, a.part);
    const long rows = (long)a.items * q.n * T2 * bins;
    hipLaunchKernelGGL(beamform_reduce_kernel, dim3((unsigned)((rows + MRT - 1) / MRT)), dim3(MRT), 0, st, a.part,
                       a.lens, a.chans, a.items, q.n, q.C, q.Lmax, bins, q.hop, SPAN / q.hop, OW, a.N);
    launch_beamform_solve(a.N, a.chans, a.ref, a.w, a.items, q.C, q.n, q.n, bins, a.reg, a.eps, a.design, a.sweeps, st);
    return;
  }
  const int slots = q.C + (a.post ? q.n : 0);
  dsn_allow_lds<beamform_apply_kernel<NFFT>>((int)mr_lds_bytes(NFFT, BF_MAX_CH + MR_MAX_SRC, 1));
  hipLaunchKernelGGL((beamform_apply_kernel<NFFT>),
                     dim3((unsigned)((q.Lmax + SPAN - 1) / SPAN), (unsigned)a.items, (unsigned)q.n), dim3(MRT),
                     mr_lds_bytes(NFFT, slots, 1), st, q, a.post, a.mix, a.est, a.lens, a.chans, a.w, a.out);
}

void bf_dispatch(int nfft, int stage, const MaskRefineShape& q, const BfArgs& a, hipStream_t st) {
  mr_for_nfft(nfft, [&](auto N) { bf_run<decltype(N)::value>(stage, q, a, st); });
}

}  // namespace

int beamform_owners(int nfft, int hop, int Lmax) {
  const int F = 1 + (Lmax + hop - 1) / hop, base = mr_span(nfft) / hop;
  return std::min(BEAMFORM_MAX_OWNERS, (F + base - 1) / base);   // (an item of L <= Lmax samples has no more owners)
}

size_t beamform_item_doubles(int nfft, int hop, int Lmax, int C, int n) {
  return ((size_t)beamform_owners(nfft, hop, Lmax) + 1) * n * 2 * bf_tri(C) * ((size_t)nfft / 2 + 1);
}

void launch_beamform_solve(const double* N, const int* chans, int ref, double* w, int items, int C, int n, int classes,
                           int bins, double reg, double eps, int design, int sweeps, hipStream_t st) {
  if (design != DSN_BEAMFORM_DESIGN_SOUDEN) {
    launch_beamform_design(N, chans, ref, w, items, C, n, classes, bins, reg, eps, design, sweeps, st);
    return;
  }
  const long systems = (long)items * n * bins;
  hipLaunchKernelGGL(beamform_weights_kernel, dim3((unsigned)((systems + BF_GROUPS - 1) / BF_GROUPS)), dim3(MRT), 0, st,
                     N, chans, ref, items, n, classes, C, bins, reg, eps, w);
}

void launch_beamform_weights(const float* mix, const float* est, const int* lens, const int* chans, int ref,
                             double* part, double* N, double* w, int items, int C, int n, int Lmax, int nfft, int hop,
                             int power, float eps, float reg, int design, int sweeps, hipStream_t st) {
  const MaskRefineShape q{n, Lmax, hop, power, eps, 0, C, reg};
  bf_dispatch(nfft, 0, q, BfArgs{mix, est, lens, chans, ref, part, N, w, nullptr, items, 0, (double)reg, (double)eps,
                                 design, sweeps}, st);
}

void launch_beamform_apply(const float* mix, const float* est, const int* lens, const int* chans, const double* w,
                           float* out, int items, int C, int n, int Lmax, int nfft, int hop, int power, float eps,
                           int post, hipStream_t st) {
  const MaskRefineShape q{n, Lmax, hop, power, eps, ((uintptr_t)out & 15) == 0 && Lmax % 4 == 0 ? 1 : 0, C, 0.f};
  bf_dispatch(nfft, 1, q, BfArgs{mix, est, lens, chans, 0, nullptr, nullptr, const_cast<double*>(w), out, items,
                                 post, 0.0, (double)eps, 0, 0}, st);
}
