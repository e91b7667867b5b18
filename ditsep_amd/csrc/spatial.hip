// Spatial mask refinement for the beamformer (dsn_beamform_spatial; the definition is in include/ditsep_hip.h, restated in
// float64 in tests/spatial_restatement.py): a complex angular central Gaussian mixture model (Ito, Araki, Nakatani 2016)
// per item and bin, with the estimates' masks as time-frequency priors (Nakatani et al. 2017; Drude & Haeb-Umbach 2017),
// gives the posteriors gamma that replace the masks in dsn_beamform's statistics.  Frames, spectra and masks are formed
// by the functions of maskrefine_dev.h that maskrefine.hip calls (mr_tables, mr_load, mr_fft, mr_split, mr_masks), so
// they have the bits they have there.  Two launches per chunk of items, then beamform.hip's weights launch on the
// chunk's statistics and, for the batch, its apply launch:
//   analysis   workgroup (group of 2048 / n_fft frames, item): the transforms of the item's C_b channels and n
//              estimates; the spectra go bin-major into X [item][bin][channel][frame], the fp32 masks into
//              M [item][bin][source][frame], so that one bin's history is contiguous rows.
//   solve      workgroup (bin, item), 256 threads, all iterations on-die in fp64.  The bin's frames pass iterations + 1
//              times in tiles of SP_TILE frames, a thread per frame: it forms z = X / sqrt(p), the priors, and per class
//              the forward substitution against the class's Cholesky factor in LDS, q, log gamma and gamma, and leaves z
//              (the last walk: X) and the class weights in LDS.  The K tri(C) complex sums and the K sums of gamma are
//              owned by fixed threads over all tiles, which add the tile's frames in increasing t, so every sum runs in
//              increasing t whatever the tiling.  After a walk thread k factors B_k in LDS.  The last walk forms gamma
//              on the fly and its owners write N straight into the layout beamform_weights_kernel reads.  An item with
//              one channel and a call with no iteration take gamma = a in their one walk.
// No floating-point atomics; nothing depends on the batch position, the padding, the alignment or the chunking.
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

#include "maskrefine_dev.h"

constexpr int SP_MAX_CH = BEAMFORM_MAX_CH;
constexpr int SP_TRI = SP_MAX_CH * (SP_MAX_CH + 1) / 2;
constexpr int SP_MAX_K = MR_MAX_SRC + 1;                                          // the sources and the noise class
constexpr int SP_TILE = MRT;                                                      // frames per tile: one per thread
constexpr int SP_ROW = SP_TILE + 1;                                               // LDS row stride of a tile (entries)
constexpr int SP_BF = (SP_MAX_CH + MR_MAX_SRC) * (MR_POINTS / 2) / MRT;           // butterflies per thread and stage

static_assert(SP_MAX_K * SP_TRI + SP_MAX_K <= MRT, "every sum has its own thread");

struct SpShape {
  int C, n, K, I, Lmax, hop, Fs, items;
  double noise, floor, reg, eps;
};

// the chunk's workspace, every array for all items in turn
struct SpWorkspace {
  double* N;      // [items][K][C (C + 1)][bins]
  float2* X;      // [items][bins][C][Fs]
  float* M;       // [items][bins][n][Fs]
  int* failed;    // [items][bins]
  double* gamma;  // [items][K][bins][Fs], or null
};

__host__ __device__ inline int sp_low(int r, int c) { return r * (r + 1) / 2 + c; }   // entry (r, c <= r), row after row
// entry (c1 <= c2) of the upper triangle of a C x C matrix, row after row (beamform.hip's bf_idx)
__host__ __device__ inline int sp_idx(int C, int c1, int c2) { return c1 * C - c1 * (c1 - 1) / 2 + (c2 - c1); }

// ---------------------------------------------------------------------------------------------------- analysis
// grid (ceil(Fs / G), items).  Dynamic LDS: float2 tw[H] | float2 buf[C + n][G][H] | float win[NFFT]
template <int NFFT>
__global__ __launch_bounds__(MRT) void spatial_analysis_kernel(const MaskRefineShape q, int Fs,
                                                               const float* __restrict__ mix,
                                                               const float* __restrict__ est,
                                                               const int* __restrict__ lens,
                                                               const int* __restrict__ chans, float2* __restrict__ Xw,
                                                               float* __restrict__ Mw) {
  constexpr int H = NFFT / 2, G = MR_POINTS / H, NP = H / 2 + 1;
  extern __shared__ __attribute__((aligned(16))) float2 sp_lds[];
  const int n = q.n, hop = q.hop, tid = threadIdx.x, b = blockIdx.y;
  const int Cb = chans ? chans[b] : q.C;
  const MrItem it = mr_item(lens, b, q.Lmax, hop);
  const int f0 = blockIdx.x * G;
  if (f0 >= it.F) return;   // (uniform)
  float2* tw = sp_lds;
  float2* buf = tw + H;
  float* win = reinterpret_cast<float*>(buf + (q.C + n) * MR_POINTS);
  mr_tables<H>(tw, win, tid);
  __syncthreads();
  const int f_last = min(it.F - 1, f0 + G - 1);
  mr_load<H>(buf, win, mix + (long)b * q.C * q.Lmax, est + (long)b * n * q.Lmax, q.Lmax, it, hop, Cb, n, f0, f_last,
             tid);
  __syncthreads();
  mr_fft<H, false, SP_BF>(buf, tw, (Cb + n) * (MR_POINTS / 2), tid);
  float2* Xb = Xw + (long)b * (H + 1) * q.C * Fs;   // bin j, channel c, frame f: Xb[(j C + c) Fs + f]
  float* Mb = Mw + (long)b * (H + 1) * n * Fs;      // bin j, source i, frame f: Mb[(j n + i) Fs + f]
  for (int e = tid; e < G * NP; e += MRT) {
    const int fg = e / NP, k = e - fg * NP, km = (H - k) & (H - 1), f = f0 + fg;
    if (f > f_last) continue;
    const float2 t = tw[k];
    for (int c = 0; c < Cb; ++c) {
      const float2* a = buf + c * MR_POINTS + fg * H;
      float2 xk, xm;
      mr_split(a[k], a[km], t, xk, xm);
      Xb[((long)k * q.C + c) * Fs + f] = xk;
      if (H - k != k) Xb[((long)(H - k) * q.C + c) * Fs + f] = xm;
    }
    float mk[MR_MAX_SRC], mm[MR_MAX_SRC];
    mr_masks(q, buf + Cb * MR_POINTS + fg * H, k, km, t, mk, mm);
#pragma unroll
    for (int i = 0; i < MR_MAX_SRC; ++i)
      if (i < n) {
        Mb[((long)k * n + i) * Fs + f] = mk[i];
        if (H - k != k) Mb[((long)(H - k) * n + i) * Fs + f] = mm[i];
      }
  }
}

// ---------------------------------------------------------------------------------------------------- solve
// grid (bins, items).  Static LDS: the tile's z (or X) per channel and the two class weights per frame, the K factors.
__global__ __launch_bounds__(MRT) void spatial_solve_kernel(const SpShape q, const int* __restrict__ lens,
                                                            const int* __restrict__ chans, const SpWorkspace ws) {
  __shared__ double2 zt[SP_MAX_CH * SP_ROW];    // channel c of the frame at tile position p: zt[c SP_ROW + p]
  __shared__ double wt[SP_MAX_K * SP_ROW];      // the weight of the frame in the sums: gamma / q, the last walk gamma
  __shared__ double gt[SP_MAX_K * SP_ROW];      // gamma (q while the E-step runs)
  __shared__ double2 Lk[SP_MAX_K * SP_TRI];     // the factors, lower triangles; B_k before it is factored
  __shared__ double ell[SP_MAX_K], sumg[SP_MAX_K];
  __shared__ int bad;
  const int tid = threadIdx.x, j = blockIdx.x, b = blockIdx.y, bins = gridDim.x;
  const int C = q.C, n = q.n, K = q.K, Fs = q.Fs;
  const int Cb = chans ? chans[b] : C;
  const int L = lens ? lens[b] : q.Lmax;
  const int F = 1 + (L + q.hop - 1) / q.hop;
  const long sys = (long)b * bins + j;
  const float2* Xb = ws.X + sys * C * Fs;
  const float* Mb = ws.M + sys * n * Fs;
  const int T = C * (C + 1) / 2, T2 = 2 * T;

  // the sum this thread owns: entry (c1 <= c2) of class ko (tid < K T), or the sum of gamma of class ko
  const bool entry = tid < K * T, total = !entry && tid < K * T + K;
  int ko = 0, c1 = 0, c2 = 0;
  if (entry) {
    ko = tid / T;
    int rest = tid - ko * T;
    while (rest >= C - c1) rest -= C - c1, ++c1;
    c2 = c1 + rest;
  } else if (total) {
    ko = tid - K * T;
  }
  const bool have = entry && c2 < Cb;   // an entry of the item's own channels

  for (int e = tid; e < K * SP_TRI; e += MRT) {   // B_k = I
    const int p = e % SP_TRI;
    int r = 0;
    while (sp_low(r + 1, 0) <= p) ++r;
    Lk[e] = make_double2(p == sp_low(r, r) ? 1.0 : 0.0, 0.0);
  }
  if (tid < K) ell[tid] = 0.0;
  if (tid == 0) bad = 0;
  const bool em = Cb > 1 && q.I > 0;   // one channel, or no iteration: gamma = a
  const int walks = em ? q.I + 1 : 1;
  int failed = 0;
  __syncthreads();

  for (int walk = 0; walk < walks; ++walk) {
    const bool last = walk == walks - 1;
    double ar = 0.0, ai = 0.0;
    for (int t0 = 0; t0 < F; t0 += SP_TILE) {
      const int Tn = min(SP_TILE, F - t0);
      __syncthreads();   // the previous tile's frames have been added; the factors are in
      if (tid < Tn) {
        const int f = t0 + tid;
        // ---- the frame: p, z
        double xr[SP_MAX_CH], xi[SP_MAX_CH];
        double p = 0.0;
#pragma unroll
        for (int c = 0; c < SP_MAX_CH; ++c) {
          xr[c] = xi[c] = 0.0;
          if (c < Cb) {
            const float2 x = Xb[(long)c * Fs + f];
            xr[c] = (double)x.x;
            xi[c] = (double)x.y;
            const double pc = xr[c] * xr[c] + xi[c] * xi[c];
            p = c == 0 ? pc : p + pc;
          }
        }
        const bool live = p > 0.0;
        const bool run = em && live;
        const double s = sqrt(p);
#pragma unroll
        for (int c = 0; c < SP_MAX_CH; ++c) {
          double zr = 0.0, zi = 0.0;
          if (c < Cb) {
            if (last) zr = xr[c], zi = xi[c];                    // the statistics take the spectra themselves
            else if (live) zr = xr[c] / s, zi = xi[c] / s;
            if (live) xr[c] = xr[c] / s, xi[c] = xi[c] / s;      // z from here on
          }
          zt[c * SP_ROW + tid] = make_double2(zr, zi);
        }
        // ---- the classes: prior, q, log gamma
        double mx = 0.0;
        for (int k = 0; k < K; ++k) {
          const double a = k < n ? (1.0 - q.noise) * ((1.0 - q.floor) * (double)Mb[(long)k * Fs + f] + q.floor / (double)n)
                                 : q.noise;
          double lg = a, qk = 1.0;
          if (run) {
            const double2* Lm = Lk + k * SP_TRI;
            double yr[SP_MAX_CH], yi[SP_MAX_CH];
            qk = 0.0;
#pragma unroll
            for (int r = 0; r < SP_MAX_CH; ++r)
              if (r < Cb) {
                double sr = xr[r], si = xi[r];
#pragma unroll
                for (int c = 0; c < r; ++c) {   // L[r][c] y[c]
                  const double2 l = Lm[sp_low(r, c)];
                  sr -= l.x * yr[c] - l.y * yi[c];
                  si -= l.x * yi[c] + l.y * yr[c];
                }
                const double d = Lm[sp_low(r, r)].x;
                yr[r] = sr / d;
                yi[r] = si / d;
                const double y2 = yr[r] * yr[r] + yi[r] * yi[r];
                qk = r == 0 ? y2 : qk + y2;
              }
            lg = log(a) - ell[k] - (double)Cb * log(qk);
            mx = k == 0 ? lg : fmax(mx, lg);   // (fmax drops a NaN: the difference below keeps it)
            if (lg != lg) mx = lg;
          }
          wt[k * SP_ROW + tid] = lg;
          gt[k * SP_ROW + tid] = qk;
        }
        if (run) {
          double se = 0.0;
          for (int k = 0; k < K; ++k) {
            const double e = exp(wt[k * SP_ROW + tid] - mx);
            wt[k * SP_ROW + tid] = e;
            se = k == 0 ? e : se + e;
          }
          for (int k = 0; k < K; ++k) {
            const double g = wt[k * SP_ROW + tid] / se, qk = gt[k * SP_ROW + tid];
            wt[k * SP_ROW + tid] = last ? g : g / qk;
            gt[k * SP_ROW + tid] = g;
          }
        } else if (!last) {   // a dead frame of an EM walk adds nothing
          for (int k = 0; k < K; ++k) wt[k * SP_ROW + tid] = gt[k * SP_ROW + tid] = 0.0;
        } else {              // gamma = a (wt holds it)
          for (int k = 0; k < K; ++k) gt[k * SP_ROW + tid] = wt[k * SP_ROW + tid];
        }
        if (last && ws.gamma)
          for (int k = 0; k < K; ++k)
            ws.gamma[(((long)b * K + k) * bins + j) * Fs + f] = gt[k * SP_ROW + tid];
      }
      __syncthreads();
      // ---- the sums, in increasing t
      if (have) {
        const double2* z1 = zt + c1 * SP_ROW;
        const double2* z2 = zt + c2 * SP_ROW;
        const double* wk = wt + ko * SP_ROW;
        for (int tt = 0; tt < Tn; ++tt) {   // w z_c1 conj(z_c2)
          const double2 u = z1[tt], v = z2[tt];
          const double w = wk[tt];
          ar += w * (u.x * v.x + u.y * v.y);
          ai += w * (u.y * v.x - u.x * v.y);
        }
      } else if (total) {
        const double* gk = gt + ko * SP_ROW;
        for (int tt = 0; tt < Tn; ++tt) ar += gk[tt];
      }
    }
    if (last) {
      // ---- N in the layout of beamform_weights_kernel; entries of channels the item does not have are zero
      if (entry) {
        double* Nb = ws.N + (((long)b * K + ko) * T2 + 2L * sp_idx(C, c1, c2)) * bins + j;
        Nb[0] = have ? ar : 0.0;
        Nb[bins] = have && c1 != c2 ? ai : 0.0;
      }
      break;
    }
    // ---- M-step: B_k = C_b sum / sum gamma (the identity where that is zero), loaded, factored by thread k
    if (total) sumg[ko] = ar;
    __syncthreads();
    if (have) {
      const double sg = sumg[ko];
      double br = c1 == c2 ? 1.0 : 0.0, bi = 0.0;
      if (sg != 0.0) {
        br = (double)Cb * ar / sg;
        bi = c1 == c2 ? 0.0 : (double)Cb * ai / sg;
      }
      Lk[ko * SP_TRI + sp_low(c2, c1)] = make_double2(br, -bi);   // the lower triangle holds conj(upper)
    }
    __syncthreads();
    if (tid < K) {
      double2* A = Lk + tid * SP_TRI;
      double tr = 0.0;
      for (int c = 0; c < Cb; ++c) tr = c == 0 ? A[sp_low(c, c)].x : tr + A[sp_low(c, c)].x;
      const double load = q.reg * tr / (double)Cb + q.eps;
      for (int c = 0; c < Cb; ++c) A[sp_low(c, c)].x += load;
      double lsum = 0.0;
      bool ok = true;
      for (int c = 0; c < Cb && ok; ++c) {
        double d = A[sp_low(c, c)].x;
        for (int k = 0; k < c; ++k) {
          const double2 l = A[sp_low(c, k)];
          d -= l.x * l.x + l.y * l.y;
        }
        if (!(d > 0.0 && d <= 1.7976931348623157e308)) {   // not finite and positive
          ok = false;
          break;
        }
        const double l = sqrt(d);
        A[sp_low(c, c)] = make_double2(l, 0.0);
        lsum = c == 0 ? log(l) : lsum + log(l);
        for (int r = c + 1; r < Cb; ++r) {
          double2 sv = A[sp_low(r, c)];
          for (int k = 0; k < c; ++k) {   // L[r][k] conj L[c][k]
            const double2 lr = A[sp_low(r, k)], lc = A[sp_low(c, k)];
            sv.x -= lr.x * lc.x + lr.y * lc.y;
            sv.y -= lr.y * lc.x - lr.x * lc.y;
          }
          A[sp_low(r, c)] = make_double2(sv.x / l, sv.y / l);
        }
      }
      ell[tid] = 2.0 * lsum;
      if (!ok) bad = 1;   // (every writer stores the same value)
    }
    __syncthreads();
    if (bad) {   // (uniform) every class of the bin is the identity for the remaining walks
      for (int e = tid; e < K * SP_TRI; e += MRT) {
        const int p = e % SP_TRI;
        int r = 0;
        while (sp_low(r + 1, 0) <= p) ++r;
        Lk[e] = make_double2(p == sp_low(r, r) ? 1.0 : 0.0, 0.0);
      }
      if (tid < K) ell[tid] = 0.0;
      failed = 1;
      walk = walks - 2;   // the next walk is the last
    }
  }
  if (tid == 0) ws.failed[sys] = failed;
  if (ws.gamma)   // frames the item does not have
    for (int e = tid; e < K * (Fs - F); e += MRT) {
      const int k = e / (Fs - F), f = F + e % (Fs - F);
      ws.gamma[(((long)b * K + k) * bins + j) * Fs + f] = 0.0;
    }
}

template <int NFFT>
void sp_analysis(const MaskRefineShape& q, int Fs, const float* mix, const float* est, const int* lens,
                 const int* chans, int items, const SpWorkspace& ws, hipStream_t st) {
  constexpr int G = MR_POINTS / (NFFT / 2);
  dsn_allow_lds<spatial_analysis_kernel<NFFT>>((int)mr_lds_bytes(NFFT, SP_MAX_CH + MR_MAX_SRC, 0));
  hipLaunchKernelGGL((spatial_analysis_kernel<NFFT>), dim3((unsigned)((Fs + G - 1) / G), (unsigned)items), dim3(MRT),
                     mr_lds_bytes(NFFT, q.C + q.n, 0), st, q, Fs, mix, est, lens, chans, ws.X, ws.M);
}

}  // namespace

int spatial_frames(int hop, int Lmax) { return 1 + (Lmax + hop - 1) / hop; }

size_t spatial_item_bytes(int nfft, int hop, int Lmax, int C, int n) {
  const size_t bins = (size_t)nfft / 2 + 1, Fs = (size_t)spatial_frames(hop, Lmax);
  return bins * (8 * ((size_t)n + 1) * C * (C + 1) + Fs * (8 * (size_t)C + 4 * (size_t)n) + 4);
}

void launch_spatial_statistics(const float* mix, const float* est, const int* lens, const int* chans, void* workspace,
                               double* gamma, int items, int C, int n, int classes, int Lmax, int nfft, int hop,
                               int power, float eps, int iterations, double noise, double floor, double mask_reg,
                               double mask_eps, hipStream_t st) {
  const int Fs = spatial_frames(hop, Lmax);
  const size_t bins = (size_t)nfft / 2 + 1, sys = (size_t)items * bins;
  SpWorkspace ws;
  ws.N = reinterpret_cast<double*>(workspace);
  ws.X = reinterpret_cast<float2*>(ws.N + (size_t)items * ((size_t)n + 1) * C * (C + 1) * bins);
  ws.M = reinterpret_cast<float*>(ws.X + sys * C * Fs);
  ws.failed = reinterpret_cast<int*>(ws.M + sys * n * Fs);
  ws.gamma = gamma;
  const MaskRefineShape q{n, Lmax, hop, power, eps, 0, C, 0.f};
  mr_for_nfft(nfft, [&](auto N) { sp_analysis<decltype(N)::value>(q, Fs, mix, est, lens, chans, items, ws, st); });
  const SpShape s{C, n, classes, iterations, Lmax, hop, Fs, items, noise, floor, mask_reg, mask_eps};
  hipLaunchKernelGGL(spatial_solve_kernel, dim3((unsigned)bins, (unsigned)items), dim3(MRT), 0, st, s, lens, chans, ws);
}
