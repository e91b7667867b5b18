// bss_eval SDR / SIR / SAR with F-tap distortion filters (dsn_bss_eval; Vincent et al. 2006, the quantity
// fast_bss_eval.bss_eval_sources / fast_bss_eval.sdr report).  Restated in float64 in tests/bss_eval_restatement.py.
//
// Per batch item, with the references scaled to unit norm (s_i = 1 / |ref_i|, 0 for an all-zero reference):
//   c_ij[k] = s_i s_j sum_t ref_i[t] ref_j[t + k]   |k| < F      G[(i,p),(j,q)] = c_ij[p - q] + load_diag [i = j, p = q]
//   d_ij[p] = s_i sum_t ref_i[t - p] est_j[t]       0 <= p < F    ee_j = sum_t est_j[t]^2
//   pt_ij = d_ij^T G_ii^-1 d_ij (the F x F Toeplitz block of reference i),  pall_j = d_j^T G^-1 d_j (all M = n F rows)
// the energies of the projections of the zero-extended est_j on the F shifts of one reference and of all of them.
// Four launches per chunk of items:
//   bss_corr_kernel    per (item, job, time tile of BSS_TILE samples counted from the item's start): one correlation
//                      corr(x, y)[k] = sum_t x[t] y[t + k], 0 <= k < F, of the tile, x and y staged through LDS.  Jobs:
//                      (ref_i, ref_j) for every ordered pair -- c_ij[-k] = c_ji[k], so F lags per ordered pair cover the
//                      2F - 1 lags of a pair and the F of a diagonal --, (ref_i, est_j), and (est_j, est_j) at lag 0.
//                      fp32 x fp32 products are exact in fp64 and are summed in fp64 in sample order; one plain store
//                      per (tile, lag).
//   bss_reduce_kernel  adds the tile partials in index order -> the lag tables tab [item][job][F] and ee.
//   bss_solve_kernel   one workgroup per system (the M x M one and the F x F block of each reference; block 0 is the
//                      leading block of the M x M system in source-major order and is read from it).  Blocked
//                      left-looking Cholesky in fp64: the n right-hand sides ride along as rows M .. M + n - 1, so after
//                      the last panel they hold Y = L^-1 D and the quadratic forms are sum_k Y[k][j]^2 -- no back
//                      substitution, no stored solution.  G is never materialised: a panel starts from entries formed
//                      from the lag tables; finished panels of L are read back from the workspace.
//   bss_finish_kernel  one thread per item: the ratios, dB values, clamps and the permutation search.
// No atomics; every sum has an order fixed by the item's own length, n and F: reruns, ragged batches and any chunking
// give the same bits, and the leading block's quadratic forms are those of its stand-alone system.
#include "kernels.h"

namespace {

constexpr int CT = 256;                  // threads of every workgroup here
constexpr int NB = 32, RB = 128, KB = 16;  // panel width, rows per pass, depth of one staged slab of finished panels

// ---- correlations -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CT) void bss_corr_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                      int n, int L, const int* __restrict__ lens, int F, int item0,
                                                      int tiles, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float xs[BSS_TILE];
  __shared__ float ys[BSS_TILE + BSS_MAX_TAPS];
  const int tid = threadIdx.x;
  const int item = blockIdx.z, b = item0 + item;
  const int len = lens ? lens[b] : L;
  const int t0 = blockIdx.x * BSS_TILE;
  if (t0 >= len) return;  // uniform over the workgroup
  const int job = blockIdx.y, nn = n * n, jobs = 2 * nn + n;
  const float* rb = ref + (long)b * n * L;
  const float* eb = est + (long)b * n * L;
  const float *x, *y;
  int nl = F;
  if (job < nn) {
    x = rb + (long)(job / n) * L;
    y = rb + (long)(job % n) * L;
  } else if (job < 2 * nn) {
    x = rb + (long)((job - nn) / n) * L;
    y = eb + (long)((job - nn) % n) * L;
  } else {
    x = y = eb + (long)(job - 2 * nn) * L;
    nl = 1;
  }
  const int tl = min(BSS_TILE, len - t0);
  const int tl4 = (tl + 3) & ~3;  // the tile's samples, zero-extended to whole quads
  for (int t = tid; t < tl4; t += CT) xs[t] = t < tl ? x[t0 + t] : 0.f;
  for (int t = tid; t < tl4 + nl - 1; t += CT) ys[t] = t0 + t < len ? y[t0 + t] : 0.f;
  __syncthreads();
  // lags tid and tid + CT (F <= 2 CT), each summed in sample order; the second lag shares the first's x reads
  double* out = part + (((long)item * jobs + job) * tiles + blockIdx.x) * F;
  const int k0 = tid, k1 = tid + CT;
  if (k1 < nl) {
    double acc0 = 0.0, acc1 = 0.0;
    for (int t = 0; t < tl4; t += 4) {
      const float4 xv = *reinterpret_cast<const float4*>(xs + t);
      acc0 = fma((double)xv.x, (double)ys[t + k0], acc0);
      acc1 = fma((double)xv.x, (double)ys[t + k1], acc1);
      acc0 = fma((double)xv.y, (double)ys[t + k0 + 1], acc0);
      acc1 = fma((double)xv.y, (double)ys[t + k1 + 1], acc1);
      acc0 = fma((double)xv.z, (double)ys[t + k0 + 2], acc0);
      acc1 = fma((double)xv.z, (double)ys[t + k1 + 2], acc1);
      acc0 = fma((double)xv.w, (double)ys[t + k0 + 3], acc0);
      acc1 = fma((double)xv.w, (double)ys[t + k1 + 3], acc1);
    }
    out[k0] = acc0;
    out[k1] = acc1;
  } else if (k0 < nl) {
    double acc = 0.0;
    for (int t = 0; t < tl4; t += 4) {
      const float4 xv = *reinterpret_cast<const float4*>(xs + t);
      acc = fma((double)xv.x, (double)ys[t + k0], acc);
      acc = fma((double)xv.y, (double)ys[t + k0 + 1], acc);
      acc = fma((double)xv.z, (double)ys[t + k0 + 2], acc);
      acc = fma((double)xv.w, (double)ys[t + k0 + 3], acc);
    }
    out[k0] = acc;
  }
}

__global__ __launch_bounds__(CT) void bss_reduce_kernel(const double* __restrict__ part, int n, int L,
                                                        const int* __restrict__ lens, int F, int item0, int tiles,
                                                        double* __restrict__ tab, double* __restrict__ ee) {
  const int item = blockIdx.z, b = item0 + item, job = blockIdx.y, nn = n * n, jobs = 2 * nn + n;
  const int k = blockIdx.x * CT + threadIdx.x;
  if (k >= (job < 2 * nn ? F : 1)) return;
  const int len = lens ? lens[b] : L;
  const int nt = (len + BSS_TILE - 1) / BSS_TILE;
  const double* p = part + (((long)item * jobs + job) * tiles) * F + k;
  double s = 0.0;
  for (int c = 0; c < nt; ++c) s += p[(long)c * F];
  tab[((long)item * jobs + job) * F + k] = s;
  if (job >= 2 * nn) ee[(long)b * n + (job - 2 * nn)] = s;
}

// ---- factor and solve ---------------------------------------------------------------------------------------------
// The system of references i0 .. i0 + nr - 1 (Mm = nr F unknowns) with the n right-hand sides as rows Mm .. Mm + n - 1.
struct BssSystem {
  const double* tab;  // the item's lag tables [jobs][F]
  int n, F, i0, Mm;
  double load_diag;
};
// where row r of a system starts in its workspace: rows r < Mm keep their r + 1 entries left of and on the diagonal
// (the factor is lower triangular), the right-hand-side rows all Mm
__device__ __forceinline__ long bss_row(int r, int Mm) {
  return r < Mm ? (long)r * (r + 1) / 2 : (long)Mm * (Mm + 1) / 2 + (long)(r - Mm) * Mm;
}
// entry (r, c), c < Mm, of the scaled system before elimination; sc = the references' scales
__device__ __forceinline__ double bss_entry(const BssSystem& q, const double* sc, int r, int c) {
  const int j = q.i0 + c / q.F, col = c % q.F;
  if (r >= q.Mm) return q.tab[((long)(q.n * q.n + j * q.n + (r - q.Mm))) * q.F + col] * sc[j];
  const int i = q.i0 + r / q.F, k = r % q.F - col;
  const double v = (k >= 0 ? q.tab[((long)(i * q.n + j)) * q.F + k] : q.tab[((long)(j * q.n + i)) * q.F - k]) *
                   (sc[i] * sc[j]);
  return r == c ? v + q.load_diag : v;
}

// grid (systems per item, items).  full != 0: system 0 is the M x M one and system m >= 1 the block of reference m;
// full == 0: system m is the block of reference m.  Q [item][2][4][4]: Q[0][j][i] = sum over rows i F .. i F + F - 1 of
// Y[.][j]^2 of the M x M system, Q[1][i][j] the same sum of reference i's block system.
__global__ __launch_bounds__(CT) void bss_solve_kernel(const double* __restrict__ tabs, int n, int F, int full,
                                                       double load_diag, long mat_stride, long full_size,
                                                       long block_size, double* mats, int item0,
                                                       double* __restrict__ Q, int* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) double a_s[KB][RB + 2];
  __shared__ __attribute__((aligned(16))) double b_s[KB][NB + 2];
  __shared__ double s_s[RB][NB + 1];
  __shared__ double d_s[NB][NB + 1];
  __shared__ double sc[BSS_MAX_SRC];
  __shared__ int bad;
  const int tid = threadIdx.x;
  const int item = blockIdx.y, b = item0 + item, sys = blockIdx.x;
  const int jobs = 2 * n * n + n;
  const bool whole = full && sys == 0;
  BssSystem q;
  q.tab = tabs + (long)item * jobs * F;
  q.n = n;
  q.F = F;
  q.i0 = whole ? 0 : sys;
  q.Mm = whole ? n * F : F;
  q.load_diag = load_diag;
  const int Mm = q.Mm, Rt = Mm + n;
  double* A = mats + (long)item * mat_stride + (full ? (sys == 0 ? 0 : full_size + (sys - 1) * block_size) : sys * block_size);
  if (tid < n) {
    const double e = q.tab[((long)(tid * n + tid)) * F];
    sc[tid] = e > 0.0 ? 1.0 / sqrt(e) : 0.0;
  }
  if (tid == 0) bad = 0;
  __syncthreads();
  const int tr = tid >> 3, tc = tid & 7;  // the thread's 4 x 4 patch of a pass: rows 4 tr .., columns 4 tc ..
  for (int c0 = 0; c0 < Mm; c0 += NB) {
    const int w = min(NB, Mm - c0);
    for (int r0 = c0; r0 < Rt; r0 += RB) {
      double acc[4][4];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int r = r0 + tr * 4 + a, cc = tc * 4 + c;
          acc[a][c] = r < Rt && cc < w ? bss_entry(q, sc, r, c0 + cc) : 0.0;
        }
      // minus the finished panels: columns [0, c0) of these rows times those of the panel's own rows, slab by slab
      // (the next slab's loads are issued before this slab's arithmetic and land in registers meanwhile)
      const int srow = tid >> 1, skh = (tid & 1) * 8, scol = tid >> 3, sk2 = (tid & 7) * 2;
      const double* ga = r0 + srow < Rt ? A + bss_row(r0 + srow, Mm) + skh : nullptr;
      const double* gb = scol < w ? A + bss_row(c0 + scol, Mm) + sk2 : nullptr;
      double pa[8], pb[2];
      if (c0 > 0) {
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) pa[kk] = ga ? ga[kk] : 0.0;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) pb[kk] = gb ? gb[kk] : 0.0;
      }
      for (int m0 = 0; m0 < c0; m0 += KB) {
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) a_s[skh + kk][srow] = pa[kk];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) b_s[sk2 + kk][scol] = pb[kk];
        __syncthreads();
        if (m0 + KB < c0) {
#pragma unroll
          for (int kk = 0; kk < 8; ++kk) pa[kk] = ga ? ga[m0 + KB + kk] : 0.0;
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) pb[kk] = gb ? gb[m0 + KB + kk] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < KB; ++k) {
          double av[4], bv[4];
#pragma unroll
          for (int a = 0; a < 4; ++a) av[a] = a_s[k][tr * 4 + a];
#pragma unroll
          for (int c = 0; c < 4; ++c) bv[c] = b_s[k][tc * 4 + c];
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[a][c] = fma(-av[a], bv[c], acc[a][c]);
        }
        __syncthreads();
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) s_s[tr * 4 + a][tc * 4 + c] = acc[a][c];
      __syncthreads();
      int first = 0;  // rows of this pass below the diagonal block
      if (r0 == c0) {
        // the w x w diagonal block, column by column (right-looking inside the block) -> d_s
        for (int c = 0; c < w; ++c) {
          const double piv = s_s[c][c];
          if (tid == 0 && !(piv > 0.0 && piv <= 1.79769313486231570815e308)) bad = 1;
          const double l = sqrt(piv);
          if (tid >= c && tid < w) d_s[tid][c] = tid == c ? l : s_s[tid][c] / l;
          __syncthreads();
          for (int e = tid; e < NB * NB; e += CT) {
            const int r = e >> 5, c2 = e & 31;
            if (c2 > c && r >= c2 && r < w) s_s[r][c2] = fma(-d_s[r][c], d_s[c2][c], s_s[r][c2]);
          }
          __syncthreads();
        }
        for (int e = tid; e < NB * NB; e += CT) {
          const int r = e >> 5, c = e & 31;
          if (r < w && c <= r) A[bss_row(c0 + r, Mm) + c0 + c] = d_s[r][c];
        }
        first = w;
      }
      // the rows below: row [c0, c0 + w) = (row - earlier columns of the panel) / diagonal, one thread per row
      if (tid < RB && tid >= first && r0 + tid < Rt) {
        double* srow = s_s[tid];
        double* arow = A + bss_row(r0 + tid, Mm) + c0;
        for (int c = 0; c < w; ++c) {
          double v = srow[c];
          for (int c1 = 0; c1 < c; ++c1) v = fma(-srow[c1], d_s[c][c1], v);
          v /= d_s[c][c];
          srow[c] = v;
          arow[c] = v;
        }
      }
      __syncthreads();  // s_s is rewritten by the next pass; the panel is read back by the next one
    }
  }
  // the quadratic forms: per right-hand side and per reference's F rows, a strided sum and a fixed tree
  double* red = &a_s[0][0];
  double* Qi = Q + (long)b * 32;
  const int nr = whole ? n : 1;
  for (int j = 0; j < n; ++j)
    for (int i = 0; i < nr; ++i) {
      const double* yrow = A + bss_row(Mm + j, Mm) + i * F;
      double v = 0.0;
      for (int k = tid; k < F; k += CT) v = fma(yrow[k], yrow[k], v);
      red[tid] = v;
      for (int s = CT / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s) red[tid] += red[tid + s];
      }
      if (tid == 0) {
        if (whole) Qi[j * 4 + i] = red[0];
        if (!whole || i == 0) Qi[16 + q.i0 * 4 + j] = red[0];
      }
      __syncthreads();
    }
  if (tid == 0 && bad) status[b] = 1;
}

// ---- ratios, dB, permutation ----------------------------------------------------------------------------------------
__device__ inline double bss_db(double num, double den, double clamp) {
  double v = 10.0 * log10(fmax(num, 1e-300) / fmax(den, 1e-300));
  if (clamp > 0.0) v = fmin(clamp, fmax(-clamp, v));
  return v;
}

__global__ __launch_bounds__(CT) void bss_finish_kernel(const double* __restrict__ Q, const double* __restrict__ ee,
                                                        const int* __restrict__ status, const int* __restrict__ perm_in,
                                                        int B, int n, int full, int perm_by, double clamp,
                                                        double* __restrict__ sdr, double* __restrict__ sir,
                                                        double* __restrict__ sar, double* __restrict__ sdr_pairs,
                                                        double* __restrict__ sir_pairs, int* __restrict__ perm_out) {
  const int b = blockIdx.x * CT + threadIdx.x;
  if (b >= B) return;
  const double* Qi = Q + (long)b * 32;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const bool ok = status[b] == 0;
  double S[4][4], I[4][4], A[4];
  for (int j = 0; j < n; ++j) {
    const double e = ee[(long)b * n + j];
    double pall = 0.0;
    if (full)
      for (int i = 0; i < n; ++i) pall += Qi[j * 4 + i];
    A[j] = ok && full ? bss_db(pall, e - pall, clamp) : nan;
    for (int i = 0; i < n; ++i) {
      const double pt = Qi[16 + i * 4 + j];
      S[i][j] = ok ? bss_db(pt, e - pt, clamp) : nan;
      I[i][j] = ok && full ? bss_db(pt, pall - pt, clamp) : nan;
    }
  }
  int best[4] = {0, 1, 2, 3};
  if (perm_in) {
    for (int i = 0; i < n; ++i) best[i] = perm_in[(long)b * n + i];
  } else if (ok) {
    int ncode = 1;  // n^n digit strings, most significant digit sigma(0): the permutations among them come in
    for (int i = 0; i < n; ++i) ncode *= n;  // lexicographic order
    double best_score = 0.0;
    bool have = false;
    for (int code = 0; code < ncode; ++code) {
      int sg[4], used = 0, r = code;
      for (int i = n - 1; i >= 0; --i) {
        sg[i] = r % n;
        r /= n;
      }
      bool isperm = true;
      for (int i = 0; i < n; ++i) {
        if (used & (1 << sg[i])) isperm = false;
        used |= 1 << sg[i];
      }
      if (!isperm) continue;
      double s = 0.0;
      for (int i = 0; i < n; ++i) s += perm_by && full ? I[i][sg[i]] : S[i][sg[i]];
      if (!have || s > best_score) {  // the first candidate is the identity
        have = true;
        best_score = s;
        for (int i = 0; i < n; ++i) best[i] = sg[i];
      }
    }
  }
  for (int i = 0; i < n; ++i) {
    const long o = (long)b * n + i;
    sdr[o] = S[i][best[i]];
    sir[o] = I[i][best[i]];
    sar[o] = A[best[i]];
    perm_out[o] = best[i];
    for (int j = 0; j < n; ++j) {
      sdr_pairs[o * n + j] = S[i][j];
      sir_pairs[o * n + j] = I[i][j];
    }
  }
}

}  // namespace

void launch_bss_corr(const float* ref, const float* est, int n, int L, const int* lens, int F, int item0, int items,
                     const BssPlan& plan, double* part, double* tab, double* ee, hipStream_t s) {
  hipLaunchKernelGGL(bss_corr_kernel, dim3(plan.tiles, plan.jobs, items), dim3(CT), 0, s, ref, est, n, L, lens, F, item0,
                     plan.tiles, part);
  hipLaunchKernelGGL(bss_reduce_kernel, dim3((F + CT - 1) / CT, plan.jobs, items), dim3(CT), 0, s, part, n, L, lens, F,
                     item0, plan.tiles, tab, ee);
}

void launch_bss_solve(const double* tab, int n, int F, int full, double load_diag, int item0, int items,
                      const BssPlan& plan, double* mats, double* Q, int* status, hipStream_t s) {
  hipLaunchKernelGGL(bss_solve_kernel, dim3(n, items), dim3(CT), 0, s, tab, n, F, full, load_diag, plan.mats,
                     plan.mat_full, plan.mat_block, mats, item0, Q, status);
}

void launch_bss_finish(const double* Q, const double* ee, const int* status, const int* perm, int B, int n, int full,
                       int perm_by, double clamp_db, double* sdr, double* sir, double* sar, double* sdr_pairs,
                       double* sir_pairs, int* perm_out, hipStream_t s) {
  hipLaunchKernelGGL(bss_finish_kernel, dim3((B + CT - 1) / CT), dim3(CT), 0, s, Q, ee, status, perm, B, n, full,
                     perm_by, clamp_db, sdr, sir, sar, sdr_pairs, sir_pairs, perm_out);
}
