// Ensemble combine (dsn_ensemble_combine): K candidate separations [B][K][n][Lmax] of the same mixtures -> one
// [B][n][Lmax], the candidates permutation-aligned to an anchor first.  include/ditsep_hip.h states the definition;
// tests/ensemble_restatement.py restates it in float64.  Three launches:
//   ens_gram_kernel    per (tile of ENS_TILE samples counted from the item's own start, item): the Gram of the item's
//                      R = K n candidate rows (+ the mixture row) over the tile, as 4 x 4 blocks of row pairs on and
//                      above the diagonal.  The rows pass through LDS in sub-tiles; a thread owns one block (16 fp64
//                      accumulators fed by 8 16-byte LDS reads per 64 multiply-adds) and, of the sub-tile's quads of
//                      samples, those congruent to its lane g modulo S -- S lanes share a block.  fp32 x fp32 products
//                      are exact in fp64, so fma is mul + add here; they are summed per thread in stride order, then
//                      across the S lanes by a fixed shuffle tree (S = 256, one block: the four wave sums in LDS added
//                      in order), one plain store per (tile, block, entry).
//   ens_solve_kernel   one workgroup per item: adds the item's own tile partials in index order into G (LDS), one
//                      thread per (a, k) searches the n! permutations in lexicographic order, one thread picks the
//                      anchor and `best`, then the info figures, all from G in fp64.
//   ens_gather_kernel  the combine, four consecutive samples per thread, fp32 with contraction off: the value does not
//                      depend on the load path taken.
// The global-to-LDS copy of the Gram takes 16-byte loads when the rows allow and guarded scalar loads otherwise; which
// thread multiplies which sample is the same on both, so the bits do not depend on the path.  Nothing at or past
// lens[b] is read.  No atomics anywhere: reruns are bit-identical.  Index arithmetic is 64-bit.
#include "../../include/ditsep_hip.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int ETPB = 256;
constexpr int ENS_LDS_FLOATS = 9216;   // 36 KB: the largest of RP (4 SUBQ + 4) over the plans ensemble_gram_plan makes
constexpr int ENS_RP_MAX = 68;         // 65 rows padded to whole blocks of 4

struct EnsShape {
  int K, n, Rc, R, RB, NB, S, SUBQ, Lmax, tiles;
};

__device__ __forceinline__ const float* ens_row(const EnsShape& q, const float* __restrict__ cands,
                                                const float* __restrict__ mix, long b, int r) {
  return r < q.Rc ? cands + (b * q.Rc + r) * (long)q.Lmax : mix + b * (long)q.Lmax;
}

// grid (x: tile, y: item).  part [B][tiles][NB][16]
__global__ void __launch_bounds__(ETPB) ens_gram_kernel(const EnsShape q, const float* __restrict__ cands,
                                                        const float* __restrict__ mix, const int* __restrict__ lens,
                                                        double* __restrict__ part, int vec) {
  __shared__ __align__(16) float xs[ENS_LDS_FLOATS];   // rows of 4 SUBQ + 4 floats: 16-byte reads, one access of padding
  const long b = blockIdx.y;
  const int c = blockIdx.x, tid = threadIdx.x;
  const int len = lens ? lens[b] : q.Lmax;
  const int t0 = c * ENS_TILE;
  if (t0 >= len) return;   // (not one of the item's own tiles: ens_solve_kernel does not read its partial)
  const int RP = 4 * q.RB, pitch = 4 * q.SUBQ + 4;
  const int blk = tid / q.S, g = tid % q.S;
  int bi = 0, bj = blk;    // block `blk` of the upper triangle, rows 4 bi .., columns 4 bj ..
  while (bi < q.RB && bj >= q.RB - bi) {
    bj -= q.RB - bi;
    ++bi;
  }
  bj += bi;
  const bool live = blk < q.NB;
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
  for (int s0 = t0; s0 < t0 + ENS_TILE && s0 < len; s0 += 4 * q.SUBQ) {
    for (int idx = tid; idx < RP * q.SUBQ; idx += ETPB) {
      const int r = idx / q.SUBQ, qd = idx % q.SUBQ;
      const int t = s0 + 4 * qd;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < q.R && t < len) {
        const float* row = ens_row(q, cands, mix, b, r);
        if (vec && t + 3 < len) {
          v = *reinterpret_cast<const float4*>(row + t);
        } else {
          v.x = row[t];
          if (t + 1 < len) v.y = row[t + 1];
          if (t + 2 < len) v.z = row[t + 2];
          if (t + 3 < len) v.w = row[t + 3];
        }
      }
      *reinterpret_cast<float4*>(xs + r * pitch + 4 * qd) = v;
    }
    __syncthreads();
    if (live) {
      const float* xa = xs + 4 * bi * pitch;
      const float* xb = xs + 4 * bj * pitch;
      for (int qd = g; qd < q.SUBQ; qd += q.S) {
        float4 av[4], bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) av[i] = *reinterpret_cast<const float4*>(xa + i * pitch + 4 * qd);
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[j] = *reinterpret_cast<const float4*>(xb + j * pitch + 4 * qd);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            acc[i][j] = fma((double)av[i].x, (double)bv[j].x, acc[i][j]);
            acc[i][j] = fma((double)av[i].y, (double)bv[j].y, acc[i][j]);
            acc[i][j] = fma((double)av[i].z, (double)bv[j].z, acc[i][j]);
            acc[i][j] = fma((double)av[i].w, (double)bv[j].w, acc[i][j]);
          }
      }
    }
    __syncthreads();
  }
  // the S lanes of a block are neighbours inside one wave (S <= 64), or the whole workgroup (S = 256, one block)
  const int width = q.S < 64 ? q.S : 64;
  double* red = reinterpret_cast<double*>(xs);   // [16][4], S = 256 only (the last barrier freed xs)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double v = acc[i][j];
      for (int off = width >> 1; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      acc[i][j] = v;
      if (q.S > 64 && (tid & 63) == 0) red[(i * 4 + j) * 4 + (tid >> 6)] = v;
    }
  double* dst = part + ((b * q.tiles + c) * q.NB) * 16;
  if (q.S > 64) {
    __syncthreads();
    if (tid < 16) dst[tid] = ((red[tid * 4] + red[tid * 4 + 1]) + red[tid * 4 + 2]) + red[tid * 4 + 3];
    return;
  }
  if (live && g == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) dst[blk * 16 + i * 4 + j] = acc[i][j];
  }
}

// The best permutation of candidate k's sources onto candidate a's: sigma maximising sum_i G[(a, i)][(k, sigma(i))],
// the n^n digit strings in order (most significant digit sigma(0)): the permutations among them come in lexicographic
// order, strictly greater replaces.  -> the score, sigma in best[0 .. n)
__device__ double ens_assign(const double* G, int RP, int n, int a, int k, int* best) {
  int ncode = 1;
  for (int i = 0; i < n; ++i) ncode *= n;
  double best_score = 0.0;
  bool have = false;
  for (int i = 0; i < 4; ++i) best[i] = i;
  for (int code = 0; code < ncode; ++code) {
    int sg[4], used = 0, r = code;
    for (int i = n - 1; i >= 0; --i) {
      sg[i] = r % n;
      r /= n;
    }
    bool ok = true;
    for (int i = 0; i < n; ++i) {
      if (used & (1 << sg[i])) ok = false;
      used |= 1 << sg[i];
    }
    if (!ok) continue;
    double sc = 0.0;
    for (int i = 0; i < n; ++i) sc += G[(a * n + i) * RP + k * n + sg[i]];
    if (!have || sc > best_score) {   // the first candidate is the identity
      have = true;
      best_score = sc;
      for (int i = 0; i < n; ++i) best[i] = sg[i];
    }
  }
  return best_score;
}

// grid (item).  perm [B][K][n], anchor / best [B], resid_db [B][K], agree_db [B][K][n], gram [B][R][R]
__global__ void __launch_bounds__(ETPB) ens_solve_kernel(const EnsShape q, const int* __restrict__ lens,
                                                         const double* __restrict__ part, double* __restrict__ gram,
                                                         int* __restrict__ perm, int* __restrict__ anchor,
                                                         int* __restrict__ best, double* __restrict__ resid_db,
                                                         double* __restrict__ agree_db, int has_mix) {
  __shared__ double G[ENS_RP_MAX * ENS_RP_MAX];
  __shared__ double Sc[16][16];
  __shared__ double Ek[16];
  __shared__ unsigned char Pm[16][16][4];
  __shared__ int sel[2];
  const long b = blockIdx.x;
  const int tid = threadIdx.x, K = q.K, n = q.n, R = q.R, RP = 4 * q.RB;
  const int len = lens ? lens[b] : q.Lmax;
  const int own = (len + ENS_TILE - 1) / ENS_TILE;   // the item's own tiles
  for (int e = tid; e < q.NB * 16; e += ETPB) {
    const int blk = e / 16, i = (e % 16) / 4, j = e % 4;
    int bi = 0, bj = blk;
    while (bj >= q.RB - bi) {
      bj -= q.RB - bi;
      ++bi;
    }
    bj += bi;
    double s = 0.0;
    for (int c = 0; c < own; ++c) s += part[((b * q.tiles + c) * q.NB + blk) * 16 + (e % 16)];
    const int p = 4 * bi + i, r = 4 * bj + j;
    G[p * RP + r] = s;
    if (bi != bj) G[r * RP + p] = s;   // (a diagonal block holds both halves, formed from the same products in order)
  }
  __syncthreads();
  for (int e = tid; e < R * R; e += ETPB) gram[b * R * R + e] = G[(e / R) * RP + e % R];
  if (tid < K * K) {
    const int a = tid / K, k = tid % K;
    int sg[4];
    Sc[a][k] = ens_assign(G, RP, n, a, k, sg);
    for (int i = 0; i < 4; ++i) Pm[a][k][i] = (unsigned char)sg[i];
  }
  const int m = q.Rc;   // the mixture's row
  if (has_mix && tid < K) {
    double cross = 0.0, self = 0.0;
    for (int i = 0; i < n; ++i) cross += G[m * RP + tid * n + i];
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) self += G[(tid * n + i) * RP + tid * n + j];
    Ek[tid] = (G[m * RP + m] - 2.0 * cross) + self;
  }
  __syncthreads();
  if (tid == 0) {
    int a_best = 0;
    double s_best = 0.0;
    for (int a = 0; a < K; ++a) {
      double s = 0.0;
      for (int k = 0; k < K; ++k)
        if (k != a) s += a < k ? Sc[a][k] : Sc[k][a];   // (S is symmetric: the one formed for a < k serves both)
      if (a == 0 || s > s_best) {
        a_best = a;
        s_best = s;
      }
    }
    int k_best = -1;
    if (has_mix) {
      k_best = 0;
      for (int k = 1; k < K; ++k)
        if (Ek[k] < Ek[k_best]) k_best = k;
    }
    sel[0] = a_best;
    sel[1] = k_best;
    anchor[b] = a_best;
    best[b] = k_best;
  }
  __syncthreads();
  const int as = sel[0];
  if (tid < K) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double v = nan;
    if (has_mix) v = 10.0 * log10((Ek[tid] > 0.0 ? Ek[tid] : 0.0) / G[m * RP + m]);
    resid_db[b * K + tid] = v;
  }
  if (tid < K * n) {
    const int k = tid / n, i = tid % n;
    const int s = k == as ? i : Pm[as][k][i];
    perm[(b * K + k) * n + i] = s;
    const int ra = as * n + i, rc = k * n + s;
    const double gaa = G[ra * RP + ra], gcc = G[rc * RP + rc], g = G[ra * RP + rc];
    double v;
    if (gaa == 0.0 || gcc == 0.0) {
      v = __longlong_as_double(0x7ff8000000000000LL);
    } else if (k == as) {
      v = __longlong_as_double(0x7ff0000000000000LL);
    } else {
      const double g2 = g * g, den = gaa * gcc - g2;
      v = 10.0 * log10(g2 / (den > 0.0 ? den : 0.0));
    }
    agree_db[(b * K + k) * n + i] = v;
  }
}

// compare-exchange of neighbours, strictly greater swaps: a stable sort, so equal values (+0 and -0) keep their
// candidate order
__device__ __forceinline__ void ens_cx(float& a, float& b) {
  const bool sw = b < a;
  const float lo = sw ? b : a, hi = sw ? a : b;
  a = lo;
  b = hi;
}

template <int K>
__device__ __forceinline__ float ens_median(float (&v)[K]) {
#pragma unroll
  for (int pass = 0; pass < K - 1; ++pass)
#pragma unroll
    for (int j = 0; j + 1 < K - pass; ++j) ens_cx(v[j], v[j + 1]);
  if (K % 2) return v[K / 2];
  return (v[(K - 1) / 2] + v[K / 2]) * 0.5f;
}

// Row (k, perm[k][i]) of item b: candidate k's source in slot i.
__device__ __forceinline__ const float* ens_slot(const EnsShape& q, const float* __restrict__ cands,
                                                 const int* __restrict__ perm, long b, int k, int i) {
  return cands + ((b * q.K + k) * q.n + perm[(b * q.K + k) * q.n + i]) * (long)q.Lmax;
}

// acc <- fl(acc + x); err collects what that addition rounded off.  Knuth's two-sum: acc + x = fl(acc + x) + d with d
// a float32 that the six operations get exactly, whatever the magnitudes (contraction is off and there is nothing to
// contract).  The mean is the candidates added in candidate order this way, then ens_sum(acc, err) / float(K): the
// sequential float32 sum with its own rounding errors given back.  K copies of x: every partial sum and every d is a
// multiple of ulp(x) and the d's add up to less than 2^7 ulp(x), so err is exact, acc + err is K x, and for K a power
// of two K x and K x / K are floats -- the mean of 2, 4, 8 or 16 copies is the copy, which the bare sequential sum
// does not give from K = 8 (5 x, 6 x, 7 x each round).
__device__ __forceinline__ void ens_add(float& acc, float& err, float x) {
  const float t = acc + x;
  const float xv = t - acc;
  const float av = t - xv;
  err = err + ((acc - av) + (x - xv));
  acc = t;
}

// acc + err; with nothing rounded off acc itself, so that a sum of -0's keeps its sign as the bare sum does.
__device__ __forceinline__ float ens_sum(float acc, float err) { return err != 0.f ? acc + err : acc; }

// One sample of slot i.  KM > 0: the median of candidates 0 .. KM - 1.  KM = 0: candidates first .. first + count - 1
// added in that order by ens_add and divided by float(count) -- the mean (first = 0, count = K), or with count = 1 a
// copy.
template <int KM>
__device__ __forceinline__ float ens_sample(const EnsShape& q, const float* __restrict__ cands,
                                            const int* __restrict__ perm, long b, int i, int first, int count, int t) {
  if (KM > 0) {
    float v[KM > 0 ? KM : 1];
#pragma unroll
    for (int k = 0; k < KM; ++k) v[k] = ens_slot(q, cands, perm, b, k, i)[t];
    return ens_median(v);
  }
  float acc = ens_slot(q, cands, perm, b, first, i)[t], err = 0.f;
  for (int k = 1; k < count; ++k) ens_add(acc, err, ens_slot(q, cands, perm, b, first + k, i)[t]);
  return count > 1 ? ens_sum(acc, err) / (float)count : acc;
}

// grid (x: groups of 4 * ETPB samples, y: source slot, z: item).  Each thread writes 4 consecutive samples t0 .. t0 + 3,
// t0 % 4 == 0; vload (Lmax a multiple of 4, aligned base): every read is a 16-byte load; vstore likewise.  pick [B]
// (best, medoid): the one candidate that is copied; null: all K.
template <int KM>
__global__ void __launch_bounds__(ETPB) ens_gather_kernel(const EnsShape q, const float* __restrict__ cands,
                                                          const int* __restrict__ lens, const int* __restrict__ perm,
                                                          const int* __restrict__ pick, float* __restrict__ out,
                                                          int vload, int vstore) {
  const int i = blockIdx.y;
  const long b = blockIdx.z;
  const long t0l = ((long)blockIdx.x * ETPB + threadIdx.x) * 4;
  if (t0l >= q.Lmax) return;
  const int t0 = (int)t0l, len = lens ? lens[b] : q.Lmax;
  float* dst = out + (b * q.n + i) * (long)q.Lmax + t0;
  const int first = pick ? pick[b] : 0, count = pick ? 1 : q.K;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (t0 + 3 < len && vload) {
    if (KM > 0) {
      constexpr int NR = KM > 0 ? KM : 1;
      float x[NR], y[NR], z[NR], w[NR];
#pragma unroll
      for (int k = 0; k < NR; ++k) {
        const float4 c = *reinterpret_cast<const float4*>(ens_slot(q, cands, perm, b, k, i) + t0);
        x[k] = c.x;
        y[k] = c.y;
        z[k] = c.z;
        w[k] = c.w;
      }
      v.x = ens_median(x);
      v.y = ens_median(y);
      v.z = ens_median(z);
      v.w = ens_median(w);
    } else {
      v = *reinterpret_cast<const float4*>(ens_slot(q, cands, perm, b, first, i) + t0);
      float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int k = 1; k < count; ++k) {
        const float4 c = *reinterpret_cast<const float4*>(ens_slot(q, cands, perm, b, first + k, i) + t0);
        ens_add(v.x, e.x, c.x);
        ens_add(v.y, e.y, c.y);
        ens_add(v.z, e.z, c.z);
        ens_add(v.w, e.w, c.w);
      }
      if (count > 1) {
        const float d = (float)count;
        v.x = ens_sum(v.x, e.x) / d;
        v.y = ens_sum(v.y, e.y) / d;
        v.z = ens_sum(v.z, e.z) / d;
        v.w = ens_sum(v.w, e.w) / d;
      }
    }
  } else {
    if (t0 < len) v.x = ens_sample<KM>(q, cands, perm, b, i, first, count, t0);
    if (t0 + 1 < len) v.y = ens_sample<KM>(q, cands, perm, b, i, first, count, t0 + 1);
    if (t0 + 2 < len) v.z = ens_sample<KM>(q, cands, perm, b, i, first, count, t0 + 2);
    if (t0 + 3 < len) v.w = ens_sample<KM>(q, cands, perm, b, i, first, count, t0 + 3);
  }
  if (t0l + 3 < q.Lmax) {
    if (vstore) {
      *reinterpret_cast<float4*>(dst) = v;
    } else {
      dst[0] = v.x;
      dst[1] = v.y;
      dst[2] = v.z;
      dst[3] = v.w;
    }
    return;
  }
  const float e[4] = {v.x, v.y, v.z, v.w};
  for (int t = t0; t < q.Lmax; ++t) dst[t - t0] = e[t - t0];
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

EnsShape ens_shape(int K, int n, int Lmax, bool has_mix) {
  EnsShape q;
  q.K = K;
  q.n = n;
  q.Rc = K * n;
  q.R = q.Rc + (has_mix ? 1 : 0);
  q.Lmax = Lmax;
  q.tiles = ensemble_tiles(Lmax);
  ensemble_gram_plan(q.R, &q.RB, &q.NB, &q.S, &q.SUBQ);
  return q;
}

template <int KM>
void gather_launch(const EnsShape& q, const float* cands, const int* lens, const int* perm, const int* pick, float* out,
                   int B, hipStream_t s) {
  const int v = q.Lmax % 4 == 0;
  const long per = 4L * ETPB;
  const dim3 grid((unsigned)((q.Lmax + per - 1) / per), (unsigned)q.n, (unsigned)B);
  hipLaunchKernelGGL((ens_gather_kernel<KM>), grid, dim3(ETPB), 0, s, q, cands, lens, perm, pick, out,
                     v && aligned16(cands), v && aligned16(out));
}

}  // namespace

// R rows as RB x RB blocks of 4 x 4 pairs, NB of them on and above the diagonal; S lanes share a block (the largest
// power of two with NB S <= 256); SUBQ quads of samples per LDS sub-tile (a multiple of S that divides ENS_TILE / 4).
void ensemble_gram_plan(int R, int* RB, int* NB, int* S, int* SUBQ) {
  *RB = (R + 3) / 4;
  *NB = *RB * (*RB + 1) / 2;
  int s = 1;
  while (2 * s * *NB <= ETPB) s *= 2;
  *S = s;
  int sub = 4 * s;
  if (sub < 32) sub = 32;
  if (sub > ENS_TILE / 4) sub = ENS_TILE / 4;
  *SUBQ = sub;
}

void launch_ensemble_gram(const float* cands, const float* mix, const int* lens, double* part, int B, int K, int n,
                          int Lmax, hipStream_t s) {
  const EnsShape q = ens_shape(K, n, Lmax, mix != nullptr);
  const int vec = Lmax % 4 == 0 && aligned16(cands) && (!mix || aligned16(mix));
  hipLaunchKernelGGL(ens_gram_kernel, dim3((unsigned)q.tiles, (unsigned)B), dim3(ETPB), 0, s, q, cands, mix, lens, part,
                     vec);
}

void launch_ensemble_solve(const int* lens, const double* part, double* gram, int* perm, int* anchor, int* best,
                           double* resid_db, double* agree_db, int B, int K, int n, int Lmax, int has_mix,
                           hipStream_t s) {
  const EnsShape q = ens_shape(K, n, Lmax, has_mix != 0);
  hipLaunchKernelGGL(ens_solve_kernel, dim3((unsigned)B), dim3(ETPB), 0, s, q, lens, part, gram, perm, anchor, best,
                     resid_db, agree_db, has_mix);
}

void launch_ensemble_gather(const float* cands, const int* lens, const int* perm, const int* anchor, const int* best,
                            float* out, int B, int K, int n, int Lmax, int mode, hipStream_t s) {
  const EnsShape q = ens_shape(K, n, Lmax, false);
  if (mode != DSN_ENSEMBLE_MEDIAN) {
    const int* pick = mode == DSN_ENSEMBLE_BEST ? best : mode == DSN_ENSEMBLE_MEDOID ? anchor : nullptr;
    gather_launch<0>(q, cands, lens, perm, pick, out, B, s);
    return;
  }
  switch (K) {
#define ENS_MEDIAN_CASE(k) \
  case k: gather_launch<k>(q, cands, lens, perm, nullptr, out, B, s); break;
    ENS_MEDIAN_CASE(1) ENS_MEDIAN_CASE(2) ENS_MEDIAN_CASE(3) ENS_MEDIAN_CASE(4) ENS_MEDIAN_CASE(5) ENS_MEDIAN_CASE(6)
    ENS_MEDIAN_CASE(7) ENS_MEDIAN_CASE(8) ENS_MEDIAN_CASE(9) ENS_MEDIAN_CASE(10) ENS_MEDIAN_CASE(11)
    ENS_MEDIAN_CASE(12) ENS_MEDIAN_CASE(13) ENS_MEDIAN_CASE(14) ENS_MEDIAN_CASE(15) ENS_MEDIAN_CASE(16)
#undef ENS_MEDIAN_CASE
    default: break;
  }
}
