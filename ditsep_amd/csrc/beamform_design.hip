// Rank-one MVDR and GEV weights for the beamformers (DSN_BEAMFORM_DESIGN_RANK1, DSN_BEAMFORM_DESIGN_GEV; the definition is
// in include/ditsep_hip.h, restated in float64 in tests/beamform_design_restatement.py).  launch_beamform_solve
// (beamform.hip) sends these two designs here; Souden's filter stays in beamform_weights_kernel.  One launch, fp64
// throughout: eight lanes per (item, source, bin) system, eight systems per one-wavefront workgroup.
//   factor   every lane forms A = Q_i + lambda I = L L^H itself (bf_factor, beamform_dev.h: the bits of the Souden
//            launch) and keeps L in registers.
//   whiten   lane c solves L y = N_i[:, c]; the columns of Y = L^-1 N_i go through LDS, lane c takes row c of Y
//            conjugated -- column c of Y^H -- and solves again: column c of G = L^-1 N_i L^-H.  The diagonal is taken as
//            real.
//   Jacobi   G and the accumulated rotations V of a system live in LDS (1 KB each, 16 KB per workgroup).  `sweeps` times,
//            for (p, q), p < q, row by row: every lane reads G_pp, G_qq, G_pq and forms the same rotation
//            J = [[c, s e], [-s conj(e), c]], e = G_pq / |G_pq|; lane l applies it to row l of G and of V (columns p
//            and q change: G J, V J), then to column l of G (rows p and q change: J^H G).  A pair with G_pq = 0 exactly
//            is skipped: the channels an item does not have are never touched.
//   weights  the lane of the reference channel picks the largest diagonal entry mu (ties: the lowest index), u = V[:, m],
//            forms h = L u and v = L^-H u from its registers and writes the design's weights, or e_ref where a pivot or
//            mu is not finite and positive.
// No atomics; nothing depends on the batch position, the padding or the chunking, so an item has the same bits alone.
#include "../../include/ditsep_hip.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

#include "maskrefine_dev.h"

#include "beamform_dev.h"

constexpr int BD_LANES = 8, BD_THREADS = 64, BD_GROUPS = BD_THREADS / BD_LANES;
constexpr double BD_HUGE = 1.7976931348623157e308;
static_assert(BD_LANES == BF_MAX_CH, "lane c owns channel c");

struct BdRot {
  double c, s, er, ei;
};

// the rotation that diagonalises [[a, g], [conj g, b]], g != 0: theta = (b - a) / (2 |g|), t the smaller root of
// t^2 + 2 theta t - 1 = 0 (1 / (2 theta) where theta^2 would overflow), c = 1 / sqrt(1 + t^2), s = t c, e = g / |g|
__device__ __forceinline__ BdRot bd_rotation(double a, double b, double gr, double gi) {
  const double m = hypot(gr, gi);
  const double th = (b - a) / (2.0 * m), ab = fabs(th);
  const double t = ab > 1e150 ? 1.0 / (2.0 * th) : (th < 0.0 ? -1.0 : 1.0) / (ab + sqrt(1.0 + th * th));
  const double c = 1.0 / sqrt(1.0 + t * t);
  return {c, t * c, gr / m, gi / m};
}

// x <- c x - s (e y),  y <- c y + s (conj(e) x), e = er + i ei: the rows p, q of J^H G; with -ei the columns p, q of G J
__device__ __forceinline__ void bd_apply(double c, double s, double er, double ei, double& xr, double& xi, double& yr,
                                         double& yi) {
  const double pr = er * yr - ei * yi, pi = er * yi + ei * yr;   // e y
  const double qr = er * xr + ei * xi, qi = er * xi - ei * xr;   // conj(e) x
  const double nxr = c * xr - s * pr, nxi = c * xi - s * pi;
  yr = c * yr + s * qr;
  yi = c * yi + s * qi;
  xr = nxr;
  xi = nxi;
}

// N [items][classes][2 tri(C)][bins] -> w [items][n][bins][C] complex doubles, as beamform_weights_kernel.  Thread
// (g, lane) of a workgroup: system blockIdx.x BD_GROUPS + g = (item, source, bin), channel `lane`.
__global__ __launch_bounds__(BD_THREADS) void beamform_design_kernel(const double* __restrict__ N,
                                                                     const int* __restrict__ chans, int ref, int items,
                                                                     int n, int classes, int C, int bins, double reg,
                                                                     double eps, int design, int sweeps,
                                                                     double* __restrict__ w) {
  __shared__ double Gr[BD_GROUPS][BD_LANES][BD_LANES], Gi[BD_GROUPS][BD_LANES][BD_LANES];
  __shared__ double Vr[BD_GROUPS][BD_LANES][BD_LANES], Vi[BD_GROUPS][BD_LANES][BD_LANES];
  const int lane = threadIdx.x % BD_LANES, g = threadIdx.x / BD_LANES;
  const long sys = (long)blockIdx.x * BD_GROUPS + g, total = (long)items * n * bins;
  const bool live = sys < total;
  const long e = live ? sys : total - 1;   // (a spare group repeats the last system and writes nothing)
  const int j = (int)(e % bins), i = (int)(e / bins % n), b = (int)(e / bins / n);
  const int Cb = chans ? chans[b] : C;
  const int T2 = 2 * bf_tri(C);
  const double* Nb = N + (long)b * classes * T2 * bins + j;   // entry u of class s: Nb[(s T2 + u) bins]

  double ar[BF_TRI], ai[BF_TRI];
  bf_factor(Nb, i, classes, C, Cb, bins, reg, eps, ar, ai);
  bool ok = true;
#pragma unroll
  for (int c = 0; c < BF_MAX_CH; ++c) {
    const double l = ar[c * (c + 1) / 2 + c];
    ok = ok && l > 0.0 && l <= BD_HUGE;   // finite and positive (false for NaN)
  }
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
  bf_forward(ar, ai, zr, zi);   // column `lane` of Y = L^-1 N_i
#pragma unroll
  for (int r = 0; r < BF_MAX_CH; ++r) {
    Gr[g][r][lane] = zr[r];
    Gi[g][r][lane] = zi[r];
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < BF_MAX_CH; ++r) {   // row `lane` of Y conjugated: column `lane` of Y^H
    zr[r] = Gr[g][lane][r];
    zi[r] = -Gi[g][lane][r];
  }
  __syncthreads();
  bf_forward(ar, ai, zr, zi);   // column `lane` of G = L^-1 Y^H
#pragma unroll
  for (int r = 0; r < BF_MAX_CH; ++r) {
    Gr[g][r][lane] = zr[r];
    Gi[g][r][lane] = r == lane ? 0.0 : zi[r];
    Vr[g][r][lane] = r == lane ? 1.0 : 0.0;
    Vi[g][r][lane] = 0.0;
  }
  __syncthreads();

  for (int sw = 0; sw < sweeps; ++sw)
    for (int p = 0; p < BD_LANES - 1; ++p)
      for (int q = p + 1; q < BD_LANES; ++q) {
        const double a = Gr[g][p][p], d = Gr[g][q][q], gr = Gr[g][p][q], gi = Gi[g][p][q];
        const bool rot = gr != 0.0 || gi != 0.0;   // (true for NaN, which then spreads and ends in the fallback)
        BdRot R{1.0, 0.0, 1.0, 0.0};
        if (rot) R = bd_rotation(a, d, gr, gi);
        __syncthreads();   // every lane has read the pair before its rows change
        if (rot) {         // columns p, q of row `lane`: G J and V J
          bd_apply(R.c, R.s, R.er, -R.ei, Gr[g][lane][p], Gi[g][lane][p], Gr[g][lane][q], Gi[g][lane][q]);
          bd_apply(R.c, R.s, R.er, -R.ei, Vr[g][lane][p], Vi[g][lane][p], Vr[g][lane][q], Vi[g][lane][q]);
        }
        __syncthreads();
        if (rot)           // rows p, q of column `lane`: J^H G
          bd_apply(R.c, R.s, R.er, R.ei, Gr[g][p][lane], Gi[g][p][lane], Gr[g][q][lane], Gi[g][q][lane]);
        __syncthreads();
      }

  if (!live || lane != ref) return;
  int m = 0;
  double mu = Gr[g][0][0];
  for (int c = 1; c < BD_LANES; ++c)
    if (Gr[g][c][c] > mu) mu = Gr[g][c][c], m = c;
  ok = ok && mu > 0.0 && mu <= BD_HUGE;
  double ur[BF_MAX_CH], ui[BF_MAX_CH], vr[BF_MAX_CH], vi[BF_MAX_CH];
#pragma unroll
  for (int r = 0; r < BF_MAX_CH; ++r) {
    vr[r] = ur[r] = Vr[g][r][m];
    vi[r] = ui[r] = Vi[g][r][m];
  }
  bf_backward(ar, ai, vr, vi);   // v = L^-H u
  // h = L u, the steering estimate; h_ref and |h|^2 over the item's channels in channel order
  double fr = 0.0, fi = 0.0, hh = 0.0;
#pragma unroll
  for (int r = 0; r < BF_MAX_CH; ++r) {
    const int pr = r * (r + 1) / 2;
    double sr = 0.0, si = 0.0;
#pragma unroll
    for (int k = 0; k <= r; ++k) {
      sr += ar[pr + k] * ur[k] - ai[pr + k] * ui[k];
      si += ar[pr + k] * ui[k] + ai[pr + k] * ur[k];
    }
    if (r == ref) fr = sr, fi = si;
    if (r < Cb) hh += sr * sr + si * si;
  }
  // the factor every v_c is multiplied with: conj(h_ref), or its phase times |h| / sqrt(Cb)
  double kr = fr, ki = -fi, scale = 1.0;
  if (design == DSN_BEAMFORM_DESIGN_GEV) {
    const double ma = hypot(fr, fi);
    kr = ma > 0.0 ? fr / ma : 1.0;
    ki = ma > 0.0 ? -fi / ma : 0.0;
    scale = sqrt(hh) / sqrt((double)Cb);
  }
  double* wo = w + 2L * e * C;
#pragma unroll
  for (int c = 0; c < BF_MAX_CH; ++c)
    if (c < C) {
      double wr = 0.0, wi = 0.0;
      if (c < Cb) {
        wr = c == ref ? 1.0 : 0.0;
        if (ok && Cb > 1) {
          wr = (vr[c] * kr - vi[c] * ki) * scale;
          wi = (vr[c] * ki + vi[c] * kr) * scale;
        }
      }
      wo[2 * c] = wr;
      wo[2 * c + 1] = wi;
    }
}

}  // namespace

void launch_beamform_design(const double* N, const int* chans, int ref, double* w, int items, int C, int n, int classes,
                            int bins, double reg, double eps, int design, int sweeps, hipStream_t st) {
  const long systems = (long)items * n * bins;
  hipLaunchKernelGGL(beamform_design_kernel, dim3((unsigned)((systems + BD_GROUPS - 1) / BD_GROUPS)), dim3(BD_THREADS), 0,
                     st, N, chans, ref, items, n, classes, C, bins, reg, eps, design, sweeps, w);
}
