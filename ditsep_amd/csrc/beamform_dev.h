// The statistics, the loaded factorisation and the channel contraction of the MVDR beamformers, dsn_beamform
// (beamform.hip, beamform_design.hip) and dsn_beamform_track (beamform_track.hip): M_src X X^H summed in frame order over
// a range of frames by one workgroup (bf_stats_frames), A = Q_i + lambda I = L L^H with its two triangular solves
// (bf_factor, bf_forward, bf_backward) and Y = sum_c conj(w_c) X_c of one frame and pair of bins (bf_contract).  The
// files call exactly these functions, floating point contraction off, so a range of frames, a factor and a weight have
// the same bits in each.
// Include it inside the file's own unnamed namespace, after maskrefine_dev.h.
#pragma once

constexpr int BF_MAX_CH = BEAMFORM_MAX_CH;
constexpr int BF_TRI = BF_MAX_CH * (BF_MAX_CH + 1) / 2;                          // Hermitian entries held in registers
constexpr int BF_BF = (BF_MAX_CH + MR_MAX_SRC) * (MR_POINTS / 2) / MRT;          // butterflies per thread and stage

__host__ __device__ inline int bf_tri(int C) { return C * (C + 1) / 2; }
// entry (c1 <= c2) of the upper triangle of a C x C matrix, row after row
__host__ __device__ inline int bf_idx(int C, int c1, int c2) { return c1 * C - c1 * (c1 - 1) / 2 + (c2 - c1); }

// Source `src`, bin j: rows [R0, R1) of M_src X X^H (upper triangle, X_c1 conj X_c2) of the `frames` frames in LDS,
// added to acc in frame order.  Products and sums in fp64 on the widened fp32 spectra and masks.
template <int H, int R0, int R1>
__device__ __forceinline__ void bf_accumulate(const MaskRefineShape& q, const float2* buf, const float2* tw, int Cb,
                                              int src, int j, int frames, double (&acc)[BF_TRI][2]) {
  const bool lower = 2 * j <= H;
  const int k = lower ? j : H - j, km = (H - k) & (H - 1);
  const float2 t = tw[k];
  for (int fg = 0; fg < frames; ++fg) {
    double xr[BF_MAX_CH], xi[BF_MAX_CH];
#pragma unroll
    for (int c = 0; c < BF_MAX_CH; ++c) {
      xr[c] = xi[c] = 0.0;
      if (c < Cb) {
        const float2* a = buf + c * MR_POINTS + fg * H;
        float2 xk, xm;
        mr_split(a[k], a[km], t, xk, xm);
        xr[c] = lower ? xk.x : xm.x;
        xi[c] = lower ? xk.y : xm.y;
      }
    }
    float mk[MR_MAX_SRC], mm[MR_MAX_SRC];
    mr_masks(q, buf + Cb * MR_POINTS + fg * H, k, km, t, mk, mm);
    float mi = 0.f;
#pragma unroll
    for (int s = 0; s < MR_MAX_SRC; ++s)
      if (s == src) mi = lower ? mk[s] : mm[s];
    const double m = mi;
#pragma unroll
    for (int c1 = R0; c1 < R1; ++c1)
#pragma unroll
      for (int c2 = c1; c2 < BF_MAX_CH; ++c2)
        if (c2 < Cb) {
          const int u = c1 * BF_MAX_CH - c1 * (c1 - 1) / 2 + (c2 - c1);
          acc[u][0] += m * (xr[c1] * xr[c2] + xi[c1] * xi[c2]);
          acc[u][1] += m * (xi[c1] * xr[c2] - xr[c1] * xi[c2]);
        }
  }
}

// Bin j >= 256 of one frame group: rows [R0, R1) summed over the group in registers, then added to the owner's partial.
template <int H, int R0, int R1>
__device__ __forceinline__ void bf_high_bin(const MaskRefineShape& q, const float2* buf, const float2* tw, int Cb,
                                            int src, int j, int frames, bool first, double* __restrict__ partw) {
  double acc[BF_TRI][2];
#pragma unroll
  for (int u = 0; u < BF_TRI; ++u) acc[u][0] = acc[u][1] = 0.0;
  bf_accumulate<H, R0, R1>(q, buf, tw, Cb, src, j, frames, acc);
#pragma unroll
  for (int c1 = R0; c1 < R1; ++c1)
#pragma unroll
    for (int c2 = c1; c2 < BF_MAX_CH; ++c2)
      if (c2 < Cb) {
        const int u = c1 * BF_MAX_CH - c1 * (c1 - 1) / 2 + (c2 - c1);
        double* d = partw + 2L * bf_idx(q.C, c1, c2) * (H + 1) + j;
        d[0] = first ? acc[u][0] : d[0] + acc[u][0];
        d[H + 1] = first ? acc[u][1] : d[H + 1] + acc[u][1];
      }
}

// The frames f_first .. f_last of item `it` for source `src`, by the whole workgroup: partw [2 tri(C)][H + 1] receives
// sum_t M_src X X^H in frame order, whatever the grouping (entries of channels >= Cb are not written).
// Dynamic LDS: float2 tw[H] | float2 buf[C + n][G][H] | float win[NFFT]
// A thread owns bin `tid` for the whole range and keeps that bin's sums of its one source in registers over all the
// frames (36 complex doubles at C = 8: one source is what the registers hold, so the source is in the grid and the
// transforms are formed once per source); they are stored once at the end.  Bins 256 and up (n_fft >= 512) are added
// a frame group at a time into the partial in global memory, by the same thread every group.
template <int NFFT>
__device__ __forceinline__ void bf_stats_frames(const MaskRefineShape& q, const float* mixb, const float* estb,
                                                const MrItem& it, int Cb, int src, int f_first, int f_last,
                                                double* __restrict__ partw) {
  constexpr int H = NFFT / 2, G = MR_POINTS / H;
  extern __shared__ __attribute__((aligned(16))) float2 bf_lds[];
  const int n = q.n, hop = q.hop, tid = threadIdx.x;
  float2* tw = bf_lds;
  float2* buf = tw + H;
  float* win = reinterpret_cast<float*>(buf + (q.C + n) * MR_POINTS);
  mr_tables<H>(tw, win, tid);
  double own[BF_TRI][2];
#pragma unroll
  for (int u = 0; u < BF_TRI; ++u) own[u][0] = own[u][1] = 0.0;

  for (int f0 = f_first; f0 <= f_last; f0 += G) {
    __syncthreads();   // the tables are in; the previous group's spectra have been read
    mr_load<H>(buf, win, mixb, estb, q.Lmax, it, hop, Cb, n, f0, f_last, tid);
    __syncthreads();
    mr_fft<H, false, BF_BF>(buf, tw, (Cb + n) * (MR_POINTS / 2), tid);
    const int frames = min(G, f_last - f0 + 1);
    if (tid <= H) bf_accumulate<H, 0, BF_MAX_CH>(q, buf, tw, Cb, src, tid, frames, own);
    if (H + 1 > MRT)
      for (int j = tid + MRT; j <= H; j += MRT) {   // (in two halves of the triangle: `own` stays in registers)
        bf_high_bin<H, 0, 3>(q, buf, tw, Cb, src, j, frames, f0 == f_first, partw);
        bf_high_bin<H, 3, BF_MAX_CH>(q, buf, tw, Cb, src, j, frames, f0 == f_first, partw);
      }
  }
  if (tid <= H) {
    int u = 0;
#pragma unroll
    for (int c1 = 0; c1 < BF_MAX_CH; ++c1)
#pragma unroll
      for (int c2 = c1; c2 < BF_MAX_CH; ++c2, ++u)
        if (c2 < Cb) {
          double* d = partw + 2L * bf_idx(q.C, c1, c2) * (H + 1) + tid;
          d[0] = own[u][0];
          d[H + 1] = own[u][1];
        }
  }
}

// Source i, one bin (Nb: entry u of class s at Nb[(s T2 + u) bins]): A = Q_i + lambda I with Q_i the sum of the other
// classes, lambda = reg tr(Q_i) / Cb + eps and an identity block for the channels >= Cb, then its Cholesky factor in
// place.  Both weights kernels (beamform.hip, beamform_design.hip) call this, so L has the same bits in either.
__device__ __forceinline__ void bf_factor(const double* __restrict__ Nb, int i, int classes, int C, int Cb, int bins,
                                          double reg, double eps, double (&ar)[BF_TRI], double (&ai)[BF_TRI]) {
  const int T2 = 2 * bf_tri(C);
  // A: the lower triangle, row after row; a[r (r + 1) / 2 + c] = A[r][c] = conj(Q[c][r]), c <= r
#pragma unroll
  for (int r = 0; r < BF_MAX_CH; ++r)
#pragma unroll
    for (int c = 0; c <= r; ++c) {
      const int p = r * (r + 1) / 2 + c;
      ar[p] = ai[p] = 0.0;
      if (r < Cb) {
        const long at = 2L * bf_idx(C, c, r) * bins;
        for (int s = 0; s < classes; ++s)
          if (s != i) {
            ar[p] += Nb[(long)s * T2 * bins + at];
            ai[p] -= Nb[(long)s * T2 * bins + at + bins];
          }
      }
    }
  double tr = 0.0;
#pragma unroll
  for (int c = 0; c < BF_MAX_CH; ++c)
    if (c < Cb) tr += ar[c * (c + 1) / 2 + c];
  const double lam = reg * (tr / (double)Cb) + eps;
#pragma unroll
  for (int c = 0; c < BF_MAX_CH; ++c) {
    const int p = c * (c + 1) / 2 + c;
    ar[p] = c < Cb ? ar[p] + lam : 1.0;
    ai[p] = 0.0;
  }
  // Cholesky A = L L^H in place, column after column; the diagonal holds L[c][c], real
#pragma unroll
  for (int c = 0; c < BF_MAX_CH; ++c) {
    const int pc = c * (c + 1) / 2;
    double d = ar[pc + c];
#pragma unroll
    for (int k = 0; k < c; ++k) d -= ar[pc + k] * ar[pc + k] + ai[pc + k] * ai[pc + k];
    const double l = sqrt(d);
    ar[pc + c] = l;
#pragma unroll
    for (int r = c + 1; r < BF_MAX_CH; ++r) {
      const int pr = r * (r + 1) / 2;
      double sr = ar[pr + c], si = ai[pr + c];
#pragma unroll
      for (int k = 0; k < c; ++k) {   // L[r][k] conj L[c][k]
        sr -= ar[pr + k] * ar[pc + k] + ai[pr + k] * ai[pc + k];
        si -= ai[pr + k] * ar[pc + k] - ar[pr + k] * ai[pc + k];
      }
      ar[pr + c] = sr / l;
      ai[pr + c] = si / l;
    }
  }
}

// L y = z in place, z one right-hand side in registers
__device__ __forceinline__ void bf_forward(const double (&ar)[BF_TRI], const double (&ai)[BF_TRI],
                                           double (&zr)[BF_MAX_CH], double (&zi)[BF_MAX_CH]) {
#pragma unroll
  for (int r = 0; r < BF_MAX_CH; ++r) {
    const int pr = r * (r + 1) / 2;
#pragma unroll
    for (int k = 0; k < r; ++k) {
      zr[r] -= ar[pr + k] * zr[k] - ai[pr + k] * zi[k];
      zi[r] -= ar[pr + k] * zi[k] + ai[pr + k] * zr[k];
    }
    zr[r] = zr[r] / ar[pr + r];
    zi[r] = zi[r] / ar[pr + r];
  }
}

// L^H z = y in place
__device__ __forceinline__ void bf_backward(const double (&ar)[BF_TRI], const double (&ai)[BF_TRI],
                                            double (&zr)[BF_MAX_CH], double (&zi)[BF_MAX_CH]) {
#pragma unroll
  for (int r = BF_MAX_CH - 1; r >= 0; --r) {
#pragma unroll
    for (int k = r + 1; k < BF_MAX_CH; ++k) {   // conj(L[k][r]) z[k]
      const int pk = k * (k + 1) / 2;
      zr[r] -= ar[pk + r] * zr[k] + ai[pk + r] * zi[k];
      zi[r] -= ar[pk + r] * zi[k] - ai[pk + r] * zr[k];
    }
    zr[r] = zr[r] / ar[r * (r + 1) / 2 + r];
    zi[r] = zi[r] / ar[r * (r + 1) / 2 + r];
  }
}

// Frame slot fg, bins k and H - k: Y = sum_c conj(w_c) X_c in fp64 in channel order, rounded once, times the source's
// mask with `post`, packed again over channel 0's slot.  weight(j, c, re, im) hands out w_c of bin j.
template <int H, class Weight>
__device__ __forceinline__ void bf_contract(const MaskRefineShape& q, int post, float2* buf, const float2* tw, int Cb,
                                            int src, int fg, int k, Weight&& weight) {
  const int km = (H - k) & (H - 1);
  const float2 t = tw[k];
  double ykr = 0.0, yki = 0.0, ymr = 0.0, ymi = 0.0;
  for (int c = 0; c < Cb; ++c) {   // conj(w_c) X_c
    const float2* a = buf + c * MR_POINTS + fg * H;
    float2 xk, xm;
    mr_split(a[k], a[km], t, xk, xm);
    double kr, ki, mr, mi;
    weight(k, c, kr, ki);
    weight(H - k, c, mr, mi);
    const double pkr = kr * (double)xk.x + ki * (double)xk.y, pki = kr * (double)xk.y - ki * (double)xk.x;
    const double pmr = mr * (double)xm.x + mi * (double)xm.y, pmi = mr * (double)xm.y - mi * (double)xm.x;
    ykr = c == 0 ? pkr : ykr + pkr;
    yki = c == 0 ? pki : yki + pki;
    ymr = c == 0 ? pmr : ymr + pmr;
    ymi = c == 0 ? pmi : ymi + pmi;
  }
  float2 yk = make_float2((float)ykr, (float)yki), ym = make_float2((float)ymr, (float)ymi);
  if (post) {
    float mk[MR_MAX_SRC], mm[MR_MAX_SRC];
    mr_masks(q, buf + Cb * MR_POINTS + fg * H, k, km, t, mk, mm);
    float sk = 0.f, sm = 0.f;
#pragma unroll
    for (int s = 0; s < MR_MAX_SRC; ++s)
      if (s == src) sk = mk[s], sm = mm[s];
    yk = make_float2(sk * yk.x, sk * yk.y);
    ym = make_float2(sm * ym.x, sm * ym.y);
  }
  float2 zk, zm;
  mr_merge(yk, ym, t, zk, zm);
  float2* o = buf + fg * H;
  o[k] = zk;
  if (km != k) o[km] = zm;
}
