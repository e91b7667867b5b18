// Weighted prediction error dereverberation (dsn_dereverb; the definition is in include/ditsep_hip.h, restated in
// float64 in tests/dereverb_restatement.py): per frequency bin a multichannel linear prediction filter over the delayed
// past of all channels is estimated against a time-varying variance and its prediction, the late reverberation, is
// subtracted (Nakatani et al. 2010; Yoshioka & Nakatani 2012).  Frames, spectra and output samples are formed by the
// functions of maskrefine_dev.h that maskrefine.hip calls (mr_tables, mr_load, mr_fft, mr_split; mr_merge, mr_add,
// mr_finish), so they have the bits they have there.  Three launches per chunk of items:
//   analysis   workgroup (group of 2048 / n_fft frames, item, channel): the frames' transforms, written bin-major into
//              Y [item][bin][channel][frame], so that one bin's history is C contiguous rows.
//   solve      workgroup (bin, item), 256 threads, all iterations on-die.  The bin's frames pass twice per iteration in
//              tiles of DV_TILE frames with a D + K - 1 halo staged in LDS as complex doubles: the first pass forms
//              X = Y - G^H y~ on the fly, lambda(t) (stored per frame) and its maximum (an integer maximum on the bits);
//              the second accumulates R (lower triangle) and P in registers, a thread owning one 4 x 4 block for all
//              tiles, so every sum runs in increasing t whatever the tiling.  The blocks go to LDS, the loaded triangle
//              is factored column by column by the whole workgroup (right-looking; the diagonal keeps the pivots), both
//              triangular solves run in place on P, which is then G.  After the last iteration X is written in fp32.
//   synthesis  workgroup (span, item, channel), the mask kernel's layout: reads X's frames, inverse-transforms and
//              overlap-adds as mask_refine does.
// No floating-point atomics; nothing depends on the batch position, the padding or the chunking.
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

#include "maskrefine_dev.h"

constexpr int DV_TILE = 64;                      // frames per tile of the solve launch
constexpr int DV_BF = MR_POINTS / 2 / MRT;       // butterflies per thread and stage: one signal

struct DvShape {
  int C, K, D, I, Lmax, hop, Fs, items;
  double reg, eps;
};

// the chunk's workspace: G | lambda | Y | X | failed, every array [items][bins]...
struct DvWorkspace {
  double2* G;     // [items][bins][C K][C]
  double* lam;    // [items][bins][Fs]
  float2* Y;      // [items][bins][C][Fs]
  float2* X;      // [items][bins][C][Fs]
  int* failed;    // [items][bins]
};

__host__ __device__ inline int dv_tri(int i, int j) { return i * (i + 1) / 2 + j; }   // entry (i, j <= i), row after row

// ---------------------------------------------------------------------------------------------------- analysis
// grid (ceil(Fs / G), items, C).  Dynamic LDS: float2 tw[H] | float2 buf[G][H] | float win[NFFT]
template <int NFFT>
__global__ __launch_bounds__(MRT) void dereverb_analysis_kernel(const DvShape q, const float* __restrict__ mix,
                                                                const int* __restrict__ lens,
                                                                const int* __restrict__ chans, float2* __restrict__ Yw) {
  constexpr int H = NFFT / 2, G = MR_POINTS / H, NP = H / 2 + 1;
  extern __shared__ __attribute__((aligned(16))) float2 dv_lds[];
  const int tid = threadIdx.x, b = blockIdx.y, c = blockIdx.z, hop = q.hop;
  const int Cb = chans ? chans[b] : q.C;
  const MrItem it = mr_item(lens, b, q.Lmax, hop);
  const int f0 = blockIdx.x * G;
  if (c >= Cb || f0 >= it.F) return;   // (uniform)
  float2* tw = dv_lds;
  float2* buf = tw + H;
  float* win = reinterpret_cast<float*>(buf + MR_POINTS);
  mr_tables<H>(tw, win, tid);
  __syncthreads();
  const int f_last = min(it.F - 1, f0 + G - 1);
  mr_load<H>(buf, win, mix + ((long)b * q.C + c) * q.Lmax, nullptr, q.Lmax, it, hop, 1, 0, f0, f_last, tid);
  __syncthreads();
  mr_fft<H, false, DV_BF>(buf, tw, MR_POINTS / 2, tid);
  const long bin_stride = (long)q.C * q.Fs;
  float2* Yb = Yw + ((long)b * (H + 1) * q.C + c) * q.Fs;   // bin j, frame f: Yb[j bin_stride + f]
  for (int e = tid; e < G * NP; e += MRT) {
    const int fg = e / NP, k = e - fg * NP, km = (H - k) & (H - 1), f = f0 + fg;
    if (f > f_last) continue;
    float2 xk, xm;
    mr_split(buf[fg * H + k], buf[fg * H + km], tw[k], xk, xm);
    Yb[(long)k * bin_stride + f] = xk;
    if (H - k != k) Yb[(long)(H - k) * bin_stride + f] = xm;
  }
}

// ---------------------------------------------------------------------------------------------------- solve
// X_c of the frame at tile position p (HALO <= p): Y_c - sum_j conj(G[j][c]) y~_j in index order, j = k Cb + c'
__device__ __forceinline__ double2 dv_predict(const double2* __restrict__ tile, const double2* __restrict__ G, int TW,
                                              int Cb, int K, int D, int c, int p, bool have) {
  const double2 y = tile[c * TW + p];
  if (!have) return y;
  double sr = 0.0, si = 0.0;
  for (int k = 0; k < K; ++k)
    for (int cc = 0; cc < Cb; ++cc) {
      const double2 v = tile[cc * TW + p - D - k], g = G[(k * Cb + cc) * Cb + c];
      sr = fma(g.x, v.x, sr);
      sr = fma(g.y, v.y, sr);
      si = fma(g.x, v.y, si);
      si = fma(-g.y, v.x, si);
    }
  return make_double2(y.x - sr, y.y - si);
}

// frames [t0 - HALO, t0 + DV_TILE) of the item's Cb rows into tile[c][p], zero where there is no frame
__device__ __forceinline__ void dv_stage(double2* __restrict__ tile, const float2* __restrict__ Yb, int TW, int HALO,
                                         int Cb, int Fs, int F, int t0, int tid) {
  for (int e = tid; e < Cb * TW; e += MRT) {
    const int c = e / TW, p = e - c * TW, f = t0 - HALO + p;
    double2 v = make_double2(0.0, 0.0);
    if (f >= 0 && f < F) {
      const float2 y = Yb[(long)c * Fs + f];
      v = make_double2((double)y.x, (double)y.y);
    }
    tile[e] = v;
  }
}

// grid (bins, items).  Dynamic LDS (doubles): double2 tri[N (N + 1) / 2] | double2 P[N][C] | double2 tile[C + 1][TW] |
// double pw[C][DV_TILE] | double inv[DV_TILE], N = C K of the call, TW = D + K - 1 + DV_TILE.
__global__ __launch_bounds__(MRT) void dereverb_solve_kernel(const DvShape q, const int* __restrict__ lens,
                                                             const int* __restrict__ chans, const DvWorkspace ws) {
  extern __shared__ __attribute__((aligned(16))) double2 dv_lds2[];
  __shared__ unsigned long long smax;
  __shared__ double sdelta;
  const int tid = threadIdx.x, j = blockIdx.x, b = blockIdx.y, bins = gridDim.x;
  const int K = q.K, D = q.D, HALO = D + K - 1, TW = HALO + DV_TILE, Nmax = q.C * K;
  const int Cb = chans ? chans[b] : q.C;
  const int L = lens ? lens[b] : q.Lmax;
  const int F = 1 + (L + q.hop - 1) / q.hop;
  const int N = Cb * K;
  double2* tri = dv_lds2;
  double2* P = tri + Nmax * (Nmax + 1) / 2;
  double2* tile = P + Nmax * q.C;
  double* pw = reinterpret_cast<double*>(tile + (q.C + 1) * TW);
  double* inv = pw + q.C * DV_TILE;
  const long sys = (long)b * bins + j;
  const float2* Yb = ws.Y + sys * q.C * q.Fs;
  double* lamg = ws.lam + sys * q.Fs;

  // the block this thread owns: rows 4 bi .. of y~ against columns 4 bj .. of y~ (R, bj <= bi) or of Y (P)
  const int NB = (N + 3) / 4, ntri = NB * (NB + 1) / 2, nblk = ntri + NB * ((Cb + 3) / 4);
  const bool owner = tid < nblk, isP = tid >= ntri;
  int bi = 0, bj = 0;
  if (owner) {
    if (!isP) {
      int rest = tid;
      while (rest > bi) rest -= bi + 1, ++bi;
      bj = rest;
    } else {
      bi = (tid - ntri) % NB;
      bj = (tid - ntri) / NB;
    }
  }
  // tile offsets of the block's rows and columns at frame position HALO + tt; what does not exist reads the zero row
  int roff[4], coff[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = 4 * bi + a, jj = 4 * bj + a;
    roff[a] = i < N ? (i % Cb) * TW + HALO - D - i / Cb : Cb * TW;
    if (isP) coff[a] = jj < Cb ? jj * TW + HALO : Cb * TW;
    else coff[a] = jj < N ? (jj % Cb) * TW + HALO - D - jj / Cb : Cb * TW;
  }
  for (int e = tid; e < TW; e += MRT) tile[Cb * TW + e] = make_double2(0.0, 0.0);   // the zero row
  for (int e = tid; e < N * Cb; e += MRT) P[e] = make_double2(0.0, 0.0);            // G = 0
  bool have = false;
  int failed = 0;

  for (int it = 0; it < q.I; ++it) {
    // ---- pass 1: lambda(t) and its maximum
    if (tid == 0) smax = 0ull;
    for (int t0 = 0; t0 < F; t0 += DV_TILE) {
      const int Tn = min(DV_TILE, F - t0);
      __syncthreads();
      dv_stage(tile, Yb, TW, HALO, Cb, q.Fs, F, t0, tid);
      __syncthreads();
      for (int e = tid; e < Cb * DV_TILE; e += MRT) {
        const int c = e / DV_TILE, tt = e % DV_TILE;
        if (tt < Tn) {
          const double2 x = dv_predict(tile, P, TW, Cb, K, D, c, HALO + tt, have);
          pw[e] = fma(x.x, x.x, x.y * x.y);
        }
      }
      __syncthreads();
      if (tid < Tn) {
        double s = pw[tid];
        for (int c = 1; c < Cb; ++c) s += pw[c * DV_TILE + tid];
        s = s / (double)Cb;
        lamg[t0 + tid] = s;
        atomicMax(&smax, (unsigned long long)__double_as_longlong(s));   // s >= 0: the order of the bits is its own
      }
    }
    __syncthreads();
    const double m = __longlong_as_double((long long)smax);
    if (m == 0.0) {   // (uniform) a silent bin passes through
      for (int e = tid; e < N * Cb; e += MRT) P[e] = make_double2(0.0, 0.0);
      have = false;
      break;
    }
    const double floor_ = 1e-10 * m;

    // ---- pass 2: R and P in registers, in increasing t
    double ar[4][4], ai[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) ar[a][c] = ai[a][c] = 0.0;
    for (int t0 = 0; t0 < F; t0 += DV_TILE) {
      const int Tn = min(DV_TILE, F - t0);
      __syncthreads();
      dv_stage(tile, Yb, TW, HALO, Cb, q.Fs, F, t0, tid);
      if (tid < Tn) inv[tid] = 1.0 / fmax(lamg[t0 + tid], floor_);
      __syncthreads();
      if (owner)
        for (int tt = 0; tt < Tn; ++tt) {
          const double w = inv[tt];
          double2 cv[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) cv[c] = tile[coff[c] + tt];
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            const double2 r = tile[roff[a] + tt];
            const double rx = r.x * w, ry = r.y * w;
#pragma unroll
            for (int c = 0; c < 4; ++c) {   // (rx + i ry) conj(cv)
              ar[a][c] = fma(rx, cv[c].x, ar[a][c]);
              ar[a][c] = fma(ry, cv[c].y, ar[a][c]);
              ai[a][c] = fma(ry, cv[c].x, ai[a][c]);
              ai[a][c] = fma(-rx, cv[c].y, ai[a][c]);
            }
          }
        }
    }
    __syncthreads();   // pass 1 of this iteration has read G: P may be overwritten
    if (owner) {
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int i = 4 * bi + a, jj = 4 * bj + c;
          if (isP) {
            if (i < N && jj < Cb) P[i * Cb + jj] = make_double2(ar[a][c], ai[a][c]);
          } else if (i < N && jj <= i) {
            tri[dv_tri(i, jj)] = make_double2(ar[a][c], jj == i ? 0.0 : ai[a][c]);
          }
        }
    }
    __syncthreads();
    if (tid == 0) {
      double tr = 0.0;
      for (int i = 0; i < N; ++i) tr += tri[dv_tri(i, i)].x;
      sdelta = q.reg * tr / (double)N + q.eps;
    }
    __syncthreads();
    if (tid < N) tri[dv_tri(tid, tid)].x += sdelta;
    __syncthreads();

    // ---- A = L L^H, right-looking; the diagonal keeps the pivots d = L[c][c]^2
    const int ty = tid >> 4, tx = tid & 15;
    bool bad = false;
    for (int c = 0; c < N; ++c) {
      const double d = tri[dv_tri(c, c)].x;
      if (!(d > 0.0 && d <= 1.7976931348623157e308)) {   // (uniform) not finite and positive
        bad = true;
        break;
      }
      const double l = sqrt(d);
      if (tid < N - c - 1) {
        double2& e = tri[dv_tri(c + 1 + tid, c)];
        e = make_double2(e.x / l, e.y / l);
      }
      __syncthreads();
      for (int r = c + 1 + ty; r < N; r += 16) {
        const double2 lr = tri[dv_tri(r, c)];
        for (int jj = c + 1 + tx; jj <= r; jj += 16) {   // A[r][jj] -= L[r][c] conj(L[jj][c])
          const double2 lj = tri[dv_tri(jj, c)];
          double2 e = tri[dv_tri(r, jj)];
          e.x = fma(-lr.x, lj.x, e.x);
          e.x = fma(-lr.y, lj.y, e.x);
          e.y = fma(-lr.y, lj.x, e.y);
          e.y = fma(lr.x, lj.y, e.y);
          tri[dv_tri(r, jj)] = e;
        }
      }
      __syncthreads();
    }
    if (bad) {   // (uniform) the bin passes through for this and the remaining iterations
      __syncthreads();
      for (int e = tid; e < N * Cb; e += MRT) P[e] = make_double2(0.0, 0.0);
      have = false;
      failed = 1;
      break;
    }
    // ---- L y = p, then L^H g = y, in place on P, all Cb right-hand sides
    for (int k = 0; k < N; ++k) {
      const double l = sqrt(tri[dv_tri(k, k)].x);
      if (tid < Cb) {
        double2& e = P[k * Cb + tid];
        e = make_double2(e.x / l, e.y / l);
      }
      __syncthreads();
      for (int e = tid; e < (N - k - 1) * Cb; e += MRT) {
        const int r = k + 1 + e / Cb, c = e % Cb;
        const double2 lr = tri[dv_tri(r, k)], y = P[k * Cb + c];
        double2 v = P[r * Cb + c];
        v.x = fma(-lr.x, y.x, v.x);
        v.x = fma(lr.y, y.y, v.x);
        v.y = fma(-lr.x, y.y, v.y);
        v.y = fma(-lr.y, y.x, v.y);
        P[r * Cb + c] = v;
      }
      __syncthreads();
    }
    for (int k = N - 1; k >= 0; --k) {
      const double l = sqrt(tri[dv_tri(k, k)].x);
      if (tid < Cb) {
        double2& e = P[k * Cb + tid];
        e = make_double2(e.x / l, e.y / l);
      }
      __syncthreads();
      for (int e = tid; e < k * Cb; e += MRT) {   // y[r] -= conj(L[k][r]) g[k]
        const int r = e / Cb, c = e % Cb;
        const double2 lk = tri[dv_tri(k, r)], g = P[k * Cb + c];
        double2 v = P[r * Cb + c];
        v.x = fma(-lk.x, g.x, v.x);
        v.x = fma(-lk.y, g.y, v.x);
        v.y = fma(-lk.x, g.y, v.y);
        v.y = fma(lk.y, g.x, v.y);
        P[r * Cb + c] = v;
      }
      __syncthreads();
    }
    have = true;
  }
  __syncthreads();

  // ---- the filter, the count and X in fp32
  double2* Gg = ws.G + sys * Nmax * q.C;
  for (int e = tid; e < Nmax * q.C; e += MRT) {
    const int r = e / q.C, c = e % q.C;
    Gg[e] = r < N && c < Cb ? P[r * Cb + c] : make_double2(0.0, 0.0);
  }
  if (tid == 0) ws.failed[sys] = failed;
  float2* Xb = ws.X + sys * q.C * q.Fs;
  for (int t0 = 0; t0 < F; t0 += DV_TILE) {
    const int Tn = min(DV_TILE, F - t0);
    __syncthreads();
    dv_stage(tile, Yb, TW, HALO, Cb, q.Fs, F, t0, tid);
    __syncthreads();
    for (int e = tid; e < Cb * DV_TILE; e += MRT) {
      const int c = e / DV_TILE, tt = e % DV_TILE;
      if (tt < Tn) {
        const double2 x = dv_predict(tile, P, TW, Cb, K, D, c, HALO + tt, have);
        Xb[(long)c * q.Fs + t0 + tt] = make_float2((float)x.x, (float)x.y);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------- synthesis
// grid (ceil(Lmax / SPAN), items, C).  Dynamic LDS: float2 tw[H] | float2 buf[G][H] | float win[NFFT] | float ola[SPAN]
template <int NFFT>
__global__ __launch_bounds__(MRT) void dereverb_synthesis_kernel(const DvShape q, int vec,
                                                                 const int* __restrict__ lens,
                                                                 const int* __restrict__ chans,
                                                                 const float2* __restrict__ Xw, float* __restrict__ out) {
  constexpr int H = NFFT / 2, G = MR_POINTS / H, NP = H / 2 + 1, SPAN = mr_span(NFFT);
  extern __shared__ __attribute__((aligned(16))) float2 dv_lds[];
  const int hop = q.hop, tid = threadIdx.x;
  const int b = blockIdx.y, c = blockIdx.z, s0 = blockIdx.x * SPAN;
  const int Cb = chans ? chans[b] : q.C;
  const MrItem it = mr_item(lens, b, q.Lmax, hop);
  float* outb = out + ((long)b * q.C + c) * q.Lmax;
  if (s0 >= it.L || c >= Cb) {   // (uniform) past the item's end, or a channel it does not have
    mr_zero<H>(outb, 0, 1, s0, q.Lmax, vec, tid);
    return;
  }
  float2* tw = dv_lds;
  float2* buf = tw + H;
  float* win = reinterpret_cast<float*>(buf + MR_POINTS);
  float* ola = win + NFFT;
  mr_tables<H>(tw, win, tid);
  for (int e = tid; e < SPAN; e += MRT) ola[e] = 0.f;

  const MrFrames fr = mr_frames<H>(it, s0, hop);
  const int f_first = fr.f_first, f_last = fr.f_last;
  const long bin_stride = (long)q.C * q.Fs;
  const float2* Xb = Xw + ((long)b * (H + 1) * q.C + c) * q.Fs;

  for (int f0 = f_first; f0 <= f_last; f0 += G) {
    __syncthreads();   // the tables are in; the previous group's frames have been added
    for (int e = tid; e < G * NP; e += MRT) {
      const int fg = e / NP, k = e - fg * NP, km = (H - k) & (H - 1), f = f0 + fg;
      float2 zk = make_float2(0.f, 0.f), zm = zk;
      if (f <= f_last) mr_merge(Xb[(long)k * bin_stride + f], Xb[(long)(H - k) * bin_stride + f], tw[k], zk, zm);
      float2* o = buf + fg * H;
      o[k] = zk;
      if (km != k) o[km] = zm;
    }
    __syncthreads();
    mr_fft<H, true, DV_BF>(buf, tw, MR_POINTS / 2, tid);
    mr_add<H>(ola, buf, win, s0, fr.pend, hop, f0, min(f0 + G - 1, f_last), tid);
  }
  mr_finish<H>(ola, win, outb, 0, 1, it, s0, fr.pend, hop, q.Lmax, vec, tid);
}

template <int NFFT>
void dv_run(const DvShape& q, const float* mix, const int* lens, const int* chans, const DvWorkspace& ws, float* out,
            hipStream_t st) {
  constexpr int H = NFFT / 2, G = MR_POINTS / H, SPAN = mr_span(NFFT);
  const size_t lds_a = mr_lds_bytes(NFFT, 1, 0), lds_s = mr_lds_bytes(NFFT, 1, 1);
  hipLaunchKernelGGL((dereverb_analysis_kernel<NFFT>), dim3((unsigned)((q.Fs + G - 1) / G), (unsigned)q.items,
                     (unsigned)q.C), dim3(MRT), lds_a, st, q, mix, lens, chans, ws.Y);
  // the launch asks for what its own C K needs; the limit is set once per device, so it is the largest any call may
  // need: 80 unknowns at 8 channels, with the longest halo (16 taps, delay 8) added to that system's own
  const size_t lds = dereverb_lds_bytes(q.C, q.K, q.D);
  dsn_allow_lds<dereverb_solve_kernel>((int)dereverb_lds_bytes(DEREVERB_MAX_CH, DEREVERB_MAX_UNKNOWNS / DEREVERB_MAX_CH,
                                                               DEREVERB_MAX_DELAY + DEREVERB_MAX_TAPS));
  hipLaunchKernelGGL(dereverb_solve_kernel, dim3((unsigned)(H + 1), (unsigned)q.items), dim3(MRT), lds, st, q, lens,
                     chans, ws);
  const int vec = ((uintptr_t)out & 15) == 0 && q.Lmax % 4 == 0 ? 1 : 0;   // mr_store: whole quads at once
  hipLaunchKernelGGL((dereverb_synthesis_kernel<NFFT>), dim3((unsigned)((q.Lmax + SPAN - 1) / SPAN), (unsigned)q.items,
                     (unsigned)q.C), dim3(MRT), lds_s, st, q, vec, lens, chans, ws.X, out);
}

}  // namespace

int dereverb_frames(int hop, int Lmax) { return 1 + (Lmax + hop - 1) / hop; }

size_t dereverb_lds_bytes(int C, int K, int D) {
  const size_t N = (size_t)C * K, TW = (size_t)D + K - 1 + DV_TILE;
  return sizeof(double2) * (N * (N + 1) / 2 + N * C + ((size_t)C + 1) * TW) + sizeof(double) * ((size_t)C + 1) * DV_TILE;
}

size_t dereverb_item_bytes(int nfft, int hop, int Lmax, int C, int K) {
  const size_t bins = (size_t)nfft / 2 + 1, Fs = (size_t)dereverb_frames(hop, Lmax), N = (size_t)C * K;
  return bins * (8 * (2 * N * C + Fs + 2 * C * Fs) + 4);
}

void launch_dereverb(const float* mix, const int* lens, const int* chans, void* workspace, float* out, int items, int C,
                     int Lmax, int nfft, int hop, int K, int D, int I, double reg, double eps, hipStream_t st) {
  const DvShape q{C, K, D, I, Lmax, hop, dereverb_frames(hop, Lmax), items, reg, eps};
  const size_t bins = (size_t)nfft / 2 + 1, sys = (size_t)items * bins, N = (size_t)C * K;
  DvWorkspace ws;
  ws.G = reinterpret_cast<double2*>(workspace);
  ws.lam = reinterpret_cast<double*>(ws.G + sys * N * C);
  ws.Y = reinterpret_cast<float2*>(ws.lam + sys * q.Fs);
  ws.X = ws.Y + sys * C * q.Fs;
  ws.failed = reinterpret_cast<int*>(ws.X + sys * C * q.Fs);
  mr_for_nfft(nfft, [&](auto N) { dv_run<decltype(N)::value>(q, mix, lens, chans, ws, out, st); });
}
