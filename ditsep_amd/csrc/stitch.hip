// Window stitch (dsn_window_stitch): the separated windows [W][n][Lw] of one long recording -> one [n][L] recording
// with consistent speakers.  Restated in float64 in tests/stitch_restatement.py.
//
// Window w covers samples [w hop, w hop + Lw), hop = Lw - O; 2 O <= Lw, so an output sample lies in at most two
// windows and the overlap-add is a gather.  Three launches:
//   stitch_gram_kernel    per (boundary w, tile of DSN_STITCH_TILE overlap positions): the n x n inner products of
//                         the tail of window w with the head of window w + 1.  fp32 x fp32 products are exact in
//                         fp64 and are summed in fp64: per thread in stride order, then a fixed tree (shuffles inside
//                         a wave, the four wave sums in LDS added in order), one plain store per (tile, i, j).
//   stitch_perm_kernel    one workgroup: adds the tile partials in index order, solves every boundary's assignment
//                         (one thread per boundary), then one thread composes the cumulative table sequentially.
//   stitch_gather_kernel  the cross-fade.  fall[k] a + rise[k] b is two fp32 products and their fp32 sum (contraction
//                         off: the value does not depend on the load path taken); everything else is a copy.
// No atomics anywhere: reruns are bit-identical.  Index arithmetic is 64-bit.
#include "../../include/ditsep_hip.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int STPB = 256;

// grid x: w tiles + c, boundary w and tile c.  VEC: 16-byte loads (Lw, hop -- and so O -- multiples of 4 and a 16-byte
// aligned base: every row start, hop + k, the tile start and the tile length are then multiples of 4 floats).
template <int N, bool VEC>
__global__ void __launch_bounds__(STPB) stitch_gram_kernel(const float* __restrict__ chunks, int Lw, int O, int tiles,
                                                           double* __restrict__ part) {
  __shared__ double red[N * N][STPB / 64];
  const long w = blockIdx.x / tiles;
  const int c = blockIdx.x % tiles, tid = threadIdx.x;
  const int hop = Lw - O;
  const int k0 = c * DSN_STITCH_TILE;
  const int k1 = k0 + DSN_STITCH_TILE < O ? k0 + DSN_STITCH_TILE : O;
  const float* a = chunks + w * N * (long)Lw + hop;        // row i: a + i Lw
  const float* b = chunks + (w + 1) * N * (long)Lw;        // row j: b + j Lw
  double acc[N][N];
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) acc[i][j] = 0.0;
  if (VEC) {
    for (int k = k0 + 4 * tid; k < k1; k += 4 * STPB) {
      float4 av[N], bv[N];
#pragma unroll
      for (int i = 0; i < N; ++i) av[i] = *reinterpret_cast<const float4*>(a + (long)i * Lw + k);
#pragma unroll
      for (int j = 0; j < N; ++j) bv[j] = *reinterpret_cast<const float4*>(b + (long)j * Lw + k);
#pragma unroll
      for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) {
          acc[i][j] += (double)av[i].x * (double)bv[j].x;
          acc[i][j] += (double)av[i].y * (double)bv[j].y;
          acc[i][j] += (double)av[i].z * (double)bv[j].z;
          acc[i][j] += (double)av[i].w * (double)bv[j].w;
        }
    }
  } else {
    for (int k = k0 + tid; k < k1; k += STPB) {
      float av[N], bv[N];
#pragma unroll
      for (int i = 0; i < N; ++i) av[i] = a[(long)i * Lw + k];
#pragma unroll
      for (int j = 0; j < N; ++j) bv[j] = b[(long)j * Lw + k];
#pragma unroll
      for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) acc[i][j] += (double)av[i] * (double)bv[j];
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) {
      double v = acc[i][j];
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if ((tid & 63) == 0) red[i * N + j][tid >> 6] = v;
    }
  __syncthreads();
  if (tid < N * N) {
    double s = 0.0;
    for (int q = 0; q < STPB / 64; ++q) s += red[tid][q];
    part[(w * tiles + c) * (N * N) + tid] = s;
  }
}

// one workgroup.  sigma_w is left in perm[(w + 1) n ..] by the boundary's thread, then composed in place by thread 0.
__global__ void __launch_bounds__(STPB) stitch_perm_kernel(const double* __restrict__ part, double* __restrict__ gram,
                                                           int* perm, int W, int n, int tiles, int align) {
  const int nn = n * n;
  if (!align) {
    for (long q = threadIdx.x; q < (long)W * n; q += STPB) perm[q] = (int)(q % n);
    return;
  }
  int ncode = 1;   // n^n digit strings, most significant digit sigma(0): the permutations among them come in
  for (int i = 0; i < n; ++i) ncode *= n;   // lexicographic order
  for (int w = threadIdx.x; w < W - 1; w += STPB) {
    double G[16];
    for (int e = 0; e < nn; ++e) {
      double s = 0.0;
      for (int c = 0; c < tiles; ++c) s += part[((long)w * tiles + c) * nn + e];
      G[e] = s;
      gram[(long)w * nn + e] = s;
    }
    int best[4] = {0, 1, 2, 3};
    double best_score = 0.0;
    bool have = false;
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
      for (int i = 0; i < n; ++i) sc += G[i * n + sg[i]];
      if (!have || sc > best_score) {   // the first candidate is the identity
        have = true;
        best_score = sc;
        for (int i = 0; i < n; ++i) best[i] = sg[i];
      }
    }
    for (int i = 0; i < n; ++i) perm[(long)(w + 1) * n + i] = best[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int P[4];
    for (int i = 0; i < n; ++i) perm[i] = P[i] = i;
    for (int w = 0; w < W - 1; ++w) {
      int sg[4];
      for (int i = 0; i < n; ++i) sg[i] = perm[(long)(w + 1) * n + i];
      for (int i = 0; i < n; ++i) perm[(long)(w + 1) * n + i] = P[i] = sg[P[i]];
    }
  }
}

struct StitchShape {
  int W, n, Lw, O, hop, L;
};

__device__ __forceinline__ float stitch_sample(const StitchShape& q, const float* __restrict__ chunks,
                                               const int* __restrict__ perm, const float* __restrict__ fall,
                                               const float* __restrict__ rise, int i, int t) {
  int w = t / q.hop;
  if (w > q.W - 1) w = q.W - 1;
  const int k = t - w * q.hop;   // (t < L <= (W - 1) hop + Lw: k < Lw)
  const float b = chunks[((long)w * q.n + perm[w * q.n + i]) * q.Lw + k];
  if (w < 1 || k >= q.O) return b;
  const float a = chunks[((long)(w - 1) * q.n + perm[(w - 1) * q.n + i]) * q.Lw + q.hop + k];
  return fall[k] * a + rise[k] * b;
}

// grid (x: groups of 4 * STPB samples, y: source).  Each thread writes 4 consecutive samples t0 .. t0 + 3, t0 % 4 == 0.
// vload (hop, Lw, O multiples of 4, aligned bases): the 4 samples share w and the side of the overlap edge, and every
// read is a 16-byte load; vstore (L a multiple of 4, aligned base): one 16-byte store.
__global__ void __launch_bounds__(STPB) stitch_gather_kernel(const StitchShape q, const float* __restrict__ chunks,
                                                             const int* __restrict__ perm,
                                                             const float* __restrict__ fall,
                                                             const float* __restrict__ rise, float* __restrict__ out,
                                                             int vload, int vstore) {
  const int i = blockIdx.y;
  const long t0l = ((long)blockIdx.x * STPB + threadIdx.x) * 4;
  if (t0l >= q.L) return;
  const int t0 = (int)t0l;
  float* dst = out + (long)i * q.L + t0;
  if (t0l + 3 >= q.L) {
    for (int t = t0; t < q.L; ++t) dst[t - t0] = stitch_sample(q, chunks, perm, fall, rise, i, t);
    return;
  }
  float4 v;
  if (vload) {
    int w = t0 / q.hop;
    if (w > q.W - 1) w = q.W - 1;
    const int k = t0 - w * q.hop;
    v = *reinterpret_cast<const float4*>(chunks + ((long)w * q.n + perm[w * q.n + i]) * q.Lw + k);
    if (w >= 1 && k < q.O) {
      const float4 a =
          *reinterpret_cast<const float4*>(chunks + ((long)(w - 1) * q.n + perm[(w - 1) * q.n + i]) * q.Lw + q.hop + k);
      const float4 f = *reinterpret_cast<const float4*>(fall + k);
      const float4 r = *reinterpret_cast<const float4*>(rise + k);
      v.x = f.x * a.x + r.x * v.x;
      v.y = f.y * a.y + r.y * v.y;
      v.z = f.z * a.z + r.z * v.z;
      v.w = f.w * a.w + r.w * v.w;
    }
  } else {
    v.x = stitch_sample(q, chunks, perm, fall, rise, i, t0);
    v.y = stitch_sample(q, chunks, perm, fall, rise, i, t0 + 1);
    v.z = stitch_sample(q, chunks, perm, fall, rise, i, t0 + 2);
    v.w = stitch_sample(q, chunks, perm, fall, rise, i, t0 + 3);
  }
  if (vstore) {
    *reinterpret_cast<float4*>(dst) = v;
  } else {
    dst[0] = v.x;
    dst[1] = v.y;
    dst[2] = v.z;
    dst[3] = v.w;
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <int N>
void gram_launch(const float* chunks, int W, int Lw, int O, double* part, hipStream_t s) {
  const int tiles = stitch_tiles(O);
  const dim3 grid((unsigned)((long)(W - 1) * tiles));   // (one workgroup per 4096 overlap samples held in memory)
  const bool vec = Lw % 4 == 0 && (Lw - O) % 4 == 0 && aligned16(chunks);
  if (vec)
    hipLaunchKernelGGL((stitch_gram_kernel<N, true>), grid, dim3(STPB), 0, s, chunks, Lw, O, tiles, part);
  else
    hipLaunchKernelGGL((stitch_gram_kernel<N, false>), grid, dim3(STPB), 0, s, chunks, Lw, O, tiles, part);
}

}  // namespace

void launch_stitch_gram(const float* chunks, int W, int n, int Lw, int O, double* part, hipStream_t s) {
  if (W < 2 || O < 1) return;   // (no boundary, or nothing to sum: launch_stitch_perm is given tiles = 0)
  switch (n) {
    case 1: gram_launch<1>(chunks, W, Lw, O, part, s); break;
    case 2: gram_launch<2>(chunks, W, Lw, O, part, s); break;
    case 3: gram_launch<3>(chunks, W, Lw, O, part, s); break;
    default: gram_launch<4>(chunks, W, Lw, O, part, s); break;
  }
}

void launch_stitch_perm(const double* part, double* gram, int* perm, int W, int n, int tiles, int align,
                        hipStream_t s) {
  hipLaunchKernelGGL(stitch_perm_kernel, dim3(1), dim3(STPB), 0, s, part, gram, perm, W, n, tiles, align);
}

void launch_stitch_gather(const float* chunks, const int* perm, const float* fall, const float* rise, float* out, int W,
                          int n, int Lw, int O, int L, hipStream_t s) {
  const StitchShape q{W, n, Lw, O, Lw - O, L};
  const int vload = Lw % 4 == 0 && O % 4 == 0 && aligned16(chunks) && aligned16(fall) && aligned16(rise);
  const int vstore = L % 4 == 0 && aligned16(out);
  const long per = 4L * STPB;
  hipLaunchKernelGGL(stitch_gather_kernel, dim3((unsigned)((L + per - 1) / per), (unsigned)n), dim3(STPB), 0, s, q,
                     chunks, perm, fall, rise, out, vload, vstore);
}
