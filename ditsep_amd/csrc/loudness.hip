// Programme loudness (ITU-R BS.1770-4 / EBU R 128), true peak and one gain for a ragged batch with per-item rates
// (dsn_loudness, dsn_apply_gain; include/ditsep_hip.h states the definition, tests/loudness_restatement.py restates it
// in float64).
//
// The K-weighting is a 4th-order recursion with poles close to the unit circle: it cannot be warmed up locally, and one
// thread per row would leave the device idle.  Every (item, channel) row is cut into chunks of LOUD_CHUNK samples counted
// from the item's own start, and the recursion is run twice per chunk, in fp64, one thread per chunk:
//   loud_state_kernel   from zero state; keeps the chunk's final state f_k (four doubles)
//   loud_carry_kernel   one workgroup per row: s_0 = 0, s_{k+1} = P s_k + f_k with P the zero-input transition over a
//                       whole chunk (host, fp64, per rate); f_k is replaced by s_k.  A row of more chunks than the
//                       workgroup has threads is walked in equal runs of m = ceil(chunks / 256): every thread folds its
//                       run, thread 0 chains the 256 run results with P^m, every thread walks its run again
//   loud_sums_kernel    from s_k; y^2 is added in sample order into the h-sample segment the chunk starts in and the
//                       next one (h >= 800 > LOUD_CHUNK: a chunk touches at most two)
//   loud_item_kernel    one workgroup per item: a segment is the sum of its chunks' parts in chunk order, a block four
//                       consecutive segments, z_j, l_j, the two gates and I in index order by one thread
// The peaks are a separate launch (loud_peak_kernel): a tile of the row plus the halo of the 1 -> 4 interpolator in LDS,
// the four phases in fp32 exactly as resample.hip forms them, max |.| by an integer maximum over the bits of the
// non-negative floats -- an exact maximum whatever the order.  Nothing is written per sample.  No floating-point
// atomics anywhere; every order above is fixed by the item's own length, rate and channel count.
#include "../../include/ditsep_hip.h"
#include "kernels.h"

namespace {

constexpr int LPB = 256;

// one sample through both biquads (transposed direct form II): c = shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2
__host__ __device__ inline double kw_step(const double* __restrict__ c, double x, double* __restrict__ s) {
  const double y1 = c[0] * x + s[0];
  s[0] = c[1] * x - c[3] * y1 + s[1];
  s[1] = c[2] * x - c[4] * y1;
  const double y2 = c[5] * y1 + s[2];
  s[2] = c[6] * y1 - c[8] * y2 + s[3];
  s[3] = c[7] * y1 - c[9] * y2;
  return y2;
}

__device__ __forceinline__ void matvec4(const double* __restrict__ P, const double* __restrict__ s,
                                        const double* __restrict__ f, double* __restrict__ out) {
  for (int r = 0; r < 4; ++r)
    out[r] = (((P[4 * r] * s[0] + P[4 * r + 1] * s[1]) + P[4 * r + 2] * s[2]) + P[4 * r + 3] * s[3]) + f[r];
}

// The n samples of a chunk at p through the cascade from state s.  SUMS: y^2 goes to acc[0] for samples before `bound`
// (counted from the chunk's start) and to acc[1] from there on.  vec: p is 16-byte aligned and n a multiple of 4.
template <bool SUMS>
__device__ __forceinline__ void loud_chunk(const double* __restrict__ c, const float* __restrict__ p, int n, bool vec,
                                           double* __restrict__ s, int bound, double* __restrict__ acc) {
  if (vec) {
    for (int i = 0; i < n; i += 4) {
      const float4 v = *reinterpret_cast<const float4*>(p + i);
      const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double y = kw_step(c, (double)e[q], s);
        if (SUMS) {
          if (i + q < bound) acc[0] += y * y;
          else acc[1] += y * y;
        }
      }
    }
  } else {
    for (int i = 0; i < n; ++i) {
      const double y = kw_step(c, (double)p[i], s);
      if (SUMS) {
        if (i < bound) acc[0] += y * y;
        else acc[1] += y * y;
      }
    }
  }
}

template <bool SUMS>
__global__ void __launch_bounds__(LPB) loud_filter_kernel(const float* __restrict__ x, const LoudItem* __restrict__ items,
                                                          const LoudRate* __restrict__ rates, int C, int Lmax,
                                                          long chunks, double* __restrict__ state,
                                                          double* __restrict__ part) {
  const int b = blockIdx.y, ch = blockIdx.z;
  const LoudItem it = items[b];
  const long k = (long)blockIdx.x * LPB + threadIdx.x;
  if (ch >= it.ch || k * LOUD_CHUNK >= it.len) return;
  const long pos = k * LOUD_CHUNK;
  const int n = it.len - pos < LOUD_CHUNK ? (int)(it.len - pos) : LOUD_CHUNK;
  const float* p = x + ((long)b * C + ch) * Lmax + pos;
  const bool vec = n == LOUD_CHUNK && ((uintptr_t)p & 15) == 0;
  double c[10];
  for (int i = 0; i < 10; ++i) c[i] = rates[it.rate].c[i];
  double* st = state + (((long)b * C + ch) * chunks + k) * 4;
  double s[4] = {0.0, 0.0, 0.0, 0.0}, acc[2] = {0.0, 0.0};
  if (SUMS) {
    for (int i = 0; i < 4; ++i) s[i] = st[i];
    const long next = (pos / it.h + 1) * it.h;   // the first sample of the following segment
    const int bound = next - pos < LOUD_CHUNK ? (int)(next - pos) : LOUD_CHUNK;
    loud_chunk<true>(c, p, n, vec, s, bound, acc);
    double* pt = part + (((long)b * C + ch) * chunks + k) * 2;
    pt[0] = acc[0], pt[1] = acc[1];
  } else {
    loud_chunk<false>(c, p, n, vec, s, 0, acc);
    for (int i = 0; i < 4; ++i) st[i] = s[i];
  }
}

__device__ void matmul4(const double* A, const double* B, double* out) {
  for (int r = 0; r < 4; ++r)
    for (int q = 0; q < 4; ++q)
      out[4 * r + q] = ((A[4 * r] * B[q] + A[4 * r + 1] * B[4 + q]) + A[4 * r + 2] * B[8 + q]) + A[4 * r + 3] * B[12 + q];
}

__global__ void __launch_bounds__(LPB) loud_carry_kernel(const LoudItem* __restrict__ items,
                                                         const LoudRate* __restrict__ rates, int C, long chunks,
                                                         double* __restrict__ state) {
  __shared__ double sh[LPB][4];
  __shared__ double Pm[16];
  const int b = blockIdx.x, ch = blockIdx.y, tid = threadIdx.x;
  const LoudItem it = items[b];
  if (ch >= it.ch) return;   // (uniform)
  const long nk = ((long)it.len + LOUD_CHUNK - 1) / LOUD_CHUNK, m = (nk + LPB - 1) / LPB;
  double P[16];
  for (int i = 0; i < 16; ++i) P[i] = rates[it.rate].P[i];
  double* st = state + ((long)b * C + ch) * chunks * 4;
  const long k0 = (long)tid * m < nk ? (long)tid * m : nk, k1 = k0 + m < nk ? k0 + m : nk;
  double s[4] = {0.0, 0.0, 0.0, 0.0}, t[4];
  for (long k = k0; k < k1; ++k) {
    matvec4(P, s, st + 4 * k, t);
    for (int i = 0; i < 4; ++i) s[i] = t[i];
  }
  for (int i = 0; i < 4; ++i) sh[tid][i] = s[i];
  if (tid == 0) {   // P^m by squaring, most significant bit first
    double A[16], T[16];
    for (int i = 0; i < 16; ++i) A[i] = P[i];
    int top = 0;
    while ((m >> (top + 1)) != 0) ++top;
    for (int bit = top - 1; bit >= 0; --bit) {
      matmul4(A, A, T);
      if ((m >> bit) & 1) matmul4(T, P, A);
      else
        for (int i = 0; i < 16; ++i) A[i] = T[i];
    }
    for (int i = 0; i < 16; ++i) Pm[i] = A[i];
  }
  __syncthreads();
  if (tid == 0) {
    double cur[4] = {0.0, 0.0, 0.0, 0.0}, f[4], nx[4], A[16];
    for (int i = 0; i < 16; ++i) A[i] = Pm[i];
    for (int r = 0; r < LPB; ++r) {
      for (int i = 0; i < 4; ++i) f[i] = sh[r][i], sh[r][i] = cur[i];
      matvec4(A, cur, f, nx);
      for (int i = 0; i < 4; ++i) cur[i] = nx[i];
    }
  }
  __syncthreads();
  for (int i = 0; i < 4; ++i) s[i] = sh[tid][i];
  for (long k = k0; k < k1; ++k) {
    double f[4];
    for (int i = 0; i < 4; ++i) f[i] = st[4 * k + i], st[4 * k + i] = s[i];
    matvec4(P, s, f, t);
    for (int i = 0; i < 4; ++i) s[i] = t[i];
  }
}

__device__ __forceinline__ double lufs(double z) { return -0.691 + 10.0 * log10(z); }

__global__ void __launch_bounds__(LPB) loud_item_kernel(const LoudItem* __restrict__ items, int C, long chunks, long segs,
                                                        const double* __restrict__ part, double* __restrict__ seg,
                                                        double* __restrict__ z, const unsigned* __restrict__ peaks,
                                                        const unsigned long long* __restrict__ bad, int want_tp,
                                                        double* __restrict__ stats) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const LoudItem it = items[b];
  const long h = it.h, nseg = it.len / h, J = nseg >= 4 ? nseg - 3 : 0;
  for (long idx = tid; idx < (long)it.ch * nseg; idx += LPB) {
    const long ch = idx / nseg, sg = idx - ch * nseg;
    const double* pt = part + ((long)b * C + ch) * chunks * 2;
    const long ka = sg * h / LOUD_CHUNK, kb = (sg * h + h - 1) / LOUD_CHUNK;
    double sum = 0.0;
    for (long k = ka; k <= kb; ++k) sum += pt[2 * k + (k * LOUD_CHUNK / h == sg ? 0 : 1)];   // (else it starts in sg - 1)
    seg[((long)b * C + ch) * segs + sg] = sum;
  }
  __syncthreads();
  double* zb = z + (long)b * 2 * segs;   // z_j, then l_j
  for (long j = tid; j < J; j += LPB) {
    double v = 0.0;
    for (int ch = 0; ch < it.ch; ++ch) {
      const double* sp = seg + ((long)b * C + ch) * segs + j;
      v += (((sp[0] + sp[1]) + sp[2]) + sp[3]) / (4.0 * (double)h);
    }
    zb[j] = v;
    zb[segs + j] = lufs(v);
  }
  __syncthreads();
  if (tid != 0) return;
  const double inf = __longlong_as_double(0x7ff0000000000000LL), nan = __longlong_as_double(0x7ff8000000000000LL);
  double sum = 0.0, I = -inf;
  long n1 = 0, n2 = 0;
  for (long j = 0; j < J; ++j)
    if (zb[segs + j] > -70.0) sum += zb[j], ++n1;
  if (n1) {
    const double gamma = lufs(sum / (double)n1) - 10.0;
    sum = 0.0;
    for (long j = 0; j < J; ++j)
      if (zb[segs + j] > -70.0 && zb[segs + j] > gamma) sum += zb[j], ++n2;
    if (n2) I = lufs(sum / (double)n2);
  }
  const unsigned long long nb = bad[b];
  double* o = stats + (long)b * 6;
  o[0] = I;
  o[1] = nb || !want_tp ? nan : (double)__uint_as_float(peaks[2 * b]);
  o[2] = nb ? nan : (double)__uint_as_float(peaks[2 * b + 1]);
  o[3] = (double)J;
  o[4] = (double)n2;
  o[5] = (double)nb;
}

struct PeakShape {
  int C, Lmax, S, stride, kmin, kspan, width, want_tp;
};

__global__ void __launch_bounds__(LPB) loud_peak_kernel(const PeakShape q, const float* __restrict__ x,
                                                        const LoudItem* __restrict__ items,
                                                        const float* __restrict__ taps, const int* __restrict__ k0,
                                                        unsigned* __restrict__ peaks, unsigned long long* __restrict__ bad) {
  extern __shared__ __attribute__((aligned(16))) float lp_lds[];
  __shared__ unsigned s_pk[2];
  __shared__ unsigned s_bad;
  const int tabw = (4 * q.stride + 3) & ~3;
  float* s_c = lp_lds;
  int* s_k0 = reinterpret_cast<int*>(lp_lds + tabw);
  float* s_x = lp_lds + tabw + 4;   // (16-byte aligned)
  const int tid = threadIdx.x, b = blockIdx.y, ch = blockIdx.z;
  const LoudItem it = items[b];
  const long m0 = (long)blockIdx.x * LOUD_PEAK_TILE;
  if (ch >= it.ch || m0 >= it.len) return;   // (uniform)
  const int len = it.len;
  const long m1 = m0 + LOUD_PEAK_TILE < len ? m0 + LOUD_PEAK_TILE : len;
  const float* row = x + ((long)b * q.C + ch) * q.Lmax;
  if (tid < 2) s_pk[tid] = 0u;
  if (tid == 2) s_bad = 0u;
  float sp = 0.f, tp = 0.f;
  unsigned nb = 0;
  if (q.want_tp) {
    for (int i = tid; i < 4 * q.stride; i += LPB) s_c[i] = taps[i];
    if (tid < 4) s_k0[tid] = k0[tid];
    const long g0 = m0 + q.kmin - q.width;                    // first sample a lane of this tile may read
    const int count = (int)(m1 - m0) + q.kspan - 1;          // .. and how many follow it
    // s_x[0] is sample g0 - lead, a multiple of 16 bytes in memory
    const int lead = (int)((((long)((uintptr_t)row >> 2) + g0) % 4 + 4) % 4);
    const long gs = g0 - lead;
    const int quads = (count + lead + 3) >> 2;
    for (int v = tid; v < quads; v += LPB) {
      const long i = gs + 4L * v;
      float4 f;
      if (i >= 0 && i + 3 < len) {
        f = *reinterpret_cast<const float4*>(row + i);
      } else {
        f.x = i >= 0 && i < len ? row[i] : 0.f;
        f.y = i + 1 >= 0 && i + 1 < len ? row[i + 1] : 0.f;
        f.z = i + 2 >= 0 && i + 2 < len ? row[i + 2] : 0.f;
        f.w = i + 3 >= 0 && i + 3 < len ? row[i + 3] : 0.f;
      }
      *reinterpret_cast<float4*>(s_x + 4 * v) = f;
    }
    __syncthreads();
    for (int r = 0; r < LOUD_PEAK_TILE / LPB; ++r) {
      const int i = tid + r * LPB;
      if (m0 + i >= m1) break;
      const float v = s_x[lead + i - q.kmin + q.width];
      if (!isfinite(v)) ++nb;
      sp = fmaxf(sp, fabsf(v));
      for (int p = 0; p < 4; ++p) {
        const float* cp = s_c + p * q.stride;
        const float* xp = s_x + lead + i + (s_k0[p] - q.kmin);
        float acc = cp[0] * xp[0];
        for (int s = 1; s < q.S; ++s) acc = fmaf(cp[s], xp[s], acc);
        tp = fmaxf(tp, fabsf(acc));
      }
    }
  } else {
    __syncthreads();
    for (long m = m0 + tid; m < m1; m += LPB) {
      const float v = row[m];
      if (!isfinite(v)) ++nb;
      sp = fmaxf(sp, fabsf(v));
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    sp = fmaxf(sp, __shfl_xor(sp, off));
    tp = fmaxf(tp, __shfl_xor(tp, off));
  }
  if ((tid & 63) == 0) {
    atomicMax(&s_pk[0], __float_as_uint(tp));
    atomicMax(&s_pk[1], __float_as_uint(sp));
  }
  if (nb) atomicAdd(&s_bad, nb);
  __syncthreads();
  if (tid == 0) {
    atomicMax(&peaks[2 * b], s_pk[0]);
    atomicMax(&peaks[2 * b + 1], s_pk[1]);
    if (s_bad) atomicAdd(&bad[b], (unsigned long long)s_bad);
  }
}

__global__ void __launch_bounds__(LPB) apply_gain_kernel(const float* x, const LoudItem* __restrict__ rows,
                                                         const float* __restrict__ gain, float* out, int C, int Lmax) {
  const int r = blockIdx.y, ch = blockIdx.z;
  const LoudItem it = rows[r];
  const long i = 4 * ((long)blockIdx.x * LPB + threadIdx.x);
  if (i >= Lmax) return;
  const long off = ((long)r * C + ch) * Lmax;
  const float* src = x + off;
  float* dst = out + off;
  const int len = ch < it.ch ? it.len : 0;   // a channel the row does not have is all padding
  const float g = gain[r];
  if (i + 3 < Lmax && (((uintptr_t)(src + i) | (uintptr_t)(dst + i)) & 15) == 0 && (i + 3 < len || i >= len)) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < len) {
      v = *reinterpret_cast<const float4*>(src + i);
      v.x = g * v.x, v.y = g * v.y, v.z = g * v.z, v.w = g * v.w;
    }
    *reinterpret_cast<float4*>(dst + i) = v;
    return;
  }
  for (int e = 0; e < 4 && i + e < Lmax; ++e) dst[i + e] = i + e < len ? g * src[i + e] : 0.f;
}

}  // namespace

void kweight_coeffs(int fs, double out[10]) {
  const double rate = (double)fs;
  {
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = tan(M_PI * f0 / rate), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Q + K * K;
    out[0] = (Vh + Vb * K / Q + K * K) / a0;
    out[1] = 2.0 * (K * K - Vh) / a0;
    out[2] = (Vh - Vb * K / Q + K * K) / a0;
    out[3] = 2.0 * (K * K - 1.0) / a0;
    out[4] = (1.0 - K / Q + K * K) / a0;
  }
  {
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = tan(M_PI * f0 / rate), a0 = 1.0 + K / Q + K * K;
    out[5] = 1.0, out[6] = -2.0, out[7] = 1.0;
    out[8] = 2.0 * (K * K - 1.0) / a0;
    out[9] = (1.0 - K / Q + K * K) / a0;
  }
}

// P [4][4]: the cascade's state after LOUD_CHUNK samples of zero input, as a function of the state before them
void kweight_chunk_transition(const double c[10], double P[16]) {
  double M[16], A[16], T[16];
  for (int col = 0; col < 4; ++col) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    s[col] = 1.0;
    kw_step(c, 0.0, s);
    for (int r = 0; r < 4; ++r) M[4 * r + col] = s[r];
  }
  static_assert((LOUD_CHUNK & (LOUD_CHUNK - 1)) == 0, "the chunk transition is formed by squaring");
  std::copy(M, M + 16, A);
  for (int n = 1; n < LOUD_CHUNK; n *= 2) {
    for (int r = 0; r < 4; ++r)
      for (int q = 0; q < 4; ++q) {
        double v = 0.0;
        for (int k = 0; k < 4; ++k) v += A[4 * r + k] * A[4 * k + q];
        T[4 * r + q] = v;
      }
    std::copy(T, T + 16, A);
  }
  std::copy(A, A + 16, P);
}

void launch_loudness(const float* x, const LoudItem* items, const LoudRate* rates, int B, int C, int Lmax, double* state,
                     double* part, double* seg, double* z, unsigned* peaks, unsigned long long* bad, double* stats,
                     const float* taps, const int* k0, int S, int stride, int kmin, int kspan, int width, int want_tp,
                     hipStream_t s) {
  const long chunks = loudness_chunks(Lmax), segs = loudness_segments(Lmax);
  const dim3 fgrid((unsigned)((chunks + LPB - 1) / LPB), (unsigned)B, (unsigned)C);
  hipLaunchKernelGGL(loud_filter_kernel<false>, fgrid, dim3(LPB), 0, s, x, items, rates, C, Lmax, chunks, state, part);
  hipLaunchKernelGGL(loud_carry_kernel, dim3((unsigned)B, (unsigned)C), dim3(LPB), 0, s, items, rates, C, chunks, state);
  hipLaunchKernelGGL(loud_filter_kernel<true>, fgrid, dim3(LPB), 0, s, x, items, rates, C, Lmax, chunks, state, part);
  const PeakShape q{C, Lmax, S, stride, kmin, kspan, width, want_tp ? 1 : 0};
  const dim3 pgrid((unsigned)(((long)Lmax + LOUD_PEAK_TILE - 1) / LOUD_PEAK_TILE), (unsigned)B, (unsigned)C);
  // the tables (4 phases, k0), a tile, its halo, up to 3 samples of lead-in and 3 to a whole quad
  const size_t lds = sizeof(float) * (size_t)(((4 * stride + 3) & ~3) + 4 + LOUD_PEAK_TILE + kspan + 8);
  hipLaunchKernelGGL(loud_peak_kernel, pgrid, dim3(LPB), lds, s, q, x, items, taps, k0, peaks, bad);
  hipLaunchKernelGGL(loud_item_kernel, dim3((unsigned)B), dim3(LPB), 0, s, items, C, chunks, segs, part, seg, z, peaks,
                     bad, want_tp ? 1 : 0, stats);
}

void launch_apply_gain(const float* x, const LoudItem* rows, const float* gain, float* out, int R, int C, int Lmax,
                       hipStream_t s) {
  const long quads = ((long)Lmax + 3) / 4;
  const dim3 grid((unsigned)((quads + LPB - 1) / LPB), (unsigned)R, (unsigned)C);
  hipLaunchKernelGGL(apply_gain_kernel, grid, dim3(LPB), 0, s, x, rows, gain, out, C, Lmax);
}
