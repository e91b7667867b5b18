// True-peak look-ahead limiter for a ragged batch with per-item rates (dsn_limiter_curve, dsn_apply_curve;
// include/ditsep_hip.h states the definition, tests/limiter_restatement.py restates it in float64).
//
// A group is the set of rows that share one gain curve.  Two launches over tiles of LIM_TILE samples counted from the
// group's own start, with a workspace between them, so that no step depends on which workgroup runs it:
//   lim_env_kernel     one workgroup per (tile, group): every (row, channel) of the group goes through LDS with the halo
//                      of the 1 -> 4 interpolator, as y = G x; each thread keeps the running envelope p of its samples
//                      in registers (max |y|, |u[4t .. 4t + 3]|, the phases in fp32 exactly as loudness.hip forms them)
//                      and writes the required gain r = min(1, c / p) to the workspace
//   lim_curve_kernel   one workgroup per (tile, group): r over the tile and 2 W samples on either side in LDS (1 outside
//                      the item), the hold m by doubling minima between two LDS arrays (a minimum does not depend on
//                      its order), the deficit 1 - m, then a[t] by fma in tap order and g.  A tile whose 2 W
//                      neighbourhood needs no reduction writes 1.0f and leaves; a sample whose does not skips the sum --
//                      every term it skips is +0, so the bits are those of the sum.
// The smallest g and the counts are integer atomics on the bits (g lies in [0, 1]); no floating-point atomics.
#include "../../include/ditsep_hip.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int LMB = 256;
constexpr int LIM_PER = LIM_TILE / LMB;

struct EnvShape {
  int C, Lmax, S, stride, kmin, kspan, width;
  float ceiling;
};

__global__ void __launch_bounds__(LMB) lim_env_kernel(const EnvShape q, const float* __restrict__ x,
                                                      const LimRow* __restrict__ rows,
                                                      const LimGroup* __restrict__ groups,
                                                      const float* __restrict__ taps, const int* __restrict__ k0,
                                                      float* __restrict__ req, float* __restrict__ env,
                                                      unsigned long long* __restrict__ bad) {
  extern __shared__ __attribute__((aligned(16))) float le_lds[];
  __shared__ unsigned s_bad;
  const int tabw = (4 * q.stride + 3) & ~3;
  float* s_c = le_lds;
  int* s_k0 = reinterpret_cast<int*>(le_lds + tabw);
  float* s_x = le_lds + tabw + 4;   // (16-byte aligned)
  const int tid = threadIdx.x, g = blockIdx.y;
  const LimGroup gr = groups[g];
  const long m0 = (long)blockIdx.x * LIM_TILE;
  if (m0 >= gr.len) return;   // (uniform)
  const int len = gr.len;
  const long m1 = m0 + LIM_TILE < len ? m0 + LIM_TILE : len;
  for (int i = tid; i < 4 * q.stride; i += LMB) s_c[i] = taps[i];
  if (tid < 4) s_k0[tid] = k0[tid];
  if (tid == 4) s_bad = 0u;
  const long g0 = m0 + q.kmin - q.width;             // first sample a lane of this tile may read
  const int count = (int)(m1 - m0) + q.kspan - 1;   // .. and how many follow it
  const float G = gr.pregain;
  float p[LIM_PER];
#pragma unroll
  for (int r = 0; r < LIM_PER; ++r) p[r] = 0.f;
  unsigned nb = 0;
  for (int row = gr.row0; row < gr.row1; ++row) {
    const int nch = rows[row].ch;
    for (int ch = 0; ch < nch; ++ch) {
      const float* src = x + ((long)row * q.C + ch) * q.Lmax;
      // s_x[0] is sample g0 - lead, a multiple of 16 bytes in memory
      const int lead = (int)((((long)((uintptr_t)src >> 2) + g0) % 4 + 4) % 4);
      const long gs = g0 - lead;
      const int quads = (count + lead + 3) >> 2;
      __syncthreads();   // the tables are in place; the previous row has been read
      for (int v = tid; v < quads; v += LMB) {
        const long i = gs + 4L * v;
        float4 f;
        if (i >= 0 && i + 3 < len) {
          f = *reinterpret_cast<const float4*>(src + i);
          f.x = G * f.x, f.y = G * f.y, f.z = G * f.z, f.w = G * f.w;
        } else {
          f.x = i >= 0 && i < len ? G * src[i] : 0.f;
          f.y = i + 1 >= 0 && i + 1 < len ? G * src[i + 1] : 0.f;
          f.z = i + 2 >= 0 && i + 2 < len ? G * src[i + 2] : 0.f;
          f.w = i + 3 >= 0 && i + 3 < len ? G * src[i + 3] : 0.f;
        }
        *reinterpret_cast<float4*>(s_x + 4 * v) = f;
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < LIM_PER; ++r) {
        const int i = tid + r * LMB;
        if (m0 + i < m1) {
          const float v = s_x[lead + i - q.kmin + q.width];
          if (!isfinite(v)) ++nb;
          float e = fmaxf(p[r], fabsf(v));
          for (int ph = 0; ph < 4; ++ph) {
            const float* cp = s_c + ph * q.stride;
            const float* xp = s_x + lead + i + (s_k0[ph] - q.kmin);
            float acc = cp[0] * xp[0];
            for (int s = 1; s < q.S; ++s) acc = fmaf(cp[s], xp[s], acc);
            e = fmaxf(e, fabsf(acc));
          }
          p[r] = e;
        }
      }
    }
  }
  const float c = q.ceiling;
#pragma unroll
  for (int r = 0; r < LIM_PER; ++r) {
    const long t = m0 + tid + r * LMB;
    if (t < m1) {
      float rq = 1.f;
      if (p[r] > 0.f) {
        rq = fminf(1.f, __fdiv_rn(c, p[r]));
        // the division is rounded to nearest, so rq p may round to the float above c: then the next float below
        if (rq * p[r] > c) rq = __uint_as_float(__float_as_uint(rq) - 1u);
      }
      req[(long)g * q.Lmax + t] = rq;
      if (env) env[(long)g * q.Lmax + t] = p[r];
    }
  }
  if (nb) atomicAdd(&s_bad, nb);
  __syncthreads();
  if (tid == 0 && s_bad) atomicAdd(&bad[g], (unsigned long long)s_bad);
}

__global__ void __launch_bounds__(LMB) lim_curve_kernel(const LimGroup* __restrict__ groups,
                                                        const float* __restrict__ window,
                                                        const float* __restrict__ req, float* __restrict__ curve,
                                                        int Lmax, int Wmax, const unsigned long long* __restrict__ bad,
                                                        unsigned long long* __restrict__ reduced,
                                                        unsigned* __restrict__ deepest) {
  extern __shared__ __attribute__((aligned(16))) float lc_lds[];
  __shared__ unsigned s_deep, s_cnt;
  const int tid = threadIdx.x, g = blockIdx.y;
  const LimGroup gr = groups[g];
  const int len = gr.len, W = gr.W;
  const long m0 = (long)blockIdx.x * LIM_TILE;
  const long mt = m0 + LIM_TILE < Lmax ? m0 + LIM_TILE : Lmax;   // the tile's end in the buffer
  const long m1 = mt < len ? mt : len;                           // .. and in the item (may lie before m0)
  float* out = curve + (long)g * Lmax;
  const float* rq = req + (long)g * Lmax;
  // at or past the item's end the curve is 1; an item with non-finite samples has a NaN curve
  const float fill = bad[g] ? __uint_as_float(0x7fc00000u) : 1.f;
  for (long t = m0 + tid; t < mt; t += LMB)
    if (t >= len) out[t] = 1.f;
  if (m0 >= len) return;   // (uniform)
  if (bad[g]) {
    for (long t = m0 + tid; t < m1; t += LMB) out[t] = fill;
    return;
  }
  const int n = (int)(m1 - m0) + 4 * W;   // r over [m0 - 2 W, m1 + 2 W)
  float* A = lc_lds;
  float* B = lc_lds + LIM_TILE + 4 * Wmax;
  float* s_w = B + LIM_TILE + 4 * Wmax;
  if (tid == 0) s_deep = 0u, s_cnt = 0u;
  int any = 0;
  for (int i = tid; i < n; i += LMB) {
    const long t = m0 - 2 * W + i;
    const float v = t >= 0 && t < len ? rq[t] : 1.f;
    A[i] = v;
    any |= v < 1.f;
  }
  const float* wg = window + (long)gr.wofs * (2 * LIM_MAX_W + 1);
  for (int i = tid; i < 2 * W + 1; i += LMB) s_w[i] = wg[i];
  if (!__syncthreads_or(any)) {   // the copy path: nothing within 2 W of the tile needs reducing
    for (long t = m0 + tid; t < m1; t += LMB) out[t] = 1.f;
    return;
  }
  // minima over windows of 1, 2, 4, .. samples to the right, up to the largest power of two <= 2 W + 1
  float *src = A, *dst = B;
  int s = 1;
  for (; 2 * s <= 2 * W + 1; s *= 2) {
    for (int i = tid; i < n; i += LMB) dst[i] = fminf(src[i], i + s < n ? src[i + s] : 1.f);
    __syncthreads();
    float* tmp = src;
    src = dst, dst = tmp;
  }
  // the hold over [i - W, i + W] from two of those, kept as the deficit 1 - m
  for (int i = W + tid; i < n - W; i += LMB) dst[i] = 1.f - fminf(src[i - W], src[i + W + 1 - s]);
  __syncthreads();
  float low = 1.f;
  unsigned cnt = 0;
  for (int r = 0; r < LIM_PER; ++r) {
    const long t = m0 + tid + r * LMB;
    if (t >= m1) break;
    const float* d = dst + 2 * W + tid + r * LMB;
    float gv = 1.f;
    if (d[-W] != 0.f || d[W] != 0.f) {   // else every term of the sum is +0
      float acc = 0.f;
      for (int k = -W; k <= W; ++k) acc = fmaf(s_w[k + W], d[k], acc);
      gv = fmaxf(0.f, fminf(rq[t], 1.f - acc));
    }
    out[t] = gv;
    low = fminf(low, gv);
    cnt += gv < 1.f;
  }
  for (int off = 32; off > 0; off >>= 1) {
    low = fminf(low, __shfl_xor(low, off));
    cnt += __shfl_xor(cnt, off);
  }
  if ((tid & 63) == 0 && cnt) {
    atomicMax(&s_deep, 0x3f800000u - __float_as_uint(low));   // (g in [0, 1]: its bits order as it does)
    atomicAdd(&s_cnt, cnt);
  }
  __syncthreads();
  if (tid == 0 && s_cnt) {
    atomicMax(&deepest[g], s_deep);
    atomicAdd(&reduced[g], (unsigned long long)s_cnt);
  }
}

__global__ void __launch_bounds__(LMB) apply_curve_kernel(const float* x, const LimRow* __restrict__ rows,
                                                          const float* __restrict__ pregain,
                                                          const float* __restrict__ curve, float* out, int C, int Lmax) {
  const int r = blockIdx.y, ch = blockIdx.z;
  const LimRow it = rows[r];
  const long i = 4 * ((long)blockIdx.x * LMB + threadIdx.x);
  if (i >= Lmax) return;
  const long off = ((long)r * C + ch) * Lmax;
  const float* src = x + off;
  const float* cv = curve + (long)it.group * Lmax;
  float* dst = out + off;
  const int len = ch < it.ch ? it.len : 0;   // a channel the row does not have is all padding
  const float G = pregain[it.group];
  if (i + 3 < Lmax && (((uintptr_t)(src + i) | (uintptr_t)(dst + i) | (uintptr_t)(cv + i)) & 15) == 0 &&
      (i + 3 < len || i >= len)) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < len) {
      v = *reinterpret_cast<const float4*>(src + i);
      const float4 c = *reinterpret_cast<const float4*>(cv + i);
      v.x = (G * v.x) * c.x, v.y = (G * v.y) * c.y, v.z = (G * v.z) * c.z, v.w = (G * v.w) * c.w;
    }
    *reinterpret_cast<float4*>(dst + i) = v;
    return;
  }
  for (int e = 0; e < 4 && i + e < Lmax; ++e) dst[i + e] = i + e < len ? (G * src[i + e]) * cv[i + e] : 0.f;
}

}  // namespace

size_t limiter_curve_lds(int Wmax) { return sizeof(float) * (size_t)(2 * (LIM_TILE + 4 * Wmax) + 2 * Wmax + 1); }

void launch_limiter_curve(const float* x, const LimRow* rows, const LimGroup* groups, int G, int C, int Lmax, int Wmax,
                          float ceiling, const float* window, const float* taps, const int* k0, int S, int stride,
                          int kmin, int kspan, int width, float* req, float* env, float* curve, unsigned long long* bad,
                          unsigned long long* reduced, unsigned* deepest, hipStream_t s) {
  const dim3 grid((unsigned)(((long)Lmax + LIM_TILE - 1) / LIM_TILE), (unsigned)G);
  const EnvShape q{C, Lmax, S, stride, kmin, kspan, width, ceiling};
  // the tables (4 phases, k0), a tile, its halo, up to 3 samples of lead-in and 3 to a whole quad
  const size_t lds = sizeof(float) * (size_t)(((4 * stride + 3) & ~3) + 4 + LIM_TILE + kspan + 8);
  hipLaunchKernelGGL(lim_env_kernel, grid, dim3(LMB), lds, s, q, x, rows, groups, taps, k0, req, env, bad);
  hipLaunchKernelGGL(lim_curve_kernel, grid, dim3(LMB), limiter_curve_lds(Wmax), s, groups, window, req, curve, Lmax,
                     Wmax, bad, reduced, deepest);
}

void launch_apply_curve(const float* x, const LimRow* rows, const float* pregain, const float* curve, float* out, int R,
                        int C, int Lmax, hipStream_t s) {
  const long quads = ((long)Lmax + 3) / 4;
  const dim3 grid((unsigned)((quads + LMB - 1) / LMB), (unsigned)R, (unsigned)C);
  hipLaunchKernelGGL(apply_curve_kernel, grid, dim3(LMB), 0, s, x, rows, pregain, curve, out, C, Lmax);
}
