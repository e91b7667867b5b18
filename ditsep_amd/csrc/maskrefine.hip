// Mixture-consistent STFT masks (dsn_mask_refine; the definition is in include/ditsep_hip.h, restated in float64 in
// tests/mask_refine_restatement.py): soft masks from the magnitudes of the estimates, applied to the mixture's STFT
// and transformed back, so every output carries the mixture's phase and the outputs add up to the mixture.
//
// One launch, no frame workspace.  Workgroup (c, b) owns the output samples [c SPAN, (c + 1) SPAN) of item b, SPAN a
// multiple of every hop, and forms all SPAN / hop + n_fft / hop - 1 frames that touch them itself: the frames it
// shares with its neighbours are recomputed, not exchanged.  Frames go through LDS in groups of 2048 / n_fft:
//   load      the n + 1 signals of a frame (mixture, estimates) from global memory, reflected at the item's own padded
//             end Lp_b and zero at or past lens[b] (never read there), times the window
//   forward   every real frame alone as ONE complex transform of half the length: z[t] = x[2t] + i x[2t + 1] packs its
//             even and odd samples, a Stockham radix-2 in LDS (fp32; twiddles from sincospi in double, rounded once)
//             transforms it, and the conjugate-symmetry split E[k] = (Z[k] + conj Z[H - k]) / 2, O[k] = (Z[k] -
//             conj Z[H - k]) / 2i, X[k] = E[k] + w^k O[k], X[H - k] = conj(E[k] - w^k O[k]) gives bins 0 .. n_fft / 2
//   masks     per bin a_i = |S_i|^power, M_i = (a_i + eps) / (((a_0 + a_1) + ..) + n eps), Y_i = M_i X -- and at once
//             the inverse of the split, so the n spectra are again half-length complex transforms in place
//   inverse   the same Stockham with conjugated twiddles; Re and Im are the even and odd samples of the frame
//   add       y w / n_fft added into the workgroup's SPAN samples in LDS, frame after frame in frame order
// and at the end every sample is divided by the sum of w^2 over the frames of the item that cover it (in frame order)
// and stored, 16 bytes at a time where the rows allow; at or past lens[b] the row is written as zero.
//
// A pair of signals is NOT packed into one full-length transform: there the rounding of one signal's spectrum depends
// on its partner, and the contract's exact cases (n = 1 hands the mixture's own transform back whatever the estimate
// holds; silent estimates give the n = 1 bits scaled by 1 / n) would not hold.  Packing a signal's own even and odd
// samples costs no more butterflies (2 x H/2 log2 H against H log2 2H for a pair) and leaves no odd source over.
//
// Bit identity: a frame's values depend on the item's samples and the frame index alone -- the same code with floating
// point contraction off and the fused multiply-adds written out, whichever workgroup and frame slot computes it --,
// every sample adds its frames in increasing frame order starting from +0, and there are no atomics.  So the result
// does not depend on SPAN, on the batch position or on the other items, and two calls give identical bits.
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int MRT = 256;                          // threads
constexpr int MR_MAX_SRC = MASK_REFINE_MAX_SRC;
constexpr int MR_POINTS = 1024;                   // complex points per signal in LDS: 2048 / NFFT frames at a time
constexpr int MR_BF = (MR_MAX_SRC + 1) * (MR_POINTS / 2) / MRT;   // butterflies per thread and stage at n = 4

template <int NFFT>
constexpr int mr_span() { return NFFT >= 2048 ? 4096 : 2048; }

struct MaskRefineShape {
  int n, Lmax, hop, power;
  float eps;
  int vec;   // out is 16-byte aligned and Lmax % 4 == 0: whole quads are stored at once
};

// `nbf` butterflies per stage = transforms * H / 2; natural order in and out.  A stage reads x[j], x[j + H / 2] of
// every transform into registers and, after a barrier, writes the butterfly to ((j - k) << 1) + k and that + Ns,
// k = j mod Ns.  tw[k] = exp(-2 pi i k / (2 H)).  Ends with a barrier.
template <int H, bool INV>
__device__ __forceinline__ void mr_fft(float2* __restrict__ base, const float2* __restrict__ tw, int nbf, int tid) {
  constexpr int LOGH = __builtin_ctz(H);
  for (int ls = 0; ls < LOGH; ++ls) {
    const int Ns = 1 << ls;
    float2 u[MR_BF], v[MR_BF];
#pragma unroll
    for (int q = 0; q < MR_BF; ++q) {
      const int bf = tid + q * MRT;
      if (bf < nbf) {
        const float2* a = base + (bf >> (LOGH - 1)) * H;
        const int j = bf & (H / 2 - 1), k = j & (Ns - 1);
        float2 tf = tw[k << (LOGH - ls)];
        if (INV) tf.y = -tf.y;
        const float2 z = a[j + H / 2];
        u[q] = a[j];
        v[q] = make_float2(fmaf(tf.x, z.x, -(tf.y * z.y)), fmaf(tf.x, z.y, tf.y * z.x));
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < MR_BF; ++q) {
      const int bf = tid + q * MRT;
      if (bf < nbf) {
        float2* a = base + (bf >> (LOGH - 1)) * H;
        const int j = bf & (H / 2 - 1), k = j & (Ns - 1), j0 = ((j - k) << 1) + k;
        a[j0] = make_float2(u[q].x + v[q].x, u[q].y + v[q].y);
        a[j0 + Ns] = make_float2(u[q].x - v[q].x, u[q].y - v[q].y);
      }
    }
    __syncthreads();
  }
}

// bins k and H - k (k = 0: bins 0 and H, both real) of the real signal whose packed transform holds zk = Z[k],
// zm = Z[H - k]; t = exp(-2 pi i k / NFFT)
__device__ __forceinline__ void mr_split(float2 zk, float2 zm, float2 t, float2& xk, float2& xm) {
  const float ex = 0.5f * (zk.x + zm.x), ey = 0.5f * (zk.y - zm.y);
  const float ox = 0.5f * (zk.y + zm.y), oy = -0.5f * (zk.x - zm.x);
  const float tx = fmaf(t.x, ox, -(t.y * oy)), ty = fmaf(t.x, oy, t.y * ox);
  xk = make_float2(ex + tx, ey + ty);
  xm = make_float2(ex - tx, -(ey - ty));
}

// .. and back: the packed transform's Z[k], Z[H - k] (times 2) of the real signal with bins yk, ym
__device__ __forceinline__ void mr_merge(float2 yk, float2 ym, float2 t, float2& zk, float2& zm) {
  const float ex = yk.x + ym.x, ey = yk.y - ym.y;
  const float dx = yk.x - ym.x, dy = yk.y + ym.y;
  const float ox = fmaf(t.x, dx, t.y * dy), oy = fmaf(t.x, dy, -(t.y * dx));   // conj(t) d
  zk = make_float2(ex - oy, ey + ox);
  zm = make_float2(ex + oy, ox - ey);
}

__device__ __forceinline__ float mr_mag(float2 s, int power) {
  const float p = fmaf(s.x, s.x, s.y * s.y);
  return power == 1 ? sqrtf(p) : p;
}

__device__ __forceinline__ void mr_store(const MaskRefineShape& q, float* __restrict__ row, int p, float4 v) {
  if (q.vec) {
    *reinterpret_cast<float4*>(row + p) = v;   // (p % 4 == 0 and Lmax % 4 == 0: the quad lies inside the row)
  } else {
    if (p < q.Lmax) row[p] = v.x;
    if (p + 1 < q.Lmax) row[p + 1] = v.y;
    if (p + 2 < q.Lmax) row[p + 2] = v.z;
    if (p + 3 < q.Lmax) row[p + 3] = v.w;
  }
}

// mix [B][Lmax], est / out [B][n][Lmax], lens [B] or null.  Grid (ceil(Lmax / SPAN), B).
// Dynamic LDS: float2 tw[H] | float2 buf[n + 1][G][H] | float win[NFFT] | float ola[n][SPAN]
template <int NFFT>
__global__ __launch_bounds__(MRT) void mask_refine_kernel(const MaskRefineShape q, const float* __restrict__ mix,
                                                          const float* __restrict__ est,
                                                          const int* __restrict__ lens, float* __restrict__ out) {
  static_assert(NFFT >= 64 && NFFT <= 2 * MR_POINTS && (NFFT & (NFFT - 1)) == 0, "FFT size");
  constexpr int H = NFFT / 2, LOGH = __builtin_ctz(H), G = MR_POINTS / H, NP = H / 2 + 1, SPAN = mr_span<NFFT>();
  extern __shared__ __attribute__((aligned(16))) float2 mr_lds[];
  const int n = q.n, hop = q.hop, r = NFFT / hop, tid = threadIdx.x;
  float2* tw = mr_lds;
  float2* buf = tw + H;
  float* win = reinterpret_cast<float*>(buf + (n + 1) * MR_POINTS);
  float* ola = win + NFFT;
  const int b = blockIdx.y, s0 = blockIdx.x * SPAN;
  const int L = lens ? lens[b] : q.Lmax;
  const int Lp = (L + hop - 1) / hop * hop, F = 1 + Lp / hop;
  const float* mixb = mix + (long)b * q.Lmax;
  const float* estb = est + (long)b * n * q.Lmax;
  float* outb = out + (long)b * n * q.Lmax;

  if (s0 >= L) {   // (uniform) the whole span lies past the item's end
    for (int i = 0; i < n; ++i)
      for (int v = tid; v < SPAN / 4; v += MRT)
        if (s0 + 4 * v < q.Lmax) mr_store(q, outb + (long)i * q.Lmax, s0 + 4 * v, make_float4(0.f, 0.f, 0.f, 0.f));
    return;
  }

  for (int t = tid; t < H; t += MRT) {
    double s, c;
    sincospi((double)t / H, &s, &c);   // exp(-2 pi i t / NFFT)
    tw[t] = make_float2((float)c, (float)-s);
  }
  for (int t = tid; t < NFFT; t += MRT) win[t] = (float)(0.5 - 0.5 * cospi((double)t / H));   // periodic Hann
  for (int e = tid; e < n * SPAN; e += MRT) ola[e] = 0.f;

  // sample p is covered by the r frames (p + H) / hop - r + 1 .. (p + H) / hop, where they exist
  const int pend = min(s0 + SPAN, L);
  const int f_first = max(0, (s0 + H) / hop - r + 1), f_last = min(F - 1, (pend - 1 + H) / hop);
  const float inv_n = 1.f / (float)NFFT;   // mr_merge hands back twice the packed transform: 1 / (2 H)

  for (int f0 = f_first; f0 <= f_last; f0 += G) {
    __syncthreads();   // the tables are in; the previous group's frames have been added
    // ---- load: slot fg holds frame f0 + fg of every signal, even samples in .x and odd in .y, windowed
    for (int e = tid; e < G * H; e += MRT) {
      const int fg = e >> LOGH, tp = e & (H - 1), f = f0 + fg;
      const bool valid = f <= f_last;
      int i0 = f * hop - H + 2 * tp, i1 = i0 + 1;   // (f hop <= Lp: no overflow)
      i0 = i0 < 0 ? -i0 : i0;
      i1 = i1 < 0 ? -i1 : i1;
      i0 = i0 >= Lp ? 2 * (Lp - 1) - i0 : i0;   // Lp > H: one reflection reaches [0, Lp)
      i1 = i1 >= Lp ? 2 * (Lp - 1) - i1 : i1;
      const float w0 = win[2 * tp], w1 = win[2 * tp + 1];
      for (int s = 0; s <= n; ++s) {
        const float* row = s == 0 ? mixb : estb + (long)(s - 1) * q.Lmax;
        const float v0 = valid && i0 < L ? row[i0] : 0.f;
        const float v1 = valid && i1 < L ? row[i1] : 0.f;
        buf[(s * G + fg) * H + tp] = make_float2(v0 * w0, v1 * w1);
      }
    }
    __syncthreads();
    mr_fft<H, false>(buf, tw, (n + 1) * (MR_POINTS / 2), tid);
    // ---- masks: one thread per (frame, pair of bins k and H - k); the estimates' slots become Y_i, packed again
    for (int e = tid; e < G * NP; e += MRT) {
      const int fg = e / NP, k = e - fg * NP, km = (H - k) & (H - 1);
      if (f0 + fg > f_last) continue;
      const float2 t = tw[k];
      float2 xk, xm, sk[MR_MAX_SRC], sm[MR_MAX_SRC];
      float ak[MR_MAX_SRC], am[MR_MAX_SRC];
      {
        const float2* a = buf + fg * H;
        mr_split(a[k], a[km], t, xk, xm);
      }
      float dk = 0.f, dm = 0.f;
#pragma unroll
      for (int i = 0; i < MR_MAX_SRC; ++i)
        if (i < n) {
          const float2* a = buf + ((i + 1) * G + fg) * H;
          mr_split(a[k], a[km], t, sk[i], sm[i]);
          ak[i] = mr_mag(sk[i], q.power);
          am[i] = mr_mag(sm[i], q.power);
          dk = i == 0 ? ak[i] : dk + ak[i];
          dm = i == 0 ? am[i] : dm + am[i];
        }
      const float ne = (float)n * q.eps;
      dk = dk + ne;
      dm = dm + ne;
#pragma unroll
      for (int i = 0; i < MR_MAX_SRC; ++i)
        if (i < n) {
          const float mk = (ak[i] + q.eps) / dk, mm = (am[i] + q.eps) / dm;
          float2 zk, zm;
          mr_merge(make_float2(mk * xk.x, mk * xk.y), make_float2(mm * xm.x, mm * xm.y), t, zk, zm);
          float2* a = buf + ((i + 1) * G + fg) * H;
          a[k] = zk;
          if (km != k) a[km] = zm;
        }
    }
    __syncthreads();
    mr_fft<H, true>(buf + MR_POINTS, tw, n * (MR_POINTS / 2), tid);
    // ---- add: a thread owns quads of samples for the whole launch, so every sample's sum runs in frame order
    const int g_last = min(f0 + G - 1, f_last);
    for (int i = 0; i < n; ++i) {
      const float* y = reinterpret_cast<const float*>(buf + (i + 1) * MR_POINTS);
      for (int v = tid; v < SPAN / 4; v += MRT) {
        const int p = s0 + 4 * v;
        if (p >= pend) continue;
        const int fhi = (p + H) / hop;   // (hop % 4 == 0: the same frames cover the whole quad)
        const int fa = max(fhi - r + 1, f0), fb = min(fhi, g_last);
        float4 acc = *reinterpret_cast<float4*>(ola + i * SPAN + 4 * v);
        for (int f = fa; f <= fb; ++f) {
          const int t = p + H - f * hop;
          const float4 yv = *reinterpret_cast<const float4*>(y + (f - f0) * NFFT + t);
          const float4 wv = *reinterpret_cast<const float4*>(win + t);
          acc.x = acc.x + (yv.x * inv_n) * wv.x;
          acc.y = acc.y + (yv.y * inv_n) * wv.y;
          acc.z = acc.z + (yv.z * inv_n) * wv.z;
          acc.w = acc.w + (yv.w * inv_n) * wv.w;
        }
        *reinterpret_cast<float4*>(ola + i * SPAN + 4 * v) = acc;
      }
    }
  }

  // ---- the envelope of the frames that exist, the division and the store (the quads this thread summed itself)
  for (int v = tid; v < SPAN / 4; v += MRT) {
    const int p = s0 + 4 * v;
    if (p >= q.Lmax) continue;
    float env[4] = {0.f, 0.f, 0.f, 0.f};
    if (p < pend) {
      const int fhi = (p + H) / hop;
      const int fa = max(fhi - r + 1, 0), fb = min(fhi, F - 1);
      for (int f = fa; f <= fb; ++f) {
        const float4 wv = *reinterpret_cast<const float4*>(win + (p + H - f * hop));
        env[0] = env[0] + wv.x * wv.x;
        env[1] = env[1] + wv.y * wv.y;
        env[2] = env[2] + wv.z * wv.z;
        env[3] = env[3] + wv.w * wv.w;
      }
    }
    for (int i = 0; i < n; ++i) {
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p < pend) {
        const float4 acc = *reinterpret_cast<const float4*>(ola + i * SPAN + 4 * v);
        o.x = acc.x / env[0];
        o.y = p + 1 < L ? acc.y / env[1] : 0.f;
        o.z = p + 2 < L ? acc.z / env[2] : 0.f;
        o.w = p + 3 < L ? acc.w / env[3] : 0.f;
      }
      mr_store(q, outb + (long)i * q.Lmax, p, o);
    }
  }
}

template <int NFFT>
size_t mr_lds_bytes(int n) {
  return sizeof(float2) * ((size_t)NFFT / 2 + (size_t)(n + 1) * MR_POINTS) +
         sizeof(float) * ((size_t)NFFT + (size_t)n * mr_span<NFFT>());
}

template <int NFFT>
void mr_launch(const MaskRefineShape& q, const float* mix, const float* est, const int* lens, float* out, int B,
               hipStream_t st) {
  dsn_allow_lds<mask_refine_kernel<NFFT>>((int)mr_lds_bytes<NFFT>(MR_MAX_SRC));
  const dim3 grid((unsigned)((q.Lmax + mr_span<NFFT>() - 1) / mr_span<NFFT>()), (unsigned)B);
  hipLaunchKernelGGL((mask_refine_kernel<NFFT>), grid, dim3(MRT), mr_lds_bytes<NFFT>(q.n), st, q, mix, est, lens, out);
}

}  // namespace

bool mask_refine_fft_ok(int nfft) { return nfft >= 64 && nfft <= 2 * MR_POINTS && (nfft & (nfft - 1)) == 0; }

void launch_mask_refine(const float* mix, const float* est, const int* lens, float* out, int B, int n, int Lmax,
                        int nfft, int hop, int power, float eps, hipStream_t st) {
  const MaskRefineShape q{n, Lmax, hop, power, eps, ((uintptr_t)out & 15) == 0 && Lmax % 4 == 0 ? 1 : 0};
  switch (nfft) {
    case 64: mr_launch<64>(q, mix, est, lens, out, B, st); break;
    case 128: mr_launch<128>(q, mix, est, lens, out, B, st); break;
    case 256: mr_launch<256>(q, mix, est, lens, out, B, st); break;
    case 512: mr_launch<512>(q, mix, est, lens, out, B, st); break;
    case 1024: mr_launch<1024>(q, mix, est, lens, out, B, st); break;
    default: mr_launch<2048>(q, mix, est, lens, out, B, st); break;
  }
}
