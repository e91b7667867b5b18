// The STFT frame pipeline of dsn_mask_refine, dsn_stems (maskrefine.hip), dsn_beamform (beamform.hip) and dsn_dereverb
// (dereverb.hip), in the order a frame passes through it: the span and LDS layout, the item's geometry, the twiddle and
// window tables (mr_tables), the frame load (mr_load), the packed real transform in LDS (mr_fft), its split and merge,
// the masks, the overlap-add (mr_add), the envelope division (mr_finish) and the row store.  Every kernel of the three
// files forms its frames, spectra, masks and output samples by calling exactly these functions, floating point
// contraction off, so they have the same bits wherever they are formed.
// Include it inside the file's own unnamed namespace, after kernels.h and `#pragma clang fp contract(off)`.
#pragma once

constexpr int MRT = 256;                          // threads
constexpr int MR_MAX_SRC = MASK_REFINE_MAX_SRC;
constexpr int MR_POINTS = 1024;                   // complex points per signal in LDS: 2048 / NFFT frames at a time

struct MaskRefineShape {
  int n, Lmax, hop, power;
  float eps;
  int vec;   // out is 16-byte aligned and Lmax % 4 == 0: whole quads are stored at once
  int C;     // channels of mix (and of every out[b][i]); the mono call has 1
  float reg;
};

// output samples a workgroup owns, a multiple of every hop; a statistics owner takes the frames of whole spans
constexpr int mr_span(int nfft) { return nfft >= 2048 ? 4096 : 2048; }

// Dynamic LDS of every kernel here: float2 tw[H] | float2 buf[slots][G][H] | float win[NFFT] | float ola[rows][SPAN]
inline size_t mr_lds_bytes(int nfft, int slots, int ola_rows) {
  return sizeof(float2) * ((size_t)nfft / 2 + (size_t)slots * MR_POINTS) +
         sizeof(float) * ((size_t)nfft + (size_t)ola_rows * mr_span(nfft));
}

// fn(std::integral_constant<int, NFFT>) for the size mask_refine_fft_ok accepted
template <class Fn>
void mr_for_nfft(int nfft, Fn&& fn) {
  switch (nfft) {
    case 64: fn(std::integral_constant<int, 64>{}); break;
    case 128: fn(std::integral_constant<int, 128>{}); break;
    case 256: fn(std::integral_constant<int, 256>{}); break;
    case 512: fn(std::integral_constant<int, 512>{}); break;
    case 1024: fn(std::integral_constant<int, 1024>{}); break;
    default: fn(std::integral_constant<int, 2048>{}); break;
  }
}

// item b: L samples, Lp = L rounded up to whole hops, F = 1 + Lp / hop frames (centred, reflected at 0 and at Lp)
struct MrItem {
  int L, Lp, F;
};
__device__ __forceinline__ MrItem mr_item(const int* __restrict__ lens, int b, int Lmax, int hop) {
  const int L = lens ? lens[b] : Lmax, Lp = (L + hop - 1) / hop * hop;
  return MrItem{L, Lp, 1 + Lp / hop};
}

// The output samples [s0, pend) of the span at s0 and the frames f_first .. f_last that touch them: sample p is
// covered by the r = 2 H / hop frames (p + H) / hop - r + 1 .. (p + H) / hop, where they exist.
struct MrFrames {
  int pend, f_first, f_last;
};
template <int H>
__device__ __forceinline__ MrFrames mr_frames(const MrItem& it, int s0, int hop) {
  const int r = 2 * H / hop, pend = min(s0 + mr_span(2 * H), it.L);
  return MrFrames{pend, max(0, (s0 + H) / hop - r + 1), min(it.F - 1, (pend - 1 + H) / hop)};
}

// tw[t] = exp(-2 pi i t / NFFT) (sincospi in double, rounded once) and the periodic Hann window
template <int H>
__device__ __forceinline__ void mr_tables(float2* tw, float* win, int tid) {
  for (int t = tid; t < H; t += MRT) {
    double s, c;
    sincospi((double)t / H, &s, &c);
    tw[t] = make_float2((float)c, (float)-s);
  }
  for (int t = tid; t < 2 * H; t += MRT) win[t] = (float)(0.5 - 0.5 * cospi((double)t / H));
}

// The load: slot fg of signal s holds frame f0 + fg (zero past f_last), even samples in .x and odd in .y, windowed,
// reflected at the item's own padded end Lp and zero at or past L (never read there).  Signals 0 .. nx - 1 are the rows
// of mixb, then the ne rows of estb, Lmax apart.
template <int H>
__device__ __forceinline__ void mr_load(float2* buf, const float* win, const float* mixb, const float* estb, int Lmax,
                                        const MrItem& it, int hop, int nx, int ne, int f0, int f_last, int tid) {
  constexpr int LOGH = __builtin_ctz(H), G = MR_POINTS / H;
  const int L = it.L, Lp = it.Lp;
  for (int e = tid; e < G * H; e += MRT) {
    const int fg = e >> LOGH, tp = e & (H - 1), f = f0 + fg;
    const bool valid = f <= f_last;
    int i0 = f * hop - H + 2 * tp, i1 = i0 + 1;   // (f hop <= Lp: no overflow)
    i0 = i0 < 0 ? -i0 : i0;
    i1 = i1 < 0 ? -i1 : i1;
    i0 = i0 >= Lp ? 2 * (Lp - 1) - i0 : i0;   // Lp > H: one reflection reaches [0, Lp)
    i1 = i1 >= Lp ? 2 * (Lp - 1) - i1 : i1;
    const float w0 = win[2 * tp], w1 = win[2 * tp + 1];
    for (int s = 0; s < nx + ne; ++s) {
      const float* row = s < nx ? mixb + (long)s * Lmax : estb + (long)(s - nx) * Lmax;
      const float v0 = valid && i0 < L ? row[i0] : 0.f;
      const float v1 = valid && i1 < L ? row[i1] : 0.f;
      buf[(s * G + fg) * H + tp] = make_float2(v0 * w0, v1 * w1);
    }
  }
}

// `nbf` butterflies per stage = transforms * H / 2; natural order in and out.  A stage reads x[j], x[j + H / 2] of
// every transform into registers and, after a barrier, writes the butterfly to ((j - k) << 1) + k and that + Ns,
// k = j mod Ns.  tw[k] = exp(-2 pi i k / (2 H)).  Ends with a barrier.
template <int H, bool INV, int BF>
__device__ __forceinline__ void mr_fft(float2* __restrict__ base, const float2* __restrict__ tw, int nbf, int tid) {
  constexpr int LOGH = __builtin_ctz(H);
  for (int ls = 0; ls < LOGH; ++ls) {
    const int Ns = 1 << ls;
    float2 u[BF], v[BF];
#pragma unroll
    for (int q = 0; q < BF; ++q) {
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
    for (int q = 0; q < BF; ++q) {
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

// vec: the row is 16-byte aligned and Lmax % 4 == 0, so whole quads are stored at once
__device__ __forceinline__ void mr_store(int vec, int Lmax, float* __restrict__ row, int p, float4 v) {
  if (vec) {
    *reinterpret_cast<float4*>(row + p) = v;   // (p % 4 == 0 and Lmax % 4 == 0: the quad lies inside the row)
  } else {
    if (p < Lmax) row[p] = v.x;
    if (p + 1 < Lmax) row[p + 1] = v.y;
    if (p + 2 < Lmax) row[p + 2] = v.z;
    if (p + 3 < Lmax) row[p + 3] = v.w;
  }
}

// The masks of bins k and km = H - k of one frame: e -> the frame's slot in the first estimate's transforms, the
// next estimate's MR_POINTS further; t = exp(-2 pi i k / NFFT).
__device__ __forceinline__ void mr_masks(const MaskRefineShape& q, const float2* __restrict__ e, int k, int km, float2 t,
                                         float* mk, float* mm) {
  const int n = q.n;
  float ak[MR_MAX_SRC], am[MR_MAX_SRC];
  float dk = 0.f, dm = 0.f;
#pragma unroll
  for (int i = 0; i < MR_MAX_SRC; ++i)
    if (i < n) {
      const float2* a = e + i * MR_POINTS;
      float2 sk, sm;
      mr_split(a[k], a[km], t, sk, sm);
      ak[i] = mr_mag(sk, q.power);
      am[i] = mr_mag(sm, q.power);
      dk = i == 0 ? ak[i] : dk + ak[i];
      dm = i == 0 ? am[i] : dm + am[i];
    }
  const float ne = (float)n * q.eps;
  dk = dk + ne;
  dm = dm + ne;
#pragma unroll
  for (int i = 0; i < MR_MAX_SRC; ++i)
    if (i < n) {
      mk[i] = (ak[i] + q.eps) / dk;
      mm[i] = (am[i] + q.eps) / dm;
    }
}

// The add: frames f0 .. g_last of one signal, inverse-transformed in y (slot f - f0; Re and Im are the even and odd
// samples, times 2 H), times the window and 1 / NFFT, added into the span's samples [s0, pend) in `ola`.  A thread owns
// its quads of samples for the whole launch, so every sample's sum runs in frame order.
template <int H>
__device__ __forceinline__ void mr_add(float* ola, const float2* y2, const float* win, int s0, int pend, int hop, int f0,
                                       int g_last, int tid) {
  constexpr int NFFT = 2 * H, SPAN = mr_span(NFFT);
  const int r = NFFT / hop;
  const float inv_n = 1.f / (float)NFFT;   // mr_merge hands back twice the packed transform: 1 / (2 H)
  const float* y = reinterpret_cast<const float*>(y2);
  for (int v = tid; v < SPAN / 4; v += MRT) {
    const int p = s0 + 4 * v;
    if (p >= pend) continue;
    const int fhi = (p + H) / hop;   // (hop % 4 == 0: the same frames cover the whole quad)
    const int fa = max(fhi - r + 1, f0), fb = min(fhi, g_last);
    float4 acc = *reinterpret_cast<float4*>(ola + 4 * v);
    for (int f = fa; f <= fb; ++f) {
      const int t = p + H - f * hop;
      const float4 yv = *reinterpret_cast<const float4*>(y + (f - f0) * NFFT + t);
      const float4 wv = *reinterpret_cast<const float4*>(win + t);
      acc.x = acc.x + (yv.x * inv_n) * wv.x;
      acc.y = acc.y + (yv.y * inv_n) * wv.y;
      acc.z = acc.z + (yv.z * inv_n) * wv.z;
      acc.w = acc.w + (yv.w * inv_n) * wv.w;
    }
    *reinterpret_cast<float4*>(ola + 4 * v) = acc;
  }
}

// The finish: the envelope (the sum of w^2 over the frames of the item that cover a sample, in frame order), formed
// once per quad, divides the n rows of `ola`; zero at or past L; stored to out + i stride (the quads this thread
// summed itself).
template <int H>
__device__ __forceinline__ void mr_finish(const float* ola, const float* win, float* __restrict__ out, long stride,
                                          int n, const MrItem& it, int s0, int pend, int hop, int Lmax, int vec,
                                          int tid) {
  constexpr int SPAN = mr_span(2 * H);
  const int r = 2 * H / hop, L = it.L;
  for (int v = tid; v < SPAN / 4; v += MRT) {
    const int p = s0 + 4 * v;
    if (p >= Lmax) continue;
    float env[4] = {0.f, 0.f, 0.f, 0.f};
    if (p < pend) {
      const int fhi = (p + H) / hop;
      const int fa = max(fhi - r + 1, 0), fb = min(fhi, it.F - 1);
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
      mr_store(vec, Lmax, out + i * stride, p, o);
    }
  }
}

// A span past the item's end, or of a channel the item does not have: the n rows are written as zero.
template <int H>
__device__ __forceinline__ void mr_zero(float* __restrict__ out, long stride, int n, int s0, int Lmax, int vec, int tid) {
  for (int i = 0; i < n; ++i)
    for (int v = tid; v < mr_span(2 * H) / 4; v += MRT)
      if (s0 + 4 * v < Lmax) mr_store(vec, Lmax, out + i * stride, s0 + 4 * v, make_float4(0.f, 0.f, 0.f, 0.f));
}
