// Device helpers shared by maskrefine.hip (dsn_mask_refine, dsn_stems) and beamform.hip (dsn_beamform): the packed real
// transform in LDS, its split and merge, the masks and the row store.  Both files form a frame's spectra and masks with
// exactly this code, floating point contraction off, so X, S and M have the same bits wherever they are formed.
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
