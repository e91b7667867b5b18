// Speaker activity of separated stems (dsn_activity, dsn_activity_gate; the definition is in include/ditsep_hip.h,
// restated in float64 in tests/activity_restatement.py): per item, source and STFT frame a decision "this stem carries
// its speaker here" from a level floor relative to the recording and a dominance test between the stems, with
// hysteresis and minimum durations; and a gate that turns the inactive stretches of a stem into digital silence.
// A decision rule, not a trained detector.  Frames and spectra are formed by the functions of maskrefine_dev.h that
// maskrefine.hip calls (mr_tables, mr_load, mr_fft, mr_split), so they have the bits they have there.
//   analysis   workgroup (group of 2048 / n_fft frames, item): the transforms of the item's n estimates; every
//              (source, frame, bin of the band) gets |S|^2 in fp64 in LDS, then one thread per (source, frame) adds the
//              band in increasing bin order and writes E [item][source][frame].
//   decision   one workgroup per item, because the peak P and the dominance test couple its sources and frames:
//              the box-smoothed level (increasing frame order, one division), P and top(t) as maxima, the on / stay
//              bits, and then per source row the hysteresis and the three run rules as chunked scans -- a thread owns
//              a contiguous chunk of ceil(F / 256) frames, composes it, one scan runs over the 256 chunk summaries in
//              LDS, and the thread replays its chunk with what the scan carries in.  The hysteresis step
//              a -> on | (a & stay) is a function of one bit and composes associatively; "the nearest frame of value v
//              before / after t" is a max / min scan.  No thread walks more than its chunk.
//   gate       workgroup (span of samples, item, source): the act bytes of the span's frames and ceil(fade / hop) + 1
//              frames either side in LDS, per frame the nearest active sample before and after, and per sample one
//              select or one multiply with the host's ramp table.
// No floating-point atomics; nothing depends on the batch position, the padding (never read), the alignment or on an
// earlier call.
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

#include "maskrefine_dev.h"

constexpr int ACT_BF = MR_MAX_SRC * (MR_POINTS / 2) / MRT;   // butterflies per thread and stage at n = 4
constexpr int ACT_GATE_SPAN = 4096;                          // samples per gate workgroup: 4 quads a thread

// Dynamic LDS of the analysis: float2 tw[H] | float2 buf[n][G][H] | float win[NFFT] | double pw[n][G][H + 1]
inline size_t act_lds_bytes(int nfft, int n) {
  return mr_lds_bytes(nfft, n, 0) + sizeof(double) * (size_t)n * (MR_POINTS + 2 * MR_POINTS / nfft);
}

// ---------------------------------------------------------------------------------------------------- analysis
// grid (ceil(Fmax / G), B).  E [B][n][Fmax]: the band energy of the frames the item has, 0 of those it has not.
template <int NFFT>
__global__ __launch_bounds__(MRT) void activity_analysis_kernel(const MaskRefineShape q, int Fmax, int j_lo, int j_hi,
                                                                const float* __restrict__ est,
                                                                const int* __restrict__ lens, double* __restrict__ E) {
  constexpr int H = NFFT / 2, G = MR_POINTS / H;
  extern __shared__ __attribute__((aligned(16))) float2 act_lds[];
  const int n = q.n, hop = q.hop, tid = threadIdx.x, b = blockIdx.y;
  const MrItem it = mr_item(lens, b, q.Lmax, hop);
  const int f0 = blockIdx.x * G;
  double* Eb = E + (long)b * n * Fmax;
  if (f0 >= it.F) {   // (uniform) frames the item does not have
    for (int e = tid; e < n * G; e += MRT) {
      const int i = e / G, f = f0 + e % G;
      if (f < Fmax) Eb[(long)i * Fmax + f] = 0.0;
    }
    return;
  }
  float2* tw = act_lds;
  float2* buf = tw + H;
  float* win = reinterpret_cast<float*>(buf + n * MR_POINTS);
  double* pw = reinterpret_cast<double*>(win + NFFT);
  mr_tables<H>(tw, win, tid);
  __syncthreads();
  const int f_last = min(it.F - 1, f0 + G - 1);
  const float* estb = est + (long)b * n * q.Lmax;
  mr_load<H>(buf, win, estb, estb, q.Lmax, it, hop, 0, n, f0, f_last, tid);
  __syncthreads();
  mr_fft<H, false, ACT_BF>(buf, tw, n * (MR_POINTS / 2), tid);
  // bin j of slot sg = (source, frame in the group): mr_split of the pair (k, H - k) that holds it, as everywhere
  const int nb = j_hi - j_lo + 1;
  for (int e = tid; e < n * G * nb; e += MRT) {
    const int sg = e / nb, j = j_lo + (e - sg * nb);
    const bool lower = 2 * j <= H;
    const int k = lower ? j : H - j, km = (H - k) & (H - 1);
    const float2* a = buf + sg * H;
    float2 xk, xm;
    mr_split(a[k], a[km], tw[k], xk, xm);
    const double re = lower ? xk.x : xm.x, im = lower ? xk.y : xm.y;
    pw[sg * (H + 1) + j] = re * re + im * im;
  }
  __syncthreads();
  for (int sg = tid; sg < n * G; sg += MRT) {
    const int i = sg / G, f = f0 + sg % G;
    if (f >= Fmax) continue;
    double s = 0.0;
    if (f <= f_last)
      for (int j = j_lo; j <= j_hi; ++j) s += pw[sg * (H + 1) + j];
    Eb[(long)i * Fmax + f] = s;
  }
}

// ---------------------------------------------------------------------------------------------------- decision
struct ActShape {
  int n, Lmax, hop, Fmax, half, min_on, min_off, pad;
  double c_r, c_d, c_rs, c_ds;
};

// The thread's chunk [c0, c1) of `row`: the nearest frame of value `want` before c0 (-1: none) and at or after c1
// (F: none).  Every thread of the workgroup calls it; sp and sn are MRT ints of LDS each.
__device__ __forceinline__ void act_nearest(const uint8_t* row, int F, int c0, int c1, int want, int* sp, int* sn,
                                            int tid, int& before, int& after) {
  int last = -1, first = F;
  for (int t = c0; t < c1; ++t)
    if (row[t] == want) {
      last = t;
      if (first == F) first = t;
    }
  __syncthreads();   // (an earlier call's carries have been read)
  sp[tid] = last;
  sn[tid] = first;
  __syncthreads();
  for (int d = 1; d < MRT; d <<= 1) {   // inclusive max scan upwards, inclusive min scan downwards
    const int p = tid >= d ? max(sp[tid], sp[tid - d]) : sp[tid];
    const int m = tid + d < MRT ? min(sn[tid], sn[tid + d]) : sn[tid];
    __syncthreads();
    sp[tid] = p;
    sn[tid] = m;
    __syncthreads();
  }
  before = tid > 0 ? sp[tid - 1] : -1;
  after = tid + 1 < MRT ? sn[tid + 1] : F;
}

// grid (B).  E, lev [B][n][Fmax] fp64, act [B][n][Fmax] bytes, frames_on [B][n].
__global__ __launch_bounds__(MRT) void activity_decide_kernel(const ActShape q, const int* __restrict__ lens,
                                                              const double* __restrict__ E, double* __restrict__ lev,
                                                              uint8_t* __restrict__ act, int* __restrict__ frames_on) {
  __shared__ double red[MRT];
  __shared__ int sp[MRT], sn[MRT];
  const int tid = threadIdx.x, b = blockIdx.x, n = q.n, Fmax = q.Fmax, h = q.half;
  const MrItem it = mr_item(lens, b, q.Lmax, q.hop);
  const int F = it.F;
  const double* Eb = E + (long)b * n * Fmax;
  double* Lb = lev + (long)b * n * Fmax;
  uint8_t* Ab = act + (long)b * n * Fmax;

  // ---- the level, and P: a NaN compares false and is passed over
  double pmax = 0.0;
  for (int i = 0; i < n; ++i)
    for (int t = tid; t < Fmax; t += MRT) {
      double v = 0.0;
      if (t < F) {
        const int ua = max(0, t - h), ub = min(F - 1, t + h);
        double s = 0.0;
        for (int u = ua; u <= ub; ++u) s += Eb[(long)i * Fmax + u];
        v = s / (double)(ub - ua + 1);
        if (v > pmax) pmax = v;
      }
      Lb[(long)i * Fmax + t] = v;
    }
  red[tid] = pmax;
  __syncthreads();
  for (int d = MRT / 2; d > 0; d >>= 1) {
    if (tid < d && red[tid + d] > red[tid]) red[tid] = red[tid + d];
    __syncthreads();
  }
  const double P = red[0];
  const double pr = P * q.c_r, prs = P * q.c_rs;

  // ---- on (bit 0) and stay (bit 1) of every source and frame; frames the item does not have are 0
  for (int t = tid; t < Fmax; t += MRT) {
    double v[MR_MAX_SRC], top = 0.0;
#pragma unroll
    for (int i = 0; i < MR_MAX_SRC; ++i)
      if (i < n) {
        v[i] = t < F ? Lb[(long)i * Fmax + t] : 0.0;
        if (v[i] > top) top = v[i];
      }
    const double td = top * q.c_d, tds = top * q.c_ds;
#pragma unroll
    for (int i = 0; i < MR_MAX_SRC; ++i)
      if (i < n) {
        const int on = t < F && P > 0.0 && v[i] >= pr && v[i] >= td;
        const int stay = t < F && P > 0.0 && v[i] >= prs && v[i] >= tds;
        Ab[(long)i * Fmax + t] = (uint8_t)(on | (stay << 1));
      }
  }
  __syncthreads();

  const int chunk = (F + MRT - 1) / MRT;
  const int c0 = min(F, tid * chunk), c1 = min(F, c0 + chunk);
  for (int i = 0; i < n; ++i) {
    uint8_t* row = Ab + (long)i * Fmax;
    // ---- hysteresis a(t) = on(t) | (a(t - 1) & stay(t)): a step is the pair (image of 0, image of 1) = (on, on | stay)
    int f = 2;   // the identity: 0 -> 0, 1 -> 1
    for (int t = c0; t < c1; ++t) {
      const int c = row[t], g = (c & 1) | (((c | (c >> 1)) & 1) << 1);
      f = ((g >> (f & 1)) & 1) | (((g >> (f >> 1)) & 1) << 1);
    }
    __syncthreads();
    sp[tid] = f;
    __syncthreads();
    for (int d = 1; d < MRT; d <<= 1) {   // inclusive scan: the chunks 0 .. tid composed in order
      int r = sp[tid];
      if (tid >= d) {
        const int lo = sp[tid - d];
        r = ((r >> (lo & 1)) & 1) | (((r >> (lo >> 1)) & 1) << 1);
      }
      __syncthreads();
      sp[tid] = r;
      __syncthreads();
    }
    int a = tid > 0 ? sp[tid - 1] & 1 : 0;   // a(-1) = 0 through every earlier chunk
    for (int t = c0; t < c1; ++t) {
      const int c = row[t];
      a = (c & 1) | (a & (c >> 1));
      row[t] = (uint8_t)a;
    }
    int before, after;
    // ---- an off-run between two on-runs that is shorter than min_off becomes on
    if (q.min_off > 1) {
      act_nearest(row, F, c0, c1, 1, sp, sn, tid, before, after);
      int prev = before, next = c0 - 1;   // next: the nearest on-frame at or after t, valid while next >= t
      for (int t = c0; t < c1; ++t) {
        if (next < t) {
          next = t;
          while (next < c1 && !row[next]) ++next;
          if (next == c1) next = after;
        }
        if (row[t]) {
          prev = t;
        } else if (prev >= 0 && next < F && next - prev - 1 < q.min_off) {
          row[t] = 2;   // (told from the frames that were on: prev stays where it is)
        }
      }
      for (int t = c0; t < c1; ++t) row[t] = row[t] ? 1 : 0;
    }
    // ---- an on-run shorter than min_on is cleared
    if (q.min_on > 1) {
      act_nearest(row, F, c0, c1, 0, sp, sn, tid, before, after);
      int prev = before, next = c0 - 1;   // the nearest off-frames before and at or after t
      for (int t = c0; t < c1; ++t) {
        if (next < t) {
          next = t;
          while (next < c1 && row[next] == 1) ++next;
          if (next == c1) next = after;
        }
        if (row[t] == 0) {
          prev = t;
        } else if (next - prev - 1 < q.min_on) {
          row[t] = 2;   // on, to be cleared: still part of its run for the frames after it
        }
      }
      for (int t = c0; t < c1; ++t) row[t] = row[t] == 1 ? 1 : 0;
    }
    // ---- every run grows by pad frames either side; runs that touch merge
    if (q.pad > 0) {
      act_nearest(row, F, c0, c1, 1, sp, sn, tid, before, after);
      int prev = before, next = c0 - 1;
      for (int t = c0; t < c1; ++t) {
        if (next < t) {
          next = t;
          while (next < c1 && row[next] != 1) ++next;
          if (next == c1) next = after;
        }
        if (row[t] == 1) {
          prev = t;
        } else if ((prev >= 0 && t - prev <= q.pad) || (next < F && next - t <= q.pad)) {
          row[t] = 2;
        }
      }
      for (int t = c0; t < c1; ++t) row[t] = row[t] ? 1 : 0;
    }
    // ---- frames_on
    int cnt = 0;
    for (int t = c0; t < c1; ++t) cnt += row[t];
    __syncthreads();
    sp[tid] = cnt;
    __syncthreads();
    for (int d = MRT / 2; d > 0; d >>= 1) {
      if (tid < d) sp[tid] += sp[tid + d];
      __syncthreads();
    }
    if (tid == 0) frames_on[(long)b * n + i] = sp[0];
  }
}

// ---------------------------------------------------------------------------------------------------- gate
struct GateShape {
  int n, Lmax, hop, Fa, fade, K, vec;   // Fa: frames a row of act holds; K = ceil(fade / hop) + 1
};

// grid (ceil(Lmax / ACT_GATE_SPAN), B, n).  Dynamic LDS: int prev[nf] | int next[nf] | bytes on[nf], nf = the span's
// frames and K either side.
__global__ __launch_bounds__(MRT) void activity_gate_kernel(const GateShape q, const float* __restrict__ x,
                                                            const uint8_t* __restrict__ act,
                                                            const int* __restrict__ lens,
                                                            const float* __restrict__ ramp, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) int gate_lds[];
  const int tid = threadIdx.x, b = blockIdx.y, i = blockIdx.z, hop = q.hop, h2 = hop / 2, K = q.K;
  const int L = lens ? lens[b] : q.Lmax, s0 = blockIdx.x * ACT_GATE_SPAN;
  const long r = (long)b * q.n + i;
  const float* xr = x + r * q.Lmax;
  float* orow = out + r * q.Lmax;
  if (s0 >= L) {   // (uniform) past the item's end
    for (int v = tid; v < ACT_GATE_SPAN / 4; v += MRT)
      if (s0 + 4 * v < q.Lmax) mr_store(q.vec, q.Lmax, orow, s0 + 4 * v, make_float4(0.f, 0.f, 0.f, 0.f));
    return;
  }
  const int pend = min(s0 + ACT_GATE_SPAN, L);
  const int t_last = min(q.Fa - 1, (L - 1 + h2) / hop);        // the last frame that owns a sample of the item
  const int fc0 = (s0 + h2) / hop, fc1 = (pend - 1 + h2) / hop;   // the frames of the span's own samples
  const int fa = fc0 - K, nf = fc1 - fc0 + 1 + 2 * K;
  int* prev = gate_lds;
  int* next = prev + nf;
  uint8_t* on = reinterpret_cast<uint8_t*>(next + nf);
  const uint8_t* arow = act + r * q.Fa;
  for (int e = tid; e < nf; e += MRT) {
    const int t = fa + e;
    on[e] = t >= 0 && t <= t_last && arow[t] ? 1 : 0;
  }
  __syncthreads();
  // per frame of the span: the last sample of the nearest active frame before it and the first sample of the nearest
  // after it, K frames at the most: further ones are more than `fade` samples away
  for (int e = tid + K; e < nf - K; e += MRT) {
    int p = -(1 << 29), m = INT_MAX;
    for (int u = 1; u <= K; ++u)
      if (on[e - u]) {
        p = (fa + e - u + 1) * hop - h2 - 1;
        break;
      }
    for (int u = 1; u <= K; ++u)
      if (on[e + u]) {
        m = (fa + e + u) * hop - h2;
        break;
      }
    prev[e] = p;
    next[e] = m;
  }
  __syncthreads();
  for (int v = tid; v < ACT_GATE_SPAN / 4; v += MRT) {
    const int p = s0 + 4 * v;
    if (p >= q.Lmax) continue;
    float xv[4] = {0.f, 0.f, 0.f, 0.f}, o[4] = {0.f, 0.f, 0.f, 0.f};
    if (q.vec && p + 3 < L) {
      const float4 t4 = *reinterpret_cast<const float4*>(xr + p);
      xv[0] = t4.x, xv[1] = t4.y, xv[2] = t4.z, xv[3] = t4.w;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (p + u < L) xv[u] = xr[p + u];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int m = p + u;
      if (m >= L) continue;
      const int e = (m + h2) / hop - fa;
      if (on[e]) {
        o[u] = xv[u];
      } else {
        const int d = min(m - prev[e], next[e] - m);
        if (d <= q.fade) o[u] = ramp[d - 1] * xv[u];
      }
    }
    mr_store(q.vec, q.Lmax, orow, p, make_float4(o[0], o[1], o[2], o[3]));
  }
}

}  // namespace

int activity_frames(int hop, int Lmax) { return 1 + (Lmax + hop - 1) / hop; }

void launch_activity(const float* est, const int* lens, int B, int n, int Lmax, int nfft, int hop, int j_lo, int j_hi,
                     int half_width, double c_r, double c_d, double c_rs, double c_ds, int min_on, int min_off, int pad,
                     double* energy, double* level, uint8_t* act, int* frames_on, hipStream_t st) {
  const int Fmax = activity_frames(hop, Lmax);
  const MaskRefineShape q{n, Lmax, hop, 2, 0.f, 0, 1, 0.f};
  mr_for_nfft(nfft, [&](auto N) {
    constexpr int NFFT = decltype(N)::value, G = 2 * MR_POINTS / NFFT;
    dsn_allow_lds<activity_analysis_kernel<NFFT>>((int)act_lds_bytes(NFFT, MR_MAX_SRC));
    hipLaunchKernelGGL((activity_analysis_kernel<NFFT>), dim3((unsigned)((Fmax + G - 1) / G), (unsigned)B), dim3(MRT),
                       act_lds_bytes(NFFT, n), st, q, Fmax, j_lo, j_hi, est, lens, energy);
  });
  const ActShape a{n, Lmax, hop, Fmax, half_width, min_on, min_off, pad, c_r, c_d, c_rs, c_ds};
  hipLaunchKernelGGL(activity_decide_kernel, dim3((unsigned)B), dim3(MRT), 0, st, a, lens, energy, level, act,
                     frames_on);
}

void launch_activity_gate(const float* x, const uint8_t* act, const int* lens, const float* ramp, float* out, int B, int n,
                          int Lmax, int Fa, int hop, int fade, hipStream_t st) {
  const int K = (fade + hop - 1) / hop + 1;
  const int vec = (((uintptr_t)out | (uintptr_t)x) & 15) == 0 && Lmax % 4 == 0 ? 1 : 0;
  const GateShape q{n, Lmax, hop, Fa, fade, K, vec};
  const int nf = ACT_GATE_SPAN / hop + 2 + 2 * K;   // the most frames a span stages
  const size_t lds = (size_t)nf * (2 * sizeof(int) + 1);
  hipLaunchKernelGGL(activity_gate_kernel, dim3((unsigned)((Lmax + ACT_GATE_SPAN - 1) / ACT_GATE_SPAN), (unsigned)B,
                     (unsigned)n), dim3(MRT), lds, st, q, x, act, lens, ramp, out);
}
