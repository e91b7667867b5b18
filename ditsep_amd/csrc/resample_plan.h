// The plan of a sinc resampling call (include/ditsep_hip.h, dsn_resample): torchaudio.transforms.Resample's default
// filter (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) as a polyphase table, cut down to the taps that are
// not exactly 0.0f.  Host-only -- no HIP.  Restated in float64 numpy in tests/resample_restatement.py;
// tests/test_resample_host.py compares the two through dsn_resample_plan.
//
//   g = gcd(fs_in, fs_out), o = fs_in / g, n = fs_out / g, base = min(o, n) 0.99, width = ceil(6 o / base),
//   K = 2 width + o;  t = clamp((-p / n + (k - width) / o) base, -6, 6),
//   h[p][k] = float32(sinc(pi t) cos^2(pi t / 12) base / o)      (float64, rounded once)
//   out[m n + p] = sum_k h[p][k] xz[m o + k - width]               (xz: x extended by zeros on both sides)
//
// At |t| = 6 the window is about 4e-33 and the sinc about 4e-17: the product underflows float32, so in every phase
// all taps but one short run are exactly 0.0f.  k0[p] is the first tap of phase p that is not, S the longest run from
// a phase's first to its last such tap, c[p][j] = h[p][k0[p] + j] (0 for k0[p] + j >= K).  A tap is dropped only when
// it compares equal to 0.0f -- nothing is rounded to zero -- so the compact and the dense sum are the same sum.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

struct ResamplePlan {
  int o = 1, n = 1, width = 0, K = 0, S = 0;
  std::vector<int32_t> k0;  // [n]
  std::vector<float> c;     // [n][S]
};

constexpr double kResampleWidth = 6.0, kResampleRolloff = 0.99;

// nullptr, or what is wrong with the rates
inline const char* resample_refusal(int fs_in, int fs_out, char* buf, size_t bufsz) {
  if (fs_in < 1 || fs_out < 1) {
    snprintf(buf, bufsz, "sample rates must be positive (fs_in = %d, fs_out = %d)", fs_in, fs_out);
    return buf;
  }
  return nullptr;
}

// ceil(n L / o): the output length of an L-sample row
inline long resample_length(int o, int n, long L) { return ((long)n * L + o - 1) / o; }

inline float resample_tap(double t, double scale) {
  const double w = cos(t * M_PI / kResampleWidth / 2.0);
  const double a = t * M_PI;
  const double s = a == 0.0 ? 1.0 : sin(a) / a;
  return (float)(s * (w * w) * scale);
}

// (rates already accepted by resample_refusal)
inline ResamplePlan resample_plan(int fs_in, int fs_out) {
  ResamplePlan p;
  const int g = std::gcd(fs_in, fs_out);
  p.o = fs_in / g, p.n = fs_out / g;
  const double base = (double)std::min(p.o, p.n) * kResampleRolloff;
  p.width = (int)ceil(kResampleWidth * (double)p.o / base);
  p.K = 2 * p.width + p.o;
  const double scale = base / (double)p.o;
  // every tap whose argument is clamped has one of these two values
  const float edge_lo = resample_tap(-kResampleWidth, scale), edge_hi = resample_tap(kResampleWidth, scale);
  std::vector<float> h((size_t)p.K);
  std::vector<int> last((size_t)p.n, -1);
  p.k0.assign((size_t)p.n, 0);
  std::vector<std::vector<float>> rows((size_t)p.n);
  for (int ph = 0; ph < p.n; ++ph) {
    int first = -1;
    for (int k = 0; k < p.K; ++k) {
      const double t = (-(double)ph / (double)p.n + (double)(k - p.width) / (double)p.o) * base;
      h[k] = t <= -kResampleWidth ? edge_lo : t >= kResampleWidth ? edge_hi : resample_tap(t, scale);
      if (h[k] != 0.0f) {   // the only test that drops a tap
        if (first < 0) first = k;
        last[ph] = k;
      }
    }
    if (first < 0) first = 0, last[ph] = -1;   // (an all-zero phase: no taps)
    p.k0[ph] = first;
    rows[ph].assign(h.begin() + first, h.begin() + (last[ph] + 1 > first ? last[ph] + 1 : first));
    p.S = std::max(p.S, (int)rows[ph].size());
  }
  p.S = std::max(p.S, 1);
  p.c.assign((size_t)p.n * p.S, 0.f);
  for (int ph = 0; ph < p.n; ++ph) std::copy(rows[ph].begin(), rows[ph].end(), p.c.begin() + (size_t)ph * p.S);
  return p;
}
