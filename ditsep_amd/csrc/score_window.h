// The plan of a window-blended DiT score call (include/ditsep_hip.h, dsn_score_windowed): which windows of the trained
// length are cut from the long latents, and which one or two of them serve every frame.  Host-only -- no HIP -- and a
// mirror of ditsep_amd/native.py::score_window_plan (dsn_score_window_plan, tests/test_score_window_host.py compares
// the two).  The device follows the tables; the kernels know nothing about hops.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/ditsep_hip.h"

struct ScoreWindowPlan {
  int R = 0, T = 0, Tw = 0, To = 0, fade = 0;
  int Wtot = 0;
  int Twin = 0;        // the DiT call's length: Tw, or the longest recording when none is longer than a window
  bool shorts = false;  // some window is shorter than Twin: the length-aware attention kernels run
  bool ragged = false;  // the recordings' frame counts differ
  std::vector<int32_t> wtab;  // [Wtot][3] recording, start, length
  std::vector<int32_t> ftab;  // [R T][4] window0, offset0, window1, offset1
  std::vector<float> fw;      // [R T][2] fall, rise
  std::vector<int32_t> wlens;  // [Wtot] tokens per window: 1 + length (the timestep token)
};

// nullptr, or what is wrong with the arguments (window_plan's words)
inline const char* score_window_refusal(const int32_t* frames, int R, int T, int Tw, int To, int fade, char* buf,
                                        size_t bufsz) {
  if (!frames || R < 1 || T < 1) return "frames is null, or R < 1 or T < 1";
  if (Tw < 1) {
    snprintf(buf, bufsz, "window = %d < 1", Tw);
    return buf;
  }
  if (To < 0) {
    snprintf(buf, bufsz, "overlap = %d < 0", To);
    return buf;
  }
  if (2L * To > Tw) {
    snprintf(buf, bufsz, "2 * overlap = %ld > window = %d: a frame may lie in at most two windows", 2L * To, Tw);
    return buf;
  }
  if (fade != DSN_FADE_HANN && fade != DSN_FADE_LINEAR) {
    snprintf(buf, bufsz, "unknown fade %d", fade);
    return buf;
  }
  for (int r = 0; r < R; ++r)
    if (frames[r] < 1 || frames[r] > T) {
      snprintf(buf, bufsz, "frame count frames[%d] = %d outside [1, T = %d]", r, (int)frames[r], T);
      return buf;
    }
  return nullptr;
}

// (arguments already accepted by score_window_refusal)
inline ScoreWindowPlan score_window_plan(const int32_t* frames, int R, int T, int Tw, int To, int fade) {
  ScoreWindowPlan p;
  p.R = R, p.T = T, p.Tw = Tw, p.To = To, p.fade = fade;
  std::vector<float> fall((size_t)To), rise((size_t)To);  // dsn_window_stitch's tables: fp64, rounded once
  for (int k = 0; k < To; ++k) {
    double r;
    if (fade == DSN_FADE_LINEAR) {
      r = ((double)k + 0.5) / (double)To;
    } else {
      const double sn = sin(M_PI * ((double)k + 0.5) / (2.0 * (double)To));
      r = sn * sn;
    }
    fall[k] = (float)(1.0 - r);
    rise[k] = (float)r;
  }
  const int hop = Tw - To;
  p.ftab.assign((size_t)R * T * 4, 0);
  p.fw.assign((size_t)R * T * 2, 0.f);
  for (int r = 0; r < R; ++r) {
    const int F = frames[r], base = (int)(p.wtab.size() / 3);
    const int W = F <= Tw ? 1 : 1 + (F - Tw + hop - 1) / hop;
    auto start = [&](int w) { return F <= Tw ? 0 : std::min(w * hop, F - Tw); };
    for (int w = 0; w < W; ++w) {
      p.wtab.push_back(r);
      p.wtab.push_back(start(w));
      p.wtab.push_back(std::min(F, Tw));
    }
    p.Twin = std::max(p.Twin, std::min(F, Tw));
    if (F != frames[0]) p.ragged = true;
    for (int f = 0; f < T; ++f) {
      int32_t* e = &p.ftab[((size_t)r * T + f) * 4];
      float* g = &p.fw[((size_t)r * T + f) * 2];
      e[0] = e[2] = -1;
      g[0] = 1.f;
      if (f >= F) continue;  // past the recording's end: the score is written as zero
      const int w = W == 1 ? 0 : std::min(f / hop, W - 1), k = f - w * hop;
      if (w >= 1 && k < To) {
        e[0] = base + w - 1, e[1] = f - start(w - 1);
        e[2] = base + w, e[3] = f - start(w);
        g[0] = fall[k], g[1] = rise[k];
      } else {
        e[0] = base + w, e[1] = f - start(w);
      }
    }
  }
  p.Wtot = (int)(p.wtab.size() / 3);
  p.wlens.resize((size_t)p.Wtot);
  for (int w = 0; w < p.Wtot; ++w) {
    p.wlens[w] = 1 + p.wtab[3 * (size_t)w + 2];
    if (p.wtab[3 * (size_t)w + 2] != p.Twin) p.shorts = true;
  }
  return p;
}
