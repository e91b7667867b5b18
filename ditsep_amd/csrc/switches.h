// The runtime switches ("Runtime switches"): the only reader of the process environment in this library.
// Host-only.  guarded() (engine.hip) takes a fresh copy into dsn_ctx::sw at the top of every API call, so a switch may
// change between two calls of one process; everything below reads that copy, the kernel files take what concerns them
// as arguments.  A captured graph remembers the copy it was built under (dsn_ctx::run_graphed).
#pragma once
#include <stdlib.h>

#include <algorithm>
#include <tuple>

struct Switches {
  bool audit = false;       // DSN_AUDIT: host-side bounds audit of every GEMM descriptor before its launch
  bool no_ln_fold = false;  // DSN_NO_LN_FOLD: acts at finalize only -- it selects which weights are packed
  bool no_gn_fin = false;   // DSN_NO_GN_FIN: GroupNorm_1 as a separate pass instead of finished by its producer conv
  bool ru_v1 = false;       // DSN_RU_V1: the 128-row fused ResidualUnit kernel instead of the 256-row one
  int skinny_max = 80;      // DSN_SKINNY_MAX: upper row limit of the skinny DiT GEMMs, at most 128
  int qa_ipp = 0;           // DSN_QA_IPP: items per panel of the forced fused to_qkv + attention kernel, 0 = not forced

  static Switches read() {
    Switches s;
    s.audit = getenv("DSN_AUDIT") != nullptr;
    s.no_ln_fold = getenv("DSN_NO_LN_FOLD") != nullptr;
    s.no_gn_fin = getenv("DSN_NO_GN_FIN") != nullptr;
    s.ru_v1 = getenv("DSN_RU_V1") != nullptr;
    if (const char* v = getenv("DSN_SKINNY_MAX")) s.skinny_max = std::min(atoi(v), 128);
    if (const char* v = getenv("DSN_QA_IPP")) s.qa_ipp = std::max(atoi(v), 0);
    return s;
  }
  bool operator==(const Switches& o) const {
    auto key = [](const Switches& s) { return std::tie(s.audit, s.no_ln_fold, s.no_gn_fin, s.ru_v1, s.skinny_max, s.qa_ipp); };
    return key(*this) == key(o);
  }
};
