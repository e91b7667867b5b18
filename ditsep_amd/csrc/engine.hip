// Engine + C-ABI (include/ditsep_hip.h) of the MI355X separation path.
//
// Host side of the native library: owns the packed weights and the activation
// workspace in HBM, and turns one call of the reference's entry points into a
// fixed sequence of gfx950 kernel launches on the caller's HIP stream
// (optionally captured into a hipGraph and replayed).  Nothing here touches
// torch; the Python facade passes raw device pointers.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <numeric>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/ditsep_hip.h"
#include "dit_plan.h"
#include "igemm.h"
#include "kernels.h"
#include "resample_plan.h"
#include "score_window.h"

namespace {

struct Err : std::runtime_error {
  int code;
  Err(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

[[noreturn]] void fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  throw Err(code, buf);
}

#define HIPCHK(expr)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) fail(DSN_EHIP, "%s -> %s (%s:%d)", #expr, hipGetErrorString(e_), \
                               __FILE__, __LINE__);                                        \
  } while (0)

struct DevTensor {
  float* p = nullptr;
  std::vector<long> shape;
  long numel = 0;
};

struct Packed {  // K-major packed operand planes of one contraction
  op16_t* w = nullptr;
  long ps = 0;
  int N = 0, K = 0, Cin = 0, taps = 0;
  float* bias = nullptr;
  int bias_mod = 1;
};

// a caller's plain [N][taps * Cin] weight planes, no bias (test and benchmark hooks)
static Packed plain_packed(op16_t* w, long ps, int N, int Cin, int taps) {
  Packed p;
  p.w = w;
  p.ps = ps;
  p.N = N;
  p.Cin = Cin;
  p.taps = taps;
  p.K = taps * Cin;
  return p;
}

struct ActP {  // producer-side activation
  int kind = DSN_ACT_NONE;
  float* a = nullptr;
  float* ib = nullptr;
  int mod = 1;
};

struct Packed8 {  // fp8 (MX) packed Linear weight: e4m3 bytes [N][K] + E8M0 block scales [N][K/32]
  unsigned char* w = nullptr;
  unsigned char* s = nullptr;
  int N = 0, K = 0;
  float* bias = nullptr;
};

struct DitLayer {
  float *g1 = nullptr, *be1 = nullptr, *g2 = nullptr, *be2 = nullptr;
  Packed qkv, out, ff1, ff2;
  Packed8 qkv8, out8, ff1_8, ff2_8;  // DSN_PREC_FP8
  // ff_norm folded into FF-in (single-plane modes): W * diag(gamma) packed, its rounded row sums, bias + W beta
  Packed ff1f;
  float* ff1_colsum = nullptr;
  Packed8 ff1f8;  // fp8 mode: the same fold on the MX-quantised W * diag(gamma), row sums of the dequantised bytes
  float* ff1_colsum8 = nullptr;
};

struct ResUnit {
  ActP act0, act2;  // act0 is applied by the PRODUCER of the unit's input
  Packed conv7, conv1;
  int dil = 1;
};

struct VaeBlock {
  ActP act;     // block-level activation (before convT / before strided conv)
  Packed conv;  // ConvTranspose1d (decoder) or strided Conv1d (encoder)
  ResUnit ru[3];
  int cin = 0, cout = 0, stride = 1;
};

struct Graph {
  hipGraphExec_t exec = nullptr;
  uint64_t epoch = ~0ull;  // workspace epoch and switches the graph (or its eager warm-up) was built against
  Switches sw;
  bool warmed = false;
};

struct ProfRec {  // what a call site states (in this order) and the events dsn_ctx::profiled adds
  const char* tag = "";  // call-site label (static string): rows of dsn_profile_rows
  double flops = 0;
  double hbm_bytes = 0;  // algorithmic HBM bytes of the launch (0 = not stated)
  bool gemm = true;      // counted in the implicit-GEMM family totals of dsn_profile_end
  bool hbm_bound = false;  // the HBM-bound member of that family (fused ResidualUnit): dsn_profile_hbm
  hipEvent_t a = nullptr, b = nullptr;
};

struct ProfRow {
  std::string name;
  double ms = 0, flops = 0, bytes = 0;
  int64_t launches = 0;
};

// what dit_plan must stay inside, from the kernel files that own each limit
DitLimits dit_limits() {
  return {qkv_attention_max_rows(), qkv_attention_panel_rows(1), PANEL_ROWS_MAX, PANEL_FP8_ROWS_MAX, PANEL_STATS_ROWS_MAX,
          RESIDUAL_NORM_MAX_SLABS};
}

}  // namespace

struct dsn_ctx {
  dsn_config cfg;
  std::string err;
  Switches sw;  // the environment's switches as of this API call (guarded)
  int P = 2;   // operand planes
  int PL = 2;  // DSN_PL(P, fp16 flag) as the kernels take it
  bool fp8 = false;  // DSN_PREC_FP8: DiT layer GEMMs on fp8 (MX) operands, the rest single-plane fp16
  bool fold_ln8 = false;  // the same in the fp8 mode (raw x' as e4m3 + block scales)
  bool fold_ln = false;  // ff_norm folded into FF-in, to_out without split-K writing the residual stream itself
  bool finalized = false;
  bool use_graphs = false;
  // producer-finished GroupNorm (GemmDesc::gnf_out): host-mapped give-up flag of its waits; counters per (row tiles per
  // image) value, zeroed once -- they only grow
  int* fin_err_host = nullptr;
  int* fin_err_dev = nullptr;
  std::map<int, std::pair<unsigned*, long>> gnf_sync;
  unsigned* gnf_counters(int nper, long count, hipStream_t st) {
    if (!fin_err_host) {
      HIPCHK(hipHostMalloc((void**)&fin_err_host, sizeof(int), hipHostMallocMapped));
      *fin_err_host = 0;
      HIPCHK(hipHostGetDevicePointer((void**)&fin_err_dev, fin_err_host, 0));
    }
    auto& c = gnf_sync[nper];
    if (!c.first || c.second < count) {
      if (c.first) {
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipFree(c.first));
      }
      c.second = std::max(count, 1024L);
      HIPCHK(hipMalloc((void**)&c.first, c.second * sizeof(unsigned)));
      HIPCHK(hipMemsetAsync(c.first, 0, c.second * sizeof(unsigned), st));
      ++ws_epoch;  // (first use is an eager warm-up call, never a capture)
    }
    return c.first;
  }
  double hbm_ms = 0, hbm_bytes = 0;  // HBM-bound launches of the last profiled region (dsn_profile_hbm)
  int64_t hbm_launches = 0;
  std::map<std::string, DevTensor> raw;
  std::vector<void*> allocs;
  std::map<std::string, std::pair<void*, size_t>> ws;
  uint64_t ws_epoch = 0;  // bumped on every workspace (re)allocation -> graphs invalid
  // dsn_stoi: the 10 kHz resampling filter per signal rate (taps in the workspace buffer "stoi_taps_<fs>")
  struct StoiFilter {
    double* taps = nullptr;
    int ntaps = 0, up = 1, down = 1, n_pre_pad = 0, n_pre_remove = 0;
  };
  std::map<int, StoiFilter> stoi_filters;
  // dsn_composite: the window and the critical-band filter table per signal rate (workspace buffers
  // "comp_win_<fs>", "comp_bw_<fs>")
  struct CompositeTables {
    double* win = nullptr;
    double* bweights = nullptr;
    CompositeBands bands;
  };
  std::map<int, CompositeTables> composite_tables;
  std::map<long, float*> mrstft_windows;  // dsn_mrstft_loss: (fft << 16 | win_length) -> zero-padded window [fft]
  OdeCtl* ode_host = nullptr;  // dsn_ode_sample: pinned host image of the solver state (upload / per-attempt poll)
  // dsn_window_stitch: the fade tables last uploaded (fall [O] then rise [O], workspace buffer "stitch_fade"); the host
  // image stays untouched while an enqueued upload may still read it
  struct StitchFade {
    std::vector<float> host;
    float* dev = nullptr;
    int O = -1, kind = -1;
  } stitch_fade;
  // dsn_resample: the compact polyphase tables per (orig, new), uploaded once (taps [new][stride], stride = the
  // support made odd; k0 [new]) and kept until the context goes
  struct ResampleTables {
    ResamplePlan plan;
    float* taps = nullptr;
    int* k0 = nullptr;
    int stride = 1, kmin = 0, kspan = 1;
  };
  std::map<std::pair<int, int>, ResampleTables> resample_tables;
  // the item lengths last uploaded and where they went (upload_lens_cached): dsn_resample's ("resample_lens"),
  // dsn_mask_refine's ("refine_lens") and dsn_ensemble_combine's ("ensemble_lens")
  struct CachedLens {
    std::vector<int> host;
    const int* dev = nullptr;
  } resample_lens, refine_lens, ensemble_lens;

  // DiT
  float* tf_w = nullptr;
  Packed t1, t2, pin, pout;  // pin / pout carry the folded pre/postprocess convs (fold_dit_io)
  std::vector<DitLayer> layers;
  // VAE
  Packed dec_in;
  std::vector<VaeBlock> dec_blocks;
  ActP dec_final_act;
  float* dec_out_w = nullptr;  // [7][C0]
  int dec_out_taps = 7;
  float *enc_in_w = nullptr, *enc_in_b = nullptr;
  std::vector<VaeBlock> enc_blocks;
  ActP enc_final_act;
  Packed enc_out;

  std::map<std::string, Graph> graphs;
  // capture / replay streams (graphs cannot be captured on the NULL stream): one per entry-point family,
  // so that the decode of one batch can overlap the sampler of the next when the caller issues them on
  // different streams (bench.py pipelines them)
  hipStream_t own[2] = {nullptr, nullptr};
  hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
  bool profiling = false;
  std::vector<ProfRec> prof;
  std::vector<ProfRow> prof_rows;  // per call-site aggregation of the last profiled region
  const char* cur_tag = "";        // label the next profiled launches carry
  struct Tag {                     // scoped call-site label
    dsn_ctx* c;
    const char* prev;
    Tag(dsn_ctx* ctx, const char* t) : c(ctx), prev(ctx->cur_tag) { c->cur_tag = t; }
    ~Tag() { c->cur_tag = prev; }
  };
  // The profiling bracket: `launch()` between two events of a record that carries what `spec` states.  Returns what
  // `launch` returns -- a launch error is the caller's to report, after the end event.  On every way out, a throw
  // included, the end event is recorded and the record kept: dsn_profile_begin / _end destroy the events of all records.
  template <class F>
  auto profiled(const ProfRec& spec, hipStream_t st, F&& launch) -> decltype(launch()) {
    if (!profiling) return launch();
    struct Bracket {
      dsn_ctx* c;
      ProfRec pr;
      hipStream_t st;
      ~Bracket() {
        (void)hipEventRecord(pr.b, st);  // (a failure shows in dsn_profile_end's hipEventElapsedTime)
        c->prof.push_back(pr);
      }
    } br{this, spec, st};
    HIPCHK(hipEventCreate(&br.pr.a));
    HIPCHK(hipEventCreate(&br.pr.b));
    HIPCHK(hipEventRecord(br.pr.a, st));
    return launch();
  }
  // a non-GEMM launch (algorithmic HBM bytes given by the caller)
  template <class F>
  void prof_launch(const char* tag, double bytes, hipStream_t st, F&& f) {
    profiled({tag, 0, bytes, false}, st, f);
  }
  std::vector<float> tv_host;  // uploaded timestep table signature
  int tv_B = -1;
  std::vector<int> lens_host;  // uploaded ragged token counts and where they went
  const int* lens_dev = nullptr;
  // A ragged batch in the codec (null = dense): the frame counts of its B mixtures on the device ("codec_frames",
  // upload_frames) and on the host (the profiled bytes), `rep` codec items per mixture (n_src in the decoder, 1 in the
  // encoder).
  struct CodecLens {
    const int* frames;
    const int32_t* host;
    int rep;
  };
  std::vector<int> frames_host;
  const int* frames_dev = nullptr;

  // Run `body(stream)` -- a pure sequence of kernel launches over workspace pointers --
  // either eagerly or as a cached hipGraph.  The first call with a given key runs
  // eagerly (it may grow the workspace), the second captures, later ones replay.  A graph built
  // against another workspace epoch or under other switches is stale: warm again, then recapture.
  template <class F>
  void run_graphed(const std::string& key, hipStream_t st, F&& body) {
    if (!use_graphs || profiling) {
      body(st);
      return;
    }
    Graph& g = graphs[key];
    const bool fresh = g.epoch == ws_epoch && g.sw == sw;
    if (g.exec && fresh) {
      HIPCHK(hipGraphLaunch(g.exec, st));
      return;
    }
    if (g.exec) {
      (void)hipGraphExecDestroy(g.exec);
      g.exec = nullptr;
    }
    if (!g.warmed || !fresh) {
      body(st);
      g.warmed = true;
      g.epoch = ws_epoch;
      g.sw = sw;
      return;
    }
    hipGraph_t graph = nullptr;
    HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    try {
      body(st);
    } catch (...) {
      (void)hipStreamEndCapture(st, &graph);
      if (graph) (void)hipGraphDestroy(graph);
      throw;
    }
    HIPCHK(hipStreamEndCapture(st, &graph));
    hipError_t e = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) fail(DSN_EHIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
    HIPCHK(hipGraphLaunch(g.exec, st));
  }
  // `st` is the stream the engine enqueues on: the caller's in eager mode, its own (ordered after the
  // caller's by an event) in graph mode.  leave() makes the caller's stream wait for that work; an exit by
  // exception joins too (unchecked), so the caller is never left unordered with what was already enqueued.
  struct StreamScope {
    dsn_ctx* c;
    hipStream_t caller, st;
    int which;
    bool joined = false;
    StreamScope(dsn_ctx* ctx, hipStream_t caller_, int which_ = 0) : c(ctx), caller(caller_), st(caller_), which(which_) {
      if (!c->use_graphs || c->profiling) return;
      if (!c->own[which]) {
        HIPCHK(hipStreamCreateWithFlags(&c->own[which], hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&c->ev_in[which], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&c->ev_out[which], hipEventDisableTiming));
      }
      HIPCHK(hipEventRecord(c->ev_in[which], caller));
      HIPCHK(hipStreamWaitEvent(c->own[which], c->ev_in[which], 0));
      st = c->own[which];
    }
    StreamScope(const StreamScope&) = delete;
    void leave() {
      joined = true;
      if (st == caller) return;
      HIPCHK(hipEventRecord(c->ev_out[which], st));
      HIPCHK(hipStreamWaitEvent(caller, c->ev_out[which], 0));
    }
    ~StreamScope() {
      if (joined || st == caller) return;
      if (hipEventRecord(c->ev_out[which], st) == hipSuccess) (void)hipStreamWaitEvent(caller, c->ev_out[which], 0);
    }
  };

  // ---------------------------------------------------------------- memory
  void* dmalloc(size_t bytes) {
    void* p = nullptr;
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) fail(DSN_ENOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    allocs.push_back(p);
    return p;
  }
  template <class T>
  T* wsbuf(const std::string& name, size_t count) {
    const size_t bytes = count * sizeof(T) + 256;
    auto it = ws.find(name);
    if (it != ws.end() && it->second.second >= bytes) return (T*)it->second.first;
    if (it != ws.end()) {
      HIPCHK(hipDeviceSynchronize());
      HIPCHK(hipFree(it->second.first));
      ws.erase(it);
    }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) fail(DSN_ENOMEM, "workspace %s: hipMalloc(%zu) failed", name.c_str(), bytes);
    ws[name] = {p, bytes};
    ++ws_epoch;
    return (T*)p;
  }
  int64_t ws_bytes() const {
    int64_t t = 0;
    for (auto& kv : ws) t += (int64_t)kv.second.second;
    return t;
  }

  // ---------------------------------------------------------------- weights
  mutable std::set<std::string> used;  // names finalize() consumed (strict loading: the rest is unexpected)
  const DevTensor& get(const std::string& name) const {
    auto it = raw.find(name);
    if (it == raw.end()) fail(DSN_ESTATE, "missing weight '%s'", name.c_str());
    used.insert(name);
    return it->second;
  }
  bool has(const std::string& name) const { return raw.count(name) != 0; }
  float* maybe(const std::string& name) const { return has(name) ? get(name).p : nullptr; }

  std::vector<float> to_host(const std::string& name) const {
    const DevTensor& t = get(name);
    std::vector<float> h((size_t)t.numel);
    HIPCHK(hipMemcpy(h.data(), t.p, sizeof(float) * h.size(), hipMemcpyDeviceToHost));
    return h;
  }
  void set_raw(const std::string& name, const std::vector<float>& h, std::vector<long> shape) {
    auto it = raw.find(name);
    if (it != raw.end()) {
      (void)hipFree(it->second.p);
      raw.erase(it);
    }
    DevTensor t;
    t.shape = std::move(shape);
    t.numel = (long)h.size();
    HIPCHK(hipMalloc((void**)&t.p, sizeof(float) * h.size()));
    HIPCHK(hipMemcpy(t.p, h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice));
    raw[name] = t;
  }
  // The DiT wraps its transformer in two residual 1x1 convs without bias (dit.py: preprocess_conv before
  // project_in, postprocess_conv after project_out).  Both pairs are linear, so they are folded once (fp64 on
  // the host) into one matrix each:  Win (I + Wpre)  and  (I + Wpost) Wout  -- two small GEMMs less per call.
  void fold_dit_io(const std::string& sp) {
    const DevTensor& win = get(sp + "transformer.project_in.weight");
    const DevTensor& wout = get(sp + "transformer.project_out.weight");
    const long D = win.shape[0], din = win.numel / D, io = wout.shape[0];
    if (wout.numel != io * D || get(sp + "preprocess_conv.weight").numel != din * din ||
        get(sp + "postprocess_conv.weight").numel != io * io)
      fail(DSN_EINVAL, "DiT: preprocess/project_in/project_out/postprocess shapes do not chain");
    const std::vector<float> a = to_host(sp + "transformer.project_in.weight"), pre = to_host(sp + "preprocess_conv.weight");
    const std::vector<float> b = to_host(sp + "transformer.project_out.weight"), post = to_host(sp + "postprocess_conv.weight");
    std::vector<float> fin((size_t)(D * din)), fout((size_t)(io * D));
    for (long r = 0; r < D; ++r)
      for (long c = 0; c < din; ++c) {
        double acc = a[r * din + c];
        for (long k = 0; k < din; ++k) acc += (double)a[r * din + k] * (double)pre[k * din + c];
        fin[r * din + c] = (float)acc;
      }
    std::vector<double> row((size_t)D);
    for (long r = 0; r < io; ++r) {
      for (long c = 0; c < D; ++c) row[c] = b[r * D + c];
      for (long k = 0; k < io; ++k) {
        const double w = post[r * io + k];
        for (long c = 0; c < D; ++c) row[c] += w * (double)b[k * D + c];
      }
      for (long c = 0; c < D; ++c) fout[r * D + c] = (float)row[c];
    }
    set_raw(sp + "__project_in_folded", fin, {D, din});
    set_raw(sp + "__project_out_folded", fout, {io, D});
  }

  Packed pack_linear(const std::string& wname, const std::string& bname, bool swiglu, hipStream_t st) {
    const DevTensor& w = get(wname);
    if (w.shape.size() < 2) fail(DSN_EINVAL, "%s: expected a matrix", wname.c_str());
    Packed p;
    p.N = (int)w.shape[0];
    p.K = (int)(w.numel / w.shape[0]);
    if (swiglu && p.N % 32 != 0)  // (the row map interleaves groups of 16 + 16 rows: a ragged last group reads past the source)
      fail(DSN_EINVAL, "%s: a SwiGLU weight needs N %% 32 == 0 (got %d)", wname.c_str(), p.N);
    p.Cin = p.K;
    p.taps = 1;
    p.ps = (long)p.N * p.K;
    p.w = (op16_t*)dmalloc(sizeof(op16_t) * p.ps * P);
    launch_pack_weight(w.p, nullptr, p.w, p.ps, PL, swiglu ? PACK_LINEAR_SWIGLU : PACK_LINEAR, p.N, p.K, p.K, p.N,
                       1, 1, st);
    if (!bname.empty() && has(bname)) {
      const DevTensor& b = get(bname);
      if (b.numel != p.N) fail(DSN_EINVAL, "%s: bias size mismatch", bname.c_str());
      if (swiglu) {
        p.bias = (float*)dmalloc(sizeof(float) * p.N);
        launch_pack_bias_swiglu(b.p, p.bias, p.N, st);
      } else {
        p.bias = b.p;
      }
      p.bias_mod = p.N;
    }
    return p;
  }

  Packed8 pack_linear_fp8(const std::string& wname, const std::string& bname, bool swiglu, hipStream_t st) {
    const DevTensor& w = get(wname);
    if (w.shape.size() < 2) fail(DSN_EINVAL, "%s: expected a matrix", wname.c_str());
    Packed8 p;
    p.N = (int)w.shape[0];
    p.K = (int)(w.numel / w.shape[0]);
    if (p.K % 128 != 0) fail(DSN_EINVAL, "%s: fp8 GEMMs need K %% 128 == 0 (got %d)", wname.c_str(), p.K);
    if (swiglu && p.N % 32 != 0) fail(DSN_EINVAL, "%s: a SwiGLU weight needs N %% 32 == 0 (got %d)", wname.c_str(), p.N);
    p.w = (unsigned char*)dmalloc((size_t)p.N * p.K);
    p.s = (unsigned char*)dmalloc((size_t)p.N * (p.K / 32));
    launch_pack_weight_fp8(w.p, p.w, p.s, p.N, p.K, swiglu ? 1 : 0, st);
    if (!bname.empty() && has(bname)) {
      const DevTensor& b = get(bname);
      if (b.numel != p.N) fail(DSN_EINVAL, "%s: bias size mismatch", bname.c_str());
      if (swiglu) {
        p.bias = (float*)dmalloc(sizeof(float) * p.N);
        launch_pack_bias_swiglu(b.p, p.bias, p.N, st);
      } else {
        p.bias = b.p;
      }
    }
    return p;
  }

  // weight-normed Conv1d [Cout][Cin][kw] (or plain `weight`) -> [Cout][kw*Cin]
  Packed pack_conv(const std::string& prefix, hipStream_t st) {
    const bool wn = has(prefix + "weight_v");
    const DevTensor& v = get(prefix + (wn ? "weight_v" : "weight"));
    if (v.shape.size() != 3) fail(DSN_EINVAL, "%s: expected [Cout,Cin,k]", prefix.c_str());
    const int Cout = (int)v.shape[0], Cin = (int)v.shape[1], kw = (int)v.shape[2];
    float* scale = nullptr;
    if (wn) {
      scale = (float*)dmalloc(sizeof(float) * Cout);
      launch_wn_scale(v.p, get(prefix + "weight_g").p, scale, Cout, (long)Cin * kw, st);
    }
    Packed p;
    p.N = Cout;
    p.Cin = Cin;
    p.taps = kw;
    p.K = Cin * kw;
    p.ps = (long)p.N * p.K;
    p.w = (op16_t*)dmalloc(sizeof(op16_t) * p.ps * P);
    launch_pack_weight(v.p, scale, p.w, p.ps, PL, PACK_CONV, p.N, p.K, Cin, Cout, kw, 1, st);
    p.bias = maybe(prefix + "bias");
    p.bias_mod = Cout;
    return p;
  }

  // weight-normed ConvTranspose1d [Cin][Cout][2s] -> phase GEMM [s*Cout][2*Cin]
  Packed pack_convT(const std::string& prefix, int stride, hipStream_t st) {
    const bool wn = has(prefix + "weight_v");
    const DevTensor& v = get(prefix + (wn ? "weight_v" : "weight"));
    if (v.shape.size() != 3) fail(DSN_EINVAL, "%s: expected [Cin,Cout,k]", prefix.c_str());
    const int Cin = (int)v.shape[0], Cout = (int)v.shape[1], kw = (int)v.shape[2];
    if (kw != 2 * stride) fail(DSN_EINVAL, "%s: kernel %d != 2*stride %d", prefix.c_str(), kw, stride);
    float* scale = nullptr;
    if (wn) {
      scale = (float*)dmalloc(sizeof(float) * Cin);
      launch_wn_scale(v.p, get(prefix + "weight_g").p, scale, Cin, (long)Cout * kw, st);
    }
    Packed p;
    p.N = stride * Cout;
    p.Cin = Cin;
    p.taps = 2;
    p.K = 2 * Cin;
    p.ps = (long)p.N * p.K;
    p.w = (op16_t*)dmalloc(sizeof(op16_t) * p.ps * P);
    launch_pack_weight(v.p, scale, p.w, p.ps, PL, PACK_CONVT, p.N, p.K, Cin, Cout, kw, stride, st);
    p.bias = maybe(prefix + "bias");
    p.bias_mod = Cout;
    return p;
  }

  ActP make_act(const std::string& prefix, int channels, hipStream_t st) {
    ActP a;
    a.mod = channels;
    if (!cfg.vae_use_snake) {
      a.kind = DSN_ACT_ELU;
      return a;
    }
    a.kind = DSN_ACT_SNAKE;
    a.a = (float*)dmalloc(sizeof(float) * channels);
    a.ib = (float*)dmalloc(sizeof(float) * channels);
    launch_snake_params(get(prefix + "alpha").p, get(prefix + "beta").p, a.a, a.ib, channels, st);
    return a;
  }

  ResUnit make_ru(const std::string& prefix, int ch, int dil, hipStream_t st) {
    ResUnit r;
    r.dil = dil;
    r.act0 = make_act(prefix + "layers.0.", ch, st);
    r.conv7 = pack_conv(prefix + "layers.1.", st);
    r.act2 = make_act(prefix + "layers.2.", ch, st);
    r.conv1 = pack_conv(prefix + "layers.3.", st);
    return r;
  }

  // Tensors the configured network does not consume.  Known buffers of the reference's modules are allowed
  // (RotaryEmbedding.inv_freq, BatchNorm counters); anything else under score_model.* / vae.* means the checkpoint
  // was trained as a different network (cross-attention, adaLN, global conditioning, qk-norm ...): strict mode
  // refuses it (nn.Module.load_state_dict(strict=True) semantics, diffsep_latent.py loads strictly), non-strict
  // drops it.  Either way the unused tensors do not stay resident in HBM.
  void check_unused(bool strict) {
    auto ends_with = [](const std::string& s, const char* suf) {
      const size_t n = strlen(suf);
      return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
    };
    std::vector<std::string> extra, drop;
    for (auto& kv : raw) {
      if (used.count(kv.first)) continue;
      drop.push_back(kv.first);
      if (ends_with(kv.first, "inv_freq") || ends_with(kv.first, "num_batches_tracked")) continue;
      extra.push_back(kv.first);
    }
    if (strict && !extra.empty()) {
      std::string msg;
      for (size_t i = 0; i < extra.size() && i < 6; ++i) msg += (i ? ", " : "") + extra[i];
      if (extra.size() > 6) msg += ", ... (+" + std::to_string(extra.size() - 6) + " more)";
      fail(DSN_ESTATE, "%zu unexpected tensor(s) the configured network does not use: %s", extra.size(), msg.c_str());
    }
    for (auto& name : drop) {
      (void)hipFree(raw[name].p);
      raw.erase(name);
    }
  }

  void finalize(hipStream_t st, bool strict = true) {
    used.clear();
    if (!allocs.empty()) {  // weights replaced (e.g. EMA <-> raw parameters): drop the old packing, graphs are stale
      HIPCHK(hipDeviceSynchronize());
      for (void* q : allocs) (void)hipFree(q);
      allocs.clear();
      ++ws_epoch;
    }
    const int D = cfg.dit_embed_dim;
    fold_ln = dit_fold_ln(cfg, sw);
    fold_ln8 = dit_fold_ln8(cfg, sw);
    if (cfg.score_kind == DSN_SCORE_DIT) {
      const std::string sp = "score_model.";
      if (D % 64 != 0 || cfg.dit_heads <= 0 || D / cfg.dit_heads != 64 || D % cfg.dit_heads != 0)
        fail(DSN_EINVAL, "DiT: embed_dim must be heads x 64 (got %d / %d heads)", D, cfg.dit_heads);
      tf_w = get(sp + "timestep_features.weight").p;
      t1 = pack_linear(sp + "to_timestep_embed.0.weight", sp + "to_timestep_embed.0.bias", false, st);
      t2 = pack_linear(sp + "to_timestep_embed.2.weight", sp + "to_timestep_embed.2.bias", false, st);
      fold_dit_io(sp);
      pin = pack_linear(sp + "__project_in_folded", "", false, st);
      pout = pack_linear(sp + "__project_out_folded", "", false, st);
      layers.resize(cfg.dit_depth);
      for (int i = 0; i < cfg.dit_depth; ++i) {
        const std::string lp = sp + "transformer.layers." + std::to_string(i) + ".";
        DitLayer& L = layers[i];
        L.g1 = get(lp + "pre_norm.gamma").p;
        L.be1 = maybe(lp + "pre_norm.beta");
        L.g2 = get(lp + "ff_norm.gamma").p;
        L.be2 = maybe(lp + "ff_norm.beta");
        if (fp8) {
          L.qkv8 = pack_linear_fp8(lp + "self_attn.to_qkv.weight", "", false, st);
          // (also in 16 bits: where the fused to_qkv + attention kernel applies, that block runs on fp16 operands and
          // hands its output to the fp8 out-projection as e4m3 + scales)
          L.qkv = pack_linear(lp + "self_attn.to_qkv.weight", "", false, st);
          L.out8 = pack_linear_fp8(lp + "self_attn.to_out.weight", "", false, st);
          L.ff1_8 = pack_linear_fp8(lp + "ff.ff.0.proj.weight", lp + "ff.ff.0.proj.bias", true, st);
          L.ff2_8 = pack_linear_fp8(lp + "ff.ff.2.weight", lp + "ff.ff.2.bias", false, st);
          if (fold_ln8) {
            // ff_norm folded into FF-in as in the 16-bit modes: gamma is multiplied in BEFORE the block quantisation, the
            // row sums are those of the dequantised bytes (what the MFMAs multiply), beta goes into the bias
            const DevTensor& w = get(lp + "ff.ff.0.proj.weight");
            Packed8& p = L.ff1f8;
            p.N = L.ff1_8.N;
            p.K = L.ff1_8.K;
            p.w = (unsigned char*)dmalloc((size_t)p.N * p.K);
            p.s = (unsigned char*)dmalloc((size_t)p.N * (p.K / 32));
            launch_pack_weight_fp8(w.p, p.w, p.s, p.N, p.K, 1, st, L.g2);
            L.ff1_colsum8 = (float*)dmalloc(sizeof(float) * p.N);
            launch_fp8_row_sum(p.w, p.s, p.N, p.K, L.ff1_colsum8, st);
            p.bias = L.ff1_8.bias;
            if (L.be2) {
              float* tmp = (float*)dmalloc(sizeof(float) * p.N);
              launch_bias_plus_wbeta(w.p, L.be2, maybe(lp + "ff.ff.0.proj.bias"), p.N, p.K, tmp, st);
              p.bias = (float*)dmalloc(sizeof(float) * p.N);
              launch_pack_bias_swiglu(tmp, p.bias, p.N, st);
            }
          }
          continue;
        }
        L.qkv = pack_linear(lp + "self_attn.to_qkv.weight", "", false, st);
        L.out = pack_linear(lp + "self_attn.to_out.weight", "", false, st);
        L.ff1 = pack_linear(lp + "ff.ff.0.proj.weight", lp + "ff.ff.0.proj.bias", true, st);
        L.ff2 = pack_linear(lp + "ff.ff.2.weight", lp + "ff.ff.2.bias", false, st);
        if (fold_ln) {
          // LN(x) W^T = rstd (x (W diag(gamma))^T - mean colsum) + (b + W beta): gamma into the packed weight, the
          // row sums from the ROUNDED packed values, beta into the bias (dit_forward: FF-in consumes raw x planes)
          const DevTensor& w = get(lp + "ff.ff.0.proj.weight");
          Packed& p = L.ff1f;
          p.N = (int)w.shape[0];
          p.K = p.Cin = (int)(w.numel / w.shape[0]);
          p.taps = 1;
          p.ps = (long)p.N * p.K;
          p.w = (op16_t*)dmalloc(sizeof(op16_t) * p.ps * P);
          launch_pack_weight(w.p, nullptr, p.w, p.ps, PL, PACK_LINEAR_SWIGLU, p.N, p.K, p.K, p.N, 1, 1, st, L.g2);
          L.ff1_colsum = (float*)dmalloc(sizeof(float) * p.N);
          launch_packed_row_sum(p.w, p.ps, PL, p.N, p.K, L.ff1_colsum, st);
          const float* b1 = maybe(lp + "ff.ff.0.proj.bias");
          p.bias = L.ff1.bias;
          if (L.be2) {
            float* tmp = (float*)dmalloc(sizeof(float) * p.N);
            launch_bias_plus_wbeta(w.p, L.be2, b1, p.N, p.K, tmp, st);
            p.bias = (float*)dmalloc(sizeof(float) * p.N);
            launch_pack_bias_swiglu(tmp, p.bias, p.N, st);
          }
          p.bias_mod = p.N;
        }
      }
    }
    if (cfg.score_kind == DSN_SCORE_NCSNPP) finalize_ncsnpp(st);
    const int nb = cfg.vae_n_blocks;
    const int ch = cfg.vae_channels;
    std::vector<int> mult(nb + 1, 1);
    for (int i = 0; i < nb; ++i) mult[i + 1] = cfg.vae_c_mults[i];
    if (cfg.vae_has_decoder) {
      const std::string dp = "vae.decoder.";
      dec_in = pack_conv(dp + "layers.0.", st);
      dec_blocks.resize(nb);
      int li = 1;
      for (int i = nb; i >= 1; --i, ++li) {
        VaeBlock& b = dec_blocks[li - 1];
        const std::string bp = dp + "layers." + std::to_string(li) + ".";
        b.cin = mult[i] * ch;
        b.cout = mult[i - 1] * ch;
        b.stride = cfg.vae_strides[i - 1];
        b.act = make_act(bp + "layers.0.", b.cin, st);
        b.conv = pack_convT(bp + "layers.1.", b.stride, st);
        const int dils[3] = {1, 3, 9};
        for (int j = 0; j < 3; ++j)
          b.ru[j] = make_ru(bp + "layers." + std::to_string(2 + j) + ".", b.cout, dils[j], st);
      }
      dec_final_act = make_act(dp + "layers." + std::to_string(li) + ".", mult[0] * ch, st);
      // final conv (Cout = 1 per io channel; io_channels == 1 on this path): fold weight norm -> [k][C]
      {
        const std::string fp = dp + "layers." + std::to_string(li + 1) + ".";
        const bool wn = has(fp + "weight_v");
        const DevTensor& v = get(fp + (wn ? "weight_v" : "weight"));
        if (v.shape[0] != 1) fail(DSN_EINVAL, "decoder io_channels must be 1 (got %ld)", v.shape[0]);
        const int C = (int)v.shape[1], kw = (int)v.shape[2];
        dec_out_taps = kw;
        std::vector<float> hv(v.numel), hg(1, 1.f);
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(hv.data(), v.p, sizeof(float) * v.numel, hipMemcpyDeviceToHost));
        double nrm = 1.0, g = 1.0;
        if (wn) {
          HIPCHK(hipMemcpy(hg.data(), get(fp + "weight_g").p, sizeof(float), hipMemcpyDeviceToHost));
          double ss = 0;
          for (float x : hv) ss += (double)x * x;
          nrm = sqrt(ss);
          g = hg[0];
        }
        std::vector<float> w(kw * C);
        for (int c = 0; c < C; ++c)
          for (int k = 0; k < kw; ++k) w[k * C + c] = (float)(hv[c * kw + k] * ((float)g / (float)nrm));
        dec_out_w = (float*)dmalloc(sizeof(float) * w.size());
        HIPCHK(hipMemcpy(dec_out_w, w.data(), sizeof(float) * w.size(), hipMemcpyHostToDevice));
      }
    }
    if (cfg.vae_has_encoder) {
      const std::string ep = "vae.encoder.";
      {
        // first conv: Cin = 1, fold weight norm on the host (tiny) -> [Cout][k]
        const std::string fp = ep + "layers.0.";
        const bool wn = has(fp + "weight_v");
        const DevTensor& v = get(fp + (wn ? "weight_v" : "weight"));
        if (v.shape[1] != 1) fail(DSN_EINVAL, "encoder in_channels must be 1");
        const int Cout = (int)v.shape[0], kw = (int)v.shape[2];
        std::vector<float> hv(v.numel), hg(Cout, 1.f);
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(hv.data(), v.p, sizeof(float) * v.numel, hipMemcpyDeviceToHost));
        if (wn) HIPCHK(hipMemcpy(hg.data(), get(fp + "weight_g").p, sizeof(float) * Cout, hipMemcpyDeviceToHost));
        for (int co = 0; co < Cout; ++co) {
          float s = 1.f;
          if (wn) {
            float ss = 0;
            for (int k = 0; k < kw; ++k) ss += hv[co * kw + k] * hv[co * kw + k];
            s = hg[co] / sqrtf(ss);
          }
          for (int k = 0; k < kw; ++k) hv[co * kw + k] *= s;
        }
        enc_in_w = (float*)dmalloc(sizeof(float) * hv.size());
        HIPCHK(hipMemcpy(enc_in_w, hv.data(), sizeof(float) * hv.size(), hipMemcpyHostToDevice));
        enc_in_b = maybe(fp + "bias");
      }
      enc_blocks.resize(nb);
      int li = 1;
      for (int i = 0; i < nb; ++i, ++li) {
        VaeBlock& b = enc_blocks[i];
        const std::string bp = ep + "layers." + std::to_string(li) + ".";
        b.cin = mult[i] * ch;
        b.cout = mult[i + 1] * ch;
        b.stride = cfg.vae_strides[i];
        const int dils[3] = {1, 3, 9};
        for (int j = 0; j < 3; ++j) b.ru[j] = make_ru(bp + "layers." + std::to_string(j) + ".", b.cin, dils[j], st);
        b.act = make_act(bp + "layers.3.", b.cin, st);
        b.conv = pack_conv(bp + "layers.4.", st);
      }
      enc_final_act = make_act(ep + "layers." + std::to_string(li) + ".", mult[nb] * ch, st);
      enc_out = pack_conv(ep + "layers." + std::to_string(li + 1) + ".", st);
    }
    HIPCHK(hipStreamSynchronize(st));
    check_unused(strict);
    finalized = true;
  }

  // ---------------------------------------------------------------- GEMM helper
  // dense conv-like contraction over channels-last planes
  GemmDesc base_desc(const op16_t* A, long a_ps, const Packed& w, int Bn, int rows_per_b, int Lin) {
    GemmDesc d;
    memset(&d, 0, sizeof d);
    d.A = A;
    d.a_ps = a_ps;
    d.W = w.w;
    d.w_ps = w.ps;
    d.M = Bn * rows_per_b;
    d.N = w.N;
    d.Cin = w.Cin;
    d.taps = w.taps;
    d.rows_per_b = rows_per_b;
    d.Lin = Lin;
    d.in_stride = 1;
    d.tap_dil = 1;
    d.in_pad = 0;
    d.in_bstride = (long)Lin * w.Cin;
    d.in_row_elems = w.Cin;
    d.out_bstride = (long)rows_per_b * w.N;
    d.out_row_elems = w.N;
    d.out_off = 0;
    d.out_limit = d.out_bstride;
    d.resid_bstride = d.out_bstride;
    d.resid_row_elems = d.out_row_elems;
    d.resid_off = d.out_off;
    d.bias = w.bias;
    d.bias_mod = w.bias_mod;
    d.out_scale = 1.f;
    d.act_mod = 1;
    return d;
  }
  void set_act(GemmDesc& d, const ActP& a) {
    d.act = a.kind;
    d.act_a = a.a;
    d.act_b = a.ib;
    d.act_mod = a.mod;
  }
  // DSN_AUDIT=1 (tests): before a GEMM-family launch, every pointer of its descriptor is checked on the HOST against
  // the device allocation that contains it (hipMemGetAddressRange), over the exact extent the kernels' guards allow --
  // the largest (item, row, column) offsets of A, W, the fp32 / plane / slab outputs, residual, bias vectors, GroupNorm
  // and LayerNorm partials -- plus the shape preconditions the epilogues rely on (GroupNorm partials: whole 64-row
  // slices of one item per wave tile, N % 4 == 0; halo conv: tiles inside one image).  An out-of-range descriptor is an
  // error naming the field instead of a GPU memory fault.
  void audit_span(const char* what, const void* p, long lo_bytes, long hi_bytes, const GemmDesc& d) const {
    if (!p || hi_bytes <= lo_bytes) return;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess)
      fail(DSN_EINVAL, "audit: %s = %p is not inside a device allocation (M=%d N=%d Cin=%d taps=%d)", what, p, d.M, d.N,
           d.Cin, d.taps);
    const char* b0 = (const char*)base;
    const char* q = (const char*)p;
    if (q + lo_bytes < b0 || q + hi_bytes > b0 + size)
      fail(DSN_EINVAL, "audit: %s spans [%ld, %ld) bytes from its pointer but the allocation holds [%ld, %ld) "
           "(M=%d N=%d Cin=%d taps=%d rows_per_b=%d)", what, lo_bytes, hi_bytes, (long)(b0 - q), (long)(b0 + size - q),
           d.M, d.N, d.Cin, d.taps, d.rows_per_b);
  }
  // engine_gn_slots: GroupNorm partials go to the engine's statistics slots (the test hook passes caller-owned buffers,
  // audited by their allocation alone)
  void audit_desc(const GemmDesc& d, bool engine_gn_slots = true) const {
    if (d.a_scale) return;  // fp8 descriptors address bytes pairwise: audited by their launcher's shape checks
    const long nb = cdiv(d.M, d.rows_per_b), rows_last = d.M - (nb - 1) * (long)d.rows_per_b;
    const long rows_max = nb > 1 ? d.rows_per_b : rows_last;
    const long e16 = sizeof(op16_t), e32 = sizeof(float);
    if (d.M <= 0 || d.N <= 0 || d.rows_per_b <= 0) fail(DSN_EINVAL, "audit: empty GEMM");
    audit_span("A", d.A, 0, ((nb - 1) * d.in_bstride + (long)(d.Lin - 1) * d.in_row_elems + d.Cin + (P - 1) * d.a_ps) * e16, d);
    audit_span("W", d.W, 0, ((long)d.N * d.taps * d.Cin + (P - 1) * d.w_ps) * e16, d);
    const long n_out = d.swiglu ? d.N / 2 : d.N;
    const long rel_hi = std::min<long>(d.out_limit, (rows_max - 1) * (long)d.out_row_elems + d.out_off + n_out);
    const long out_hi = (nb - 1) * d.out_bstride + rel_hi;
    const long ks = std::max(d.ksplit, 1);
    if (d.stat_out) {  // residual-stream producer: plain row-major [M][N]
      audit_span("out_f32", d.out_f32, 0, (long)d.M * d.N * e32, d);
      audit_span("out_planes", d.out_planes, 0, ((long)d.M * d.N + (P - 1) * d.out_ps) * e16, d);
      audit_span("stat_out", d.stat_out, 0, (long)d.M * d.stat_np * 2 * e32, d);
    } else {
      audit_span("out_f32", d.out_f32, 0, (out_hi + (ks - 1) * d.slab_stride) * e32, d);
      audit_span("out_planes", d.out_planes, 0, (out_hi + (P - 1) * d.out_ps) * e16, d);
    }
    audit_span("resid", d.resid, 0, ((nb - 1) * d.resid_bstride + (rows_max - 1) * (long)d.resid_row_elems + d.resid_off + d.N) * e32, d);
    if (d.resid && d.resid_off < 0) fail(DSN_EINVAL, "audit: negative residual offset");
    audit_span("bias", d.bias, 0, (long)d.bias_mod * e32, d);
    audit_span("bbias", d.bbias, 0, ((nb - 1) * (long)d.bbias_stride + d.N) * e32, d);
    if (d.act == DSN_ACT_SNAKE) {
      audit_span("act_a", d.act_a, 0, (long)d.act_mod * e32, d);
      audit_span("act_b", d.act_b, 0, (long)d.act_mod * e32, d);
    }
    if (d.gn_stats) {
      if (d.rows_per_b % 64 != 0 || d.N % 4 != 0 || d.M % d.rows_per_b != 0 || d.ksplit > 1)
        fail(DSN_EINVAL, "audit: GroupNorm partials need whole 64-row slices (rows_per_b=%d M=%d N=%d ksplit=%d)",
             d.rows_per_b, d.M, d.N, d.ksplit);
      audit_span("gn_stats", d.gn_stats, 0, nb * (d.rows_per_b / 64) * (long)(d.N / 4) * 2 * e32, d);
      if (engine_gn_slots && nb * (d.rows_per_b / 64) * (long)(d.N / 4) * 2 > ncs_slot_floats)
        fail(DSN_EINVAL, "audit: GroupNorm partials overflow their statistics slot");
      if (d.gn_stats2) {
        if (d.gn_qoff2 < 0 || d.gn_qoff2 + d.N / 4 > d.gn_nq2 ||
            (engine_gn_slots && nb * (d.rows_per_b / 64) * (long)d.gn_nq2 * 2 > ncs_slot_floats))
          fail(DSN_EINVAL, "audit: concat GroupNorm partials outside their slot (nq2=%d qoff2=%d N=%d)", d.gn_nq2,
               d.gn_qoff2, d.N);
        audit_span("gn_stats2", d.gn_stats2, 0, nb * (d.rows_per_b / 64) * (long)d.gn_nq2 * 2 * e32, d);
      }
    }
    if (d.ln_stats) {
      audit_span("ln_stats", d.ln_stats, 0, (long)d.M * d.ln_np * 2 * e32, d);
      audit_span("ln_colsum", d.ln_colsum, 0, (long)d.N * e32, d);
    }
    if (d.rope_cos) {
      audit_span("rope_cos", d.rope_cos, 0, (long)d.rope_S * 32 * e32, d);
      audit_span("rope_sin", d.rope_sin, 0, (long)d.rope_S * 32 * e32, d);
    }
    if (d.sc_A) {  // 1x1 shortcut of the halo conv (single-plane modes)
      audit_span("sc_A", d.sc_A, 0, ((nb - 1) * d.sc_bstride + (rows_max - 1) * (long)d.sc_row_elems + d.sc_Cin) * e16, d);
      audit_span("sc_W", d.sc_W, 0, (long)d.N * d.sc_Cin * e16, d);
      audit_span("sc_bias", d.sc_bias, 0, (long)d.N * e32, d);
    }
    if (d.img_w > 0 && (d.rows_per_b != d.img_w * d.img_h || d.taps != 9))
      fail(DSN_EINVAL, "audit: 2-D conv descriptor with rows_per_b != H*W");
  }
  void run(const GemmDesc& d, hipStream_t st, int panel_bn = 0, bool skinny = false) {
    if (sw.audit) audit_desc(d);
    const double flops = 2.0 * (double)d.M * (double)d.N * ((double)d.taps * (double)d.Cin + (d.sc_A ? (double)d.sc_Cin : 0.0));
    // NCSN++ convs of single mixtures: a handful of 128 x 128 tiles each walking a long K alone -> split-K over enough
    // workgroups for a quarter of the chip, then the slab epilogue (B = 1, T = 16: score call 3.07 -> see DESIGN 5)
    const long ctiles = (long)cdiv(d.M, 128) * cdiv(d.N, 128);
    const bool split = P == 1 && cfg.score_kind == DSN_SCORE_NCSNPP && !skinny && panel_bn == 0 && d.ksplit <= 1 &&
        d.Cin % 32 == 0 && d.N % 64 == 0 && ctiles <= 32 && d.taps * d.Cin >= 512 && !d.swiglu && !d.rope_cos &&
        (d.out_f32 || d.out_planes) && d.out_off >= 0 && d.tap_dil >= 0 && d.in_stride == 1 &&
        (d.img_w > 0 || (d.taps == 1 && d.in_pad == 0));
    const hipError_t e = profiled({cur_tag, flops}, st, [&] {
      if (!split)
        return skinny ? igemm_skinny_launch(d, PL, st)
                      : (panel_bn > 0 ? igemm_panel_launch(d, PL, panel_bn, st) : igemm2_launch(d, PL, st));
      const int nkt = d.taps * d.Cin / 32;
      const int ks = (int)std::max(2L, std::min<long>(std::min<long>(8, nkt / 4), 64 / ctiles));
      const long span = (long)cdiv(d.M, d.rows_per_b) * d.out_bstride;  // floats one slab covers: the output view
      float* slabs = wsbuf<float>("conv_slabs", span * 8);
      GemmDesc g = d;
      g.ksplit = ks;
      g.slab_stride = span;
      g.out_f32 = slabs;
      g.out_planes = nullptr;
      g.gn_stats = nullptr;
      g.gn_stats2 = nullptr;
      g.cfg_bm = 128;
      g.cfg_bn = 128;
      g.cfg_nst = 3;
      g.cfg_bk = 32;
      hipError_t e1 = igemm2_launch(g, PL, st);
      if (e1 == hipSuccess) e1 = igemm_slab_epilogue_launch(d, PL, slabs, ks, span, st);
      return e1;
    });
    if (e != hipSuccess && split) fail(DSN_EHIP, "split conv launch failed: %s", hipGetErrorString(e));
    if (e != hipSuccess) fail(DSN_EHIP, "igemm launch failed: %s (M=%d N=%d Cin=%d taps=%d)", hipGetErrorString(e),
                              d.M, d.N, d.Cin, d.taps);
  }

  // descriptor of an fp8 (MX) row-major GEMM: A8 [M][K] bytes + scales [M][K/32], weight w
  GemmDesc fp8_desc(const unsigned char* A8, const unsigned char* SA, const Packed8& w, int M) {
    Packed pk = plain_packed(reinterpret_cast<op16_t*>(w.w), 0, w.N, w.K / 2, 1);  // Cin in byte pairs
    pk.bias = w.bias;
    pk.bias_mod = w.N;
    GemmDesc d = base_desc(reinterpret_cast<const op16_t*>(A8), 0, pk, 1, M, M);
    d.a_scale = SA;
    d.w_scale = w.s;
    d.mx_kblocks = w.K / 32;
    return d;
  }
  void run_fp8(const GemmDesc& d, hipStream_t st, int bn) {
    const hipError_t e = profiled({cur_tag, 2.0 * (double)d.M * (double)d.N * 2.0 * (double)d.Cin}, st,
                                  [&] { return igemm_panel_fp8_launch(d, bn, st); });
    if (e != hipSuccess) fail(DSN_EHIP, "fp8 igemm launch failed: %s (M=%d N=%d K=%d rows=%d bn=%d)", hipGetErrorString(e),
                              d.M, d.N, 2 * d.Cin, d.panel_rows, bn);
  }

  // fused ResidualUnit (ru_fused.hip) for the 128-channel layers; `in` and `out` planes must differ
  bool ru_fusable(const ResUnit& r) const {
    return r.conv7.taps == 7 && r.conv7.Cin == 128 && r.conv7.N == 128 && r.conv1.taps == 1 &&
           r.conv1.Cin == 128 && r.conv1.N == 128 && r.dil <= 9;
  }
  void run_ru(const ResUnit& r, const op16_t* in, long ps, float* xf, float* out_f32, op16_t* out, const ActP& next,
              int S, long L, hipStream_t st) {
    RuDesc d;
    memset(&d, 0, sizeof d);
    d.A = in;
    d.a_ps = ps;
    d.X = xf;
    d.W7 = r.conv7.w;
    d.w7_ps = r.conv7.ps;
    d.b7 = r.conv7.bias;
    d.W1 = r.conv1.w;
    d.w1_ps = r.conv1.ps;
    d.b1 = r.conv1.bias;
    d.out_f32 = out_f32;
    d.out_planes = out;
    d.out_ps = ps;
    d.act_mid = r.act2.kind;
    d.mid_a = r.act2.a;
    d.mid_b = r.act2.ib;
    d.act_out = next.kind;
    d.out_a = next.a;
    d.out_b = next.ib;
    d.S = S;
    d.L = (int)L;
    d.dil = r.dil;
    const double flops = 2.0 * (double)S * (double)L * 128.0 * 128.0 * 8.0;
    // algorithmic HBM bytes: planes in, fp32 residual in, fp32 out (when kept), planes out
    const double bytes = (double)S * (double)L * 128.0 * (2.0 * P + 4.0 + (out_f32 ? 4.0 : 0.0) + 2.0 * P);
    const hipError_t e = profiled({"vae.residual_unit_fused", flops, bytes, true, true}, st,
                                  [&] { return ru_fused_launch(d, PL, sw.ru_v1, st); });
    if (e != hipSuccess) fail(DSN_EHIP, "fused residual unit launch failed: %s (S=%d L=%ld dil=%d)",
                              hipGetErrorString(e), S, L, r.dil);
  }

  // One ResidualUnit of the coders on the stream planes `x` (plane stride ps, fp32 copy in xf) with scratch planes `h`:
  // the fused kernel x -> h, after which the two trade places, or a dilated k7 conv into h and a k1 conv + residual back
  // into x.  keep_f32: a further unit of the block reads the fp32 stream; `next`: the activation of x's consumer.
  // cl (null = dense) / mul: ragged batch -- the unit's output rows past an item's end are cleared (tail_zero)
  void res_unit(const ResUnit& r, op16_t*& x, op16_t*& h, long ps, float* xf, bool keep_f32, const ActP& next, int S,
                long L, hipStream_t st, const CodecLens* cl = nullptr, long mul = 0) {
    if (ru_fusable(r)) {
      run_ru(r, x, ps, xf, keep_f32 ? xf : nullptr, h, next, S, L, st);
      std::swap(x, h);
      if (cl) tail_zero(*cl, x, ps, keep_f32 ? xf : nullptr, nullptr, S, L, r.conv1.N, mul, st);
      return;
    }
    Tag tg(this, "vae.residual_unit_2gemm");
    {
      GemmDesc d = base_desc(x, ps, r.conv7, S, (int)L, (int)L);
      d.tap_dil = r.dil;
      d.in_pad = r.dil * (r.conv7.taps - 1) / 2;
      d.out_planes = h;
      d.out_ps = ps;
      set_act(d, r.act2);
      run(d, st);
    }
    {
      GemmDesc d = base_desc(h, ps, r.conv1, S, (int)L, (int)L);
      d.resid = xf;
      d.out_planes = x;
      d.out_ps = ps;
      if (keep_f32) d.out_f32 = xf;
      set_act(d, next);
      run(d, st);
    }
    if (cl) tail_zero(*cl, x, ps, keep_f32 ? xf : nullptr, nullptr, S, L, r.conv1.N, mul, st);
  }
  // Ragged batch in the codec: rows [frames * mul, L) of every item of a layer's output [S][L][C] -- operand planes,
  // fp32 stream and / or plain fp32 output, null where the layer wrote none -- are written as zero, so that the next
  // convolution reads past an item's end what it reads for the item alone (include/ditsep_hip.h).  One
  // launch whose grid depends on (S, L, C) alone.
  void tail_zero(const CodecLens& cl, op16_t* planes, long ps, float* xf, float* out, int S, long L, int C, long mul,
                 hipStream_t st) {
    double rows = 0;  // algorithmic bytes: the tail rows of every destination, written once
    for (int s = 0; s < S; ++s) rows += (double)std::max(0L, L - (long)cl.host[s / cl.rep] * mul);
    const double bytes = rows * C * ((planes ? 2.0 * P : 0.0) + (xf ? 4.0 : 0.0) + (out ? 4.0 : 0.0));
    prof_launch("vae.ragged_tail_zero", bytes, st, [&] {
      const char* why = launch_codec_tail_zero(planes, ps, P, xf, out, S, (int)L, C, cl.frames, cl.rep, (int)mul, st);
      if (why) fail(DSN_EINVAL, "ragged codec tail launch refused: %s (S=%d L=%ld C=%d mul=%ld)", why, S, L, C, mul);
    });
  }

  // ---------------------------------------------------------------- DiT score
  // xt [B,n,Dl,T], t [B], mix [B,1,Dl,T] -> score token-major [B*T][n*Dl] in ws "sc"
  // timestep token: t [rows] -> to_timestep_embed(FourierFeatures(t)) fp32 [rows][D]  (dit.py: timestep_features,
  // to_timestep_embed).  The sampler calls it once for all N x B step times (time_cache) instead of per score call.
  void dit_time_embed(const float* t, int rows, float* out, hipStream_t st) {
    const int D = cfg.dit_embed_dim;
    op16_t* TF = wsbuf<op16_t>("dit_TF", (long)rows * 256 * P);
    op16_t* TE = wsbuf<op16_t>("dit_TE", (long)rows * D * P);
    launch_timestep_features(t, tf_w, rows, 128, TF, (long)rows * 256, PL, st);
    GemmDesc d = base_desc(TF, (long)rows * 256, t1, rows, 1, 1);
    d.out_planes = TE;
    d.out_ps = (long)rows * D;
    d.act = DSN_ACT_SILU;
    run(d, st);
    GemmDesc e = base_desc(TE, (long)rows * D, t2, rows, 1, 1);
    e.out_f32 = out;
    run(e, st);
  }
  // Per-sampler-pass cache of network time inputs: tv [N][B] step times -> rows of `data` ([N*B][width])
  struct TimeCache {
    const float* t0 = nullptr;  // first element of the cached time vector
    long rows = 0;
    float* data = nullptr;
    int width = 0;
    const float* find(const float* t, int B) const {
      if (!data || t < t0 || t + B > t0 + rows) return nullptr;
      return data + (long)(t - t0) * width;
    }
  } time_cache;

  // lens (device int [B], null = dense): a ragged batch padded to T frames -- tokens per item, 1 + its frame count.
  // The kernel-family choice below is that of (B, T); only the attention launch takes its length-aware variant (every
  // other operation acts per token, so an item's valid rows come out as in a call of its own).
  // wm (null = none): the items are windows cut from longer tensors -- xt [R,n,Dl,wm->Tsrc], mix [R,1,Dl,wm->Tsrc], item b
  // the window wm->wtab[b] = (recording, start, length) -- gathered by the pack launch; the score tokens go to wm->sc.
  // Everything between the pack and the last store is the dense call at (B, T).
  struct WinMap {
    const int* wtab;
    int Tsrc;
    float* sc;
  };
  float* dit_forward(const float* xt, const float* t, const float* mix, int B, int T, hipStream_t st,
                     const int* lens = nullptr, const WinMap* wm = nullptr) {
    const int n = cfg.n_src, Dl = cfg.latent_dim, D = cfg.dit_embed_dim, H = cfg.dit_heads;
    const int io = n * Dl, din = io + Dl, S = T + 1;
    const long Mt = (long)B * T, M = (long)B * S;
    op16_t* Up = wsbuf<op16_t>("dit_Up", Mt * din * P);
    float* X = wsbuf<float>("dit_X", M * D);
    op16_t* Ap = wsbuf<op16_t>("dit_Ap", M * D * P);
    op16_t* QKVp = wsbuf<op16_t>("dit_QKVp", M * 3 * D * P);
    op16_t* FF = wsbuf<op16_t>("dit_FF", M * 4 * D * P);
    float* SC = wm ? wm->sc : wsbuf<float>("sc", Mt * io);
    // DSN_PREC_FP8: the layer GEMMs' A operands as e4m3 bytes + E8M0 block scales (LayerNorm output / attention
    // output share one buffer, the SwiGLU hidden state has its own)
    unsigned char* A8 = fp8 ? wsbuf<unsigned char>("dit_A8", M * D) : nullptr;
    unsigned char* SA8 = fp8 ? wsbuf<unsigned char>("dit_SA8", M * D / 32) : nullptr;
    unsigned char* H8 = fp8 ? wsbuf<unsigned char>("dit_H8", M * 4 * D) : nullptr;
    unsigned char* SH8 = fp8 ? wsbuf<unsigned char>("dit_SH8", M * 4 * D / 32) : nullptr;
    op16_t* lnout = fp8 ? reinterpret_cast<op16_t*>(A8) : Ap;
    // every decision of the call -- kernel families, panel heights, split-K factors -- and why: dit_plan.h
    const DitPlan plan = dit_plan(cfg, B, T, fold_ln, fold_ln8, sw, dit_limits());
    const bool skinny = plan.skinny != 0;
    const int fold_rows = plan.fold_rows, qa_ipp = plan.qa_ipp;
    op16_t* Xp = (fold_rows && !fp8) ? wsbuf<op16_t>("dit_Xp", M * D) : nullptr;
    // (fp8: raw x' as e4m3 + block scales; NOT the to_out input buffer -- other column tiles still read those rows)
    unsigned char* X8 = (fold_rows && fp8) ? wsbuf<unsigned char>("dit_X8", M * D) : nullptr;
    unsigned char* SX8 = (fold_rows && fp8) ? wsbuf<unsigned char>("dit_SX8", M * D / 32) : nullptr;
    float* ST = fold_rows ? wsbuf<float>("dit_ST", M * (D / 64) * 2) : nullptr;
    const int rot = 32;  // max(dim_heads/2, 32) with 64-wide heads
    const bool new_rope = !ws.count("rope_cos_" + std::to_string(S));
    float* rc = wsbuf<float>("rope_cos_" + std::to_string(S), (long)S * rot);
    float* rs = wsbuf<float>("rope_sin_" + std::to_string(S), (long)S * rot);
    if (new_rope) launch_rope_tables(rc, rs, S, rot, st);

    if (wm) launch_win_pack_tokens(xt, io, mix, Dl, wm->wtab, B, T, wm->Tsrc, nullptr, Up, Mt * din, PL, st);
    else launch_pack_tokens(xt, io, mix, Dl, B, T, nullptr, Up, Mt * din, PL, st);
    {  // X[b, 1+t] = (U + U Wpre^T) Win^T, one folded matrix (fold_dit_io)
      Tag tg(this, "dit.project_in");
      GemmDesc d = base_desc(Up, Mt * din, pin, B, T, T);
      d.out_f32 = X;
      d.out_bstride = (long)S * D;
      d.out_off = D;
      d.out_limit = (long)S * D;
      run(d, st);
    }
    {  // timestep token -> X[b, 0]
      const float* te = time_cache.find(t, B);
      if (!te) {
        float* tmp = wsbuf<float>("dit_te1", (long)B * D);
        Tag tg(this, "dit.time_embed");
        dit_time_embed(t, B, tmp, st);
        te = tmp;
      }
      launch_copy_rows(te, X, B, D, (long)S * D, st);
    }
    op16_t* AOp = qa_ipp ? wsbuf<op16_t>("dit_AOp", M * D) : nullptr;
    float* slabs = nullptr;
    int pend_n = 0;
    const float* pend_bias = nullptr;
    const long slab_stride = M * D;
    // A layer GEMM's descriptor over M token rows: the fp8 operand with its scales and weight in the fp8 mode, else the
    // 16-bit planes and weight
    auto layer_desc = [&](const op16_t* A16, const unsigned char* A8b, const unsigned char* SA, const Packed& w,
                          const Packed8& w8) {
      return fp8 ? fp8_desc(A8b, SA, w8, (int)M) : base_desc(A16, M * w.Cin, w, 1, (int)M, (int)M);
    };
    // ... and its kernel family: fp8 row panels, the weight-streaming skinny kernel, or the 16-bit kernels (row panels in
    // bn-column tiles where the plan gave it a panel height)
    auto layer_gemm = [&](const GemmDesc& d, int bn) {
      if (fp8) run_fp8(d, st, bn);
      else if (skinny) run(d, st, 0, true);
      else run(d, st, d.panel_rows ? bn : 0);
    };
    // A residual-stream GEMM (out-proj, FF-out) in bn-column tiles: split-K into fp32 slabs, whose reduction + bias +
    // residual the following residual_norm does (pend_n, pend_bias); without split-K it adds the residual and writes X
    // itself.  (to_out has no bias: pack_linear gives it none to defer.)
    auto stream_gemm = [&](GemmDesc& d, int bn, int ksplit, int rows) {
      d.ksplit = ksplit;
      d.panel_rows = rows;
      if (d.ksplit > 1) {
        slabs = wsbuf<float>("dit_slabs", slab_stride * RESIDUAL_NORM_MAX_SLABS);
        d.out_f32 = slabs;
        d.slab_stride = slab_stride;
        pend_bias = d.bias;
        d.bias = nullptr;
      } else {
        d.resid = X;
        d.out_f32 = X;
        pend_bias = nullptr;
      }
      layer_gemm(d, bn);
      pend_n = d.ksplit > 1 ? d.ksplit : 0;
    };
    for (int i = 0; i < cfg.dit_depth; ++i) {
      const DitLayer& L = layers[i];
      // algorithmic bytes of the fused reduce + LayerNorm: x in/out (when slabs are pending), slabs in, planes out
      auto ln_bytes = [&](int np) { return (double)M * D * (4.0 * (np ? 2 : 1) + 4.0 * np + 2.0 * P); };
      prof_launch("dit.residual_norm", ln_bytes(pend_n), st, [&] {
        // (fused to_qkv + attention reads 16-bit planes, in the fp8 mode too)
        launch_residual_norm(X, slabs, pend_n, slab_stride, pend_bias, L.g1, L.be1, qa_ipp ? Ap : lnout, M * D, PL,
                             (int)M, D, 1e-5f, 1, st, qa_ipp ? nullptr : SA8);
      });
      if (qa_ipp) {
        // to_qkv + rotary + attention in one launch (qkv_attn.hip): panels of qa_ipp whole items x one head
        QkvAttnDesc q;
        memset(&q, 0, sizeof q);
        q.A = Ap;
        q.W = L.qkv.w;
        q.bias = L.qkv.bias;
        q.rope_cos = rc;
        q.rope_sin = rs;
        q.out = fp8 ? nullptr : AOp;
        q.out8 = fp8 ? A8 : nullptr;       // fp8 mode: e4m3 + E8M0 scales for the fp8 out-projection
        q.out8_scale = fp8 ? SA8 : nullptr;
        q.M = (int)M;
        q.D = D;
        q.H = H;
        q.S = S;
        q.ipp = qa_ipp;
        q.q_scale = 0.125f;
        const double flops = 2.0 * (double)M * 3.0 * D * D + 4.0 * (double)B * H * (double)S * S * 64.0;
        const hipError_t e = profiled({"dit.qkv_attention", flops}, st, [&] { return qkv_attention_launch(q, PL, st, lens); });
        if (e != hipSuccess) fail(DSN_EHIP, "qkv_attention launch failed: %s", hipGetErrorString(e));
      } else {
        {  // q|k|v operand planes: rotary + 1/sqrt(dh) fused into the epilogue
          Tag tg(this, "dit.qkv");
          GemmDesc d = layer_desc(Ap, A8, SA8, L.qkv, L.qkv8);
          d.out_planes = QKVp;
          d.out_ps = M * 3 * D;
          d.rope_cos = rc;
          d.rope_sin = rs;
          d.rope_S = S;
          d.qkv_D = D;
          d.q_scale = 0.125f;
          d.m_fast = 1;
          d.panel_rows = plan.qkv_rows;
          layer_gemm(d, 256);
        }
        prof_launch("dit.attention", (double)M * D * 2.0 * P * 4.0, st, [&] {
          const hipError_t e = launch_attention_mfma(QKVp, M * 3 * D, lnout, M * D, PL, B, S, H, 64, st, SA8, lens);
          if (e != hipSuccess) fail(DSN_EHIP, "dit attention launch failed: %s", hipGetErrorString(e));
        });
      }
      {
        Tag tg(this, "dit.attn_out");
        GemmDesc d = layer_desc(qa_ipp ? AOp : Ap, A8, SA8, L.out, L.out8);
        if (fold_rows) {
          d.panel_rows = fold_rows;
          d.resid = X;
          d.out_f32 = X;
          d.out_planes = Xp;
          d.out_fp8 = X8;
          d.out_fp8_scale = SX8;
          d.out_ps = M * D;
          d.stat_out = ST;
          d.stat_np = D / 64;
          d.m_fast = 0;  // an XCD's share walks ACROSS the 8 column tiles of a few row panels: the whole
                         // 2 MB weight and 4 panels fit its L2 (m_fast = 1: every XCD re-fetches all of A)
          layer_gemm(d, 128);  // (never skinny: fold_rows excludes it)
          pend_n = 0;
          pend_bias = nullptr;
        } else {
          stream_gemm(d, 128, plan.attn_out_ksplit, plan.attn_out_rows);
        }
      }
      if (!fold_rows)
        prof_launch("dit.residual_norm", ln_bytes(pend_n), st, [&] {
          launch_residual_norm(X, slabs, pend_n, slab_stride, pend_bias, L.g2, L.be2, lnout, M * D, PL, (int)M, D,
                               1e-5f, 1, st, SA8);
        });
      {
        Tag tg(this, "dit.ff_in");
        GemmDesc d = fold_rows ? layer_desc(Xp, X8, SX8, L.ff1f, L.ff1f8) : layer_desc(Ap, A8, SA8, L.ff1, L.ff1_8);
        d.swiglu = 1;
        if (fold_rows) {
          d.ln_stats = ST;
          d.ln_np = D / 64;
          d.ln_colsum = fp8 ? L.ff1_colsum8 : L.ff1_colsum;
          d.ln_eps = 1e-5f;
        }
        if (fp8) {
          d.out_fp8 = H8;
          d.out_fp8_scale = SH8;
        } else {
          d.out_planes = FF;
        }
        d.out_ps = M * 4 * D;
        d.out_bstride = M * 4L * D;
        d.out_row_elems = 4 * D;
        d.out_limit = d.out_bstride;
        d.m_fast = 1;
        d.panel_rows = plan.ff_in_rows;
        layer_gemm(d, 256);
      }
      {
        Tag tg(this, "dit.ff_out");
        GemmDesc d = layer_desc(FF, H8, SH8, L.ff2, L.ff2_8);
        stream_gemm(d, 256, plan.ff_out_ksplit, plan.ff_out_rows);
      }
    }
    // final residual update + planes of X (no norm before project_out)
    prof_launch("dit.residual_norm", (double)M * D * (8.0 + 4.0 * pend_n + 2.0 * P), st, [&] {
      launch_residual_norm(X, slabs, pend_n, slab_stride, pend_bias, nullptr, nullptr, Ap, M * D, PL, (int)M, D, 1e-5f,
                           0, st);
    });
    {  // score = o + o Wpost^T with o = X[b, 1+t] Wout^T, one folded matrix
      Tag tg(this, "dit.project_out");
      GemmDesc d = base_desc(Ap, M * D, pout, B, T, S);
      d.in_pad = -1;
      d.in_bstride = (long)S * D;
      d.out_f32 = SC;
      d.panel_rows = plan.project_out_rows;  // (one 128-column tile)
      run(d, st, d.panel_rows ? 128 : 0);
    }
    return SC;
  }

#include "engine_ncsnpp.inc"

  float* score_tokens(const float* xt, const float* t, const float* mix, int B, int T, hipStream_t st,
                      const int* lens = nullptr) {
    if (!finalized) fail(DSN_ESTATE, "weights not finalized");
    if (cfg.score_kind == DSN_SCORE_DIT) return dit_forward(xt, t, mix, B, T, st, lens);
    if (lens) fail(DSN_EINVAL, "ragged batches need the DiT score network");
    if (cfg.score_kind == DSN_SCORE_NCSNPP) {
      Tag tg(this, "ncsnpp.conv");
      return ncsnpp_forward(xt, t, mix, B, T, st);
    }
    fail(DSN_ESTATE, "no score network configured (score_kind=%d)", cfg.score_kind);
  }

  // The window-blended score (include/ditsep_hip.h, dsn_score_windowed).  upload_window_tables: the plan's tables into
  // the fixed workspace buffers "win_tab_i" (wtab | ftab | token counts) and "win_tab_f" (fw) the kernels read -- outside
  // any capture, so they are data of a cached graph, not constants of it.
  struct WinTables {
    const ScoreWindowPlan* plan;
    const int *wtab, *ftab, *wlens;
    const float* fw;
    int batch;  // windows per DiT call (<= 0: all)
  };
  std::vector<int32_t> win_host_i;
  std::vector<float> win_host_f;
  const int* win_dev_i = nullptr;
  const float* win_dev_f = nullptr;
  WinTables upload_window_tables(const ScoreWindowPlan& p, int batch, hipStream_t st) {
    std::vector<int32_t> hi(p.wtab);
    hi.insert(hi.end(), p.ftab.begin(), p.ftab.end());
    hi.insert(hi.end(), p.wlens.begin(), p.wlens.end());
    int* di = wsbuf<int>("win_tab_i", hi.size());
    float* df = wsbuf<float>("win_tab_f", p.fw.size());
    if (hi != win_host_i || di != win_dev_i || p.fw != win_host_f || df != win_dev_f) {
      HIPCHK(hipMemcpyAsync(di, hi.data(), sizeof(int32_t) * hi.size(), hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(df, p.fw.data(), sizeof(float) * p.fw.size(), hipMemcpyHostToDevice, st));
      HIPCHK(hipStreamSynchronize(st));
      win_host_i = hi;
      win_host_f = p.fw;
      win_dev_i = di;
      win_dev_f = df;
    }
    return {&p, di, di + p.wtab.size(), di + p.wtab.size() + p.ftab.size(), df, batch};
  }
  // xt [R,n,Dl,T], tw [Wtot] (every window's time: its recording's), mix [R,1,Dl,T] -> blended score token-major
  // [R*T][n*Dl] in ws "win_blend".  The windows run as dense DiT calls of at most `batch` items whose score tokens land
  // in one [Wtot][Twin][n*Dl] buffer; one gather launch then blends them.
  float* score_windowed(const float* xt, const float* tw, const float* mix, const WinTables& w, hipStream_t st) {
    if (!finalized) fail(DSN_ESTATE, "weights not finalized");
    if (cfg.score_kind != DSN_SCORE_DIT) fail(DSN_EINVAL, "window-blended scores need the DiT score network");
    const ScoreWindowPlan& p = *w.plan;
    const int io = cfg.n_src * cfg.latent_dim;
    float* WS = wsbuf<float>("win_sc", (long)p.Wtot * p.Twin * io);
    float* out = wsbuf<float>("win_blend", (long)p.R * p.T * io);
    const int nb = w.batch > 0 ? std::min(w.batch, p.Wtot) : p.Wtot;
    for (int lo = 0; lo < p.Wtot; lo += nb) {
      const WinMap wm{w.wtab + 3L * lo, p.T, WS + (long)lo * p.Twin * io};
      dit_forward(xt, tw + lo, mix, std::min(nb, p.Wtot - lo), p.Twin, st, p.shorts ? w.wlens + lo : nullptr, &wm);
    }
    // algorithmic bytes: every output row written once, one or two window rows read for it
    prof_launch("score.win_blend", (double)p.R * p.T * io * 4.0 * 2.0, st, [&] {
      launch_win_blend_tokens(WS, w.ftab, w.fw, out, (long)p.R * p.T, io, p.Twin, st);
    });
    return out;
  }

  // ---------------------------------------------------------------- OUVE scalars
  struct Sched {
    std::vector<float> t, std, step, gain, G, g;
    float stdT;
  };
  float ouve_std(float t) const {
    const double th = cfg.sde_theta, smin = cfg.sde_sigma_min, ls = log((double)cfg.sde_sigma_max / smin);
    const float a = expf((float)(-2.0 * th) * t);
    const float b = expf((float)(2.0 * (th + ls)) * t) - 1.f;
    const float num = (float)(smin * smin) * a * b * (float)ls;
    return sqrtf(num / (float)(th + ls));
  }
  // torch.linspace(start, end, steps) in fp32: step = (end-start)/(steps-1); symmetric fill
  static std::vector<float> linspace32(float start, float end, int steps) {
    std::vector<float> v((size_t)steps);
    const float stp = steps > 1 ? (end - start) / (float)(steps - 1) : 0.f;
    const int halfway = steps / 2;
    for (int i = 0; i < steps; ++i) v[i] = i < halfway ? start + stp * (float)i : end - stp * (float)(steps - 1 - i);
    return v;
  }
  std::vector<float> t_override;  // scheduled sampler: explicit timesteps (first N used), empty = linspace
  Sched schedule(int N, float t_eps, float snr) const {
    Sched s;
    const double smin = cfg.sde_sigma_min, smax = cfg.sde_sigma_max, ls = log(smax / smin);
    s.t = linspace32(1.f, t_eps, N);
    s.std.resize(N);
    s.step.resize(N);
    s.gain.resize(N);
    s.G.resize(N);
    s.g.resize(N);
    if ((int)t_override.size() >= N)
      for (int i = 0; i < N; ++i) s.t[i] = t_override[i];
    const float sqdt = sqrtf((float)(1.0 / N));
    for (int i = 0; i < N; ++i) {
      const float t = s.t[i];
      s.std[i] = ouve_std(t);
      const float q = snr * s.std[i];
      s.step[i] = q * q * 2.f;
      s.gain[i] = sqrtf(s.step[i] * 2.f);
      const float sigma = (float)smin * powf((float)(smax / smin), t);
      s.g[i] = sigma * (float)sqrt(2.0 * ls);
      s.G[i] = s.g[i] * sqdt;
    }
    s.stdT = ouve_std(1.f);
    return s;
  }

  // ---------------------------------------------------------------- sampler
  // y [B,1,Dl,T]; noise [(1+N(c+1))][B,n,Dl,T]; returns device pointer of the result
  // vec_t = ones(B) * t_per_step[i] for every step ("pc_t", [N][B]), uploaded once per (B, table)
  void upload_step_times(const std::vector<float>& t_per_step, int B, hipStream_t st) {
    const int N = (int)t_per_step.size();
    std::vector<float> ht((size_t)B * N);
    for (int i = 0; i < N; ++i)
      for (int b = 0; b < B; ++b) ht[(size_t)i * B + b] = t_per_step[i];
    float* tv = wsbuf<float>("pc_t", (long)B * N);
    if (ht == tv_host && tv_B == B) return;
    HIPCHK(hipMemcpyAsync(tv, ht.data(), sizeof(float) * ht.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    tv_host = ht;
    tv_B = B;
  }
  // Ragged batches.  check_frames: the refusals, before anything is allocated or launched.  upload_lens: the token
  // counts 1 + frames[b] into the fixed workspace buffer "ragged_lens" the length-aware attention kernels read --
  // outside any capture, so the lengths are data of a cached graph, not constants of it.
  // needs: what the call runs -- the DiT (the ragged score call and samplers), the encoder, the decoder
  enum { RAGGED_DIT = 1, RAGGED_ENC = 2, RAGGED_DEC = 4 };
  void check_frames(const char* who, const int32_t* frames, int B, int T, int needs = RAGGED_DIT) const {
    if (!frames) fail(DSN_EINVAL, "%s: frames is null", who);
    if ((needs & RAGGED_DIT) && cfg.score_kind != DSN_SCORE_DIT)
      fail(DSN_EINVAL, "%s: ragged batches need the DiT score network (NCSN++ convolves across time: padding would "
           "change an item's result)", who);
    if ((needs & RAGGED_ENC) && !cfg.vae_has_encoder) fail(DSN_ESTATE, "%s: encoder not configured", who);
    if ((needs & RAGGED_DEC) && !cfg.vae_has_decoder) fail(DSN_ESTATE, "%s: decoder not configured", who);
    if ((needs & (RAGGED_ENC | RAGGED_DEC)) && !finalized) fail(DSN_ESTATE, "%s: weights not finalized", who);
    // the tail launch of the ragged codec stores 16 bytes per lane: the waveform is cleared as rows of 8 samples
    if ((needs & RAGGED_DEC) && hop() % 8 != 0)
      fail(DSN_EINVAL, "%s: the ragged decoder needs a hop length that is a multiple of 8 (hop = %d)", who, hop());
    if ((needs & (RAGGED_ENC | RAGGED_DEC)) && cfg.latent_dim % 8 != 0)
      fail(DSN_EINVAL, "%s: the ragged codec needs a latent width that is a multiple of 8 (latent_dim = %d)", who,
           cfg.latent_dim);
    for (int b = 0; b < B; ++b)
      if (frames[b] < 1 || frames[b] > T)
        fail(DSN_EINVAL, "%s: frame count frames[%d] = %d outside [1, T = %d]", who, b, (int)frames[b], T);
  }
  const int* upload_lens(const int32_t* frames, int B, hipStream_t st) {
    std::vector<int> h((size_t)B);
    for (int b = 0; b < B; ++b) h[b] = 1 + frames[b];
    int* d = wsbuf<int>("ragged_lens", B);
    if (h == lens_host && d == lens_dev) return d;
    HIPCHK(hipMemcpyAsync(d, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    lens_host = h;
    lens_dev = d;
    return d;
  }
  // the frame counts themselves into "codec_frames" (the codec's tail launches read them), outside any capture as well
  const int* upload_frames(const int32_t* frames, int B, hipStream_t st) {
    std::vector<int> h(frames, frames + B);
    int* d = wsbuf<int>("codec_frames", B);
    if (h == frames_host && d == frames_dev) return d;
    HIPCHK(hipMemcpyAsync(d, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    frames_host = h;
    frames_dev = d;
    return d;
  }
  // Every step's time embedding in one batch, off the per-call path (-1.3 % sampler time).  time_cache is only
  // valid while the sampler pass that holds this object (or its graph capture) runs.
  struct TimeEmbedPass {
    TimeCache& cache;
    TimeEmbedPass(dsn_ctx* c, const float* tv, int N, int B, hipStream_t st) : cache(c->time_cache) {
      const bool dit = c->cfg.score_kind == DSN_SCORE_DIT;
      const int width = dit ? c->cfg.dit_embed_dim : c->ncs_dense_total;
      float* all = c->wsbuf<float>("te_all", (long)N * B * width);
      Tag tg(c, "score.time_embed");
      if (dit) c->dit_time_embed(tv, N * B, all, st);
      else c->ncs_time_dense(tv, N * B, all, st);
      cache.t0 = tv;
      cache.rows = (long)N * B;
      cache.data = all;
      cache.width = width;
    }
    TimeEmbedPass(const TimeEmbedPass&) = delete;
    ~TimeEmbedPass() { cache = TimeCache(); }
  };
  struct PcOpts {
    int pred = DSN_PRED_REVERSE_DIFFUSION, corr = DSN_CORR_ALD, c = 1, denoise = 1;
    float snr = 0.5f, t_eps = 0.03f;
    const float* prior_mean = nullptr;
    float* inter = nullptr;
    long draws(int N) const { return 1 + (long)N * (c + (pred == DSN_PRED_NONE ? 0 : 1)); }
  };
  // lens (device, null = dense): ragged batch -- every score call takes it, and the result's frames past an item's
  // length are written as zero (the update kernels are elementwise: padding costs them the padded positions only)
  // win (null = none): the window-blended score of the long state (score_windowed); the step times are then one per
  // window ("pc_t" [N][Wtot], as is the time-embedding pass), and lens only marks the tail to clear
  float* pc_sample(const float* y, const float* noise, int B, int T, int N, const PcOpts& o, hipStream_t st,
                   const int* lens = nullptr, const WinTables* win = nullptr) {
    const int n = cfg.n_src, Dl = cfg.latent_dim;
    const long sz = (long)B * n * Dl * T;
    const int tB = win ? win->plan->Wtot : B;  // step times per step
    float* x = wsbuf<float>("pc_x", sz);
    float* xm = wsbuf<float>("pc_xm", sz);
    float* tv = wsbuf<float>("pc_t", (long)tB * N);
    float* norms = o.corr == DSN_CORR_LANGEVIN ? wsbuf<float>("pc_norms", 2L * B) : nullptr;
    const Sched s = schedule(N, o.t_eps, o.snr);
    const float dt = (float)(1.0 / N);
    const float* z = noise;
    TimeEmbedPass te(this, tv, N, tB, st);
    auto score = [&](const float* ti) {
      return win ? score_windowed(x, ti, y, *win, st) : score_tokens(x, ti, y, B, T, st, lens);
    };
    launch_pc_prior(o.prior_mean ? o.prior_mean : y, o.prior_mean != nullptr, z, x, s.stdT, B, n, Dl, T, st);
    z += sz;
    const bool keep_mean = o.inter != nullptr;  // only `intermediate` reads the corrector's x_mean
    for (int i = 0; i < N; ++i) {
      const float* ti = tv + (long)i * tB;
      for (int k = 0; k < o.c; ++k) {
        float* sc = score(ti);
        if (norms) {
          launch_pc_item_norms(sc, (long)n * Dl * T, B, norms, st);
          launch_pc_item_norms(z, (long)n * Dl * T, B, norms + B, st);
        }
        launch_pc_corrector(x, keep_mean ? xm : nullptr, sc, z, s.step[i], s.gain[i], norms, o.snr, B, n, Dl, T, st);
        z += sz;
      }
      if (o.inter) {  // (xt, xt_mean) as the corrector returned them; c == 0 / a fresh loop: x_mean = x
        if (o.c == 0) HIPCHK(hipMemcpyAsync(xm, x, sizeof(float) * sz, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(o.inter + (2L * i) * sz, x, sizeof(float) * sz, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(o.inter + (2L * i + 1) * sz, xm, sizeof(float) * sz, hipMemcpyDeviceToDevice, st));
      }
      if (o.pred == DSN_PRED_NONE) {  // x, x_mean = x, x
        if (o.denoise && i == N - 1) HIPCHK(hipMemcpyAsync(xm, x, sizeof(float) * sz, hipMemcpyDeviceToDevice, st));
        continue;
      }
      float* sc = score(ti);
      launch_pc_predictor(x, xm, y, sc, z, cfg.sde_theta, dt, s.G[i], s.g[i], o.pred == DSN_PRED_EULER_MARUYAMA, B, n,
                          Dl, T, st);
      z += sz;
    }
    if (lens) launch_zero_tail(o.denoise ? xm : x, lens, B, n, Dl, T, st);
    return o.denoise ? xm : x;
  }

  // ---------------------------------------------------------------- secondary sampler family
  // MixSDE / PriorMixSDE predictor-corrector loop with the ald2 corrector (reference sdes.py:182-593,
  // correctors.py:87-121, __init__.py:133-193) on the latent state read as [B, n, D*T]; scalar schedules in fp32 as
  // torch evaluates them on a [B]-vector of equal times.
  struct MixOpts {
    int prior_mix = 0, avg_len = 510, pred = DSN_PRED_REVERSE_DIFFUSION, corr = DSN_MIXCORR_ALD2, c = 1, denoise = 1;
    float d_lambda = 2.f, sigma_min = 0.05f, sigma_max = 0.5f, snr = 0.5f, t_eps = 0.03f;
    long draws(int N) const { return 1 + (long)N * (c + (pred == DSN_PRED_NONE ? 0 : 1)); }
  };
  static void mix_eigval(const MixOpts& o, float t, float& ev1, float& ev2) {
    const double ratio = (double)o.sigma_max / o.sigma_min, logsig = log(ratio);
    const float mult = (float)((double)o.sigma_min * o.sigma_min);
    const float srp = powf((float)ratio, 2.f * t);
    ev1 = mult * (srp - 1.f);
    ev2 = mult * (srp - expf((float)(-2.0 * o.d_lambda) * t)) / (float)(1.0 + o.d_lambda / logsig);
  }
  float* pc_sample_mix(const float* y, const float* noise, int B, int T, int N, const MixOpts& o, hipStream_t st) {
    const int n = cfg.n_src, Dl = cfg.latent_dim;
    const long sz = (long)B * n * Dl * T;
    float* x = wsbuf<float>("pc_x", sz);
    float* xm = wsbuf<float>("pc_xm", sz);
    float* tv = wsbuf<float>("pc_t", (long)B * N);
    float* smix = o.prior_mix ? wsbuf<float>("pc_smix", (long)B * Dl * T) : nullptr;
    const Sched s = schedule(N, o.t_eps, o.snr);  // timesteps = linspace(1, eps, N)
    const float dt = (float)(1.0 / N), sqdt = sqrtf(dt);
    const double ratio = (double)o.sigma_max / o.sigma_min, logsig = log(ratio);
    TimeEmbedPass te(this, tv, N, B, st);
    if (smix) launch_sigma_mix(y, smix, B, Dl * T, o.avg_len, st);
    const float* z = noise;
    float ev1, ev2;
    mix_eigval(o, 1.f, ev1, ev2);
    launch_mix_prior(y, z, x, smix, sqrtf(ev1), sqrtf(ev2), B, n, Dl, T, st);
    z += sz;
    HIPCHK(hipMemcpyAsync(xm, x, sizeof(float) * sz, hipMemcpyDeviceToDevice, st));
    for (int i = 0; i < N; ++i) {
      const float* ti = tv + (long)i * B;
      const float t = s.t[i];
      if (o.corr == DSN_MIXCORR_ALD2 && o.c > 0) {
        mix_eigval(o, t, ev1, ev2);
        for (int k = 0; k < o.c; ++k) {
          float* sc = score_tokens(x, ti, y, B, T, st);
          launch_mix_corrector(x, xm, sc, z, smix, sqrtf(ev1), sqrtf(ev2), o.snr, B, n, Dl, T, st);
          z += sz;
        }
      }
      if (o.pred == DSN_PRED_NONE) {
        HIPCHK(hipMemcpyAsync(xm, x, sizeof(float) * sz, hipMemcpyDeviceToDevice, st));
        continue;
      }
      const float g = (float)o.sigma_min * powf((float)ratio, t) * (float)sqrt(2.0 * logsig);
      float* sc = score_tokens(x, ti, y, B, T, st);
      launch_mix_predictor(x, xm, sc, z, smix, o.d_lambda, dt, g, sqdt, o.pred == DSN_PRED_EULER_MARUYAMA, B, n, Dl, T, st);
      z += sz;
    }
    return o.denoise ? xm : x;
  }

  // get_sb_sampler (reference src/sdes/__init__.py:284-389) with SBVESDE (sdes.py:701-779): xt = y repeated over
  // the sources, N first-order bridge steps over linspace(1, eps, N + 1); the score network's output is the data
  // estimate.  sde type consumes one noise tensor per step (the last step's weight is zero, the draw still happens).
  float* sb_sample(const float* y, const float* noise, int B, int T, int N, float k, float c, float sbeps, float t_eps,
                   int ode, hipStream_t st) {
    const int n = cfg.n_src, Dl = cfg.latent_dim;
    const long sz = (long)B * n * Dl * T;
    float* x = wsbuf<float>("pc_x", sz);
    float* tv = wsbuf<float>("pc_t", (long)B * N);
    TimeEmbedPass te(this, tv, N, B, st);
    auto sig = [&](float t) { return sqrtf((c * (powf(k, 2.f * t) - 1.f)) / (2.f * logf(k))); };
    const std::vector<float> ts = sb_times(N, t_eps);
    const float sig_T = sig(1.f);
    float sig_p = sig(ts[0]), sigb_p = sqrtf(sig_T * sig_T - sig_p * sig_p + sbeps);
    launch_repeat_sources(y, x, B, n, Dl, T, st);
    const float* z = noise;
    for (int i = 0; i < N; ++i) {
      const float t = ts[i + 1];
      const float sig_t = sig(t), sigb_t = sqrtf(sig_T * sig_T - sig_t * sig_t + sbeps);
      float* est = score_tokens(x, tv + (long)i * B, y, B, T, st);
      if (!ode) {
        const float w_prev = sig_t * sig_t / (sig_p * sig_p + sbeps);
        const float tmp = 1.f - sig_t * sig_t / (sig_p * sig_p + sbeps);
        const float w_z = (i == N - 1) ? 0.f : sig_t * sqrtf(tmp);
        launch_sb_update(x, est, z, w_prev, tmp, w_z, 0, B, n, Dl, T, st);
        z += sz;
      } else {
        const float w_prev = sig_t * sigb_t / (sig_p * sigb_p + sbeps);
        const float w_est = 1.f / (sig_T * sig_T + sbeps) * (sigb_t * sigb_t - sigb_p * sig_t * sigb_t / (sig_p + sbeps));
        const float w_pm = 1.f / (sig_T * sig_T + sbeps) * (sig_t * sig_t - sig_p * sig_t * sigb_t / (sigb_p + sbeps));
        launch_sb_update(x, est, y, w_prev, w_est, w_pm, 1, B, n, Dl, T, st);
      }
      sig_p = sig_t;
      sigb_p = sigb_t;
    }
    return x;
  }
  // torch.linspace(1, eps, N + 1), entries 0..N
  static std::vector<float> sb_times(int N, float t_eps) { return linspace32(1.f, t_eps, N + 1); }

  // injected standard normals, else draws 0.. of the device RNG stream for `seed`
  static void stage_noise(float* dst, const float* src, long count, uint64_t seed, hipStream_t st) {
    if (src) HIPCHK(hipMemcpyAsync(dst, src, sizeof(float) * count, hipMemcpyDeviceToDevice, st));
    else launch_randn(dst, count, seed, 0, st);
  }
  // One call of dsn_pc_sample_ex / dsn_pc_sample_mix / dsn_sb_sample: stable workspace copies of the caller's
  // tensors (graph replay needs fixed pointers), the step-time table, then `body(y, noise, prior_mean, stream)`
  // eagerly or as the graph cached under `key`.  `result` names the buffer body returns (a replayed graph wrote
  // the same one).
  struct SamplerCall {
    const float *y, *noise, *prior_mean;
    uint64_t seed;
    float* x_out;
    int B, T;
    long draws;
    hipStream_t caller;
    int time_rows = 0;  // step times per step when not B (the windowed sampler: one per window)
  };
  template <class F>
  void run_sampler(const SamplerCall& a, const std::vector<float>& t_per_step, const char* key, const char* result,
                   F&& body) {
    if (!finalized) fail(DSN_ESTATE, "weights not finalized");
    const long ysz = (long)a.B * cfg.latent_dim * a.T, sz = ysz * cfg.n_src;
    float* yb = wsbuf<float>("pc_y", ysz);
    float* nz = a.draws ? wsbuf<float>("pc_noise", sz * a.draws) : nullptr;
    float* pm = a.prior_mean ? wsbuf<float>("pc_prior_mean", sz) : nullptr;
    upload_step_times(t_per_step, a.time_rows ? a.time_rows : a.B, a.caller);
    StreamScope sc(this, a.caller);
    HIPCHK(hipMemcpyAsync(yb, a.y, sizeof(float) * ysz, hipMemcpyDeviceToDevice, sc.st));
    if (pm) HIPCHK(hipMemcpyAsync(pm, a.prior_mean, sizeof(float) * sz, hipMemcpyDeviceToDevice, sc.st));
    if (a.draws) stage_noise(nz, a.noise, sz * a.draws, a.seed, sc.st);
    float* res = nullptr;
    run_graphed(key, sc.st, [&](hipStream_t s2) { res = body(yb, nz, pm, s2); });
    if (!res) res = wsbuf<float>(result, sz);
    HIPCHK(hipMemcpyAsync(a.x_out, res, sizeof(float) * sz, hipMemcpyDeviceToDevice, sc.st));
    sc.leave();
    HIPCHK(hipGetLastError());
  }

  // ---------------------------------------------------------------- decoder
  int hop() const {
    int h = 1;
    for (int i = 0; i < cfg.vae_n_blocks; ++i) h *= cfg.vae_strides[i];
    return h;
  }
  // est [S][Dl][T] (S = B*n) -> wav fp32 [S][hop*T] in ws "dec_wav"
  // cl (null = dense): ragged batch, item s holds cl->frames[s / cl->rep] frames -- one tail_zero after every layer
  float* decode(const float* est, int S, int T, hipStream_t st, const CodecLens* cl = nullptr) {
    if (!cfg.vae_has_decoder) fail(DSN_ESTATE, "decoder not configured");
    const int Dl = cfg.latent_dim;
    long maxel = (long)S * T * dec_in.N;
    {
      long L = T;
      for (auto& b : dec_blocks) {
        L *= b.stride;
        maxel = std::max(maxel, (long)S * L * b.cout);
      }
    }
    op16_t* zp = wsbuf<op16_t>("dec_z", (long)S * T * Dl * P);
    op16_t* pa = wsbuf<op16_t>("dec_pa", maxel * P);
    op16_t* pb = wsbuf<op16_t>("dec_pb", maxel * P);
    op16_t* ph = wsbuf<op16_t>("dec_ph", maxel * P);
    float* xf = wsbuf<float>("dec_x", maxel);
    launch_pack_tokens(est, Dl, nullptr, 0, S, T, nullptr, zp, (long)S * T * Dl, PL, st);
    if (cl) tail_zero(*cl, zp, (long)S * T * Dl, nullptr, nullptr, S, T, Dl, 1, st);  // (est's padding holds anything)
    long L = T;
    long mul = 1;  // rows per latent frame at the current level
    {
      Tag tg(this, "vae.dec_conv_in");
      GemmDesc d = base_desc(zp, (long)S * T * Dl, dec_in, S, T, T);
      d.in_pad = (dec_in.taps - 1) / 2;
      d.out_planes = pa;
      d.out_ps = (long)S * T * dec_in.N;
      set_act(d, dec_blocks[0].act);
      run(d, st);
    }
    if (cl) tail_zero(*cl, pa, (long)S * T * dec_in.N, nullptr, nullptr, S, T, dec_in.N, 1, st);
    long a_ps = (long)S * T * dec_in.N;
    for (size_t bi = 0; bi < dec_blocks.size(); ++bi) {
      const VaeBlock& b = dec_blocks[bi];
      const long Lo = L * b.stride;
      const long o_ps = (long)S * Lo * b.cout;
      {  // ConvTranspose1d as a 2-tap phase GEMM
        Tag tg(this, "vae.dec_convT");
        GemmDesc d = base_desc(pa, a_ps, b.conv, S, (int)L + 1, (int)L);
        d.tap_dil = -1;
        d.out_bstride = Lo * b.cout;
        d.out_row_elems = b.stride * b.cout;
        d.out_off = -((b.stride + 1) / 2) * b.cout;
        d.out_limit = Lo * b.cout;
        d.out_f32 = xf;
        d.out_planes = pb;
        d.out_ps = o_ps;
        set_act(d, b.ru[0].act0);
        // Shallow-K phase GEMMs (the last up-sampling layers: K = 2 x 128 or 2 x 256): while the 256 x 256 kernel
        // spilled ~200 registers a 3-stage 256 x 128 tile was faster there (8.3 vs 9.2 ms over the 5 layers); with
        // the lean epilogue the default 256 x 256 x BK 64 tile wins again (6.2 vs 7.3 ms)
        run(d, st);
      }
      mul *= b.stride;
      if (cl) tail_zero(*cl, pb, o_ps, xf, nullptr, S, Lo, b.cout, mul, st);
      for (int j = 0; j < 3; ++j) {
        const ResUnit& r = b.ru[j];
        const ActP& next = j < 2 ? b.ru[j + 1].act0 : (bi + 1 < dec_blocks.size() ? dec_blocks[bi + 1].act : dec_final_act);
        res_unit(r, pb, ph, o_ps, xf, j < 2, next, S, Lo, st, cl, mul);
      }
      std::swap(pa, pb);
      a_ps = o_ps;
      L = Lo;
    }
    float* wav = wsbuf<float>("dec_wav", (long)S * L);
    prof_launch("vae.dec_conv_out", (double)S * L * (dec_blocks.back().cout * 2.0 * P + 4.0), st, [&] {
      launch_conv_out1(pa, a_ps, PL, dec_out_w, wav, S, (int)L, dec_blocks.back().cout, dec_out_taps,
                       cfg.vae_final_tanh, st);
    });
    if (cl) tail_zero(*cl, nullptr, 0, nullptr, wav, S, L / 8, 8, mul / 8, st);  // (rows of 8 samples: hop % 8 == 0)
    return wav;
  }

  // ---------------------------------------------------------------- encoder
  // wav [S][L] (L multiple of hop) + noise [S][Dl][T] -> y [S][Dl][T]
  // cl (null = dense): ragged batch -- item s holds cl->frames[s] frames and its samples past them are zero;
  // y[s, :, frames[s]:] is written as zero
  void encode(const float* wav, const float* noise, float* y, int S, int L, hipStream_t st, const CodecLens* cl = nullptr) {
    float* enc = encode_body(wav, S, L, st, cl);
    if (cl) launch_vae_sample_ragged(enc, noise, cl->frames, y, S, cfg.latent_dim, L / hop(), st);
    else launch_vae_sample(enc, noise, y, S, cfg.latent_dim, L / hop(), st);
  }
  // wav [S][L] -> encoder output (mean ++ scale) channels-last [S][L/hop][2*Dl] in ws "enc_out"
  // cl: as in encode -- one tail_zero after every layer
  float* encode_body(const float* wav, int S, int L, hipStream_t st, const CodecLens* cl = nullptr) {
    if (!cfg.vae_has_encoder) fail(DSN_ESTATE, "encoder not configured");
    const int Dl = cfg.latent_dim, c0 = cfg.vae_channels;
    long maxel = (long)S * L * c0;
    {
      long l = L;
      for (auto& b : enc_blocks) {
        l /= b.stride;
        maxel = std::max(maxel, (long)S * l * b.cout);
      }
    }
    op16_t* pa = wsbuf<op16_t>("enc_pa", maxel * P);
    op16_t* ph = wsbuf<op16_t>("enc_ph", maxel * P);
    op16_t* pb = wsbuf<op16_t>("enc_pb", maxel * P);
    float* xf = wsbuf<float>("enc_x", maxel);
    long l = L;
    long a_ps = (long)S * l * c0;
    {
      const ActP& a = enc_blocks[0].ru[0].act0;
      launch_conv_in1(wav, enc_in_w, enc_in_b, S, L, c0, 7, xf, pa, a_ps, PL, a.kind, a.a, a.ib, st);
    }
    long mul = hop();  // rows per latent frame at the current level
    if (cl) tail_zero(*cl, pa, a_ps, xf, nullptr, S, l, c0, mul, st);
    for (size_t bi = 0; bi < enc_blocks.size(); ++bi) {
      const VaeBlock& b = enc_blocks[bi];
      for (int j = 0; j < 3; ++j) {
        const ResUnit& r = b.ru[j];
        const ActP& next = j < 2 ? b.ru[j + 1].act0 : b.act;
        res_unit(r, pa, ph, a_ps, xf, j < 2, next, S, l, st, cl, mul);
      }
      const long lo = l / b.stride;
      const long o_ps = (long)S * lo * b.cout;
      {  // strided conv k = 2s
        Tag tg(this, "vae.enc_strided_conv");
        GemmDesc d = base_desc(pa, a_ps, b.conv, S, (int)lo, (int)l);
        d.in_stride = b.stride;
        d.in_pad = (b.stride + 1) / 2;
        d.out_planes = pb;
        d.out_ps = o_ps;
        if (bi + 1 < enc_blocks.size()) {
          d.out_f32 = xf;
          set_act(d, enc_blocks[bi + 1].ru[0].act0);
        } else {
          set_act(d, enc_final_act);
        }
        run(d, st);
      }
      mul /= b.stride;
      if (cl) tail_zero(*cl, pb, o_ps, bi + 1 < enc_blocks.size() ? xf : nullptr, nullptr, S, lo, b.cout, mul, st);
      std::swap(pa, pb);
      a_ps = o_ps;
      l = lo;
    }
    float* enc = wsbuf<float>("enc_out", (long)S * l * enc_out.N);
    {
      Tag tg(this, "vae.enc_conv_out");
      GemmDesc d = base_desc(pa, a_ps, enc_out, S, (int)l, (int)l);
      d.in_pad = (enc_out.taps - 1) / 2;
      d.out_f32 = enc;
      run(d, st);
    }
    if (cl) tail_zero(*cl, nullptr, 0, nullptr, enc, S, l, enc_out.N, mul, st);
    if (enc_out.N != 2 * Dl) fail(DSN_EINVAL, "encoder latent %d != 2*latent_dim %d", enc_out.N, 2 * Dl);
    return enc;
  }

  // chunk / paste schedule of AudioAutoencoder.decode_audio / encode_audio (autoencoders.py:596-731), latent frames
  struct ChunkPaste {
    int src, t0, t1, c0, c1;
  };
  std::vector<ChunkPaste> chunk_plan(int total, int chunk, int overlap) {
    if (overlap < 0 || chunk <= overlap || total < chunk)
      fail(DSN_EINVAL, "chunked coding needs 0 <= overlap < chunk_size <= frames (got %d, %d, %d)", overlap, chunk, total);
    const int hopf = chunk - overlap, ol = overlap / 2;
    std::vector<int> starts;
    for (int a = 0; a + chunk <= total; a += hopf) starts.push_back(a);
    if (starts.back() + chunk != total) starts.push_back(total - chunk);
    std::vector<ChunkPaste> plan;
    for (size_t i = 0; i < starts.size(); ++i) {
      const bool last = i + 1 == starts.size();
      ChunkPaste c;
      c.src = starts[i];
      c.t1 = last ? total : (int)i * hopf + chunk;
      c.t0 = last ? total - chunk : (int)i * hopf;
      c.c0 = 0;
      c.c1 = chunk;
      if (i > 0) {
        c.t0 += ol;
        c.c0 += ol;
      }
      if (!last) {
        c.t1 -= ol;
        c.c1 -= ol;
      }
      plan.push_back(c);
    }
    return plan;
  }
  // est [S][Dl][T] -> wav [S][hop*T] in ws "dec_long": every chunk is an independent decode of `chunk` frames
  float* decode_chunked(const float* est, int S, int T, int chunk, int overlap, hipStream_t st) {
    const int Dl = cfg.latent_dim, h = hop();
    const auto plan = chunk_plan(T, chunk, overlap);
    float* zc = wsbuf<float>("dec_chunk_in", (long)S * Dl * chunk);
    float* out = wsbuf<float>("dec_long", (long)S * h * T);
    const long Lc = (long)h * chunk, Lt = (long)h * T;
    for (const auto& c : plan) {
      HIPCHK(hipMemcpy2DAsync(zc, sizeof(float) * chunk, est + c.src, sizeof(float) * T, sizeof(float) * chunk,
                              (size_t)S * Dl, hipMemcpyDeviceToDevice, st));
      char key[64];
      snprintf(key, sizeof key, "dec:%d:%d", S, chunk);
      float* w = nullptr;
      run_graphed(key, st, [&](hipStream_t s2) { w = decode(zc, S, chunk, s2); });
      if (!w) w = wsbuf<float>("dec_wav", (long)S * Lc);
      HIPCHK(hipMemcpy2DAsync(out + (long)c.t0 * h, sizeof(float) * Lt, w + (long)c.c0 * h, sizeof(float) * Lc,
                              sizeof(float) * (size_t)(c.t1 - c.t0) * h, S, hipMemcpyDeviceToDevice, st));
    }
    return out;
  }
  // wav [S][hop*T] -> stitched encoder output [S][T][2*Dl] in ws "enc_long"
  float* encode_chunked(const float* wav, int S, int T, int chunk, int overlap, hipStream_t st) {
    const int h = hop(), E = 2 * cfg.latent_dim;
    const auto plan = chunk_plan(T, chunk, overlap);
    float* wc = wsbuf<float>("enc_chunk_in", (long)S * h * chunk);
    float* out = wsbuf<float>("enc_long", (long)S * T * E);
    const long Lc = (long)h * chunk, Lt = (long)h * T;
    for (const auto& c : plan) {
      HIPCHK(hipMemcpy2DAsync(wc, sizeof(float) * Lc, wav + (long)c.src * h, sizeof(float) * Lt, sizeof(float) * Lc, S,
                              hipMemcpyDeviceToDevice, st));
      float* e = encode_body(wc, S, (int)Lc, st);
      HIPCHK(hipMemcpy2DAsync(out + (long)c.t0 * E, sizeof(float) * (size_t)T * E, e + (long)c.c0 * E,
                              sizeof(float) * (size_t)chunk * E, sizeof(float) * (size_t)(c.t1 - c.t0) * E, S,
                              hipMemcpyDeviceToDevice, st));
    }
    return out;
  }
};

// =========================================================================== C-ABI
namespace {
thread_local std::string g_create_err;

template <class F>
int guarded(dsn_ctx* ctx, F&& f) {
  if (!ctx) return DSN_EINVAL;
  try {
    HIPCHK(hipSetDevice(ctx->cfg.device));
    ctx->sw = Switches::read();
    if (ctx->fin_err_host && *ctx->fin_err_host) {
      *ctx->fin_err_host = 0;
      fail(DSN_EHIP, "a GroupNorm hand-off wait of an earlier call gave up (the workgroups of one conv were not resident "
                     "together): that call's results are invalid; DSN_NO_GN_FIN=1 selects the separate GroupNorm pass");
    }
    f();
    return DSN_OK;
  } catch (const Err& e) {
    ctx->err = e.what();
    return e.code;
  } catch (const std::exception& e) {
    ctx->err = e.what();
    return DSN_EINVAL;
  }
}

// The permutation p of 0 .. n-1 with the largest score(p), in lexicographic order; the first one wins a tie.
template <class Score>
std::vector<int> best_permutation(int n, Score score) {
  std::vector<int> p(n);
  std::iota(p.begin(), p.end(), 0);
  std::vector<int> bestp = p;
  double best = -1e300;
  do {
    const double s = score(p);
    if (s > best) {
      best = s;
      bestp = p;
    }
  } while (std::next_permutation(p.begin(), p.end()));
  return bestp;
}
}  // namespace

extern "C" {

dsn_ctx* dsn_create(const dsn_config* cfg) {
  try {
    if (!cfg) fail(DSN_EINVAL, "null config");
    if (cfg->precision < DSN_PREC_BF16 || cfg->precision > DSN_PREC_FP8)
      fail(DSN_EINVAL, "precision must be one of DSN_PREC_{BF16,BF16X3,FP16,FP16X3,FP8}");
    if (cfg->vae_n_blocks < 0 || cfg->vae_n_blocks > DSN_MAX_VAE_BLOCKS) fail(DSN_EINVAL, "bad vae_n_blocks");
    if (cfg->n_src < 1 || cfg->latent_dim % 32 != 0) fail(DSN_EINVAL, "bad n_src / latent_dim");
    if (cfg->score_kind == DSN_SCORE_DIT &&
        (cfg->dit_heads <= 0 || cfg->dit_embed_dim <= 0 || cfg->dit_embed_dim % cfg->dit_heads != 0 ||
         cfg->dit_embed_dim / cfg->dit_heads != 64))
      fail(DSN_EINVAL, "DiT: only 64-wide attention heads are implemented (embed_dim %d / %d heads = %d)",
           cfg->dit_embed_dim, cfg->dit_heads, cfg->dit_heads > 0 ? cfg->dit_embed_dim / cfg->dit_heads : 0);
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev) fail(DSN_EINVAL, "device %d out of range (%d GPUs)", cfg->device, ndev);
    HIPCHK(hipSetDevice(cfg->device));
    dsn_ctx* c = new dsn_ctx();
    c->cfg = *cfg;
    c->P = prec_planes(cfg->precision);
    c->PL = DSN_PL(c->P, cfg->precision >= DSN_PREC_FP16 ? 1 : 0);
    c->fp8 = prec_fp8(cfg->precision);
    if (c->fp8 && cfg->score_kind == DSN_SCORE_DIT && cfg->dit_embed_dim % 128 != 0)
      fail(DSN_EINVAL, "DSN_PREC_FP8: embed_dim must be a multiple of 128 (got %d)", cfg->dit_embed_dim);
    return c;
  } catch (const std::exception& e) {
    g_create_err = e.what();
    return nullptr;
  }
}

void dsn_destroy(dsn_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->cfg.device);
  (void)hipDeviceSynchronize();
  for (auto& g : ctx->graphs)
    if (g.second.exec) (void)hipGraphExecDestroy(g.second.exec);
  for (int k = 0; k < 2; ++k) {
    if (ctx->own[k]) (void)hipStreamDestroy(ctx->own[k]);
    if (ctx->ev_in[k]) (void)hipEventDestroy(ctx->ev_in[k]);
    if (ctx->ev_out[k]) (void)hipEventDestroy(ctx->ev_out[k]);
  }
  for (auto& kv : ctx->raw) (void)hipFree(kv.second.p);
  for (void* p : ctx->allocs) (void)hipFree(p);
  for (auto& kv : ctx->ws) (void)hipFree(kv.second.first);
  for (auto& kv : ctx->gnf_sync) (void)hipFree(kv.second.first);
  if (ctx->fin_err_host) (void)hipHostFree(ctx->fin_err_host);
  if (ctx->ode_host) (void)hipHostFree(ctx->ode_host);
  delete ctx;
}

const char* dsn_last_error(const dsn_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int dsn_load_tensor(dsn_ctx* ctx, const char* name, const float* data, const int64_t* shape, int ndim,
                    int is_device) {
  return guarded(ctx, [&] {
    if (!name || !data || ndim < 0 || ndim > 8) fail(DSN_EINVAL, "dsn_load_tensor: bad arguments");
    DevTensor t;
    t.numel = 1;
    for (int i = 0; i < ndim; ++i) {
      t.shape.push_back(shape[i]);
      t.numel *= shape[i];
    }
    if (t.numel <= 0) fail(DSN_EINVAL, "%s: empty tensor", name);
    auto it = ctx->raw.find(name);
    if (it != ctx->raw.end()) {
      HIPCHK(hipFree(it->second.p));
      ctx->raw.erase(it);
    }
    HIPCHK(hipMalloc((void**)&t.p, sizeof(float) * t.numel));
    HIPCHK(hipMemcpy(t.p, data, sizeof(float) * t.numel, is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    ctx->raw[name] = t;
    ctx->finalized = false;
  });
}

int dsn_finalize_weights(dsn_ctx* ctx) { return dsn_finalize_weights_ex(ctx, 1); }

int dsn_finalize_weights_ex(dsn_ctx* ctx, int strict) {
  return guarded(ctx, [&] { ctx->finalize(nullptr, strict != 0); });
}

int dsn_score(dsn_ctx* ctx, const float* xt, const float* t, const float* mix, float* out, int B, int T,
              void* stream) {
  return guarded(ctx, [&] {
    if (!xt || !t || !mix || !out || B <= 0 || T <= 0) fail(DSN_EINVAL, "dsn_score: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    float* sc = ctx->score_tokens(xt, t, mix, B, T, st);
    launch_unpack_tokens(sc, out, B, ctx->cfg.n_src * ctx->cfg.latent_dim, T, st);
    HIPCHK(hipGetLastError());
  });
}

int dsn_ouve_schedule(const dsn_ctx* ctx, int N, float t_eps, float snr, float* timesteps, float* std_,
                      float* corr_step, float* corr_gain, float* G, float* std_T) {
  if (!ctx || N <= 0) return DSN_EINVAL;
  const dsn_ctx::Sched s = ctx->schedule(N, t_eps, snr);
  for (int i = 0; i < N; ++i) {
    if (timesteps) timesteps[i] = s.t[i];
    if (std_) std_[i] = s.std[i];
    if (corr_step) corr_step[i] = s.step[i];
    if (corr_gain) corr_gain[i] = s.gain[i];
    if (G) G[i] = s.G[i];
  }
  if (std_T) *std_T = s.stdT;
  return DSN_OK;
}

int dsn_score_ragged(dsn_ctx* ctx, const float* xt, const float* t, const float* mix, const int32_t* frames, float* out,
                     int B, int T, void* stream) {
  return guarded(ctx, [&] {
    if (!xt || !t || !mix || !out || B <= 0 || T <= 0) fail(DSN_EINVAL, "dsn_score_ragged: bad arguments");
    ctx->check_frames("dsn_score_ragged", frames, B, T);
    hipStream_t st = (hipStream_t)stream;
    const int* lens = ctx->upload_lens(frames, B, st);
    float* sc = ctx->score_tokens(xt, t, mix, B, T, st, lens);
    launch_unpack_tokens(sc, out, B, ctx->cfg.n_src * ctx->cfg.latent_dim, T, st);
    HIPCHK(hipGetLastError());
  });
}

// The refusals and the plan of the window-blended entry points (include/ditsep_hip.h), before anything is allocated
struct WindowArgs {
  int Tw, To, fade, batch;
};
static ScoreWindowPlan windowed_plan(dsn_ctx* ctx, const char* who, const int32_t* frames, int R, int T,
                                     const WindowArgs& wa) {
  if (ctx->cfg.score_kind != DSN_SCORE_DIT)
    fail(DSN_EINVAL, "%s: window-blended scores need the DiT score network (their windows are batch items of the "
         "trained length)", who);
  char buf[160];
  if (const char* why = score_window_refusal(frames, R, T, wa.Tw, wa.To, wa.fade, buf, sizeof buf))
    fail(DSN_EINVAL, "%s: %s", who, why);
  if (ctx->cfg.n_src * ctx->cfg.latent_dim % 4 != 0)
    fail(DSN_EINVAL, "%s: the blend launch loads 16 bytes per lane: n_src * latent_dim = %d is not a multiple of 4", who,
         ctx->cfg.n_src * ctx->cfg.latent_dim);
  if (!ctx->finalized) fail(DSN_ESTATE, "weights not finalized");
  return score_window_plan(frames, R, T, wa.Tw, wa.To, wa.fade);
}

// dsn_pc_sample_ex (frames == null), dsn_pc_sample_ragged and dsn_pc_sample_windowed (wa)
static int pc_sample_call(dsn_ctx* ctx, const float* y, const int32_t* frames, bool ragged, const float* noise,
                          uint64_t seed, float* x_out, int B, int T, int N, const dsn_sampler_opts* opts, int* nfe_out,
                          void* stream, const WindowArgs* wa = nullptr) {
  return guarded(ctx, [&] {
    if (!y || !x_out || !opts || B <= 0 || T <= 0 || N <= 0 || opts->corrector_steps < 0)
      fail(DSN_EINVAL, "dsn_pc_sample: bad arguments");
    if (opts->predictor < 0 || opts->predictor > DSN_PRED_NONE || opts->corrector < 0 ||
        opts->corrector > DSN_CORR_LANGEVIN)
      fail(DSN_EINVAL, "dsn_pc_sample: unknown predictor %d / corrector %d", opts->predictor, opts->corrector);
    const int* lens = nullptr;
    if (ragged) {
      ctx->check_frames("dsn_pc_sample_ragged", frames, B, T);
      if (opts->corrector == DSN_CORR_LANGEVIN)
        fail(DSN_EINVAL, "dsn_pc_sample_ragged: the langevin corrector (DSN_CORR_LANGEVIN) has no ragged form: its "
             "per-item norms would run over the padding");
      if (!ctx->finalized) fail(DSN_ESTATE, "weights not finalized");
      lens = ctx->upload_lens(frames, B, (hipStream_t)stream);
    }
    ScoreWindowPlan wplan;
    dsn_ctx::WinTables wt{};
    if (wa) {
      const char* who = "dsn_pc_sample_windowed";
      if (opts->prior_mean || opts->intermediates || opts->timesteps)
        fail(DSN_EINVAL, "%s: prior_mean, intermediates and timesteps are not supported", who);
      wplan = windowed_plan(ctx, who, frames, B, T, *wa);
      if (opts->corrector == DSN_CORR_LANGEVIN && wplan.ragged)
        fail(DSN_EINVAL, "%s: the langevin corrector (DSN_CORR_LANGEVIN) has no form for recordings of different "
             "lengths: its per-item norms would run over the padding", who);
      if (wplan.ragged) lens = ctx->upload_lens(frames, B, (hipStream_t)stream);  // (the tail to clear)
      wt = ctx->upload_window_tables(wplan, wa->batch, (hipStream_t)stream);
    }
    dsn_ctx::PcOpts o;
    o.pred = opts->predictor;
    o.corr = opts->corrector;
    o.c = opts->corrector_steps;
    o.denoise = opts->denoise;
    o.snr = opts->snr;
    o.t_eps = opts->timesteps ? opts->timesteps[N - 1] : opts->t_eps;
    o.inter = opts->intermediates;
    // free-form schedules / intermediates are not worth a graph cache entry each
    const bool graphs = ctx->use_graphs;
    if (opts->timesteps) ctx->t_override.assign(opts->timesteps, opts->timesteps + N);
    if (opts->timesteps || opts->intermediates) ctx->use_graphs = false;
    struct Restore {
      dsn_ctx* c;
      bool g;
      ~Restore() {
        c->use_graphs = g;
        c->t_override.clear();
      }
    } restore{ctx, graphs};
    char key[256];
    // (the last field marks a ragged call: the same graph whatever the lengths, another one than the dense call's)
    int kn = snprintf(key, sizeof key, "pc:%d:%d:%d:%d:%a:%a:%d:%d:%d:%d:%d", B, T, N, o.c, o.snr, o.t_eps, o.denoise,
                      o.pred, o.corr, opts->prior_mean != nullptr, lens != nullptr);
    // (a windowed call: the shape of its plan -- the tables themselves are data of the graph)
    if (wa)
      snprintf(key + kn, sizeof key - kn, ":w%d:%d:%d:%d:%d:%d", wplan.Wtot, wplan.Twin, wa->Tw, wa->To,
               wa->batch > 0 ? std::min(wa->batch, wplan.Wtot) : wplan.Wtot, (int)wplan.shorts);
    ctx->run_sampler({y, noise, opts->prior_mean, seed, x_out, B, T, o.draws(N), (hipStream_t)stream,
                      wa ? wplan.Wtot : 0},
                     ctx->schedule(N, o.t_eps, o.snr).t, key, o.denoise ? "pc_xm" : "pc_x",
                     [&](const float* yb, const float* nz, const float* pm, hipStream_t s2) {
                       o.prior_mean = pm;
                       return ctx->pc_sample(yb, nz, B, T, N, o, s2, lens, wa ? &wt : nullptr);
                     });
    if (nfe_out) *nfe_out = N * (o.c + 1);
  });
}

int dsn_pc_sample_ex(dsn_ctx* ctx, const float* y, const float* noise, uint64_t seed, float* x_out, int B, int T,
                     int N, const dsn_sampler_opts* opts, int* nfe_out, void* stream) {
  return pc_sample_call(ctx, y, nullptr, false, noise, seed, x_out, B, T, N, opts, nfe_out, stream);
}

int dsn_pc_sample_ragged(dsn_ctx* ctx, const float* y, const int32_t* frames, const float* noise, uint64_t seed,
                         float* x_out, int B, int T, int N, const dsn_sampler_opts* opts, int* nfe_out, void* stream) {
  return pc_sample_call(ctx, y, frames, true, noise, seed, x_out, B, T, N, opts, nfe_out, stream);
}

int dsn_pc_sample_windowed(dsn_ctx* ctx, const float* y, const int32_t* frames, const float* noise, uint64_t seed,
                           float* x_out, int R, int T, int N, int Tw, int To, int fade, int batch,
                           const dsn_sampler_opts* opts, int* nfe_out, void* stream) {
  const WindowArgs wa{Tw, To, fade, batch};
  return pc_sample_call(ctx, y, frames, false, noise, seed, x_out, R, T, N, opts, nfe_out, stream, &wa);
}

int dsn_score_window_plan(const int32_t* frames, int R, int T, int Tw, int To, int fade, int32_t* wtab, int32_t* ftab,
                          float* fw, int* Wtot, int* Twin) {
  char buf[160];
  if (score_window_refusal(frames, R, T, Tw, To, fade, buf, sizeof buf)) return DSN_EINVAL;
  const ScoreWindowPlan p = score_window_plan(frames, R, T, Tw, To, fade);
  if (wtab) std::copy(p.wtab.begin(), p.wtab.end(), wtab);
  if (ftab) std::copy(p.ftab.begin(), p.ftab.end(), ftab);
  if (fw) std::copy(p.fw.begin(), p.fw.end(), fw);
  if (Wtot) *Wtot = p.Wtot;
  if (Twin) *Twin = p.Twin;
  return DSN_OK;
}

int dsn_score_windowed(dsn_ctx* ctx, const float* xt, const float* t, const float* mix, const int32_t* frames, float* out,
                       int R, int T, int Tw, int To, int fade, int batch, void* stream) {
  return guarded(ctx, [&] {
    if (!xt || !t || !mix || !out) fail(DSN_EINVAL, "dsn_score_windowed: bad arguments");
    const ScoreWindowPlan p = windowed_plan(ctx, "dsn_score_windowed", frames, R, T, {Tw, To, fade, batch});
    hipStream_t st = (hipStream_t)stream;
    const dsn_ctx::WinTables wt = ctx->upload_window_tables(p, batch, st);
    float* tw = ctx->wsbuf<float>("win_t", p.Wtot);
    launch_win_times(t, wt.wtab, p.Wtot, tw, st);  // every window's time: its recording's
    float* sc = ctx->score_windowed(xt, tw, mix, wt, st);
    launch_unpack_tokens(sc, out, R, ctx->cfg.n_src * ctx->cfg.latent_dim, T, st);
    HIPCHK(hipGetLastError());
  });
}

int dsn_pc_sample(dsn_ctx* ctx, const float* y, const float* noise, uint64_t seed, float* x_out, int B, int T, int N,
                  int corrector_steps, float snr, float t_eps, int denoise, int* nfe_out, void* stream) {
  dsn_sampler_opts o;
  memset(&o, 0, sizeof o);
  o.corrector_steps = corrector_steps;
  o.snr = snr;
  o.t_eps = t_eps;
  o.denoise = denoise;
  return dsn_pc_sample_ex(ctx, y, noise, seed, x_out, B, T, N, &o, nfe_out, stream);
}

// get_pc_scheduled_sampler (src/sdes/__init__.py:49-130): same loop with caller-provided timesteps
// (linear / log / revlog grids of N+1 points, the first N are used).  The reference's `dt` stays 1/N in
// this sampler too (its `getattr(kwargs, "dt", ...)` on a dict never finds the key).
int dsn_pc_sample_sched(dsn_ctx* ctx, const float* y, const float* noise, uint64_t seed, float* x_out, int B, int T,
                        int N, const float* timesteps_host, int corrector_steps, float snr, int denoise, int* nfe_out,
                        void* stream) {
  if (!ctx || !timesteps_host || N <= 0) return DSN_EINVAL;
  dsn_sampler_opts o;
  memset(&o, 0, sizeof o);
  o.corrector_steps = corrector_steps;
  o.snr = snr;
  o.denoise = denoise;
  o.timesteps = timesteps_host;
  return dsn_pc_sample_ex(ctx, y, noise, seed, x_out, B, T, N, &o, nfe_out, stream);
}

int dsn_pc_sample_mix(dsn_ctx* ctx, const float* y, const float* noise, uint64_t seed, float* x_out, int B, int T, int N,
                      const dsn_mix_opts* opts, int* nfe_out, void* stream) {
  return guarded(ctx, [&] {
    if (!y || !x_out || !opts || B <= 0 || T <= 0 || N <= 0 || opts->corrector_steps < 0)
      fail(DSN_EINVAL, "dsn_pc_sample_mix: bad arguments");
    if (opts->predictor < 0 || opts->predictor > DSN_PRED_NONE || opts->corrector < 0 || opts->corrector > DSN_MIXCORR_NONE)
      fail(DSN_EINVAL, "dsn_pc_sample_mix: unknown predictor %d / corrector %d", opts->predictor, opts->corrector);
    const int n = ctx->cfg.n_src;
    if (n > 4) fail(DSN_EINVAL, "dsn_pc_sample_mix: at most 4 sources");
    if (!opts->prior_mix && n != 2)
      fail(DSN_EINVAL, "MixSDE.prior_sampling is written for 2 sources (reference sdes.py:347); use PriorMixSDE");
    if (opts->prior_mix && opts->avg_len < 1) fail(DSN_EINVAL, "PriorMixSDE: avg_len must be >= 1");
    if (!(opts->sigma_max > opts->sigma_min) || !(opts->sigma_min > 0)) fail(DSN_EINVAL, "need 0 < sigma_min < sigma_max");
    dsn_ctx::MixOpts o;
    o.prior_mix = opts->prior_mix;
    o.avg_len = opts->avg_len;
    o.pred = opts->predictor;
    o.corr = opts->corrector;
    o.c = opts->corrector == DSN_MIXCORR_NONE ? 0 : opts->corrector_steps;
    o.denoise = opts->denoise;
    o.d_lambda = opts->d_lambda;
    o.sigma_min = opts->sigma_min;
    o.sigma_max = opts->sigma_max;
    o.snr = opts->snr;
    o.t_eps = opts->t_eps;
    char key[224];
    snprintf(key, sizeof key, "pcmix:%d:%d:%d:%d:%d:%d:%d:%d:%a:%a:%a:%a:%a:%d", B, T, N, o.prior_mix, o.avg_len, o.pred,
             o.corr, o.c, o.d_lambda, o.sigma_min, o.sigma_max, o.snr, o.t_eps, o.denoise);
    ctx->run_sampler({y, noise, nullptr, seed, x_out, B, T, o.draws(N), (hipStream_t)stream},
                     ctx->schedule(N, o.t_eps, o.snr).t, key, o.denoise ? "pc_xm" : "pc_x",
                     [&](const float* yb, const float* nz, const float*, hipStream_t s2) {
                       return ctx->pc_sample_mix(yb, nz, B, T, N, o, s2);
                     });
    if (nfe_out) *nfe_out = N * (o.c + 1);
  });
}

int dsn_sb_sample(dsn_ctx* ctx, const float* y, const float* noise, uint64_t seed, float* x_out, int B, int T, int N, float k,
                  float c, float sb_eps, float t_eps, int sampler_type, void* stream) {
  return guarded(ctx, [&] {
    if (!y || !x_out || B <= 0 || T <= 0 || N <= 0) fail(DSN_EINVAL, "dsn_sb_sample: bad arguments");
    if (sampler_type != DSN_SB_SDE && sampler_type != DSN_SB_ODE) fail(DSN_EINVAL, "Invalid type. Choose 'ode' or 'sde'.");
    if (!(k > 0) || k == 1.f || !(c > 0)) fail(DSN_EINVAL, "SBVESDE: need k > 0, k != 1, c > 0");
    const long draws = sampler_type == DSN_SB_SDE ? N : 0;
    // step times t_1 .. t_N of linspace(1, eps, N + 1) as the network's time input
    const std::vector<float> ts = dsn_ctx::sb_times(N, t_eps);
    char key[160];
    snprintf(key, sizeof key, "sb:%d:%d:%d:%a:%a:%a:%a:%d", B, T, N, k, c, sb_eps, t_eps, sampler_type);
    ctx->run_sampler({y, noise, nullptr, seed, x_out, B, T, draws, (hipStream_t)stream},
                     std::vector<float>(ts.begin() + 1, ts.end()), key, "pc_x",
                     [&](const float* yb, const float* nz, const float*, hipStream_t s2) {
                       return ctx->sb_sample(yb, nz, B, T, N, k, c, sb_eps, t_eps, sampler_type == DSN_SB_ODE, s2);
                     });
  });
}

// ---------------------------------------------------------------- probability-flow ODE sampler
// Butcher tableaux of scipy's RK45 (Dormand-Prince 5(4)) and RK23 (Bogacki-Shampine 3(2)), scipy/integrate/_ivp/rk.py
static OdeTableau ode_tableau(int method) {
  OdeTableau t;
  memset(&t, 0, sizeof t);
  if (method == DSN_ODE_RK45) {
    t.stages = 6;
    t.err_order = 4;
    const double c[6] = {0, 1. / 5, 3. / 10, 4. / 5, 8. / 9, 1};
    const double a[6][5] = {{0, 0, 0, 0, 0},
                            {1. / 5, 0, 0, 0, 0},
                            {3. / 40, 9. / 40, 0, 0, 0},
                            {44. / 45, -56. / 15, 32. / 9, 0, 0},
                            {19372. / 6561, -25360. / 2187, 64448. / 6561, -212. / 729, 0},
                            {9017. / 3168, -355. / 33, 46732. / 5247, 49. / 176, -5103. / 18656}};
    const double b[6] = {35. / 384, 0, 500. / 1113, 125. / 192, -2187. / 6784, 11. / 84};
    const double e[7] = {-71. / 57600, 0, 71. / 16695, -71. / 1920, 17253. / 339200, -22. / 525, 1. / 40};
    for (int i = 0; i < 6; ++i) {
      t.c[i] = c[i];
      t.b[i] = b[i];
      for (int j = 0; j < 5; ++j) t.a[i][j] = a[i][j];
    }
    for (int i = 0; i < 7; ++i) t.e[i] = e[i];
  } else {
    t.stages = 3;
    t.err_order = 2;
    const double c[3] = {0, 1. / 2, 3. / 4};
    const double b[3] = {2. / 9, 1. / 3, 4. / 9};
    const double e[4] = {5. / 72, -1. / 12, -1. / 9, 1. / 8};
    for (int i = 0; i < 3; ++i) {
      t.c[i] = c[i];
      t.b[i] = b[i];
    }
    t.a[1][0] = 1. / 2;
    t.a[2][1] = 3. / 4;
    for (int i = 0; i < 4; ++i) t.e[i] = e[i];
  }
  return t;
}

int dsn_ode_sample(dsn_ctx* ctx, const float* y, const float* noise, uint64_t seed, float* x_out, int B, int T,
                   const DsnOdeOpts* o, DsnOdeStats* stats, void* stream) {
  if (stats) {
    memset(stats, 0, sizeof *stats);
    stats->status = -1;
  }
  return guarded(ctx, [&] {
    if (!y || !x_out || !o || B <= 0 || T <= 0) fail(DSN_EINVAL, "dsn_ode_sample: bad arguments");
    if (o->method != DSN_ODE_RK45 && o->method != DSN_ODE_RK23)
      fail(DSN_EINVAL, "dsn_ode_sample: method %d is neither DSN_ODE_RK45 nor DSN_ODE_RK23", o->method);
    if (!(o->t_eps > 0 && o->t_eps < 1)) fail(DSN_EINVAL, "dsn_ode_sample: t_eps must lie in (0, 1)");
    if (!(o->rtol > 0) || !(o->atol >= 0) || std::isnan(o->max_step))
      fail(DSN_EINVAL, "dsn_ode_sample: need rtol > 0, atol >= 0 and a max_step that is not NaN");
    if (o->max_attempts <= 0) fail(DSN_EINVAL, "dsn_ode_sample: max_attempts must be positive");
    if (o->denoise && o->N <= 0) fail(DSN_EINVAL, "dsn_ode_sample: denoise needs N > 0");
    const double interval = 1.0 - o->t_eps;
    const float t_eps32 = (float)o->t_eps;
    if (!(o->first_step >= 0 && o->first_step <= interval))   // (NaN fails too)
      fail(DSN_EINVAL, "dsn_ode_sample: first_step must lie in (0, 1 - t_eps] (0 = automatic)");
    if (!ctx->finalized) fail(DSN_ESTATE, "weights not finalized");
    const dsn_config& cfg = ctx->cfg;
    const int n = cfg.n_src, Dl = cfg.latent_dim;
    const long ysz = (long)B * Dl * T, sz = ysz * n;
    const OdeTableau tab = ode_tableau(o->method);
    const int S = tab.stages;
    OdeSde q;
    q.theta = cfg.sde_theta;
    q.sigma_min = cfg.sde_sigma_min;
    q.ratio = (double)cfg.sde_sigma_max / (double)cfg.sde_sigma_min;
    q.logratio = log(q.ratio);
    const bool auto_h = o->first_step == 0;
    // rtol below 100 eps is raised to it (scipy common.validate_tol)
    const double rtol = std::max(o->rtol, 100 * 2.220446049250313e-16);

    hipStream_t caller = (hipStream_t)stream;
    float* yb = ctx->wsbuf<float>("ode_ymix", ysz);
    float* nz = ctx->wsbuf<float>("ode_noise", sz);
    double* ys = ctx->wsbuf<double>("ode_y", sz);
    double* yn = ctx->wsbuf<double>("ode_ynew", sz);
    double* xs64 = ctx->wsbuf<double>("ode_xs64", sz);
    double* K = ctx->wsbuf<double>("ode_K", (long)(S + 1) * sz);
    float* xs32 = ctx->wsbuf<float>("ode_xs32", sz);
    float* xo = ctx->wsbuf<float>("ode_out", sz);
    float* zero = o->denoise ? ctx->wsbuf<float>("ode_zero", sz) : nullptr;
    float* tv = ctx->wsbuf<float>("ode_t", B);
    double* part = ctx->wsbuf<double>("ode_part", 2L * ode_grid(sz));
    OdeCtl* ctl = ctx->wsbuf<OdeCtl>("ode_ctl", 1);
    if (!ctx->ode_host) HIPCHK(hipHostMalloc((void**)&ctx->ode_host, sizeof(OdeCtl), hipHostMallocDefault));
    OdeCtl* hc = ctx->ode_host;
    memset(hc, 0, sizeof *hc);
    hc->t = 1.0;
    hc->t_bound = o->t_eps;
    hc->direction = -1.0;
    hc->max_step = (o->max_step > 0) ? o->max_step : INFINITY;
    hc->first_step = o->first_step;
    hc->rtol = rtol;
    hc->atol = o->atol;
    hc->status = -1;
    hc->max_attempts = o->max_attempts;

    dsn_ctx::StreamScope sc(ctx, caller);
    hipStream_t st = sc.st;
    HIPCHK(hipMemcpyAsync(ctl, hc, sizeof(OdeCtl), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(yb, y, sizeof(float) * ysz, hipMemcpyDeviceToDevice, st));
    dsn_ctx::stage_noise(nz, noise, sz, seed, st);  // draw 0 of the stream dsn_pc_sample uses: the same x_T for a seed
    const float stdT = ctx->ouve_std(1.f);
    char key[160];
    // prior, f0 = fun(t0, y0) and the initial step (scipy select_initial_step: one more evaluation)
    snprintf(key, sizeof key, "ode_init:%d:%d:%d:%d", B, T, o->method, (int)auto_h);
    ctx->run_graphed(key, st, [&](hipStream_t s2) {
      launch_ode_prior(yb, nz, ys, xs32, tv, stdT, B, n, Dl, T, s2);
      const float* sc = ctx->score_tokens(xs32, tv, yb, B, T, s2);
      launch_ode_init_f0(q, ctl, yb, sc, ys, K, part, B, n, Dl, T, s2);
      launch_ode_init_h0(ctl, part, sz, s2);
      if (auto_h) {
        launch_ode_init_y1(ctl, ys, K, xs64, xs32, tv, B, sz, s2);
        sc = ctx->score_tokens(xs32, tv, yb, B, T, s2);
        launch_ode_init_f1(q, ctl, yb, sc, ys, K, xs64, part, B, n, Dl, T, s2);
        launch_ode_init_h1(ctl, part, sz, tab.err_order, s2);
      }
    });
    // step attempts: one launch sequence, replayed until the controller sets `done` (polled after every attempt)
    snprintf(key, sizeof key, "ode_step:%d:%d:%d", B, T, o->method);
    for (int k = 0;; ++k) {
      ctx->run_graphed(key, st, [&](hipStream_t s2) {
        launch_ode_prep(tab, ctl, ys, yn, K, xs64, xs32, tv, B, sz, s2);
        for (int i = 1; i <= S; ++i) {
          const float* sc = ctx->score_tokens(xs32, tv, yb, B, T, s2);
          launch_ode_stage(tab, q, ctl, i, yb, sc, ys, yn, K, xs64, xs32, tv, part, B, n, Dl, T, s2);
        }
        launch_ode_control(ctl, part, sz, S, tab.err_order, s2);
      });
      HIPCHK(hipMemcpyAsync(hc, ctl, sizeof(OdeCtl), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (hc->done) break;
      if (k + 1 >= o->max_attempts)  // the controller stops at max_attempts: not reached unless the state is corrupt
        fail(DSN_ESOLVER, "dsn_ode_sample: the solver did not stop after max_attempts = %d attempts", o->max_attempts);
    }
    if (stats) {
      stats->nfev = hc->nfev;
      stats->n_accepted = hc->accepted;
      stats->n_rejected = hc->rejected;
      stats->t_final = hc->t;
      stats->status = hc->status;
    }
    if (hc->status == DSN_ODE_STEP_TOO_SMALL)
      fail(DSN_ESOLVER, "dsn_ode_sample: required step size is less than spacing between numbers (t = %.17g, h = %g)",
           hc->t, hc->h_abs);
    if (hc->status == DSN_ODE_TOO_MANY_ATTEMPTS)
      fail(DSN_ESOLVER, "dsn_ode_sample: t = %.17g not reached after max_attempts = %d step attempts (%d accepted)",
           hc->t, hc->attempts, hc->accepted);
    // final state (fp32), then the optional noise-free reverse-diffusion step at t_eps (dt = 1/N)
    const float dt = o->denoise ? (float)(1.0 / o->N) : 0.f;
    const double smin = cfg.sde_sigma_min, smax = cfg.sde_sigma_max, ls = log(smax / smin);
    const float sigma = (float)smin * powf((float)(smax / smin), t_eps32);
    const float G = sigma * (float)sqrt(2.0 * ls) * sqrtf(dt);
    snprintf(key, sizeof key, "ode_out:%d:%d:%d:%a:%a", B, T, o->denoise, t_eps32, dt);
    ctx->run_graphed(key, st, [&](hipStream_t s2) {
      launch_ode_emit(ctl, ys, yn, xo, tv, t_eps32, B, sz, s2);
      if (o->denoise) {
        const float* sc = ctx->score_tokens(xo, tv, yb, B, T, s2);
        // pc_predictor_kernel itself with z = 0: x_mean -> xs32 (x <- x_mean + G * 0 in xo)
        HIPCHK(hipMemsetAsync(zero, 0, sizeof(float) * sz, s2));
        launch_pc_predictor(xo, xs32, yb, sc, zero, cfg.sde_theta, dt, G, 0.f, 0, B, n, Dl, T, s2);
      }
    });
    HIPCHK(hipMemcpyAsync(x_out, o->denoise ? xs32 : xo, sizeof(float) * sz, hipMemcpyDeviceToDevice, st));
    sc.leave();
    HIPCHK(hipGetLastError());
  });
}

// dsn_score_loss (ragged == false) and dsn_score_loss_ragged (frames: HOST [B])
static int score_loss_call(dsn_ctx* ctx, const float* y, const float* x0, const int32_t* frames, bool ragged,
                           const float* t, const float* noise, const int32_t* perm, uint64_t seed, float* loss_out,
                           float* xt_out, float* t_out, float* sigma_out, float* z_out, int B, int T,
                           const DsnLossOpts* o, void* stream) {
  return guarded(ctx, [&] {
    if (!y || !x0 || !o || B <= 0 || T <= 0 || B > 65535) fail(DSN_EINVAL, "dsn_score_loss: bad arguments");
    if (ragged) ctx->check_frames("dsn_score_loss_ragged", frames, B, T);
    if (o->mode != DSN_LOSS_DSM && o->mode != DSN_LOSS_INIT_PIT)
      fail(DSN_EINVAL, "dsn_score_loss: mode %d is neither DSN_LOSS_DSM nor DSN_LOSS_INIT_PIT", o->mode);
    if (o->reduction != DSN_LOSS_REDUCE_NONE && o->reduction != DSN_LOSS_REDUCE_MEAN)
      fail(DSN_EINVAL, "dsn_score_loss: unknown reduction %d", o->reduction);
    const bool pit = o->mode == DSN_LOSS_INIT_PIT;
    if (pit && (t || perm)) fail(DSN_EINVAL, "dsn_score_loss: DSN_LOSS_INIT_PIT fixes t = 1 and takes no t / perm");
    if (!pit && !t && !(o->t_eps > 0 && o->t_eps < 1)) fail(DSN_EINVAL, "dsn_score_loss: t_eps must lie in (0, 1)");
    const dsn_config& cfg = ctx->cfg;
    const int n = cfg.n_src, Dl = cfg.latent_dim;
    if (n > 4) fail(DSN_EINVAL, "dsn_score_loss: n_src = %d (at most 4 sources)", n);
    if (loss_out && !ctx->finalized) fail(DSN_ESTATE, "weights not finalized");
    const long DT = (long)Dl * T, ysz = (long)B * DT, sz = ysz * n;
    hipStream_t caller = (hipStream_t)stream;
    // injected t / perm: checked on the host before anything is launched
    if (t || perm) {
      HIPCHK(hipStreamSynchronize(caller));
      if (t) {
        std::vector<float> ht((size_t)B);
        HIPCHK(hipMemcpy(ht.data(), t, sizeof(float) * B, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b)
          if (!(ht[b] > 0.f && ht[b] <= 1.f))
            fail(DSN_EINVAL, "dsn_score_loss: t[%d] = %g lies outside (0, 1]", b, ht[b]);
      }
      if (perm) {
        std::vector<int32_t> hp((size_t)B * n);
        HIPCHK(hipMemcpy(hp.data(), perm, sizeof(int32_t) * hp.size(), hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b) {
          unsigned seen = 0;
          for (int s = 0; s < n; ++s) {
            const int32_t v = hp[(size_t)b * n + s];
            if (v < 0 || v >= n || (seen >> v & 1u))
              fail(DSN_EINVAL, "dsn_score_loss: perm row %d is not a permutation of 0..%d", b, n - 1);
            seen |= 1u << v;
          }
        }
      }
    }
    LossSde q;
    q.theta = cfg.sde_theta;
    q.sigma_min = cfg.sde_sigma_min;
    q.logsig = log((double)cfg.sde_sigma_max / (double)cfg.sde_sigma_min);
    const int nj = pit ? n : 1, chunks = loss_chunks(Dl, T);
    // stable workspace copies of the caller's tensors (graph replay needs fixed pointers)
    float* yb = ctx->wsbuf<float>("loss_y", ysz);
    float* xb = ctx->wsbuf<float>("loss_x0", sz);
    float* nz = ctx->wsbuf<float>("loss_z", sz);
    float* xt = ctx->wsbuf<float>("loss_xt", sz);
    float* tin = ctx->wsbuf<float>("loss_tin", B);
    float* tv = ctx->wsbuf<float>("loss_t", B);
    float* sg = ctx->wsbuf<float>("loss_sigma", B);
    int* pb = ctx->wsbuf<int>("loss_perm", (long)B * n);
    double* part = ctx->wsbuf<double>("loss_part", (long)B * n * n * chunks);
    double* rows = ctx->wsbuf<double>("loss_rows", (long)B * n);
    float* lo = ctx->wsbuf<float>("loss_out", (long)B * n);
    // the token counts 1 + frames[b] of the length-aware attention, which the loss kernels read as well: uploaded
    // outside the capture, so the lengths are data of the cached graph
    const int* tok = ragged ? ctx->upload_lens(frames, B, caller) : nullptr;
    dsn_ctx::StreamScope sc(ctx, caller);
    hipStream_t st = sc.st;
    HIPCHK(hipMemcpyAsync(yb, y, sizeof(float) * ysz, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(xb, x0, sizeof(float) * sz, hipMemcpyDeviceToDevice, st));
    dsn_ctx::stage_noise(nz, noise, sz, seed, st);  // draw 0 of the stream the samplers use
    if (t) HIPCHK(hipMemcpyAsync(tin, t, sizeof(float) * B, hipMemcpyDeviceToDevice, st));
    else if (!pit) launch_rand_uniform(tin, B, seed ^ 0x9E3779B97F4A7C15ULL, 0, o->t_eps, 1.f, st);
    if (perm) HIPCHK(hipMemcpyAsync(pb, perm, sizeof(int) * B * n, hipMemcpyDeviceToDevice, st));
    char key[160];
    snprintf(key, sizeof key, "loss:%d:%d:%d:%d:%d:%d:%d", B, T, o->mode, o->reduction, perm != nullptr,
             loss_out != nullptr, ragged);
    ctx->run_graphed(key, st, [&](hipStream_t s2) {
      launch_loss_perturb(q, yb, xb, nz, pit ? nullptr : tin, 1.f, perm ? pb : nullptr, pit, xt, tv, sg, B, n, Dl, T,
                          s2, tok);
      if (!loss_out) return;
      const float* sc = ctx->score_tokens(xt, tv, yb, B, T, s2, tok);
      launch_loss_reduce(q, sc, nz, yb, xb, tv, sg, pit, part, B, n, Dl, T, s2, tok);
      launch_loss_combine(part, rows, lo, B, n, nj, chunks, Dl, T, o->reduction == DSN_LOSS_REDUCE_MEAN, s2, tok);
    });
    if (loss_out) {
      const long cnt = o->reduction == DSN_LOSS_REDUCE_MEAN ? 1 : (long)B * n;
      HIPCHK(hipMemcpyAsync(loss_out, lo, sizeof(float) * cnt, hipMemcpyDeviceToDevice, st));
    }
    if (xt_out) HIPCHK(hipMemcpyAsync(xt_out, xt, sizeof(float) * sz, hipMemcpyDeviceToDevice, st));
    if (t_out) HIPCHK(hipMemcpyAsync(t_out, tv, sizeof(float) * B, hipMemcpyDeviceToDevice, st));
    if (sigma_out) HIPCHK(hipMemcpyAsync(sigma_out, sg, sizeof(float) * B, hipMemcpyDeviceToDevice, st));
    if (z_out) HIPCHK(hipMemcpyAsync(z_out, nz, sizeof(float) * sz, hipMemcpyDeviceToDevice, st));
    sc.leave();
    HIPCHK(hipGetLastError());
  });
}

int dsn_score_loss(dsn_ctx* ctx, const float* y, const float* x0, const float* t, const float* noise,
                   const int32_t* perm, uint64_t seed, float* loss_out, float* xt_out, float* t_out, float* sigma_out,
                   float* z_out, int B, int T, const DsnLossOpts* o, void* stream) {
  return score_loss_call(ctx, y, x0, nullptr, false, t, noise, perm, seed, loss_out, xt_out, t_out, sigma_out, z_out, B,
                         T, o, stream);
}

int dsn_score_loss_ragged(dsn_ctx* ctx, const float* y, const float* x0, const int32_t* frames, const float* t,
                          const float* noise, const int32_t* perm, uint64_t seed, float* loss_out, float* xt_out,
                          float* t_out, float* sigma_out, float* z_out, int B, int T, const DsnLossOpts* o,
                          void* stream) {
  return score_loss_call(ctx, y, x0, frames, true, t, noise, perm, seed, loss_out, xt_out, t_out, sigma_out, z_out, B, T,
                         o, stream);
}

int dsn_hop_length(const dsn_ctx* ctx) { return ctx ? ctx->hop() : DSN_EINVAL; }

int dsn_latent_frames(const dsn_ctx* ctx, int L) {
  if (!ctx || L < 0) return DSN_EINVAL;
  const int h = ctx->hop();
  return (L + (h - L % h)) / h;  // reference utils.pad: a full extra hop when L % hop == 0
}

// dsn_decode (one graphed decode of all T frames) and dsn_decode_chunked (`chunked`: decode_chunked, whose chunks
// are graphed one by one)
static int decode_call(dsn_ctx* ctx, const char* who, const float* est, float* wav, int B, int T, int target_len,
                       bool chunked, int chunk_size, int overlap, void* stream) {
  return guarded(ctx, [&] {
    if (!est || !wav || B <= 0 || T <= 0) fail(DSN_EINVAL, "%s: bad arguments", who);
    const int S = B * ctx->cfg.n_src;
    const long Lfull = (long)ctx->hop() * T;
    const long Lt = target_len > 0 ? target_len : Lfull;
    if (Lt > Lfull) fail(DSN_EINVAL, "target_len %ld > decoded length %ld", Lt, Lfull);
    const long esz = (long)S * ctx->cfg.latent_dim * T;
    float* eb = ctx->wsbuf<float>("dec_est", esz);
    dsn_ctx::StreamScope sc(ctx, (hipStream_t)stream, 1);
    HIPCHK(hipMemcpyAsync(eb, est, sizeof(float) * esz, hipMemcpyDeviceToDevice, sc.st));
    float* w = nullptr;
    if (chunked) {
      w = ctx->decode_chunked(eb, S, T, chunk_size, overlap, sc.st);
    } else {
      char key[64];
      snprintf(key, sizeof key, "dec:%d:%d", S, T);
      ctx->run_graphed(key, sc.st, [&](hipStream_t s2) { w = ctx->decode(eb, S, T, s2); });
      if (!w) w = ctx->wsbuf<float>("dec_wav", (long)S * Lfull);
    }
    HIPCHK(hipMemcpy2DAsync(wav, sizeof(float) * Lt, w, sizeof(float) * Lfull, sizeof(float) * Lt, S,
                            hipMemcpyDeviceToDevice, sc.st));
    sc.leave();
  });
}

int dsn_decode(dsn_ctx* ctx, const float* est, float* wav, int B, int T, int target_len, void* stream) {
  return decode_call(ctx, "dsn_decode", est, wav, B, T, target_len, false, 0, 0, stream);
}

// zero-padded copy of the mixture ("enc_wav", T frames of hop() samples) and the VAE noise, drawn into
// "enc_noise" unless injected
struct EncodeIn {
  float* padded;
  const float* vae_noise;
  int T;
  long Lp;
};
static EncodeIn stage_encode(dsn_ctx* ctx, const float* mix, const float* vae_noise, uint64_t seed, int B, int L,
                             hipStream_t st) {
  const int h = ctx->hop();
  const int T = dsn_latent_frames(ctx, L);
  const long Lp = (long)T * h;
  float* padded = ctx->wsbuf<float>("enc_wav", (long)B * Lp);
  HIPCHK(hipMemsetAsync(padded, 0, sizeof(float) * B * Lp, st));
  if (L > 0)
    HIPCHK(hipMemcpy2DAsync(padded, sizeof(float) * Lp, mix, sizeof(float) * L, sizeof(float) * L, B,
                            hipMemcpyDeviceToDevice, st));
  const long nsz = (long)B * ctx->cfg.latent_dim * T;
  if (!vae_noise) {
    float* nz = ctx->wsbuf<float>("enc_noise", nsz);
    launch_randn(nz, nsz, seed ^ 0x5851F42D4C957F2DULL, 0, st);
    vae_noise = nz;
  }
  return {padded, vae_noise, T, Lp};
}

int dsn_encode(dsn_ctx* ctx, const float* mix, const float* vae_noise, uint64_t seed, float* y, int B, int L,
               void* stream) {
  return guarded(ctx, [&] {
    if (!mix || !y || B <= 0 || L < 0) fail(DSN_EINVAL, "dsn_encode: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const EncodeIn in = stage_encode(ctx, mix, vae_noise, seed, B, L, st);
    ctx->encode(in.padded, in.vae_noise, y, B, (int)in.Lp, st);
    HIPCHK(hipGetLastError());
  });
}

int dsn_decode_chunked(dsn_ctx* ctx, const float* est, float* wav, int B, int T, int target_len, int chunk_size,
                       int overlap, void* stream) {
  return decode_call(ctx, "dsn_decode_chunked", est, wav, B, T, target_len, true, chunk_size, overlap, stream);
}

int dsn_encode_chunked(dsn_ctx* ctx, const float* mix, const float* vae_noise, uint64_t seed, float* y, int B, int L,
                       int chunk_size, int overlap, void* stream) {
  return guarded(ctx, [&] {
    if (!mix || !y || B <= 0 || L < 0) fail(DSN_EINVAL, "dsn_encode_chunked: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const EncodeIn in = stage_encode(ctx, mix, vae_noise, seed, B, L, st);
    float* enc = ctx->encode_chunked(in.padded, B, in.T, chunk_size, overlap, st);
    launch_vae_sample(enc, in.vae_noise, y, B, ctx->cfg.latent_dim, in.T, st);
    HIPCHK(hipGetLastError());
  });
}

int dsn_separate(dsn_ctx* ctx, const float* mix, const float* vae_noise, const float* noise, uint64_t seed,
                 float* wav, int B, int L, int target_len, int N, int corrector_steps, float snr, float t_eps,
                 int denoise, int* nfe_out, void* stream) {
  if (!ctx) return DSN_EINVAL;
  const int T = dsn_latent_frames(ctx, L);
  int rc = DSN_OK;
  float* y = nullptr;
  float* x = nullptr;
  rc = guarded(ctx, [&] {
    const long ysz = (long)B * ctx->cfg.latent_dim * T;
    y = ctx->wsbuf<float>("sep_y", ysz);
    x = ctx->wsbuf<float>("sep_x", ysz * ctx->cfg.n_src);
  });
  if (rc) return rc;
  if ((rc = dsn_encode(ctx, mix, vae_noise, seed, y, B, L, stream))) return rc;
  if ((rc = dsn_pc_sample(ctx, y, noise, seed + 1, x, B, T, N, corrector_steps, snr, t_eps, denoise, nfe_out, stream)))
    return rc;
  return dsn_decode(ctx, x, wav, B, T, target_len > 0 ? target_len : L, stream);
}

// Ragged batches through the codec in one padded pass (include/ditsep_hip.h).  Every refusal comes from check_frames,
// before the workspace is touched.
int dsn_decode_ragged(dsn_ctx* ctx, const float* est, const int32_t* frames, float* wav, int B, int T, void* stream) {
  return guarded(ctx, [&] {
    if (!est || !wav || B <= 0 || T <= 0) fail(DSN_EINVAL, "dsn_decode_ragged: bad arguments");
    ctx->check_frames("dsn_decode_ragged", frames, B, T, dsn_ctx::RAGGED_DEC);
    const int S = B * ctx->cfg.n_src;
    const long Lfull = (long)ctx->hop() * T;
    const long esz = (long)S * ctx->cfg.latent_dim * T;
    float* eb = ctx->wsbuf<float>("dec_est", esz);
    const dsn_ctx::CodecLens cl{ctx->upload_frames(frames, B, (hipStream_t)stream), frames, ctx->cfg.n_src};
    dsn_ctx::StreamScope sc(ctx, (hipStream_t)stream, 1);
    HIPCHK(hipMemcpyAsync(eb, est, sizeof(float) * esz, hipMemcpyDeviceToDevice, sc.st));
    float* w = nullptr;
    char key[64];
    snprintf(key, sizeof key, "decr:%d:%d", S, T);  // (the lengths are data of the graph, not part of its key)
    ctx->run_graphed(key, sc.st, [&](hipStream_t s2) { w = ctx->decode(eb, S, T, s2, &cl); });
    if (!w) w = ctx->wsbuf<float>("dec_wav", (long)S * Lfull);
    HIPCHK(hipMemcpyAsync(wav, w, sizeof(float) * S * Lfull, hipMemcpyDeviceToDevice, sc.st));
    sc.leave();
  });
}

int dsn_encode_ragged(dsn_ctx* ctx, const float* mix, const int32_t* frames, const float* vae_noise, uint64_t seed,
                      float* y, int B, int T, void* stream) {
  return guarded(ctx, [&] {
    if (!mix || !y || B <= 0 || T <= 0) fail(DSN_EINVAL, "dsn_encode_ragged: bad arguments");
    ctx->check_frames("dsn_encode_ragged", frames, B, T, dsn_ctx::RAGGED_ENC);
    hipStream_t st = (hipStream_t)stream;
    const long Lp = (long)ctx->hop() * T;
    if (!vae_noise) {  // (the dense call's stream: stage_encode)
      const long nsz = (long)B * ctx->cfg.latent_dim * T;
      float* nz = ctx->wsbuf<float>("enc_noise", nsz);
      launch_randn(nz, nsz, seed ^ 0x5851F42D4C957F2DULL, 0, st);
      vae_noise = nz;
    }
    const dsn_ctx::CodecLens cl{ctx->upload_frames(frames, B, st), frames, 1};
    ctx->encode(mix, vae_noise, y, B, (int)Lp, st, &cl);
    HIPCHK(hipGetLastError());
  });
}

int dsn_separate_ragged(dsn_ctx* ctx, const float* mix, const int32_t* frames, const float* vae_noise, const float* noise,
                        uint64_t seed, float* wav, int B, int T, int N, const dsn_sampler_opts* opts, int* nfe_out,
                        void* stream) {
  float* y = nullptr;
  float* x = nullptr;
  int rc = guarded(ctx, [&] {
    if (!mix || !wav || !opts || B <= 0 || T <= 0 || N <= 0) fail(DSN_EINVAL, "dsn_separate_ragged: bad arguments");
    ctx->check_frames("dsn_separate_ragged", frames, B, T,
                      dsn_ctx::RAGGED_DIT | dsn_ctx::RAGGED_ENC | dsn_ctx::RAGGED_DEC);
    if (opts->corrector == DSN_CORR_LANGEVIN)
      fail(DSN_EINVAL, "dsn_separate_ragged: the langevin corrector (DSN_CORR_LANGEVIN) has no ragged form: its "
           "per-item norms would run over the padding");
    const long ysz = (long)B * ctx->cfg.latent_dim * T;
    y = ctx->wsbuf<float>("sep_y", ysz);
    x = ctx->wsbuf<float>("sep_x", ysz * ctx->cfg.n_src);
  });
  if (rc) return rc;
  if ((rc = dsn_encode_ragged(ctx, mix, frames, vae_noise, seed, y, B, T, stream))) return rc;
  if ((rc = dsn_pc_sample_ragged(ctx, y, frames, noise, seed + 1, x, B, T, N, opts, nfe_out, stream))) return rc;
  return dsn_decode_ragged(ctx, x, frames, wav, B, T, stream);
}

int dsn_separate_windowed(dsn_ctx* ctx, const float* mix, const int32_t* frames, const float* vae_noise,
                          const float* noise, uint64_t seed, float* wav, int R, int T, int N, int Tw, int To, int fade,
                          int batch, const dsn_sampler_opts* opts, int* nfe_out, void* stream) {
  float* y = nullptr;
  float* x = nullptr;
  int rc = guarded(ctx, [&] {
    if (!mix || !wav || !opts || R <= 0 || T <= 0 || N <= 0) fail(DSN_EINVAL, "dsn_separate_windowed: bad arguments");
    ctx->check_frames("dsn_separate_windowed", frames, R, T,
                      dsn_ctx::RAGGED_DIT | dsn_ctx::RAGGED_ENC | dsn_ctx::RAGGED_DEC);
    const ScoreWindowPlan p = windowed_plan(ctx, "dsn_separate_windowed", frames, R, T, {Tw, To, fade, batch});
    if (opts->corrector == DSN_CORR_LANGEVIN && p.ragged)
      fail(DSN_EINVAL, "dsn_separate_windowed: the langevin corrector (DSN_CORR_LANGEVIN) has no form for recordings of "
           "different lengths: its per-item norms would run over the padding");
    const long ysz = (long)R * ctx->cfg.latent_dim * T;
    y = ctx->wsbuf<float>("sep_y", ysz);
    x = ctx->wsbuf<float>("sep_x", ysz * ctx->cfg.n_src);
  });
  if (rc) return rc;
  if ((rc = dsn_encode_ragged(ctx, mix, frames, vae_noise, seed, y, R, T, stream))) return rc;
  if ((rc = dsn_pc_sample_windowed(ctx, y, frames, noise, seed + 1, x, R, T, N, Tw, To, fade, batch, opts, nfe_out,
                                   stream)))
    return rc;
  return dsn_decode_ragged(ctx, x, frames, wav, R, T, stream);
}

// Scale-invariant SDR with permutation-invariant assignment (the step right after the path in
// evaluate_latent.py:118-136, where the reference calls fast_bss_eval.si_bss_eval_sources with
// compute_permutation=True).  Device: all n x n correlation / energy sums; host: SI-SDR matrix
// (no mean removal, eps 1e-10) and the best of the n! <= 24 permutations.
int dsn_si_sdr_pit(dsn_ctx* ctx, const float* ref, const float* est, int B, int n, int L, float* si_sdr_out,
                   int* perm_out, void* stream) {
  return guarded(ctx, [&] {
    if (!ref || !est || B <= 0 || n <= 0 || n > 4 || L <= 0) fail(DSN_EINVAL, "dsn_si_sdr_pit: bad arguments (n <= 4)");
    hipStream_t st = (hipStream_t)stream;
    double* dd = ctx->wsbuf<double>("sisdr", (long)B * n * n * 3);
    launch_sisdr_dots(ref, est, B, n, L, nullptr, dd, st);
    std::vector<double> h((size_t)B * n * n * 3);
    HIPCHK(hipMemcpyAsync(h.data(), dd, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int b = 0; b < B; ++b) {
      // sdr[i][j]: est_j scored against ref_i
      double sdr[4][4];
      for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
          const double* v = &h[(((size_t)b * n + i) * n + j) * 3];
          const double eps = 1e-10;
          const double alpha = v[0] / (v[1] + eps);
          const double tgt = alpha * alpha * v[1];
          const double noise = v[2] - 2.0 * alpha * v[0] + tgt;
          sdr[i][j] = 10.0 * log10((tgt + eps) / (noise + eps));
        }
      const std::vector<int> bestp = best_permutation(n, [&](const std::vector<int>& p) {
        double s = 0;
        for (int i = 0; i < n; ++i) s += sdr[i][p[i]];
        return s / n;
      });
      for (int i = 0; i < n; ++i) {
        if (si_sdr_out) si_sdr_out[(size_t)b * n + i] = (float)sdr[i][bestp[i]];
        if (perm_out) perm_out[(size_t)b * n + i] = bestp[i];
      }
    }
  });
}

// The ragged metric calls (dsn_si_bss_eval_ragged, dsn_stoi_ragged, dsn_composite_ragged) read [B, n, Lmax] batches
// whose item b holds lens[b] samples.  check_item_lens is their refusal, made before anything is allocated or
// launched; upload_item_ints copies the per-item tables a call derived from lens (asynchronously on `st` from `h`,
// which the caller keeps alive until it has synchronised) into the workspace buffer `buf`.
static void check_item_lens(const char* who, const int32_t* lens, int B, int Lmax) {
  if (!lens) fail(DSN_EINVAL, "%s: lens is null", who);
  for (int b = 0; b < B; ++b)
    if (lens[b] < 1 || lens[b] > Lmax)
      fail(DSN_EINVAL, "%s: sample count lens[%d] = %d outside [1, Lmax = %d]", who, b, (int)lens[b], Lmax);
}
static const int* upload_item_ints(dsn_ctx* ctx, const char* buf, const std::vector<int>& h, hipStream_t st) {
  int* d = ctx->wsbuf<int>(buf, (long)h.size());
  HIPCHK(hipMemcpyAsync(d, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice, st));
  return d;
}

// SI-SDR / SI-SIR / SI-SAR of every estimate against the references (the decomposition of bss_eval with a
// one-tap, i.e. scale-invariant, distortion filter; evaluate_latent.py:118-136 calls
// fast_bss_eval.si_bss_eval_sources(ref, est, zero_mean=False, compute_permutation=True, clamp_db=100)):
//   e_target = <est_j, ref_i> ref_i / |ref_i|^2          (projection on the matched reference)
//   P est_j  = projection of est_j on span{ref_0 .. ref_{n-1}}   (n x n Gram solve)
//   e_interf = P est_j - e_target,  e_artif = est_j - P est_j
//   SI-SDR = |e_target|^2 / |est_j - e_target|^2,  SI-SIR = |e_target|^2 / |e_interf|^2,
//   SI-SAR = |P est_j|^2 / |e_artif|^2
// Device: all inner products (two launches of the dots kernel: ref x est and ref x ref), fp64 accumulation;
// host: the n <= 4 Gram solves and the permutation (perm_by: 0 = best mean SI-SDR, 1 = best mean SI-SIR --
// bss_eval's convention, "order according to SIR" evaluate_latent.py:124).  Values clamped to +-clamp_db.
// With lens (ragged) item b's inner products run over its first lens[b] samples of the Lmax-strided rows.
// dsn_si_bss_eval (lens null, ragged false) and dsn_si_bss_eval_ragged (`who` names the entry point in errors)
static int si_bss_eval_call(dsn_ctx* ctx, const char* who, const float* ref, const float* est, int B, int n, int L,
                            const int32_t* lens, bool ragged, int perm_by, float clamp_db, float* si_sdr_out,
                            float* si_sir_out, float* si_sar_out, int* perm_out, void* stream) {
  return guarded(ctx, [&] {
    if (!ref || !est || B <= 0 || n <= 0 || n > 4 || L <= 0 || perm_by < 0 || perm_by > 1)
      fail(DSN_EINVAL, "%s: bad arguments (n <= 4, perm_by 0|1)", who);
    if (ragged) check_item_lens(who, lens, B, L);
    hipStream_t st = (hipStream_t)stream;
    const size_t cnt = (size_t)B * n * n * 3;
    double* dd = ctx->wsbuf<double>("sibss", (long)cnt * 2);
    std::vector<int> hl;
    const int* dlens = nullptr;
    if (ragged) {
      hl.assign(lens, lens + B);
      dlens = upload_item_ints(ctx, "sibss_lens", hl, st);
    }
    launch_sisdr_dots(ref, est, B, n, L, dlens, dd, st);
    launch_sisdr_dots(ref, ref, B, n, L, dlens, dd + cnt, st);
    std::vector<double> h(cnt * 2);
    HIPCHK(hipMemcpyAsync(h.data(), dd, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const double clamp = clamp_db > 0 ? clamp_db : 1e30, tiny = 1e-300;
    auto db = [&](double num, double den) {
      double v = 10.0 * log10(std::max(num, tiny) / std::max(den, tiny));
      return std::min(clamp, std::max(-clamp, v));
    };
    for (int b = 0; b < B; ++b) {
      double G[4][4], X[4][4], ee[4], sdr[4][4], sir[4][4], sar[4];
      for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
          const double* v = &h[(((size_t)b * n + i) * n + j) * 3];
          X[i][j] = v[0];
          ee[j] = v[2];
          G[i][j] = h[cnt + (((size_t)b * n + i) * n + j) * 3];
        }
      for (int j = 0; j < n; ++j) {
        // solve G c = X[:, j] by Gaussian elimination with partial pivoting (fp64, n <= 4).  A column without a pivot
        // (a reference inside the span of the earlier ones, as with fewer samples than sources) keeps the coefficient
        // 0: the system is consistent, so the rest still gives the projection on the span.  With full rank the
        // arithmetic is the plain elimination's.
        double A[4][5], gmax = 0.0;
        for (int r = 0; r < n; ++r) {
          for (int c = 0; c < n; ++c) A[r][c] = G[r][c];
          A[r][n] = X[r][j];
          gmax = std::max(gmax, G[r][r]);
        }
        const double floor_ = std::max(1e-300, 1e-14 * gmax);
        int pcol[4], rank = 0;
        for (int c = 0; c < n; ++c) {
          int piv = rank;
          for (int r = rank + 1; r < n; ++r)
            if (fabs(A[r][c]) > fabs(A[piv][c])) piv = r;
          if (fabs(A[piv][c]) < floor_) continue;
          if (piv != rank)
            for (int k = 0; k <= n; ++k) std::swap(A[piv][k], A[rank][k]);
          for (int r = rank + 1; r < n; ++r) {
            const double f = A[r][c] / A[rank][c];
            for (int k = c; k <= n; ++k) A[r][k] -= f * A[rank][k];
          }
          pcol[rank++] = c;
        }
        double cvec[4] = {0, 0, 0, 0}, pe = 0;
        for (int r = rank - 1; r >= 0; --r) {
          double acc = A[r][n];
          for (int q = r + 1; q < rank; ++q) acc -= A[r][pcol[q]] * cvec[pcol[q]];
          cvec[pcol[r]] = acc / A[r][pcol[r]];
        }
        for (int k = 0; k < n; ++k) pe += cvec[k] * X[k][j];  // |P est_j|^2 = c^T G c = c^T x
        pe = std::min(std::max(pe, 0.0), ee[j]);
        sar[j] = db(pe, ee[j] - pe);
        for (int i = 0; i < n; ++i) {
          const double et = G[i][i] > 0 ? X[i][j] * X[i][j] / G[i][i] : 0.0;  // |e_target|^2
          sdr[i][j] = db(et, ee[j] - et);
          sir[i][j] = db(et, pe - et);
        }
      }
      const std::vector<int> bestp = best_permutation(n, [&](const std::vector<int>& p) {
        double sc = 0;
        for (int i = 0; i < n; ++i) sc += perm_by ? sir[i][p[i]] : sdr[i][p[i]];
        return sc;
      });
      for (int i = 0; i < n; ++i) {
        const size_t o = (size_t)b * n + i;
        if (si_sdr_out) si_sdr_out[o] = (float)sdr[i][bestp[i]];
        if (si_sir_out) si_sir_out[o] = (float)sir[i][bestp[i]];
        if (si_sar_out) si_sar_out[o] = (float)sar[bestp[i]];
        if (perm_out) perm_out[o] = bestp[i];
      }
    }
  });
}

int dsn_si_bss_eval(dsn_ctx* ctx, const float* ref, const float* est, int B, int n, int L, int perm_by, float clamp_db,
                    float* si_sdr_out, float* si_sir_out, float* si_sar_out, int* perm_out, void* stream) {
  return si_bss_eval_call(ctx, "dsn_si_bss_eval", ref, est, B, n, L, nullptr, false, perm_by, clamp_db, si_sdr_out,
                          si_sir_out, si_sar_out, perm_out, stream);
}
int dsn_si_bss_eval_ragged(dsn_ctx* ctx, const float* ref, const float* est, int B, int n, int L, const int32_t* lens,
                           int perm_by, float clamp_db, float* si_sdr_out, float* si_sir_out, float* si_sar_out,
                           int* perm_out, void* stream) {
  return si_bss_eval_call(ctx, "dsn_si_bss_eval_ragged", ref, est, B, n, L, lens, true, perm_by, clamp_db, si_sdr_out,
                          si_sir_out, si_sar_out, perm_out, stream);
}

// dsn_window_stitch's fade tables on the device: fall [O], then rise [O] from the next multiple of 4 floats (both
// 16-byte aligned).  fp64 on the host, rounded once to fp32 (native.fade_table restates it with the same libm sin).
// Uploaded only when (O, kind) or the buffer changed; the stream is drained before the host image is rewritten.
static void stitch_fade_tables(dsn_ctx* ctx, int O, int kind, hipStream_t st, const float** fall, const float** rise) {
  const long Oq = ((long)O + 3) & ~3L;
  auto& f = ctx->stitch_fade;
  float* dev = ctx->wsbuf<float>("stitch_fade", std::max(2 * Oq, 4L));
  if (f.dev != dev || f.O != O || f.kind != kind) {
    if (O > 0) {
      HIPCHK(hipStreamSynchronize(st));
      f.host.assign((size_t)(2 * Oq), 0.f);
      for (int k = 0; k < O; ++k) {
        double r;
        if (kind == DSN_FADE_LINEAR) {
          r = ((double)k + 0.5) / (double)O;
        } else {
          const double sn = sin(M_PI * ((double)k + 0.5) / (2.0 * (double)O));
          r = sn * sn;
        }
        f.host[k] = (float)(1.0 - r);
        f.host[Oq + k] = (float)r;
      }
      HIPCHK(hipMemcpyAsync(dev, f.host.data(), sizeof(float) * f.host.size(), hipMemcpyHostToDevice, st));
    }
    f.dev = dev;
    f.O = O;
    f.kind = kind;
  }
  *fall = dev;
  *rise = dev + Oq;
}

int dsn_window_stitch(dsn_ctx* ctx, const float* chunks, int W, int n, int Lw, int overlap, int L, int fade, int align,
                      float* out, int32_t* perm_out, double* gram_out, void* stream) {
  return guarded(ctx, [&] {
    const char* who = "dsn_window_stitch";
    if (!chunks || !out) fail(DSN_EINVAL, "%s: chunks or out is null", who);
    if (n < 1 || n > 4) fail(DSN_EINVAL, "%s: n = %d outside [1, 4]", who, n);
    if (W < 1) fail(DSN_EINVAL, "%s: W = %d < 1", who, W);
    if (Lw < 1) fail(DSN_EINVAL, "%s: Lw = %d < 1", who, Lw);
    if (overlap < 0) fail(DSN_EINVAL, "%s: overlap = %d < 0", who, overlap);
    if (2L * overlap > Lw)
      fail(DSN_EINVAL, "%s: 2 * overlap = %ld > Lw = %d (a sample may lie in at most two windows)", who, 2L * overlap,
           Lw);
    if (fade != DSN_FADE_HANN && fade != DSN_FADE_LINEAR)
      fail(DSN_EINVAL, "%s: fade = %d is neither 0 (hann) nor 1 (linear)", who, fade);
    const long hop = Lw - overlap, base = (long)(W - 1) * hop;
    if (W == 1 && (L < 1 || L > Lw)) fail(DSN_EINVAL, "%s: L = %d outside [1, Lw = %d] for W = 1", who, L, Lw);
    if (W > 1 && (L <= base + overlap || L > base + Lw))
      fail(DSN_EINVAL, "%s: L = %d outside (%ld, %ld] for W = %d windows of hop %ld", who, L, base + overlap, base + Lw,
           W, hop);
    hipStream_t st = (hipStream_t)stream;
    const long nb = W - 1, nn = (long)n * n;
    const int tiles = align ? stitch_tiles(overlap) : 0;
    double* part = ctx->wsbuf<double>("stitch_part", std::max(nb * tiles * nn, 1L));
    double* gram = ctx->wsbuf<double>("stitch_gram", std::max(nb * nn, 1L));
    int* perm = ctx->wsbuf<int>("stitch_perm", (long)W * n);
    const float *fall, *rise;
    stitch_fade_tables(ctx, overlap, fade, st, &fall, &rise);
    if (align) launch_stitch_gram(chunks, W, n, Lw, overlap, part, st);
    launch_stitch_perm(part, gram, perm, W, n, tiles, align, st);
    launch_stitch_gather(chunks, perm, fall, rise, out, W, n, Lw, overlap, L, st);
    HIPCHK(hipGetLastError());
    if (!perm_out && !gram_out) return;
    if (perm_out) HIPCHK(hipMemcpyAsync(perm_out, perm, sizeof(int32_t) * (size_t)W * n, hipMemcpyDeviceToHost, st));
    if (gram_out && align && nb > 0)
      HIPCHK(hipMemcpyAsync(gram_out, gram, sizeof(double) * (size_t)(nb * nn), hipMemcpyDeviceToHost, st));
    if (gram_out && !align) std::fill(gram_out, gram_out + nb * nn, 0.0);
    HIPCHK(hipStreamSynchronize(st));
  });
}

// ---- sinc resampling (resample_plan.h, resample.hip)
int dsn_resample_plan(int fs_in, int fs_out, int* orig, int* new_, int* width, int* support, int32_t* k0, float* taps) {
  char buf[128];
  if (resample_refusal(fs_in, fs_out, buf, sizeof buf)) return DSN_EINVAL;
  const ResamplePlan p = resample_plan(fs_in, fs_out);
  if (orig) *orig = p.o;
  if (new_) *new_ = p.n;
  if (width) *width = p.width;
  if (support) *support = p.S;
  if (k0) std::copy(p.k0.begin(), p.k0.end(), k0);
  if (taps) std::copy(p.c.begin(), p.c.end(), taps);
  return DSN_OK;
}

int dsn_resample_length(int fs_in, int fs_out, int L) {
  if (fs_in < 1 || fs_out < 1 || L < 0) return -1;
  const int g = std::gcd(fs_in, fs_out);
  return (int)resample_length(fs_in / g, fs_out / g, L);
}

// A host table on the device (workspace buffer `name`).  The stream is drained before the buffer is rewritten (an
// earlier call may still read it) and after the copy (the host image is the caller's local).
static const void* upload_table(dsn_ctx* ctx, const char* name, const void* h, size_t bytes, hipStream_t st) {
  char* d = ctx->wsbuf<char>(name, bytes);
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  return d;
}

// lens [B] (or null) on the device (workspace buffer `name`), drained as upload_table drains; a repeated call with the
// lengths the buffer already holds uploads nothing and drains nothing.
static const int* upload_lens_cached(dsn_ctx* ctx, const char* name, dsn_ctx::CachedLens& last, const int32_t* lens,
                                     int B, hipStream_t st) {
  if (!lens) return nullptr;
  std::vector<int> h(lens, lens + B);
  int* d = ctx->wsbuf<int>(name, B);
  if (h != last.host || d != last.dev) {
    HIPCHK(hipStreamSynchronize(st));   // (an earlier call on this stream may still read the buffer)
    HIPCHK(hipMemcpyAsync(d, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    last.host = h;
    last.dev = d;
  }
  return d;
}

// ---- what dsn_mask_refine, dsn_stems, dsn_beamform and dsn_dereverb refuse alike, each under the caller's name
static void check_stft(const char* who, int n_fft, int hop) {
  if (!mask_refine_fft_ok(n_fft)) fail(DSN_EINVAL, "%s: n_fft = %d is not a power of two in [64, 2048]", who, n_fft);
  if (hop < 1 || n_fft % hop != 0 || (n_fft / hop != 2 && n_fft / hop != 4 && n_fft / hop != 8))
    fail(DSN_EINVAL, "%s: n_fft / hop = %d / %d is not one of 2, 4, 8", who, n_fft, hop);
}

static void check_power(const char* who, int power) {
  if (power != 1 && power != 2) fail(DSN_EINVAL, "%s: power = %d is not 1 or 2", who, power);
}

static void check_eps(const char* who, float eps) {
  if (!std::isfinite(eps) || !(eps > 0.f)) fail(DSN_EINVAL, "%s: eps = %g is not a finite positive number", who, eps);
}

static void check_reg(const char* who, float reg) {
  if (!std::isfinite(reg) || reg < 0.f) fail(DSN_EINVAL, "%s: reg = %g is not a finite number >= 0", who, reg);
}

static void check_lmax(const char* who, int Lmax) {
  if (Lmax > (1 << 30)) fail(DSN_EINVAL, "%s: Lmax = %d > 2^30", who, Lmax);
}

// every item: lens[b] (null: Lmax) long enough for one reflection, channels[b] (null: C) in [1, C], *ref (null: the
// call has none) one of the item's channels
static void check_items(const char* who, int B, int Lmax, int n_fft, const int32_t* lens, const int32_t* channels, int C,
                        const int* ref) {
  const int need = n_fft / 2 + 1;
  for (int b = 0; b < B; ++b) {
    const int len = lens ? lens[b] : Lmax;
    if (len < need || len > Lmax)
      fail(DSN_EINVAL, "%s: item %d has %d samples, outside [n_fft / 2 + 1 = %d, Lmax = %d] (%d samples needed: one "
           "reflection must reach the item)", who, b, len, need, Lmax, need);
    const int cb = channels ? (int)channels[b] : C;
    if (cb < 1 || cb > C) fail(DSN_EINVAL, "%s: channels[%d] = %d outside [1, C = %d]", who, b, cb, C);
    if (ref && (*ref < 0 || *ref >= cb))
      fail(DSN_EINVAL, "%s: ref = %d outside [0, %d): item %d has %d channels", who, *ref, cb, b, cb);
    if (!lens && !channels) break;   // (every item is the first)
  }
}

// the items of one chunk under workspace_budget bytes (0: fallback), per_item bytes each; `unit` names what, with C,
// sizes an item ("n", "taps")
static int items_per_chunk(const char* who, int64_t workspace_budget, int64_t fallback, size_t per_item, int B, int C,
                           const char* unit, int units, int n_fft, int hop, int Lmax) {
  if (workspace_budget < 0) fail(DSN_EINVAL, "%s: workspace_budget = %ld < 0", who, (long)workspace_budget);
  const size_t fit = (size_t)(workspace_budget ? workspace_budget : fallback) / per_item;
  if (fit < 1)
    fail(DSN_EINVAL, "%s: workspace_budget = %ld bytes is smaller than one item (%ld bytes at C = %d, %s = %d, "
         "n_fft = %d, hop = %d, Lmax = %d)", who, (long)workspace_budget, (long)per_item, C, unit, units, n_fft, hop, Lmax);
  return (int)std::min<size_t>(fit, (size_t)B);
}

static bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  return (const char*)a < (const char*)b + nb && (const char*)b < (const char*)a + na;
}

// The tables of (orig, new) on the device.  Equal rates are the one-tap filter h = 1: a copy that honours lens and
// downmix.  Refuses a plan that does not fit the kernel's LDS before anything is allocated.
static const dsn_ctx::ResampleTables& resample_tables(dsn_ctx* ctx, const char* who, int fs_in, int fs_out) {
  const int g = std::gcd(fs_in, fs_out);
  const int o = fs_in / g, n = fs_out / g;
  auto it = ctx->resample_tables.find({o, n});
  if (it != ctx->resample_tables.end()) return it->second;
  char buf[256];
  // (a phase has at least 12 taps inside the window: a table that cannot fit is refused before it is computed)
  if (const char* why = resample_lds_refusal(o, n, o == n ? 1 : 13, o == n ? 1 : 12, buf, sizeof buf))
    fail(DSN_EINVAL, "%s: %s", who, why);
  dsn_ctx::ResampleTables t;
  if (o == n) {
    t.plan.k0.assign(1, 0);
    t.plan.c.assign(1, 1.f);
    t.plan.S = 1;
  } else {
    t.plan = resample_plan(fs_in, fs_out);
  }
  const ResamplePlan& p = t.plan;
  t.stride = p.S | 1;
  t.kmin = *std::min_element(p.k0.begin(), p.k0.end());
  t.kspan = *std::max_element(p.k0.begin(), p.k0.end()) + p.S - t.kmin;
  if (const char* why = resample_lds_refusal(p.o, p.n, t.stride, t.kspan, buf, sizeof buf))
    fail(DSN_EINVAL, "%s: %s", who, why);
  std::vector<float> padded((size_t)p.n * t.stride, 0.f);
  for (int ph = 0; ph < p.n; ++ph)
    std::copy(p.c.begin() + (size_t)ph * p.S, p.c.begin() + (size_t)(ph + 1) * p.S, padded.begin() + (size_t)ph * t.stride);
  t.taps = (float*)ctx->dmalloc(sizeof(float) * padded.size());
  t.k0 = (int*)ctx->dmalloc(sizeof(int) * p.k0.size());
  HIPCHK(hipMemcpy(t.taps, padded.data(), sizeof(float) * padded.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(t.k0, p.k0.data(), sizeof(int) * p.k0.size(), hipMemcpyHostToDevice));
  return ctx->resample_tables.emplace(std::make_pair(o, n), std::move(t)).first->second;
}

int dsn_resample(dsn_ctx* ctx, const float* x, int B, int C, int L, const int32_t* lens, int fs_in, int fs_out,
                 int downmix, float* out, int Lout, void* stream) {
  return guarded(ctx, [&] {
    const char* who = "dsn_resample";
    char buf[128];
    if (!x || !out) fail(DSN_EINVAL, "%s: x or out is null", who);
    if (const char* why = resample_refusal(fs_in, fs_out, buf, sizeof buf)) fail(DSN_EINVAL, "%s: %s", who, why);
    if (B < 1) fail(DSN_EINVAL, "%s: B = %d < 1", who, B);
    if (C < 1) fail(DSN_EINVAL, "%s: C = %d < 1", who, C);
    if (L < 1) fail(DSN_EINVAL, "%s: L = %d < 1", who, L);
    if ((long)B * C > 65535) fail(DSN_EINVAL, "%s: B * C = %ld > 65535 rows in one call", who, (long)B * C);
    for (int b = 0; lens && b < B; ++b)
      if (lens[b] < 1 || lens[b] > L)
        fail(DSN_EINVAL, "%s: sample count lens[%d] = %d outside [1, L = %d]", who, b, (int)lens[b], L);
    const int g = std::gcd(fs_in, fs_out);
    const long need = resample_length(fs_in / g, fs_out / g, L);
    if (need > INT32_MAX) fail(DSN_EINVAL, "%s: ceil(new * L / orig) = %ld does not fit 32 bits", who, need);
    if (Lout < need) fail(DSN_EINVAL, "%s: Lout = %d < ceil(new * L / orig) = %ld", who, Lout, need);
    const dsn_ctx::ResampleTables& t = resample_tables(ctx, who, fs_in, fs_out);
    hipStream_t st = (hipStream_t)stream;
    const int* dlens = upload_lens_cached(ctx, "resample_lens", ctx->resample_lens, lens, B, st);
    const ResamplePlan& p = t.plan;
    ctx->prof_launch("resample", 4.0 * ((double)B * C * L + (double)B * (downmix ? 1 : C) * Lout), st, [&] {
      launch_resample(x, dlens, t.taps, t.k0, out, B, C, L, Lout, p.o, p.n, p.width, p.S, t.stride, t.kmin, t.kspan,
                      downmix, st);
    });
    HIPCHK(hipGetLastError());
  });
}

// ---- mixture-consistent STFT masks (maskrefine.hip; include/ditsep_hip.h states the definition)
int dsn_mask_refine(dsn_ctx* ctx, const float* mix, const float* est, int B, int n, int Lmax, const int32_t* lens,
                    int n_fft, int hop, int power, float eps, float* out, void* stream) {
  return guarded(ctx, [&] {
    const char* who = "dsn_mask_refine";
    if (!mix || !est || !out) fail(DSN_EINVAL, "%s: mix, est or out is null", who);
    if (B < 1 || B > 65535) fail(DSN_EINVAL, "%s: B = %d outside [1, 65535]", who, B);
    if (n < 1 || n > MASK_REFINE_MAX_SRC) fail(DSN_EINVAL, "%s: n = %d outside [1, %d]", who, n, MASK_REFINE_MAX_SRC);
    check_stft(who, n_fft, hop);
    check_power(who, power);
    check_eps(who, eps);
    check_lmax(who, Lmax);
    check_items(who, B, Lmax, n_fft, lens, nullptr, 1, nullptr);
    const size_t row = sizeof(float) * (size_t)B * Lmax;
    if (overlaps(out, row * n, mix, row) || overlaps(out, row * n, est, row * n))
      fail(DSN_EINVAL, "%s: out overlaps mix or est (neighbouring workgroups read the samples around a span)", who);
    hipStream_t st = (hipStream_t)stream;
    const int* dlens = upload_lens_cached(ctx, "refine_lens", ctx->refine_lens, lens, B, st);
    ctx->prof_launch("mask_refine", 4.0 * (double)B * Lmax * (2 * n + 1), st, [&] {
      launch_mask_refine(mix, est, dlens, out, B, n, Lmax, n_fft, hop, power, eps, st);
    });
    HIPCHK(hipGetLastError());
  });
}

// ---- ensemble combine (ensemble.hip; include/ditsep_hip.h states the definition)
int dsn_ensemble_combine(dsn_ctx* ctx, const float* cands, const float* mix, int B, int K, int n, int Lmax,
                         const int32_t* lens, int mode, float* out, int32_t* perm_out, int32_t* anchor_out,
                         int32_t* best_out, double* resid_db_out, double* agree_db_out, double* gram_out, void* stream) {
  return guarded(ctx, [&] {
    const char* who = "dsn_ensemble_combine";
    if (!cands || !out) fail(DSN_EINVAL, "%s: cands or out is null", who);
    if (B < 1 || B > 65535) fail(DSN_EINVAL, "%s: B = %d outside [1, 65535]", who, B);
    if (K < 1 || K > ENSEMBLE_MAX_K) fail(DSN_EINVAL, "%s: K = %d outside [1, %d]", who, K, ENSEMBLE_MAX_K);
    if (n < 1 || n > ENSEMBLE_MAX_SRC) fail(DSN_EINVAL, "%s: n = %d outside [1, %d]", who, n, ENSEMBLE_MAX_SRC);
    if (Lmax < 1 || Lmax > (1 << 30)) fail(DSN_EINVAL, "%s: Lmax = %d outside [1, 2^30]", who, Lmax);
    if (mode < DSN_ENSEMBLE_MEAN || mode > DSN_ENSEMBLE_MEDOID)
      fail(DSN_EINVAL, "%s: mode = %d is not one of 0 (mean), 1 (median), 2 (best), 3 (medoid)", who, mode);
    if (mode == DSN_ENSEMBLE_BEST && !mix)
      fail(DSN_EINVAL, "%s: mode best ranks the candidates by their residual against the mixture: mix is null", who);
    for (int b = 0; lens && b < B; ++b)
      if (lens[b] < 1 || lens[b] > Lmax)
        fail(DSN_EINVAL, "%s: sample count lens[%d] = %d outside [1, Lmax = %d]", who, b, lens[b], Lmax);
    const char *c0 = (const char*)cands, *o0 = (const char*)out;
    const size_t row = sizeof(float) * (size_t)B * n * Lmax;
    if (o0 < c0 + row * K && c0 < o0 + row) fail(DSN_EINVAL, "%s: out overlaps cands", who);
    hipStream_t st = (hipStream_t)stream;
    const int* dlens = upload_lens_cached(ctx, "ensemble_lens", ctx->ensemble_lens, lens, B, st);
    const long R = (long)K * n + (mix ? 1 : 0), tiles = ensemble_tiles(Lmax);
    int RB, NB, S, SUBQ;
    ensemble_gram_plan((int)R, &RB, &NB, &S, &SUBQ);
    double* part = ctx->wsbuf<double>("ensemble_part", (size_t)B * tiles * NB * 16);
    // gram [B][R][R], resid_db [B][K], agree_db [B][K][n]; perm [B][K][n], anchor [B], best [B]
    double* gram = ctx->wsbuf<double>("ensemble_info", (size_t)B * (R * R + K + (long)K * n));
    double *resid = gram + (size_t)B * R * R, *agree = resid + (size_t)B * K;
    int* perm = ctx->wsbuf<int>("ensemble_perm", (size_t)B * ((long)K * n + 2));
    int *anchor = perm + (size_t)B * K * n, *best = anchor + B;
    const double bytes = 4.0 * (double)B * Lmax * ((double)K * n + (mix ? 1 : 0));
    ctx->prof_launch("ensemble_gram", bytes, st, [&] { launch_ensemble_gram(cands, mix, dlens, part, B, K, n, Lmax, st); });
    ctx->prof_launch("ensemble_solve", 8.0 * (double)B * tiles * NB * 16, st, [&] {
      launch_ensemble_solve(dlens, part, gram, perm, anchor, best, resid, agree, B, K, n, Lmax, mix ? 1 : 0, st);
    });
    const double rows = mode == DSN_ENSEMBLE_MEAN || mode == DSN_ENSEMBLE_MEDIAN ? K : 1;
    ctx->prof_launch("ensemble_gather", 4.0 * (double)B * n * Lmax * (rows + 1), st, [&] {
      launch_ensemble_gather(cands, dlens, perm, anchor, best, out, B, K, n, Lmax, mode, st);
    });
    HIPCHK(hipGetLastError());
    if (!perm_out && !anchor_out && !best_out && !resid_db_out && !agree_db_out && !gram_out) return;
    auto back = [&](void* dst, const void* src, size_t nbytes) {
      if (dst) HIPCHK(hipMemcpyAsync(dst, src, nbytes, hipMemcpyDeviceToHost, st));
    };
    back(perm_out, perm, sizeof(int32_t) * (size_t)B * K * n);
    back(anchor_out, anchor, sizeof(int32_t) * (size_t)B);
    back(best_out, best, sizeof(int32_t) * (size_t)B);
    back(resid_db_out, resid, sizeof(double) * (size_t)B * K);
    back(agree_db_out, agree, sizeof(double) * (size_t)B * K * n);
    back(gram_out, gram, sizeof(double) * (size_t)B * R * R);
    HIPCHK(hipStreamSynchronize(st));
  });
}

// ---- WAV payloads and the output gain (pcm.hip)
int dsn_pcm_decode(dsn_ctx* ctx, const void* bytes, int64_t nbytes, int B, const int64_t* offset, const int32_t* frames,
                   const int32_t* channels, const int32_t* encoding, int downmix, float* out, int Cout, int Lmax,
                   void* stream) {
  return guarded(ctx, [&] {
    const char* who = "dsn_pcm_decode";
    if (!bytes || !out) fail(DSN_EINVAL, "%s: bytes or out is null", who);
    if (!offset || !frames || !channels || !encoding)
      fail(DSN_EINVAL, "%s: offset, frames, channels or encoding is null", who);
    if (nbytes < 1) fail(DSN_EINVAL, "%s: nbytes = %ld < 1", who, (long)nbytes);
    if (B < 1 || B > 65535) fail(DSN_EINVAL, "%s: B = %d outside [1, 65535]", who, B);
    if (Lmax < 1) fail(DSN_EINVAL, "%s: Lmax = %d < 1", who, Lmax);
    if (Cout < 1) fail(DSN_EINVAL, "%s: Cout = %d < 1", who, Cout);
    if (downmix && Cout != 1) fail(DSN_EINVAL, "%s: downmix gives one channel, Cout = %d", who, Cout);
    std::vector<PcmItem> items((size_t)B);
    int widest = 1;
    for (int b = 0; b < B; ++b) {
      const int w = pcm_sample_bytes(encoding[b]);
      if (!w) fail(DSN_EINVAL, "%s: encoding[%d] = %d is none of DSN_PCM_U8 .. DSN_PCM_F64", who, b, (int)encoding[b]);
      if (channels[b] < 1) fail(DSN_EINVAL, "%s: channels[%d] = %d < 1", who, b, (int)channels[b]);
      if (!downmix && channels[b] > Cout)
        fail(DSN_EINVAL, "%s: channels[%d] = %d > Cout = %d without downmix", who, b, (int)channels[b], Cout);
      if ((long)channels[b] * w > DSN_PCM_MAX_FRAME_BYTES)
        fail(DSN_EINVAL, "%s: item %d has frames of %ld bytes, more than DSN_PCM_MAX_FRAME_BYTES = %d", who, b,
             (long)channels[b] * w, DSN_PCM_MAX_FRAME_BYTES);
      if (frames[b] < 1 || frames[b] > Lmax)
        fail(DSN_EINVAL, "%s: frames[%d] = %d outside [1, Lmax = %d]", who, b, (int)frames[b], Lmax);
      const long fb = (long)channels[b] * w, need = fb * frames[b];
      if (offset[b] < 0 || offset[b] > nbytes - need)
        fail(DSN_EINVAL, "%s: item %d takes bytes [%ld, %ld), outside [0, nbytes = %ld)", who, b, (long)offset[b],
             (long)offset[b] + need, (long)nbytes);
      items[b] = PcmItem{(long)offset[b], frames[b], channels[b], encoding[b], 0};
      widest = std::max(widest, (int)fb);
    }
    hipStream_t st = (hipStream_t)stream;
    const PcmItem* d = (const PcmItem*)upload_table(ctx, "pcm_items", items.data(), sizeof(PcmItem) * items.size(), st);
    ctx->prof_launch("pcm_decode", (double)nbytes + 4.0 * B * Cout * Lmax, st, [&] {
      launch_pcm_decode((const unsigned char*)bytes, (long)nbytes, d, B, downmix, out, Cout, Lmax, widest, st);
    });
    HIPCHK(hipGetLastError());
  });
}

// dsn_pcm_encode (C = 1, channels null) and dsn_pcm_encode_frames: x [R][C][Lmax] -> interleaved payloads
static void pcm_encode_rows(dsn_ctx* ctx, const char* who, const float* x, int R, int C, int Lmax, const int32_t* lens,
                            const int32_t* channels, int encoding, void* bytes, int64_t nbytes, const int64_t* offset,
                            int64_t* clipped, void* stream) {
  if (!x || !bytes) fail(DSN_EINVAL, "%s: x or bytes is null", who);
  if (!offset) fail(DSN_EINVAL, "%s: offset is null", who);
  if (R < 1 || R > 65535) fail(DSN_EINVAL, "%s: R = %d outside [1, 65535]", who, R);
  if (C < 1) fail(DSN_EINVAL, "%s: C = %d < 1", who, C);
  if (Lmax < 1) fail(DSN_EINVAL, "%s: Lmax = %d < 1", who, Lmax);
  if (encoding != DSN_PCM_S16 && encoding != DSN_PCM_S24 && encoding != DSN_PCM_F32)
    fail(DSN_EINVAL, "%s: encoding = %d is none of DSN_PCM_S16, DSN_PCM_S24, DSN_PCM_F32", who, encoding);
  const int w = pcm_sample_bytes(encoding);
  std::vector<PcmItem> items((size_t)R);
  std::vector<std::pair<long, int>> order((size_t)R);
  std::vector<long> need((size_t)R);
  for (int r = 0; r < R; ++r) {
    const int len = lens ? lens[r] : Lmax, ch = channels ? channels[r] : C;
    if (len < 1 || len > Lmax)
      fail(DSN_EINVAL, "%s: sample count lens[%d] = %d outside [1, Lmax = %d]", who, r, len, Lmax);
    if (ch < 1 || ch > C) fail(DSN_EINVAL, "%s: channels[%d] = %d outside [1, C = %d]", who, r, ch, C);
    if ((long)ch * w > DSN_PCM_MAX_FRAME_BYTES)
      fail(DSN_EINVAL, "%s: row %d has frames of %ld bytes, more than DSN_PCM_MAX_FRAME_BYTES = %d", who, r,
           (long)ch * w, DSN_PCM_MAX_FRAME_BYTES);
    need[r] = (long)len * ch * w;
    if (offset[r] < 0 || nbytes < need[r] || offset[r] > nbytes - need[r])
      fail(DSN_EINVAL, "%s: row %d takes bytes [%ld, %ld), outside [0, nbytes = %ld)", who, r, (long)offset[r],
           (long)offset[r] + need[r], (long)nbytes);
    items[r] = PcmItem{(long)offset[r], len, ch, encoding, 0};
    order[r] = {(long)offset[r], r};
  }
  std::sort(order.begin(), order.end());
  for (int k = 1; k < R; ++k) {
    const int p = order[k - 1].second, q = order[k].second;
    if (order[k - 1].first + need[p] > order[k].first)
      fail(DSN_EINVAL, "%s: the payloads of rows %d and %d overlap", who, p, q);
  }
  hipStream_t st = (hipStream_t)stream;
  const PcmItem* d = (const PcmItem*)upload_table(ctx, "pcm_rows", items.data(), sizeof(PcmItem) * items.size(), st);
  unsigned long long* cnt = ctx->wsbuf<unsigned long long>("pcm_clipped", R);
  HIPCHK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * (size_t)R, st));
  ctx->prof_launch(C == 1 && !channels ? "pcm_encode" : "pcm_encode_frames", (4.0 + w) * R * C * Lmax, st, [&] {
    launch_pcm_encode(x, d, R, C, Lmax, encoding, (unsigned char*)bytes, cnt, st);
  });
  HIPCHK(hipGetLastError());
  if (!clipped) return;
  HIPCHK(hipMemcpyAsync(clipped, cnt, sizeof(int64_t) * (size_t)R, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
}

int dsn_pcm_encode(dsn_ctx* ctx, const float* x, int R, int Lmax, const int32_t* lens, int encoding, void* bytes,
                   int64_t nbytes, const int64_t* offset, int64_t* clipped, void* stream) {
  return guarded(ctx, [&] {
    const char* who = "dsn_pcm_encode";
    if (!x || !bytes) fail(DSN_EINVAL, "%s: x or bytes is null", who);
    if (!lens || !offset) fail(DSN_EINVAL, "%s: lens or offset is null", who);
    pcm_encode_rows(ctx, who, x, R, 1, Lmax, lens, nullptr, encoding, bytes, nbytes, offset, clipped, stream);
  });
}

int dsn_pcm_encode_frames(dsn_ctx* ctx, const float* x, int R, int C, int Lmax, const int32_t* lens,
                          const int32_t* channels, int encoding, void* bytes, int64_t nbytes, const int64_t* offset,
                          int64_t* clipped, void* stream) {
  return guarded(ctx, [&] {
    pcm_encode_rows(ctx, "dsn_pcm_encode_frames", x, R, C, Lmax, lens, channels, encoding, bytes, nbytes, offset,
                    clipped, stream);
  });
}

int dsn_scale_output(dsn_ctx* ctx, const float* mix, const float* sep, int B, int n, int Lmax, const int32_t* lens,
                     float* out, float* alpha_out, void* stream) {
  return guarded(ctx, [&] {
    const char* who = "dsn_scale_output";
    if (!mix || !sep || !out) fail(DSN_EINVAL, "%s: mix, sep or out is null", who);
    if (B < 1) fail(DSN_EINVAL, "%s: B = %d < 1", who, B);
    if (n < 1) fail(DSN_EINVAL, "%s: n = %d < 1", who, n);
    if ((long)B * n > 65535) fail(DSN_EINVAL, "%s: B * n = %ld > 65535 rows in one call", who, (long)B * n);
    if (Lmax < 1) fail(DSN_EINVAL, "%s: Lmax = %d < 1", who, Lmax);
    for (int b = 0; lens && b < B; ++b)
      if (lens[b] < 1 || lens[b] > Lmax)
        fail(DSN_EINVAL, "%s: sample count lens[%d] = %d outside [1, Lmax = %d]", who, b, (int)lens[b], Lmax);
    hipStream_t st = (hipStream_t)stream;
    const long rows = (long)B * n;
    double* part = ctx->wsbuf<double>("scale_part", (size_t)(rows * scale_output_tiles(Lmax) * 2));
    float* alpha = ctx->wsbuf<float>("scale_alpha", (size_t)rows);
    const int* dlens = nullptr;
    if (lens) dlens = (const int*)upload_table(ctx, "scale_lens", lens, sizeof(int32_t) * (size_t)B, st);
    ctx->prof_launch("scale_output", 4.0 * (3.0 * rows + B) * Lmax, st, [&] {
      launch_scale_output(mix, sep, dlens, B, n, Lmax, part, alpha, out, st);
    });
    HIPCHK(hipGetLastError());
    if (!alpha_out) return;
    HIPCHK(hipMemcpyAsync(alpha_out, alpha, sizeof(float) * (size_t)rows, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  });
}

// ---- multichannel stems from mono estimates (maskrefine.hip; include/ditsep_hip.h states the definition)
int dsn_stems(dsn_ctx* ctx, const float* mix, const float* est, int B, int C, int n, int Lmax, const int32_t* lens,
              const int32_t* channels, int mode, int n_fft, int hop, int power, float eps, float reg, float* out,
              double* info_R, double* info_den, void* stream) {
  return guarded(ctx, [&] {
    const char* who = "dsn_stems";
    if (!mix || !est || !out) fail(DSN_EINVAL, "%s: mix, est or out is null", who);
    if (mode != DSN_STEMS_MASK && mode != DSN_STEMS_WIENER)
      fail(DSN_EINVAL, "%s: mode = %d is not one of 0 (DSN_STEMS_MASK), 1 (DSN_STEMS_WIENER)", who, mode);
    const int wiener = mode == DSN_STEMS_WIENER, Cmax = wiener ? STEMS_WIENER_MAX_CH : STEMS_MASK_MAX_CH;
    if (B < 1 || B > 65535) fail(DSN_EINVAL, "%s: B = %d outside [1, 65535]", who, B);
    if (C < 1 || C > Cmax)
      fail(DSN_EINVAL, "%s: C = %d outside [1, %d] (%s)", who, C, Cmax,
           wiener ? "DSN_STEMS_WIENER solves 1 x 1 and 2 x 2 systems" : "DSN_STEMS_MASK");
    if (n < 1 || n > MASK_REFINE_MAX_SRC) fail(DSN_EINVAL, "%s: n = %d outside [1, %d]", who, n, MASK_REFINE_MAX_SRC);
    check_stft(who, n_fft, hop);
    check_power(who, power);
    check_eps(who, eps);
    check_reg(who, reg);
    check_lmax(who, Lmax);
    check_items(who, B, Lmax, n_fft, lens, channels, C, nullptr);
    const size_t row = sizeof(float) * (size_t)B * Lmax;
    if (overlaps(out, row * n * C, mix, row * C) || overlaps(out, row * n * C, est, row * n))
      fail(DSN_EINVAL, "%s: out overlaps mix or est (neighbouring workgroups read the samples around a span)", who);
    hipStream_t st = (hipStream_t)stream;
    const int *dlens = nullptr, *dch = nullptr;
    if (lens) dlens = (const int*)upload_table(ctx, "stems_lens", lens, sizeof(int32_t) * (size_t)B, st);
    if (channels) dch = (const int*)upload_table(ctx, "stems_channels", channels, sizeof(int32_t) * (size_t)B, st);
    const size_t bins = (size_t)n_fft / 2 + 1, nR = (size_t)B * n * bins * C * C * 2, nd = (size_t)B * n * bins;
    double *part = nullptr, *R = nullptr, *den = nullptr;
    if (wiener) {
      part = ctx->wsbuf<double>("stems_part", (size_t)B * stems_stat_spans(n_fft, hop, Lmax) * n * 5 * bins);
      R = ctx->wsbuf<double>("stems_R", nR + nd);
      den = R + nR;
    }
    ctx->prof_launch(wiener ? "stems_wiener" : "stems_mask", 4.0 * (double)B * Lmax * (C + n + (double)n * C), st, [&] {
      launch_stems(mix, est, dlens, dch, out, part, R, den, B, C, n, Lmax, wiener, n_fft, hop, power, eps, reg, st);
    });
    HIPCHK(hipGetLastError());
    if (!info_R && !info_den) return;
    if (info_R) {
      if (wiener) HIPCHK(hipMemcpyAsync(info_R, R, sizeof(double) * nR, hipMemcpyDeviceToHost, st));
      else std::fill(info_R, info_R + nR, 0.0);
    }
    if (info_den) {
      if (wiener) HIPCHK(hipMemcpyAsync(info_den, den, sizeof(double) * nd, hipMemcpyDeviceToHost, st));
      else std::fill(info_den, info_den + nd, 0.0);
    }
    HIPCHK(hipStreamSynchronize(st));
  });
}

// ---- the design of the beamforming weights (beamform_design.hip): what the three _design calls and dsn_beamform_solve
// refuse alike
static void check_design(const char* who, int design, int sweeps) {
  if (design != DSN_BEAMFORM_DESIGN_SOUDEN && design != DSN_BEAMFORM_DESIGN_RANK1 && design != DSN_BEAMFORM_DESIGN_GEV)
    fail(DSN_EINVAL, "%s: design = %d is not one of 0 (DSN_BEAMFORM_DESIGN_SOUDEN), 1 (DSN_BEAMFORM_DESIGN_RANK1), 2 "
         "(DSN_BEAMFORM_DESIGN_GEV)", who, design);
  if (sweeps < 1 || sweeps > BEAMFORM_MAX_SWEEPS)
    fail(DSN_EINVAL, "%s: sweeps = %d outside [1, %d]", who, sweeps, BEAMFORM_MAX_SWEEPS);
}

// ---- mask-based MVDR beamforming (beamform.hip; include/ditsep_hip.h states the definition)
static int beamform_call(dsn_ctx* ctx, const char* who, const float* mix, const float* est, int B, int C, int n,
                         int Lmax, const int32_t* lens, const int32_t* channels, int ref, int n_fft, int hop, int power,
                         float eps, float reg, int design, int sweeps, int postfilter, int64_t workspace_budget,
                         float* out, double* info_w, void* stream) {
  return guarded(ctx, [&] {
    if (!mix || !est || !out) fail(DSN_EINVAL, "%s: mix, est or out is null", who);
    if (postfilter != DSN_BEAMFORM_POST_NONE && postfilter != DSN_BEAMFORM_POST_MASK)
      fail(DSN_EINVAL, "%s: postfilter = %d is not one of 0 (DSN_BEAMFORM_POST_NONE), 1 (DSN_BEAMFORM_POST_MASK)", who,
           postfilter);
    if (B < 1 || B > 65535) fail(DSN_EINVAL, "%s: B = %d outside [1, 65535]", who, B);
    if (C < 1 || C > BEAMFORM_MAX_CH) fail(DSN_EINVAL, "%s: C = %d outside [1, %d]", who, C, BEAMFORM_MAX_CH);
    if (n < 1 || n > MASK_REFINE_MAX_SRC) fail(DSN_EINVAL, "%s: n = %d outside [1, %d]", who, n, MASK_REFINE_MAX_SRC);
    check_stft(who, n_fft, hop);
    check_power(who, power);
    check_eps(who, eps);
    check_reg(who, reg);
    check_design(who, design, sweeps);
    check_lmax(who, Lmax);
    check_items(who, B, Lmax, n_fft, lens, channels, C, &ref);
    const int ipc = items_per_chunk(who, workspace_budget, BEAMFORM_DEFAULT_BUDGET,
                                    sizeof(double) * beamform_item_doubles(n_fft, hop, Lmax, C, n), B, C, "n", n, n_fft,
                                    hop, Lmax);
    const size_t row = sizeof(float) * (size_t)B * Lmax;
    if (overlaps(out, row * n, mix, row * C) || overlaps(out, row * n, est, row * n))
      fail(DSN_EINVAL, "%s: out overlaps mix or est (neighbouring workgroups read the samples around a span)", who);
    hipStream_t st = (hipStream_t)stream;
    const int *dlens = nullptr, *dch = nullptr;
    if (lens) dlens = (const int*)upload_table(ctx, "beamform_lens", lens, sizeof(int32_t) * (size_t)B, st);
    if (channels) dch = (const int*)upload_table(ctx, "beamform_channels", channels, sizeof(int32_t) * (size_t)B, st);
    const size_t bins = (size_t)n_fft / 2 + 1, T2 = (size_t)C * (C + 1), nw = (size_t)B * n * bins * C * 2;
    const size_t npart = (size_t)ipc * beamform_owners(n_fft, hop, Lmax) * n * T2 * bins;
    double* part = ctx->wsbuf<double>("beamform_part", npart + (size_t)ipc * n * T2 * bins);
    double* N = part + npart;
    double* w = ctx->wsbuf<double>("beamform_w", nw);
    ctx->prof_launch("beamform", 4.0 * (double)B * Lmax * ((double)C * (n + 1) + (postfilter ? 2.0 : 1.0) * n + n), st, [&] {
      for (int b0 = 0; b0 < B; b0 += ipc) {   // the chunk's partials are reused from chunk to chunk on the one stream
        const int items = std::min(ipc, B - b0);
        launch_beamform_weights(mix + (size_t)b0 * C * Lmax, est + (size_t)b0 * n * Lmax, dlens ? dlens + b0 : nullptr,
                                dch ? dch + b0 : nullptr, ref, part, N, w + (size_t)b0 * n * bins * C * 2, items, C, n,
                                Lmax, n_fft, hop, power, eps, reg, design, sweeps, st);
      }
      launch_beamform_apply(mix, est, dlens, dch, w, out, B, C, n, Lmax, n_fft, hop, power, eps,
                            postfilter == DSN_BEAMFORM_POST_MASK, st);
    });
    HIPCHK(hipGetLastError());
    if (!info_w) return;
    HIPCHK(hipMemcpyAsync(info_w, w, sizeof(double) * nw, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  });
}

int dsn_beamform(dsn_ctx* ctx, const float* mix, const float* est, int B, int C, int n, int Lmax, const int32_t* lens,
                 const int32_t* channels, int ref, int n_fft, int hop, int power, float eps, float reg, int postfilter,
                 int64_t workspace_budget, float* out, double* info_w, void* stream) {
  return beamform_call(ctx, "dsn_beamform", mix, est, B, C, n, Lmax, lens, channels, ref, n_fft, hop, power, eps, reg,
                       DSN_BEAMFORM_DESIGN_SOUDEN, BEAMFORM_DEFAULT_SWEEPS, postfilter, workspace_budget, out, info_w,
                       stream);
}

int dsn_beamform_design(dsn_ctx* ctx, const float* mix, const float* est, int B, int C, int n, int Lmax,
                        const int32_t* lens, const int32_t* channels, int ref, int n_fft, int hop, int power, float eps,
                        float reg, int design, int sweeps, int postfilter, int64_t workspace_budget, float* out,
                        double* info_w, void* stream) {
  return beamform_call(ctx, "dsn_beamform_design", mix, est, B, C, n, Lmax, lens, channels, ref, n_fft, hop, power, eps,
                       reg, design, sweeps, postfilter, workspace_budget, out, info_w, stream);
}

// the weights launch alone on the caller's statistics (device), one chunk
int dsn_beamform_solve(dsn_ctx* ctx, const double* N, const int32_t* channels, int ref, int items, int C, int n,
                       int classes, int bins, float reg, float eps, int design, int sweeps, double* w, void* stream) {
  return guarded(ctx, [&] {
    const char* who = "dsn_beamform_solve";
    if (!N || !w) fail(DSN_EINVAL, "%s: N or w is null", who);
    if (items < 1 || items > (1 << 24)) fail(DSN_EINVAL, "%s: items = %d outside [1, 2^24]", who, items);
    if (C < 1 || C > BEAMFORM_MAX_CH) fail(DSN_EINVAL, "%s: C = %d outside [1, %d]", who, C, BEAMFORM_MAX_CH);
    if (n < 1 || n > MASK_REFINE_MAX_SRC) fail(DSN_EINVAL, "%s: n = %d outside [1, %d]", who, n, MASK_REFINE_MAX_SRC);
    if (classes < n || classes > n + 1) fail(DSN_EINVAL, "%s: classes = %d is not n = %d or n + 1", who, classes, n);
    if (bins < 1 || bins > 1025) fail(DSN_EINVAL, "%s: bins = %d outside [1, 1025]", who, bins);
    if ((long)items * n * bins > (1L << 31))
      fail(DSN_EINVAL, "%s: items n bins = %d x %d x %d = %ld systems, more than the 2^31 one launch takes", who, items, n,
           bins, (long)items * n * bins);
    check_eps(who, eps);
    check_reg(who, reg);
    check_design(who, design, sweeps);
    for (int b = 0; b < items; ++b) {
      const int cb = channels ? (int)channels[b] : C;
      if (cb < 1 || cb > C) fail(DSN_EINVAL, "%s: channels[%d] = %d outside [1, C = %d]", who, b, cb, C);
      if (ref < 0 || ref >= cb)
        fail(DSN_EINVAL, "%s: ref = %d outside [0, %d): item %d has %d channels", who, ref, cb, b, cb);
      if (!channels) break;   // (every item is the first)
    }
    hipStream_t st = (hipStream_t)stream;
    const int* dch = nullptr;
    if (channels) dch = (const int*)upload_table(ctx, "beamform_channels", channels, sizeof(int32_t) * (size_t)items, st);
    ctx->prof_launch("beamform_solve", 8.0 * (double)items * bins * C * ((double)classes * (C + 1) + 2.0 * n), st, [&] {
      launch_beamform_solve(N, dch, ref, w, items, C, n, classes, bins, (double)reg, (double)eps, design, sweeps, st);
    });
    HIPCHK(hipGetLastError());
  });
}

// ---- block-adaptive MVDR weights (beamform_track.hip, beamform.hip; include/ditsep_hip.h states the definition)
static int track_call(dsn_ctx* ctx, const char* who, const float* mix, const float* est, int B, int C, int n, int Lmax,
                      const int32_t* lens, const int32_t* channels, int ref, int n_fft, int hop, int power, float eps,
                      float reg, int design, int sweeps, int postfilter, int block_frames, int context, int interpolate,
                      int64_t workspace_budget, float* out, double* info_w, void* stream) {
  return guarded(ctx, [&] {
    if (!mix || !est || !out) fail(DSN_EINVAL, "%s: mix, est or out is null", who);
    if (postfilter != DSN_BEAMFORM_POST_NONE && postfilter != DSN_BEAMFORM_POST_MASK)
      fail(DSN_EINVAL, "%s: postfilter = %d is not one of 0 (DSN_BEAMFORM_POST_NONE), 1 (DSN_BEAMFORM_POST_MASK)", who,
           postfilter);
    if (B < 1 || B > 65535) fail(DSN_EINVAL, "%s: B = %d outside [1, 65535]", who, B);
    if (C < 1 || C > BEAMFORM_MAX_CH) fail(DSN_EINVAL, "%s: C = %d outside [1, %d]", who, C, BEAMFORM_MAX_CH);
    if (n < 1 || n > MASK_REFINE_MAX_SRC) fail(DSN_EINVAL, "%s: n = %d outside [1, %d]", who, n, MASK_REFINE_MAX_SRC);
    if (block_frames < TRACK_MIN_BLOCK || block_frames > TRACK_MAX_BLOCK)
      fail(DSN_EINVAL, "%s: block_frames = %d outside [%d, 2^20]", who, block_frames, TRACK_MIN_BLOCK);
    if (context < 0 || context > TRACK_MAX_CONTEXT)
      fail(DSN_EINVAL, "%s: context = %d outside [0, %d]", who, context, TRACK_MAX_CONTEXT);
    if (interpolate != 0 && interpolate != 1) fail(DSN_EINVAL, "%s: interpolate = %d is not 0 or 1", who, interpolate);
    check_stft(who, n_fft, hop);
    check_power(who, power);
    check_eps(who, eps);
    check_reg(who, reg);
    check_design(who, design, sweeps);
    check_lmax(who, Lmax);
    check_items(who, B, Lmax, n_fft, lens, channels, C, &ref);
    const int Kmax = track_blocks(hop, Lmax, block_frames);
    if (Kmax > TRACK_MAX_BLOCKS)
      fail(DSN_EINVAL, "%s: %d blocks of block_frames = %d frames at Lmax = %d, hop = %d: more than %d", who, Kmax,
           block_frames, Lmax, hop, TRACK_MAX_BLOCKS);
    const size_t per_item = track_item_bytes(n_fft, hop, Lmax, C, n, block_frames);
    const int ipc = items_per_chunk(who, workspace_budget, TRACK_DEFAULT_BUDGET, per_item, B, C, "n", n, n_fft, hop, Lmax);
    const size_t row = sizeof(float) * (size_t)B * Lmax;
    if (overlaps(out, row * n, mix, row * C) || overlaps(out, row * n, est, row * n))
      fail(DSN_EINVAL, "%s: out overlaps mix or est (neighbouring workgroups read the samples around a span)", who);
    hipStream_t st = (hipStream_t)stream;
    const int *dlens = nullptr, *dch = nullptr;
    if (lens) dlens = (const int*)upload_table(ctx, "track_lens", lens, sizeof(int32_t) * (size_t)B, st);
    if (channels) dch = (const int*)upload_table(ctx, "track_channels", channels, sizeof(int32_t) * (size_t)B, st);
    const size_t bins = (size_t)n_fft / 2 + 1, T2 = (size_t)C * (C + 1);
    const size_t npart = (size_t)ipc * Kmax * n * T2 * bins, nw = (size_t)Kmax * n * bins * C * 2;   // (nw: per item)
    char* ws = ctx->wsbuf<char>("track_ws", per_item * ipc);   // part | N | w | the blocks' channel counts
    double* part = (double*)ws;
    double* N = part + npart;
    double* w = N + npart;
    int* blockch = (int*)(w + nw * ipc);
    for (int b0 = 0; b0 < B; b0 += ipc) {   // the chunk's workspace is reused from chunk to chunk on the one stream
      const int items = std::min(ipc, B - b0);
      const float *mixc = mix + (size_t)b0 * C * Lmax, *estc = est + (size_t)b0 * n * Lmax;
      const int *lensc = dlens ? dlens + b0 : nullptr, *chc = dch ? dch + b0 : nullptr;
      ctx->prof_launch("beamform_track",
                       4.0 * (double)items * Lmax * ((double)C * (n + 1) + (postfilter ? 2.0 : 1.0) * n + n), st, [&] {
        launch_track_weights(mixc, estc, lensc, chc, ref, part, N, w, blockch, items, C, n, Lmax, n_fft, hop, power, eps,
                             reg, block_frames, context, design, sweeps, st);
        launch_track_apply(mixc, estc, lensc, chc, w, out + (size_t)b0 * n * Lmax, items, C, n, Lmax, n_fft, hop, power,
                           eps, postfilter == DSN_BEAMFORM_POST_MASK, block_frames, interpolate, st);
      });
      HIPCHK(hipGetLastError());
      if (info_w) {
        HIPCHK(hipMemcpyAsync(info_w + (size_t)b0 * nw, w, sizeof(double) * nw * items, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
      }
    }
  });
}

int dsn_beamform_track(dsn_ctx* ctx, const float* mix, const float* est, int B, int C, int n, int Lmax,
                       const int32_t* lens, const int32_t* channels, int ref, int n_fft, int hop, int power, float eps,
                       float reg, int postfilter, int block_frames, int context, int interpolate,
                       int64_t workspace_budget, float* out, double* info_w, void* stream) {
  return track_call(ctx, "dsn_beamform_track", mix, est, B, C, n, Lmax, lens, channels, ref, n_fft, hop, power, eps,
                    reg, DSN_BEAMFORM_DESIGN_SOUDEN, BEAMFORM_DEFAULT_SWEEPS, postfilter, block_frames, context,
                    interpolate, workspace_budget, out, info_w, stream);
}

int dsn_beamform_track_design(dsn_ctx* ctx, const float* mix, const float* est, int B, int C, int n, int Lmax,
                              const int32_t* lens, const int32_t* channels, int ref, int n_fft, int hop, int power,
                              float eps, float reg, int design, int sweeps, int postfilter, int block_frames, int context,
                              int interpolate, int64_t workspace_budget, float* out, double* info_w, void* stream) {
  return track_call(ctx, "dsn_beamform_track_design", mix, est, B, C, n, Lmax, lens, channels, ref, n_fft, hop, power,
                    eps, reg, design, sweeps, postfilter, block_frames, context, interpolate, workspace_budget, out,
                    info_w, stream);
}

// ---- beamforming on spatially refined masks (spatial.hip, beamform.hip; include/ditsep_hip.h states the definition)
static int spatial_call(dsn_ctx* ctx, const char* who, const float* mix, const float* est, int B, int C, int n,
                        int Lmax, const int32_t* lens, const int32_t* channels, int ref, int n_fft, int hop, int power,
                        float eps, float reg, int design, int sweeps, int iterations, float noise, float floor,
                        float mask_reg, float mask_eps, int64_t workspace_budget, float* out, double* info_w,
                        double* info_gamma, int32_t* info_fail, void* stream) {
  return guarded(ctx, [&] {
    if (!mix || !est || !out) fail(DSN_EINVAL, "%s: mix, est or out is null", who);
    if (B < 1 || B > 65535) fail(DSN_EINVAL, "%s: B = %d outside [1, 65535]", who, B);
    if (C < 1 || C > BEAMFORM_MAX_CH) fail(DSN_EINVAL, "%s: C = %d outside [1, %d]", who, C, BEAMFORM_MAX_CH);
    if (n < 1 || n > MASK_REFINE_MAX_SRC) fail(DSN_EINVAL, "%s: n = %d outside [1, %d]", who, n, MASK_REFINE_MAX_SRC);
    if (iterations < 0 || iterations > SPATIAL_MAX_ITER)
      fail(DSN_EINVAL, "%s: iterations = %d outside [0, %d]", who, iterations, SPATIAL_MAX_ITER);
    if (!(noise >= 0.f && noise <= 0.9f)) fail(DSN_EINVAL, "%s: noise = %g outside [0, 0.9]", who, noise);
    if (!(floor >= 0.f && floor <= 1.f)) fail(DSN_EINVAL, "%s: floor = %g outside [0, 1]", who, floor);
    check_stft(who, n_fft, hop);
    check_power(who, power);
    check_eps(who, eps);
    check_reg(who, reg);
    check_design(who, design, sweeps);
    if (!std::isfinite(mask_reg) || mask_reg < 0.f)
      fail(DSN_EINVAL, "%s: mask_reg = %g is not a finite number >= 0", who, mask_reg);
    if (!std::isfinite(mask_eps) || !(mask_eps > 0.f))
      fail(DSN_EINVAL, "%s: mask_eps = %g is not a finite positive number", who, mask_eps);
    check_lmax(who, Lmax);
    check_items(who, B, Lmax, n_fft, lens, channels, C, &ref);
    const size_t per_item = spatial_item_bytes(n_fft, hop, Lmax, C, n);
    const int ipc = items_per_chunk(who, workspace_budget, SPATIAL_DEFAULT_BUDGET, per_item, B, C, "n", n, n_fft, hop,
                                    Lmax);
    const size_t row = sizeof(float) * (size_t)B * Lmax;
    if (overlaps(out, row * n, mix, row * C) || overlaps(out, row * n, est, row * n))
      fail(DSN_EINVAL, "%s: out overlaps mix or est (neighbouring workgroups read the samples around a span)", who);
    hipStream_t st = (hipStream_t)stream;
    const int *dlens = nullptr, *dch = nullptr;
    if (lens) dlens = (const int*)upload_table(ctx, "spatial_lens", lens, sizeof(int32_t) * (size_t)B, st);
    if (channels) dch = (const int*)upload_table(ctx, "spatial_channels", channels, sizeof(int32_t) * (size_t)B, st);
    const int K = noise > 0.f ? n + 1 : n;
    const size_t bins = (size_t)n_fft / 2 + 1, Fs = (size_t)spatial_frames(hop, Lmax);
    const size_t nw = (size_t)B * n * bins * C * 2, ng = (size_t)K * bins * Fs;   // (gamma: per item)
    char* ws = ctx->wsbuf<char>("spatial_ws", per_item * ipc);
    double* w = ctx->wsbuf<double>("spatial_w", nw);
    double* gamma = info_gamma ? ctx->wsbuf<double>("spatial_gamma", ng * ipc) : nullptr;
    for (int b0 = 0; b0 < B; b0 += ipc) {   // the chunk's workspace is reused from chunk to chunk on the one stream
      const int items = std::min(ipc, B - b0);
      ctx->prof_launch("beamform_spatial", 4.0 * (double)items * Lmax * (C + n), st, [&] {
        launch_spatial_statistics(mix + (size_t)b0 * C * Lmax, est + (size_t)b0 * n * Lmax,
                                  dlens ? dlens + b0 : nullptr, dch ? dch + b0 : nullptr, ws, gamma, items, C, n, K,
                                  Lmax, n_fft, hop, power, eps, iterations, (double)noise, (double)floor,
                                  (double)mask_reg, (double)mask_eps, st);
        launch_beamform_solve((const double*)ws, dch ? dch + b0 : nullptr, ref, w + (size_t)b0 * n * bins * C * 2, items,
                              C, n, K, (int)bins, (double)reg, (double)eps, design, sweeps, st);
      });
      HIPCHK(hipGetLastError());
      if (info_gamma)
        HIPCHK(hipMemcpyAsync(info_gamma + (size_t)b0 * ng, gamma, sizeof(double) * ng * items, hipMemcpyDeviceToHost,
                              st));
      if (info_fail) {   // (failed is the last array of the workspace)
        const char* failed = ws + (size_t)items * (per_item - 4 * bins);
        HIPCHK(hipMemcpyAsync(info_fail + (size_t)b0 * bins, failed, sizeof(int32_t) * items * bins,
                              hipMemcpyDeviceToHost, st));
      }
      if (info_gamma || info_fail) HIPCHK(hipStreamSynchronize(st));
    }
    ctx->prof_launch("beamform_spatial", 4.0 * (double)B * Lmax * (C + 2.0 * n), st, [&] {
      launch_beamform_apply(mix, est, dlens, dch, w, out, B, C, n, Lmax, n_fft, hop, power, eps, 0, st);
    });
    HIPCHK(hipGetLastError());
    if (!info_w) return;
    HIPCHK(hipMemcpyAsync(info_w, w, sizeof(double) * nw, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  });
}

int dsn_beamform_spatial(dsn_ctx* ctx, const float* mix, const float* est, int B, int C, int n, int Lmax,
                         const int32_t* lens, const int32_t* channels, int ref, int n_fft, int hop, int power, float eps,
                         float reg, int iterations, float noise, float floor, float mask_reg, float mask_eps,
                         int64_t workspace_budget, float* out, double* info_w, double* info_gamma, int32_t* info_fail,
                         void* stream) {
  return spatial_call(ctx, "dsn_beamform_spatial", mix, est, B, C, n, Lmax, lens, channels, ref, n_fft, hop, power, eps,
                      reg, DSN_BEAMFORM_DESIGN_SOUDEN, BEAMFORM_DEFAULT_SWEEPS, iterations, noise, floor, mask_reg,
                      mask_eps, workspace_budget, out, info_w, info_gamma, info_fail, stream);
}

int dsn_beamform_spatial_design(dsn_ctx* ctx, const float* mix, const float* est, int B, int C, int n, int Lmax,
                                const int32_t* lens, const int32_t* channels, int ref, int n_fft, int hop, int power,
                                float eps, float reg, int design, int sweeps, int iterations, float noise, float floor,
                                float mask_reg, float mask_eps, int64_t workspace_budget, float* out, double* info_w,
                                double* info_gamma, int32_t* info_fail, void* stream) {
  return spatial_call(ctx, "dsn_beamform_spatial_design", mix, est, B, C, n, Lmax, lens, channels, ref, n_fft, hop,
                      power, eps, reg, design, sweeps, iterations, noise, floor, mask_reg, mask_eps, workspace_budget,
                      out, info_w, info_gamma, info_fail, stream);
}

// ---- WPE dereverberation (dereverb.hip; include/ditsep_hip.h states the definition)
int dsn_dereverb(dsn_ctx* ctx, const float* mix, int B, int C, int Lmax, const int32_t* lens, const int32_t* channels,
                 int n_fft, int hop, int taps, int delay, int iterations, float reg, float eps, int64_t workspace_budget,
                 float* out, double* info_G, int32_t* info_fail, void* stream) {
  return guarded(ctx, [&] {
    const char* who = "dsn_dereverb";
    if (!mix || !out) fail(DSN_EINVAL, "%s: mix or out is null", who);
    if (B < 1 || B > 65535) fail(DSN_EINVAL, "%s: B = %d outside [1, 65535]", who, B);
    if (C < 1 || C > DEREVERB_MAX_CH) fail(DSN_EINVAL, "%s: C = %d outside [1, %d]", who, C, DEREVERB_MAX_CH);
    if (taps < 1 || taps > DEREVERB_MAX_TAPS)
      fail(DSN_EINVAL, "%s: taps = %d outside [1, %d]", who, taps, DEREVERB_MAX_TAPS);
    if (delay < 1 || delay > DEREVERB_MAX_DELAY)
      fail(DSN_EINVAL, "%s: delay = %d outside [1, %d]", who, delay, DEREVERB_MAX_DELAY);
    if (C * taps > DEREVERB_MAX_UNKNOWNS)
      fail(DSN_EINVAL, "%s: C taps = %d x %d = %d unknowns per bin, more than %d", who, C, taps, C * taps,
           DEREVERB_MAX_UNKNOWNS);
    if (iterations < 1 || iterations > DEREVERB_MAX_ITER)
      fail(DSN_EINVAL, "%s: iterations = %d outside [1, %d]", who, iterations, DEREVERB_MAX_ITER);
    check_stft(who, n_fft, hop);
    check_reg(who, reg);
    check_eps(who, eps);
    check_lmax(who, Lmax);
    check_items(who, B, Lmax, n_fft, lens, channels, C, nullptr);
    const size_t per_item = dereverb_item_bytes(n_fft, hop, Lmax, C, taps);
    const int ipc = items_per_chunk(who, workspace_budget, DEREVERB_DEFAULT_BUDGET, per_item, B, C, "taps", taps, n_fft,
                                    hop, Lmax);
    const size_t all = sizeof(float) * (size_t)B * C * Lmax;
    if (overlaps(out, all, mix, all))
      fail(DSN_EINVAL, "%s: out overlaps mix (the analysis of one chunk of items runs after the synthesis of another)",
           who);
    hipStream_t st = (hipStream_t)stream;
    const int *dlens = nullptr, *dch = nullptr;
    if (lens) dlens = (const int*)upload_table(ctx, "dereverb_lens", lens, sizeof(int32_t) * (size_t)B, st);
    if (channels) dch = (const int*)upload_table(ctx, "dereverb_channels", channels, sizeof(int32_t) * (size_t)B, st);
    const size_t bins = (size_t)n_fft / 2 + 1, gsz = bins * C * taps * C * 2;   // doubles of G per item
    char* ws = ctx->wsbuf<char>("dereverb_ws", per_item * ipc);
    std::vector<int32_t> flags;
    if (info_fail) flags.resize((size_t)ipc * bins);
    for (int b0 = 0; b0 < B; b0 += ipc) {   // the chunk's workspace is reused from chunk to chunk on the one stream
      const int items = std::min(ipc, B - b0);
      ctx->prof_launch("dereverb", 8.0 * (double)items * C * Lmax, st, [&] {
        launch_dereverb(mix + (size_t)b0 * C * Lmax, dlens ? dlens + b0 : nullptr, dch ? dch + b0 : nullptr, ws,
                        out + (size_t)b0 * C * Lmax, items, C, Lmax, n_fft, hop, taps, delay, iterations, (double)reg,
                        (double)eps, st);
      });
      HIPCHK(hipGetLastError());
      if (info_G)   // (G is the first array of the workspace)
        HIPCHK(hipMemcpyAsync(info_G + (size_t)b0 * gsz, ws, sizeof(double) * gsz * items, hipMemcpyDeviceToHost, st));
      if (info_fail) {
        const size_t Fs = (size_t)dereverb_frames(hop, Lmax), sys = (size_t)items * bins;
        const char* failed = ws + 8 * gsz * items + sys * (8 * Fs + 16 * C * Fs);
        HIPCHK(hipMemcpyAsync(flags.data(), failed, sizeof(int32_t) * sys, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int b = 0; b < items; ++b) {
          int32_t count = 0;
          for (size_t j = 0; j < bins; ++j) count += flags[(size_t)b * bins + j];
          info_fail[b0 + b] = count;
        }
      }
    }
    if (info_G || info_fail) HIPCHK(hipStreamSynchronize(st));
  });
}

// ---- loudness, true peak and the gain (loudness.hip; include/ditsep_hip.h states the definition)
int dsn_kweight_coeffs(int fs, double* out) {
  if (!out || fs < LOUD_MIN_RATE || fs > LOUD_MAX_RATE) return DSN_EINVAL;
  kweight_coeffs(fs, out);
  return DSN_OK;
}

// the refusals dsn_loudness and dsn_apply_gain share, and the rows as the kernels take them (h and rate left 0)
static std::vector<LoudItem> loudness_rows(const char* who, int B, int C, int Lmax, const int32_t* lens,
                                           const int32_t* channels) {
  if (B < 1 || B > 65535) fail(DSN_EINVAL, "%s: %d rows, outside [1, 65535]", who, B);
  if (C < 1 || C > LOUD_MAX_CH) fail(DSN_EINVAL, "%s: C = %d outside [1, %d]", who, C, LOUD_MAX_CH);
  if (Lmax < 1 || Lmax > (1 << 30)) fail(DSN_EINVAL, "%s: Lmax = %d outside [1, 2^30]", who, Lmax);
  std::vector<LoudItem> rows((size_t)B);
  for (int b = 0; b < B; ++b) {
    const int len = lens ? lens[b] : Lmax, ch = channels ? channels[b] : C;
    if (len < 1 || len > Lmax)
      fail(DSN_EINVAL, "%s: sample count lens[%d] = %d outside [1, Lmax = %d]", who, b, len, Lmax);
    if (ch < 1 || ch > C) fail(DSN_EINVAL, "%s: channels[%d] = %d outside [1, C = %d]", who, b, ch, C);
    rows[b] = LoudItem{len, ch, 0, 0};
  }
  return rows;
}

int dsn_loudness(dsn_ctx* ctx, const float* x, int B, int C, int Lmax, const int32_t* lens, const int32_t* channels,
                 const int32_t* rates, int want_true_peak, double* stats_host, void* stream) {
  return guarded(ctx, [&] {
    const char* who = "dsn_loudness";
    if (!x || !rates || !stats_host) fail(DSN_EINVAL, "%s: x, rates or stats_host is null", who);
    std::vector<LoudItem> items = loudness_rows(who, B, C, Lmax, lens, channels);
    std::vector<int> distinct;
    for (int b = 0; b < B; ++b) {
      if (rates[b] < LOUD_MIN_RATE || rates[b] > LOUD_MAX_RATE)
        fail(DSN_EINVAL, "%s: rates[%d] = %d Hz outside [%d, %d]", who, b, (int)rates[b], LOUD_MIN_RATE, LOUD_MAX_RATE);
      auto it = std::find(distinct.begin(), distinct.end(), (int)rates[b]);
      items[b].rate = (int)(it - distinct.begin());
      items[b].h = (rates[b] + 5) / 10;
      if (it == distinct.end()) distinct.push_back(rates[b]);
    }
    std::vector<LoudRate> table(distinct.size());
    for (size_t r = 0; r < distinct.size(); ++r) {
      kweight_coeffs(distinct[r], table[r].c);
      kweight_chunk_transition(table[r].c, table[r].P);
    }
    const dsn_ctx::ResampleTables& t = resample_tables(ctx, who, 1, 4);   // the true-peak interpolator
    hipStream_t st = (hipStream_t)stream;
    const long rows = (long)B * C, chunks = loudness_chunks(Lmax), segs = loudness_segments(Lmax);
    double* state = ctx->wsbuf<double>("loud_state", (size_t)(rows * chunks * 4));
    double* part = ctx->wsbuf<double>("loud_part", (size_t)(rows * chunks * 2));
    double* seg = ctx->wsbuf<double>("loud_seg", (size_t)(rows * segs + (long)B * 2 * segs));
    double* z = seg + rows * segs;
    double* stats = ctx->wsbuf<double>("loud_stats", (size_t)B * 6);
    unsigned long long* bad = ctx->wsbuf<unsigned long long>("loud_count", (size_t)B * 2);
    unsigned* peaks = (unsigned*)(bad + B);
    const LoudItem* ditems = (const LoudItem*)upload_table(ctx, "loud_items", items.data(), sizeof(LoudItem) * items.size(), st);
    const LoudRate* drates = (const LoudRate*)upload_table(ctx, "loud_rates", table.data(), sizeof(LoudRate) * table.size(), st);
    HIPCHK(hipMemsetAsync(bad, 0, sizeof(unsigned long long) * (size_t)B * 2, st));
    const ResamplePlan& p = t.plan;
    ctx->prof_launch("loudness", 4.0 * (double)rows * Lmax * (want_true_peak ? 3 : 2), st, [&] {
      launch_loudness(x, ditems, drates, B, C, Lmax, state, part, seg, z, peaks, bad, stats, t.taps, t.k0, p.S, t.stride,
                      t.kmin, t.kspan, p.width, want_true_peak, st);
    });
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(stats_host, stats, sizeof(double) * (size_t)B * 6, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  });
}

int dsn_apply_gain(dsn_ctx* ctx, const float* x, int R, int C, int Lmax, const int32_t* lens, const int32_t* channels,
                   const float* gain, float* out, void* stream) {
  return guarded(ctx, [&] {
    const char* who = "dsn_apply_gain";
    if (!x || !gain || !out) fail(DSN_EINVAL, "%s: x, gain or out is null", who);
    const std::vector<LoudItem> rows = loudness_rows(who, R, C, Lmax, lens, channels);
    const char *x0 = (const char*)x, *o0 = (const char*)out;
    const size_t bytes = sizeof(float) * (size_t)R * C * Lmax;
    if (o0 != x0 && o0 < x0 + bytes && x0 < o0 + bytes)
      fail(DSN_EINVAL, "%s: out overlaps x without being x (in place is fine, a shifted copy is not)", who);
    hipStream_t st = (hipStream_t)stream;
    const LoudItem* drows = (const LoudItem*)upload_table(ctx, "gain_rows", rows.data(), sizeof(LoudItem) * rows.size(), st);
    const float* dgain = (const float*)upload_table(ctx, "gain_values", gain, sizeof(float) * (size_t)R, st);
    ctx->prof_launch("apply_gain", 8.0 * (double)R * C * Lmax, st, [&] {
      launch_apply_gain(x, drows, dgain, out, R, C, Lmax, st);
    });
    HIPCHK(hipGetLastError());
  });
}

// ---- the true-peak look-ahead limiter (limiter.hip; include/ditsep_hip.h states the definition)
// W = max(1, floor(lookahead_ms fs / 1000 + 1/2)), or -1 when that is not in [1, LIM_MAX_W]
static int limiter_half_window(double lookahead_ms, int fs) {
  const double w = floor(lookahead_ms * (double)fs / 1000.0 + 0.5);
  if (!(lookahead_ms >= 0.0) || !(w <= (double)LIM_MAX_W)) return -1;
  return w < 1.0 ? 1 : (int)w;
}

static std::vector<LimRow> limiter_rows(const char* who, int R, int C, int Lmax, const int32_t* lens,
                                        const int32_t* channels, const int32_t* group, int G) {
  if (R < 1 || R > 65535) fail(DSN_EINVAL, "%s: %d rows, outside [1, 65535]", who, R);
  if (C < 1 || C > LOUD_MAX_CH) fail(DSN_EINVAL, "%s: C = %d outside [1, %d]", who, C, LOUD_MAX_CH);
  if (Lmax < 1 || Lmax > (1 << 30)) fail(DSN_EINVAL, "%s: Lmax = %d outside [1, 2^30]", who, Lmax);
  if (G < 1 || G > 65535) fail(DSN_EINVAL, "%s: %d groups, outside [1, 65535]", who, G);
  std::vector<LimRow> rows((size_t)R);
  for (int r = 0; r < R; ++r) {
    const int len = lens ? lens[r] : Lmax, ch = channels ? channels[r] : C;
    if (len < 1 || len > Lmax)
      fail(DSN_EINVAL, "%s: sample count lens[%d] = %d outside [1, Lmax = %d]", who, r, len, Lmax);
    if (ch < 1 || ch > C) fail(DSN_EINVAL, "%s: channels[%d] = %d outside [1, C = %d]", who, r, ch, C);
    if (group[r] < 0 || group[r] >= G) fail(DSN_EINVAL, "%s: group[%d] = %d outside [0, G = %d)", who, r, (int)group[r], G);
    rows[r] = LimRow{len, ch, (int)group[r], 0};
  }
  return rows;
}

int dsn_limiter_curve(dsn_ctx* ctx, const float* x, int R, int C, int Lmax, const int32_t* lens, const int32_t* channels,
                      const int32_t* rates, const int32_t* group, int G, const float* pregain, float ceiling,
                      double lookahead_ms, float* curve, float* envelope, double* stats_host, void* stream) {
  return guarded(ctx, [&] {
    const char* who = "dsn_limiter_curve";
    if (!x || !rates || !group || !pregain || !curve || !stats_host)
      fail(DSN_EINVAL, "%s: x, rates, group, pregain, curve or stats_host is null", who);
    if (R >= 1 && G > R) fail(DSN_EINVAL, "%s: %d groups of %d rows: every group needs a row", who, G, R);
    const std::vector<LimRow> rows = limiter_rows(who, R, C, Lmax, lens, channels, group, G);
    if (!std::isfinite(ceiling) || !(ceiling > 0.f))
      fail(DSN_EINVAL, "%s: the ceiling %g is not finite and positive", who, (double)ceiling);
    if (!std::isfinite(lookahead_ms)) fail(DSN_EINVAL, "%s: lookahead_ms = %g is not finite", who, lookahead_ms);
    std::vector<LimGroup> groups((size_t)G);
    std::vector<int> distinct;   // half-windows
    for (int r = 0; r < R; ++r) {
      if (rates[r] < LOUD_MIN_RATE || rates[r] > LOUD_MAX_RATE)
        fail(DSN_EINVAL, "%s: rates[%d] = %d Hz outside [%d, %d]", who, r, (int)rates[r], LOUD_MIN_RATE, LOUD_MAX_RATE);
      const int g = rows[r].group;
      if (r == 0 ? g != 0 : (g != rows[r - 1].group && g != rows[r - 1].group + 1))
        fail(DSN_EINVAL, "%s: group[%d] = %d: the groups must be 0 .. G - 1 in non-decreasing order", who, r, g);
      if (r > 0 && g == rows[r - 1].group) {
        if (rows[r].len != rows[r - 1].len || rates[r] != rates[r - 1])
          fail(DSN_EINVAL, "%s: rows %d and %d of group %d disagree on length or rate (%d at %d Hz, %d at %d Hz)", who,
               r - 1, r, g, rows[r - 1].len, (int)rates[r - 1], rows[r].len, (int)rates[r]);
        groups[g].row1 = r + 1;
        continue;
      }
      const int W = limiter_half_window(lookahead_ms, rates[r]);
      if (W < 0)
        fail(DSN_EINVAL, "%s: a look-ahead of %g ms at %d Hz is a half-window W outside [1, %d]", who, lookahead_ms,
             (int)rates[r], LIM_MAX_W);
      if (!std::isfinite(pregain[g])) fail(DSN_EINVAL, "%s: pregain[%d] = %g is not finite", who, g, (double)pregain[g]);
      auto it = std::find(distinct.begin(), distinct.end(), W);
      groups[g] = LimGroup{r, r + 1, rows[r].len, W, (int)(it - distinct.begin()), pregain[g]};
      if (it == distinct.end()) distinct.push_back(W);
    }
    if (rows[R - 1].group != G - 1) fail(DSN_EINVAL, "%s: the last row is of group %d, not G - 1 = %d", who, rows[R - 1].group, G - 1);
    // w[k] = (1/2 + 1/2 cos(pi k / (W + 1))) / (W + 1), k = -W .. W, in fp64 and rounded once
    const int wrow = 2 * LIM_MAX_W + 1;
    std::vector<float> window(distinct.size() * (size_t)wrow, 0.f);
    for (size_t i = 0; i < distinct.size(); ++i) {
      const int W = distinct[i];
      for (int k = -W; k <= W; ++k)
        window[i * wrow + (size_t)(k + W)] = (float)((0.5 + 0.5 * cos(M_PI * (double)k / (double)(W + 1))) / (double)(W + 1));
    }
    const int Wmax = *std::max_element(distinct.begin(), distinct.end());
    const dsn_ctx::ResampleTables& t = resample_tables(ctx, who, 1, 4);
    hipStream_t st = (hipStream_t)stream;
    float* req = ctx->wsbuf<float>("lim_req", (size_t)G * Lmax);
    unsigned long long* counts = ctx->wsbuf<unsigned long long>("lim_count", (size_t)G * 3);
    unsigned long long *bad = counts, *reduced = counts + G;
    unsigned* deepest = (unsigned*)(counts + 2 * (size_t)G);
    const LimRow* drows = (const LimRow*)upload_table(ctx, "lim_rows", rows.data(), sizeof(LimRow) * rows.size(), st);
    const LimGroup* dgroups = (const LimGroup*)upload_table(ctx, "lim_groups", groups.data(), sizeof(LimGroup) * groups.size(), st);
    const float* dwin = (const float*)upload_table(ctx, "lim_window", window.data(), sizeof(float) * window.size(), st);
    HIPCHK(hipMemsetAsync(counts, 0, sizeof(unsigned long long) * (size_t)G * 3, st));
    const ResamplePlan& p = t.plan;
    ctx->prof_launch("limiter_curve", 4.0 * ((double)R * C + 3.0 * G) * Lmax, st, [&] {
      launch_limiter_curve(x, drows, dgroups, G, C, Lmax, Wmax, ceiling, dwin, t.taps, t.k0, p.S, t.stride, t.kmin,
                           t.kspan, p.width, req, envelope, curve, bad, reduced, deepest, st);
    });
    HIPCHK(hipGetLastError());
    std::vector<unsigned long long> host((size_t)G * 3);
    HIPCHK(hipMemcpyAsync(host.data(), counts, sizeof(unsigned long long) * host.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const unsigned* deep = (const unsigned*)(host.data() + 2 * (size_t)G);
    for (int g = 0; g < G; ++g) {
      const uint32_t bits = 0x3f800000u - deep[g];
      float low;
      memcpy(&low, &bits, sizeof low);
      stats_host[3 * g] = host[g] ? (double)NAN : (double)low;
      stats_host[3 * g + 1] = (double)host[(size_t)G + g];
      stats_host[3 * g + 2] = (double)host[g];
    }
  });
}

int dsn_apply_curve(dsn_ctx* ctx, const float* x, int R, int C, int Lmax, const int32_t* lens, const int32_t* channels,
                    const int32_t* group, int G, const float* pregain, const float* curve, float* out, void* stream) {
  return guarded(ctx, [&] {
    const char* who = "dsn_apply_curve";
    if (!x || !group || !pregain || !curve || !out) fail(DSN_EINVAL, "%s: x, group, pregain, curve or out is null", who);
    // (the groups of these rows are the curve's: any order, and a group may have no row here)
    const std::vector<LimRow> rows = limiter_rows(who, R, C, Lmax, lens, channels, group, G);
    const char *x0 = (const char*)x, *o0 = (const char*)out;
    const size_t bytes = sizeof(float) * (size_t)R * C * Lmax;
    if (o0 != x0 && o0 < x0 + bytes && x0 < o0 + bytes)
      fail(DSN_EINVAL, "%s: out overlaps x without being x (in place is fine, a shifted copy is not)", who);
    hipStream_t st = (hipStream_t)stream;
    const LimRow* drows = (const LimRow*)upload_table(ctx, "curve_rows", rows.data(), sizeof(LimRow) * rows.size(), st);
    const float* dgain = (const float*)upload_table(ctx, "curve_pregain", pregain, sizeof(float) * (size_t)G, st);
    ctx->prof_launch("apply_curve", 4.0 * (2.0 * R * C + G) * Lmax, st, [&] {
      launch_apply_curve(x, drows, dgain, curve, out, R, C, Lmax, st);
    });
    HIPCHK(hipGetLastError());
  });
}

// ---- speaker activity of separated stems (activity.hip; include/ditsep_hip.h states the definition)
int dsn_activity(dsn_ctx* ctx, const float* est, int B, int n, int Lmax, const int32_t* lens, int n_fft, int hop, int j_lo,
                 int j_hi, int half_width, double c_r, double c_d, double c_r_stay, double c_d_stay, int min_on,
                 int min_off, int pad, uint8_t* act, int32_t* frames_on, double* energy, double* level, void* stream) {
  return guarded(ctx, [&] {
    const char* who = "dsn_activity";
    if (!est || !act || !frames_on || !energy || !level)
      fail(DSN_EINVAL, "%s: est, act, frames_on, energy or level is null", who);
    if (B < 1 || B > 65535) fail(DSN_EINVAL, "%s: B = %d outside [1, 65535]", who, B);
    if (n < 1 || n > MASK_REFINE_MAX_SRC) fail(DSN_EINVAL, "%s: n = %d outside [1, %d]", who, n, MASK_REFINE_MAX_SRC);
    check_stft(who, n_fft, hop);
    check_lmax(who, Lmax);
    check_items(who, B, Lmax, n_fft, lens, nullptr, 1, nullptr);
    if (j_lo < 0 || j_hi > n_fft / 2 || j_lo > j_hi)
      fail(DSN_EINVAL, "%s: the band of bins [%d, %d] is empty or outside [0, n_fft / 2 = %d]", who, j_lo, j_hi, n_fft / 2);
    if (half_width < 0 || half_width > ACTIVITY_MAX_HALF_WIDTH)
      fail(DSN_EINVAL, "%s: half_width = %d outside [0, %d]", who, half_width, ACTIVITY_MAX_HALF_WIDTH);
    const double c[4] = {c_r, c_d, c_r_stay, c_d_stay};
    const char* cn[4] = {"c_r", "c_d", "c_r_stay", "c_d_stay"};
    for (int k = 0; k < 4; ++k)
      if (!(c[k] >= 0.0 && c[k] <= 1.0)) fail(DSN_EINVAL, "%s: %s = %g outside [0, 1]", who, cn[k], c[k]);
    if (c_r_stay > c_r || c_d_stay > c_d)
      fail(DSN_EINVAL, "%s: a stay threshold above its on threshold (c_r %g -> %g, c_d %g -> %g): the hysteresis is "
           "negative", who, c_r, c_r_stay, c_d, c_d_stay);
    if (min_on < 1 || min_off < 1) fail(DSN_EINVAL, "%s: min_on = %d or min_off = %d < 1 frame", who, min_on, min_off);
    if (pad < 0) fail(DSN_EINVAL, "%s: pad = %d < 0", who, pad);
    const int Fmax = activity_frames(hop, Lmax);
    if (Fmax > ACTIVITY_MAX_FRAMES)
      fail(DSN_EINVAL, "%s: %d frames (Lmax = %d, hop = %d) > 2^22 per item", who, Fmax, Lmax, hop);
    hipStream_t st = (hipStream_t)stream;
    const int* dlens = nullptr;
    if (lens) dlens = (const int*)upload_table(ctx, "activity_lens", lens, sizeof(int32_t) * (size_t)B, st);
    ctx->prof_launch("activity", (double)B * n * (4.0 * Lmax + 42.0 * Fmax), st, [&] {
      launch_activity(est, dlens, B, n, Lmax, n_fft, hop, j_lo, j_hi, half_width, c_r, c_d, c_r_stay, c_d_stay, min_on,
                      min_off, pad, energy, level, act, frames_on, st);
    });
    HIPCHK(hipGetLastError());
  });
}

int dsn_activity_gate(dsn_ctx* ctx, const float* x, const uint8_t* act, int B, int n, int Lmax, int Fa,
                      const int32_t* lens, int hop, int fade, const float* ramp, float* out, void* stream) {
  return guarded(ctx, [&] {
    const char* who = "dsn_activity_gate";
    if (!x || !act || !out) fail(DSN_EINVAL, "%s: x, act or out is null", who);
    if (B < 1 || B > 65535) fail(DSN_EINVAL, "%s: B = %d outside [1, 65535]", who, B);
    if (n < 1 || n > MASK_REFINE_MAX_SRC) fail(DSN_EINVAL, "%s: n = %d outside [1, %d]", who, n, MASK_REFINE_MAX_SRC);
    if (Lmax < 1 || Lmax > (1 << 30)) fail(DSN_EINVAL, "%s: Lmax = %d outside [1, 2^30]", who, Lmax);
    if (hop < ACTIVITY_MIN_HOP || hop > ACTIVITY_MAX_HOP)
      fail(DSN_EINVAL, "%s: hop = %d outside [%d, %d]", who, hop, ACTIVITY_MIN_HOP, ACTIVITY_MAX_HOP);
    if (fade < 0 || fade > ACTIVITY_MAX_FADE) fail(DSN_EINVAL, "%s: fade = %d outside [0, %d]", who, fade, ACTIVITY_MAX_FADE);
    if (fade > 0 && !ramp) fail(DSN_EINVAL, "%s: fade = %d needs the ramp table: ramp is null", who, fade);
    for (int b = 0; lens && b < B; ++b)
      if (lens[b] < 1 || lens[b] > Lmax)
        fail(DSN_EINVAL, "%s: sample count lens[%d] = %d outside [1, Lmax = %d]", who, b, (int)lens[b], Lmax);
    const int need = (Lmax - 1 + hop / 2) / hop + 1;
    if (Fa < need)
      fail(DSN_EINVAL, "%s: act holds %d frames per row, %d needed for Lmax = %d at hop = %d", who, Fa, need, Lmax, hop);
    const char *x0 = (const char*)x, *o0 = (const char*)out;
    const size_t bytes = sizeof(float) * (size_t)B * n * Lmax;
    if (o0 != x0 && o0 < x0 + bytes && x0 < o0 + bytes)
      fail(DSN_EINVAL, "%s: out overlaps x without being x (in place is fine, a shifted copy is not)", who);
    hipStream_t st = (hipStream_t)stream;
    const int* dlens = nullptr;
    if (lens) dlens = (const int*)upload_table(ctx, "gate_lens", lens, sizeof(int32_t) * (size_t)B, st);
    const float* dramp = nullptr;
    if (fade > 0) {
      for (int d = 0; d < fade; ++d)
        if (!(ramp[d] >= 0.f && ramp[d] <= 1.f)) fail(DSN_EINVAL, "%s: ramp[%d] = %g outside [0, 1]", who, d, (double)ramp[d]);
      dramp = (const float*)upload_table(ctx, "gate_ramp", ramp, sizeof(float) * (size_t)fade, st);
    }
    ctx->prof_launch("activity_gate", (double)B * n * (8.0 * Lmax + Fa), st, [&] {
      launch_activity_gate(x, act, dlens, dramp, out, B, n, Lmax, Fa, hop, fade, st);
    });
    HIPCHK(hipGetLastError());
  });
}

// Modified Bessel function I0 by its power series sum_k ((x/2)^k / k!)^2 (numpy.kaiser's window function)
static double bessel_i0(double x) {
  double s = 1.0, t = 1.0;
  for (int k = 1; k < 500; ++k) {
    t *= (x / (2.0 * k)) * (x / (2.0 * k));
    s += t;
    if (t < s * 1e-17) break;
  }
  return s;
}

// The resampler pystoi.stoi applies when fs != 10000: scipy.signal.resample_poly(x, 10000, fs, window=h / sum(h))
// with h the Octave-style Kaiser-windowed sinc of pystoi.utils._resample_window_oct (60 dB rejection), designed in
// double precision.  resample_poly scales the window by `up` and aligns the output by n_pre_pad / n_pre_remove.
static constexpr int kStoiMaxTaps = 1 << 16;
static const dsn_ctx::StoiFilter& stoi_filter(dsn_ctx* ctx, int fs) {
  auto it = ctx->stoi_filters.find(fs);
  if (it != ctx->stoi_filters.end()) return it->second;
  const int g = std::gcd(10000, fs);
  const int p = 10000 / g, q = fs / g;
  const double cutoff = 1.0 / (2.0 * std::max(p, q));
  const double roll_off = cutoff / 10.0;
  const double Ld = ceil((60.0 - 8.0) / (28.714 * roll_off));
  if (2.0 * Ld + 1.0 > kStoiMaxTaps)
    fail(DSN_EINVAL, "dsn_stoi: fs = %d needs a %.0f-tap resampling filter (at most %d; 10000/fs reduces to %d/%d)", fs,
         2.0 * Ld + 1.0, kStoiMaxTaps, p, q);
  const int L = (int)Ld, ntaps = 2 * L + 1;
  const double beta = 0.1102 * (60.0 - 8.7), i0b = bessel_i0(beta);
  std::vector<double> h(ntaps);
  double sum = 0.0;
  for (int i = 0; i < ntaps; ++i) {
    const double t = i - L;
    const double r = t / L;
    const double win = bessel_i0(beta * sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
    const double xs = 2.0 * cutoff * t;
    const double sinc = t == 0 ? 1.0 : sin(M_PI * xs) / (M_PI * xs);
    h[i] = win * 2.0 * p * cutoff * sinc;
    sum += h[i];
  }
  for (double& v : h) v = v / sum * p;
  dsn_ctx::StoiFilter f;
  f.ntaps = ntaps;
  f.up = p;
  f.down = q;
  f.n_pre_pad = q - L % q;
  f.n_pre_remove = (L + f.n_pre_pad) / q;
  f.taps = ctx->wsbuf<double>("stoi_taps_" + std::to_string(fs), ntaps);
  HIPCHK(hipMemcpy(f.taps, h.data(), sizeof(double) * ntaps, hipMemcpyHostToDevice));
  return ctx->stoi_filters[fs] = f;
}

// perm [B][n] (estimate perm[b*n + i] is scored against reference i) as the item map b*n + perm[b*n + i], uploaded to
// the workspace buffer `buf`; null when perm is null.  `who` prefixes the error of an entry outside [0, n).  The copy
// is asynchronous on `st` from `ymap`, which the caller keeps alive until it has synchronised.
static const int* upload_item_map(dsn_ctx* ctx, const char* who, const char* buf, const int* perm, int B, int n,
                                  std::vector<int>& ymap, hipStream_t st) {
  if (!perm) return nullptr;
  ymap.resize(B * n);
  for (int k = 0; k < B * n; ++k) {
    if (perm[k] < 0 || perm[k] >= n) fail(DSN_EINVAL, "%s: perm[%d] = %d outside [0, %d)", who, k, perm[k], n);
    ymap[k] = k / n * n + perm[k];
  }
  int* dmap = ctx->wsbuf<int>(buf, B * n);
  HIPCHK(hipMemcpyAsync(dmap, ymap.data(), sizeof(int) * ymap.size(), hipMemcpyHostToDevice, st));
  return dmap;
}

// STOI / ESTOI of every estimate against its reference (pystoi.stoi(ref, est, fs, extended), restated in
// tests/stoi_restatement.py).  Device: resampling, silent-frame removal, STFT envelopes and segment scores
// (stoi.hip); host: the filter design, the band table and the permutation map.
// dsn_stoi (lens null, ragged false) and dsn_stoi_ragged (`who` names the entry point in errors): with lens the host
// also derives every item's 10 kHz frame count, F_b = (ceil(lens[b] up / down) - 256) / 128 + 1 or 0, and uploads
// lens and F_b together ("stoi_lens": [2][B]); L sizes the buffers and grids.
static int stoi_call(dsn_ctx* ctx, const char* who, const float* ref, const float* est, int B, int n, int L,
                     const int32_t* lens, bool ragged, int fs, int extended, const int* perm, float* out,
                     int* frames_out, void* stream) {
  return guarded(ctx, [&] {
    if (!ref || !est || !out || B <= 0 || n <= 0 || L <= 0)
      fail(DSN_EINVAL, "%s: bad arguments (ref, est, out non-null, B, n, L > 0)", who);
    if (n > 4) fail(DSN_EINVAL, "%s: n = %d sources (at most 4)", who, n);
    if (fs <= 0) fail(DSN_EINVAL, "%s: fs = %d (must be positive)", who, fs);
    if (extended != 0 && extended != 1) fail(DSN_EINVAL, "%s: extended = %d (0 or 1)", who, extended);
    if (ragged) check_item_lens(who, lens, B, L);
    const int items = B * n;
    hipStream_t st = (hipStream_t)stream;
    std::vector<int> ymap, hl;
    const int* dmap = upload_item_map(ctx, who, "stoi_map", perm, B, n, ymap, st);
    const int* dlens = nullptr;  // [2][B]: samples, then 10 kHz frames
    auto frames_of = [](long n10) { return n10 >= 256 ? (int)((n10 - 256) / 128 + 1) : 0; };
    // the 10 kHz signals: the inputs themselves, or their resampled copies [2][items][n10]
    const float* xs = ref;
    const float* ys = est;
    const int* xymap = dmap;
    long n10 = L;
    int up = 1, down = 1;
    const dsn_ctx::StoiFilter* f = nullptr;
    if (fs != 10000) {
      f = &stoi_filter(ctx, fs);
      up = f->up;
      down = f->down;
      n10 = ((long)L * up + down - 1) / down;
      if (n10 > (1L << 30)) fail(DSN_EINVAL, "%s: %ld samples at 10 kHz (L = %d too long)", who, n10, L);
    }
    if (ragged) {
      hl.resize(2 * (size_t)B);
      for (int b = 0; b < B; ++b) {
        hl[b] = lens[b];
        hl[B + b] = frames_of(((long)lens[b] * up + down - 1) / down);
      }
      dlens = upload_item_ints(ctx, "stoi_lens", hl, st);
    }
    if (f) {
      float* rs = ctx->wsbuf<float>("stoi_rs", 2 * items * n10);
      launch_stoi_resample(ref, est, dmap, items, L, dlens, n, f->taps, f->ntaps, up, down, f->n_pre_pad,
                           f->n_pre_remove, (int)n10, rs, st);
      xs = rs;
      ys = rs + items * n10;
      xymap = nullptr;  // the resampler already placed est source perm[i] at row i
    }
    const int F = frames_of(n10);
    if (F == 0) {  // not one frame: no STFT frames at all
      HIPCHK(hipStreamSynchronize(st));  // the uploads above read ymap and hl
      for (int i = 0; i < items; ++i) {
        out[i] = 1e-5f;
        if (frames_out) frames_out[i] = 0;
      }
      return;
    }
    // one-third-octave bands of pystoi.utils.thirdoct: edges 150 * 2^((2k -+ 1)/6) Hz snapped to the nearest of the
    // bins linspace(0, 10000, 513)[:257] (first bin on a tie)
    StoiBands bands;
    for (int k = 0; k < 15; ++k)
      for (int e = 0; e < 2; ++e) {
        const double fe = 150.0 * pow(2.0, (2.0 * k + (e ? 1.0 : -1.0)) / 6.0);
        int best = 0;
        double bd = 1e300;
        for (int bin = 0; bin <= 256; ++bin) {
          const double d = bin * (10000.0 / 512.0) - fe;
          if (d * d < bd) {
            bd = d * d;
            best = bin;
          }
        }
        (e ? bands.hi : bands.lo)[k] = best;
      }
    const long Fs = std::max(F - 1, 1), Jmax = std::max(F - 30, 1);
    double* en = ctx->wsbuf<double>("stoi_en", (long)items * F);
    int* idx = ctx->wsbuf<int>("stoi_idx", (long)items * F);
    int* Kc = ctx->wsbuf<int>("stoi_K", items);
    double* tob = ctx->wsbuf<double>("stoi_tob", (long)items * 2 * 15 * Fs);
    double* part = ctx->wsbuf<double>("stoi_part", (long)items * Jmax);
    double* score = ctx->wsbuf<double>("stoi_score", items);
    int* frames = ctx->wsbuf<int>("stoi_frames", items);
    launch_stoi_frames(xs, ys, n10, xymap, items, F, dlens ? dlens + B : nullptr, n, bands, extended, en, idx, Kc, tob,
                       part, score, frames, st);
    HIPCHK(hipGetLastError());
    std::vector<double> hs(items);
    std::vector<int> hf(items);
    HIPCHK(hipMemcpyAsync(hs.data(), score, sizeof(double) * items, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hf.data(), frames, sizeof(int) * items, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < items; ++i) {
      out[i] = (float)hs[i];
      if (frames_out) frames_out[i] = hf[i];
    }
  });
}

int dsn_stoi(dsn_ctx* ctx, const float* ref, const float* est, int B, int n, int L, int fs, int extended,
             const int* perm, float* out, int* frames_out, void* stream) {
  return stoi_call(ctx, "dsn_stoi", ref, est, B, n, L, nullptr, false, fs, extended, perm, out, frames_out, stream);
}
int dsn_stoi_ragged(dsn_ctx* ctx, const float* ref, const float* est, int B, int n, int L, const int32_t* lens, int fs,
                    int extended, const int* perm, float* out, int* frames_out, void* stream) {
  return stoi_call(ctx, "dsn_stoi_ragged", ref, est, B, n, L, lens, true, fs, extended, perm, out, frames_out, stream);
}

// The window 0.5 (1 - cos(2 pi k / (win + 1))), k = 1 .. win, and the 25 critical-band filters of the WSS measure
// (Klatt 1982; centre frequencies and bandwidths in Hz as tabulated by Hu & Loizou's composite measure): Gaussians
// exp(-11 ((j - floor f0) / bw)^2 + ln(bw_min) - ln(bw_i)) over the FFT bins j < nfft / 2, entries at or below the
// -30 dB factor exp(-30 / (2 * 2.303)) dropped.  The cut is made here, once, in fp64.
static const dsn_ctx::CompositeTables& composite_tables(dsn_ctx* ctx, int fs, const CompositeShape& sh) {
  auto it = ctx->composite_tables.find(fs);
  if (it != ctx->composite_tables.end()) return it->second;
  static const double cent[COMPOSITE_BANDS] = {50.0,    120.0,   190.0,   260.0,   330.0,   400.0,   470.0,
                                               540.0,   617.372, 703.378, 798.717, 904.128, 1020.38, 1148.30,
                                               1288.72, 1442.54, 1610.70, 1794.16, 1993.93, 2211.08, 2446.71,
                                               2701.97, 2978.04, 3276.17, 3597.63};
  static const double bwid[COMPOSITE_BANDS] = {70.0,    70.0,    70.0,    70.0,    70.0,    70.0,    70.0,
                                               77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423,
                                               153.823, 168.154, 183.457, 199.776, 217.153, 235.631, 255.255,
                                               276.072, 298.126, 321.465, 346.136};
  const int n2 = sh.nfft / 2;
  const double max_freq = fs / 2.0, min_factor = exp(-30.0 / (2 * 2.303));
  dsn_ctx::CompositeTables t;
  std::vector<double> w;
  for (int i = 0; i < COMPOSITE_BANDS; ++i) {
    const double f0 = floor(cent[i] / max_freq * n2), bw = bwid[i] / max_freq * n2;
    const double norm = log(bwid[0]) - log(bwid[i]);
    t.bands.start[i] = 0;
    t.bands.len[i] = 0;
    t.bands.off[i] = (int)w.size();
    for (int j = 0; j < n2; ++j) {
      const double d = (j - f0) / bw, v = exp(-11.0 * (d * d) + norm);
      if (!(v > min_factor)) continue;
      if (t.bands.len[i] == 0) t.bands.start[i] = j;
      if (j != t.bands.start[i] + t.bands.len[i]) fail(DSN_EINVAL, "dsn_composite: band %d is not contiguous", i);
      ++t.bands.len[i];
      w.push_back(v);
    }
  }
  std::vector<double> win(sh.win);
  for (int k = 0; k < sh.win; ++k) win[k] = 0.5 * (1.0 - cos(2.0 * M_PI * ((k + 1.0) / (sh.win + 1.0))));
  t.win = ctx->wsbuf<double>("comp_win_" + std::to_string(fs), sh.win);
  t.bweights = ctx->wsbuf<double>("comp_bw_" + std::to_string(fs), (long)std::max<size_t>(w.size(), 1));
  HIPCHK(hipMemcpy(t.win, win.data(), sizeof(double) * sh.win, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(t.bweights, w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice));
  return ctx->composite_tables[fs] = t;
}

// LLR, WSS, segmental SNR and overall SNR of every estimate against its reference, and from them and a caller's PESQ
// the composite scores (the reference's src/evaluate/evaluate_covl.py, restated in tests/composite_restatement.py).
// Device: conditioning, the per-frame measures and their trimmed means (composite.hip); host: the window, the filter
// table, k = round(0.95 F), the permutation map and the composite arithmetic.
// dsn_composite (lens null, ragged false) and dsn_composite_ragged (`who` names the entry point in errors): with lens
// the host forms F and k for every item by the same two rules and uploads lens, F_b and k_b together ("comp_lens":
// [3][B]); L sizes the buffers and grids.
static int composite_call(dsn_ctx* ctx, const char* who, const float* ref, const float* est, int B, int n, int L,
                          const int32_t* lens, bool ragged, int fs, const int* perm, const float* pesq,
                          const DsnCompositeOut* out, void* stream) {
  return guarded(ctx, [&] {
    if (!ref || !est || !out || B <= 0 || n <= 0 || L <= 0)
      fail(DSN_EINVAL, "%s: bad arguments (ref, est, out non-null, B, n, L > 0)", who);
    if (n > 4) fail(DSN_EINVAL, "%s: n = %d sources (at most 4)", who, n);
    if ((long)B * n > 65535) fail(DSN_EINVAL, "%s: B * n = %ld items (at most 65535)", who, (long)B * n);
    CompositeShape sh;
    if (!composite_shape(fs, &sh)) fail(DSN_EINVAL, "%s: fs = %d (kernels exist for 8000 and 16000)", who, fs);
    if ((out->csig || out->cbak || out->covl) && !pesq) fail(DSN_EINVAL, "%s: csig / cbak / covl need pesq", who);
    // the reference's int(L / hop - win / hop); win = 4 hop at the supported rates
    auto frames_of = [&](int len) { return len / sh.hop - sh.win / sh.hop; };
    auto trimmed = [](int frames) { return (int)nearbyint(frames * 0.95); };  // Python's round(): half to even
    const int F = frames_of(L);
    if (F < 1)
      fail(DSN_EINVAL, "%s: L = %d is shorter than one frame (%d samples needed at fs = %d)", who, L,
           sh.win + sh.hop, fs);
    if (ragged) {
      check_item_lens(who, lens, B, L);
      for (int b = 0; b < B; ++b)
        if (frames_of(lens[b]) < 1)
          fail(DSN_EINVAL, "%s: item %d (lens[%d] = %d) is shorter than one frame (%d samples needed at fs = %d)", who,
               b, b, (int)lens[b], sh.win + sh.hop, fs);
    }
    const int k = trimmed(F);
    const int items = B * n;
    hipStream_t st = (hipStream_t)stream;
    std::vector<int> ymap, hl;
    const int* dmap = upload_item_map(ctx, who, "comp_map", perm, B, n, ymap, st);
    const int* dlens = nullptr;  // [3][B]: samples, frames, trimmed counts
    if (ragged) {
      hl.resize(3 * (size_t)B);
      for (int b = 0; b < B; ++b) {
        hl[b] = lens[b];
        hl[B + b] = frames_of(lens[b]);
        hl[2 * B + b] = trimmed(hl[B + b]);
      }
      dlens = upload_item_ints(ctx, "comp_lens", hl, st);
    }
    const dsn_ctx::CompositeTables& tab = composite_tables(ctx, fs, sh);
    double* cond = ctx->wsbuf<double>("comp_cond", (long)items * COMPOSITE_COND);
    double* fl = ctx->wsbuf<double>("comp_llr", (long)items * F);
    double* fw = ctx->wsbuf<double>("comp_wss", (long)items * F);
    double* fsn = ctx->wsbuf<double>("comp_ssnr", (long)items * F);
    double* res = ctx->wsbuf<double>("comp_out", (long)items * 3);
    launch_composite(fs, ref, est, dmap, items, L, F, k, dlens, dlens ? dlens + B : nullptr,
                     dlens ? dlens + 2 * B : nullptr, n, tab.win, tab.bands, tab.bweights, cond, fl, fw, fsn, res, st);
    HIPCHK(hipGetLastError());
    std::vector<double> hc((size_t)items * COMPOSITE_COND), hr((size_t)items * 3);
    HIPCHK(hipMemcpyAsync(hc.data(), cond, sizeof(double) * hc.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hr.data(), res, sizeof(double) * hr.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    auto mos = [](double v) { return std::isnan(v) ? v : std::min(std::max(v, 1.0), 5.0); };
    for (int i = 0; i < items; ++i) {
      // the composites are formed from the float results the caller sees
      const float l = (float)hr[3 * i], w = (float)hr[3 * i + 1], s = (float)hr[3 * i + 2];
      if (out->llr) out->llr[i] = l;
      if (out->wss) out->wss[i] = w;
      if (out->segsnr) out->segsnr[i] = s;
      if (out->snr) out->snr[i] = (float)hc[(size_t)i * COMPOSITE_COND + 3];
      if (out->frames) out->frames[i] = ragged ? hl[B + i / n] : F;
      if (pesq) {
        const double q = pesq[i];
        if (out->csig) out->csig[i] = (float)mos(3.093 - 1.029 * l + 0.603 * q - 0.009 * w);
        if (out->cbak) out->cbak[i] = (float)mos(1.634 + 0.478 * q - 0.007 * w + 0.063 * s);
        if (out->covl) out->covl[i] = (float)mos(1.594 + 0.805 * q - 0.512 * l - 0.007 * w);
      }
    }
  });
}

int dsn_composite(dsn_ctx* ctx, const float* ref, const float* est, int B, int n, int L, int fs, const int* perm,
                  const float* pesq, const DsnCompositeOut* out, void* stream) {
  return composite_call(ctx, "dsn_composite", ref, est, B, n, L, nullptr, false, fs, perm, pesq, out, stream);
}
int dsn_composite_ragged(dsn_ctx* ctx, const float* ref, const float* est, int B, int n, int L, const int32_t* lens,
                         int fs, const int* perm, const float* pesq, const DsnCompositeOut* out, void* stream) {
  return composite_call(ctx, "dsn_composite_ragged", ref, est, B, n, L, lens, true, fs, perm, pesq, out, stream);
}

// bss_eval SDR / SIR / SAR with F-tap distortion filters (include/ditsep_hip.h states the definition; restated in
// tests/bss_eval_restatement.py).  Device: everything from the correlations to the permutation (bss_eval.hip); host:
// the refusals, the chunking under the workspace budget (bss_eval_plan: the same chunk sizes dsn_bss_eval_plan
// reports, whatever sir_sar is) and one copy back.  Per-batch buffers (lens, perm, ee, Q, status, results) are small;
// the chunk's partials, lag tables and systems are reused from chunk to chunk on the one stream.
int dsn_bss_eval_plan(int B, int n, int L, int F, int64_t budget, int* tiles, int* M, int* items_per_chunk,
                      int64_t* workspace_bytes) {
  BssPlan p;
  if (!bss_eval_plan(B, n, L, F, budget, &p)) return DSN_EINVAL;
  if (tiles) *tiles = p.tiles;
  if (M) *M = p.M;
  if (items_per_chunk) *items_per_chunk = p.items_per_chunk;
  if (workspace_bytes) *workspace_bytes = p.per_item * p.items_per_chunk;
  return DSN_OK;
}

int dsn_bss_eval(dsn_ctx* ctx, const float* ref, const float* est, int B, int n, int L, const int32_t* lens,
                 const int* perm, const DsnBssEvalOpts* opts, const DsnBssEvalOut* out, void* stream) {
  return guarded(ctx, [&] {
    const char* who = "dsn_bss_eval";
    if (!ref || !est) fail(DSN_EINVAL, "%s: ref or est is null", who);
    if (!opts || !out || B <= 0 || L <= 0) fail(DSN_EINVAL, "%s: bad arguments (opts, out non-null, B, L > 0)", who);
    if (n < 1 || n > BSS_MAX_SRC) fail(DSN_EINVAL, "%s: n = %d outside [1, %d]", who, n, BSS_MAX_SRC);
    const int F = opts->filter_length;
    if (F < 1 || F > BSS_MAX_TAPS) fail(DSN_EINVAL, "%s: filter_length = %d outside [1, %d]", who, F, BSS_MAX_TAPS);
    if (!(opts->load_diag >= 0)) fail(DSN_EINVAL, "%s: load_diag = %g < 0", who, opts->load_diag);
    if (opts->perm_by < 0 || opts->perm_by > 1) fail(DSN_EINVAL, "%s: perm_by = %d (0 = SDR, 1 = SIR)", who, opts->perm_by);
    if (lens) check_item_lens(who, lens, B, L);
    if (perm)
      for (int k = 0; k < B * n; ++k)
        if (perm[k] < 0 || perm[k] >= n) fail(DSN_EINVAL, "%s: perm[%d] = %d outside [0, %d)", who, k, perm[k], n);
    if (opts->workspace_budget < 0) fail(DSN_EINVAL, "%s: workspace_budget = %ld < 0", who, (long)opts->workspace_budget);
    BssPlan plan;
    if (!bss_eval_plan(B, n, L, F, opts->workspace_budget, &plan)) {
      bss_eval_plan(1, n, L, F, 0, &plan);
      fail(DSN_EINVAL, "%s: workspace_budget = %ld bytes is smaller than one item (%ld bytes at n = %d, L = %d, "
           "filter_length = %d)", who, (long)opts->workspace_budget, (long)plan.per_item, n, L, F);
    }
    hipStream_t st = (hipStream_t)stream;
    const int full = opts->sir_sar != 0, ipc = plan.items_per_chunk;
    const long bn = (long)B * n;
    std::vector<int> hl, hp;
    const int *dlens = nullptr, *dperm = nullptr;
    if (lens) {
      hl.assign(lens, lens + B);
      dlens = upload_item_ints(ctx, "bss_lens", hl, st);
    }
    if (perm) {
      hp.assign(perm, perm + bn);
      dperm = upload_item_ints(ctx, "bss_perm", hp, st);
    }
    double* part = ctx->wsbuf<double>("bss_part", (size_t)ipc * plan.part);
    double* tab = ctx->wsbuf<double>("bss_tab", (size_t)ipc * plan.tab);
    double* mats = ctx->wsbuf<double>("bss_gram", (size_t)ipc * plan.mats);
    double* Q = ctx->wsbuf<double>("bss_q", (size_t)B * 32);
    double* ee = ctx->wsbuf<double>("bss_ee", (size_t)bn);
    // results: sdr, sir, sar [B n], then the two pair tables [B n n]
    double* res = ctx->wsbuf<double>("bss_out", (size_t)bn * (3 + 2 * n));
    int* ints = ctx->wsbuf<int>("bss_ints", (size_t)B + bn);  // status [B], perm_out [B n]
    HIPCHK(hipMemsetAsync(ints, 0, sizeof(int) * B, st));
    HIPCHK(hipMemsetAsync(Q, 0, sizeof(double) * B * 32, st));
    for (int item0 = 0; item0 < B; item0 += ipc) {
      const int items = std::min(ipc, B - item0);
      launch_bss_corr(ref, est, n, L, dlens, F, item0, items, plan, part, tab, ee, st);
      launch_bss_solve(tab, n, F, full, opts->load_diag, item0, items, plan, mats, Q, ints, st);
    }
    double *d_sdr = res, *d_sir = res + bn, *d_sar = res + 2 * bn, *d_sdrp = res + 3 * bn, *d_sirp = d_sdrp + bn * n;
    launch_bss_finish(Q, ee, ints, dperm, B, n, full, opts->perm_by, opts->clamp_db, d_sdr, d_sir, d_sar, d_sdrp, d_sirp,
                      ints + B, st);
    HIPCHK(hipGetLastError());
    const struct { void* host; const void* dev; size_t bytes; } copies[7] = {
        {out->sdr, d_sdr, sizeof(double) * bn},          {out->sir, d_sir, sizeof(double) * bn},
        {out->sar, d_sar, sizeof(double) * bn},          {out->sdr_pairs, d_sdrp, sizeof(double) * bn * n},
        {out->sir_pairs, d_sirp, sizeof(double) * bn * n}, {out->perm_out, ints + B, sizeof(int) * bn},
        {out->status, ints, sizeof(int) * B}};
    for (const auto& c : copies)
      if (c.host) HIPCHK(hipMemcpyAsync(c.host, c.dev, c.bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  });
}

// torch.hann_window(win) (periodic: 0.5 - 0.5 cos(2 pi k / win)) centred in fft zeros as torch.stft pads it,
// (fft - win) / 2 on the left.  The reference's window is a float32 tensor, so it is formed in float32 the way torch
// forms it (k times the rounded step, cos, times -0.5, plus 0.5): the leakage floor of a spectrum follows the window's
// rounding, and the log-magnitude term sees that floor.
static const float* mrstft_window(dsn_ctx* ctx, int fft, int win) {
  const long key = ((long)fft << 16) | win;
  auto it = ctx->mrstft_windows.find(key);
  if (it != ctx->mrstft_windows.end()) return it->second;
  std::vector<float> w(fft, 0.f);
  const int left = (fft - win) / 2;
  const float step = (float)(M_PI * 2.0 / (double)win);
  for (int k = 0; k < win; ++k) w[left + k] = win == 1 ? 1.f : cosf((float)k * step) * -0.5f + 0.5f;
  float* d = ctx->wsbuf<float>("mrstft_win_" + std::to_string(fft) + "_" + std::to_string(win), fft);
  HIPCHK(hipMemcpy(d, w.data(), sizeof(float) * fft, hipMemcpyHostToDevice));
  return ctx->mrstft_windows[key] = d;
}

// Pair tables of the multi-resolution STFT loss and of the L1 / L2 waveform losses (the reference's
// auraloss.py::MultiResolutionSTFTLoss and losses.py::L1Loss / MSELoss under PITLoss, restated in
// tests/mrstft_restatement.py).  Device: prefilter, spectra and every sum (mrstft.hip); host: the windows, the launch
// plan and the zeroing of the terms whose weight is zero.
// dsn_mrstft_loss (lens == null) and dsn_mrstft_loss_ragged (lens: HOST [B])
static int mrstft_call(dsn_ctx* ctx, const float* reals, const float* decoded, const int32_t* lens, bool ragged, int B,
                       int n, int L, const DsnMrstftConfig* cfg, const DsnMrstftOut* out, void* stream) {
  return guarded(ctx, [&] {
    if (!reals || !decoded || !cfg || !out || B <= 0 || n <= 0 || L <= 0)
      fail(DSN_EINVAL, "dsn_mrstft_loss: bad arguments (reals, decoded, cfg, out non-null, B, n, L > 0)");
    if (n > MRSTFT_MAX_SRC) fail(DSN_EINVAL, "dsn_mrstft_loss: n = %d sources (at most %d)", n, MRSTFT_MAX_SRC);
    if (B > 65535) fail(DSN_EINVAL, "dsn_mrstft_loss: B = %d items (at most 65535)", B);
    const int R = cfg->n_res;
    if (R < 0 || R > MRSTFT_MAX_RES) fail(DSN_EINVAL, "dsn_mrstft_loss: %d resolutions (0 .. %d)", R, MRSTFT_MAX_RES);
    if (R > 0 && (!cfg->fft || !cfg->hop || !cfg->win)) fail(DSN_EINVAL, "dsn_mrstft_loss: fft / hop / win missing");
    int max_fft = 0;
    for (int r = 0; r < R; ++r) {
      if (!mrstft_fft_ok(cfg->fft[r]))
        fail(DSN_EINVAL, "dsn_mrstft_loss: fft[%d] = %d (a power of two from 32 to 2048)", r, cfg->fft[r]);
      if (cfg->win[r] < 1 || cfg->win[r] > cfg->fft[r])
        fail(DSN_EINVAL, "dsn_mrstft_loss: win[%d] = %d outside [1, fft = %d]", r, cfg->win[r], cfg->fft[r]);
      if (cfg->hop[r] < 1) fail(DSN_EINVAL, "dsn_mrstft_loss: hop[%d] = %d (must be positive)", r, cfg->hop[r]);
      max_fft = std::max(max_fft, cfg->fft[r]);
    }
    if (L <= max_fft / 2)
      fail(DSN_EINVAL, "dsn_mrstft_loss: L = %d needs reflect padding of %d samples (L must exceed it)", L, max_fft / 2);
    if (ragged) {
      check_item_lens("dsn_mrstft_loss_ragged", lens, B, L);
      for (int b = 0; b < B; ++b)
        if (lens[b] <= max_fft / 2)
          fail(DSN_EINVAL, "dsn_mrstft_loss_ragged: lens[%d] = %d needs reflect padding of %d samples (it must exceed "
               "it)", b, lens[b], max_fft / 2);
    }
    const bool filter = R > 0 && cfg->taps != nullptr;
    if (filter && (cfg->n_taps < 1 || cfg->n_taps % 2 == 0 || cfg->n_taps > MRSTFT_MAX_TAPS))
      fail(DSN_EINVAL, "dsn_mrstft_loss: %d prefilter taps (odd, at most %d)", cfg->n_taps, MRSTFT_MAX_TAPS);
    hipStream_t st = (hipStream_t)stream;
    const long per = (long)B * n * n, sig = (long)B * n * L;
    MrstftPlan plan;
    plan.R = R;
    const std::vector<int> hl(lens, lens + (ragged ? B : 0));
    for (int r = 0; r < R; ++r)
      mrstft_plan_resolution(&plan, r, cfg->fft[r], cfg->hop[r], B, L, ragged ? hl.data() : nullptr);
    const long nparts = R ? plan.off[R - 1] + (long)B * plan.wgs[R - 1] * MRSTFT_SACC : 1;
    std::vector<const float*> wins(R);
    for (int r = 0; r < R; ++r) wins[r] = mrstft_window(ctx, cfg->fft[r], cfg->win[r]);
    double* part = ctx->wsbuf<double>("mrstft_part", nparts);
    double* tpart = ctx->wsbuf<double>("mrstft_tpart", (long)B * mrstft_time_chunks(L) * MRSTFT_TACC);
    double* tabs = ctx->wsbuf<double>("mrstft_tables", per * (3 * std::max(R, 1) + 2));
    double *d_sc = tabs, *d_lg = tabs + per * std::max(R, 1), *d_lin = d_lg + per * std::max(R, 1);
    double *d_l1 = d_lin + per * std::max(R, 1), *d_l2 = d_l1 + per;
    float* dtaps = nullptr;
    double *xf = nullptr, *yf = nullptr;  // the prefiltered signals, fp64 (mrstft.hip says why)
    if (filter) {
      dtaps = ctx->wsbuf<float>("mrstft_taps", MRSTFT_MAX_TAPS);
      xf = ctx->wsbuf<double>("mrstft_filtered", 2 * sig);
      yf = xf + sig;
      HIPCHK(hipMemcpyAsync(dtaps, cfg->taps, sizeof(float) * cfg->n_taps, hipMemcpyHostToDevice, st));
    }
    // the lengths on the device (hl outlives the copy: the call ends with a synchronisation)
    const int* dl = ragged ? upload_item_ints(ctx, "mrstft_lens", hl, st) : nullptr;
    launch_mrstft_time(reals, decoded, B, n, L, dtaps, filter ? cfg->n_taps : 0, xf, yf, tpart, st, dl);
    for (int r = 0; r < R; ++r) launch_mrstft_spec(plan, r, reals, decoded, xf, yf, wins[r], B, n, L, part, st, dl);
    launch_mrstft_finish(plan, part, tpart, B, n, L, d_sc, d_lg, d_lin, d_l1, d_l2, st, dl);
    HIPCHK(hipGetLastError());
    // a term whose weight is zero is the reference's constant 0.0 (STFTLoss.forward skips it)
    const struct { double* host; const double* dev; long count; bool on; } copies[5] = {
        {out->sc, d_sc, per * R, cfg->w_sc != 0.f},
        {out->log_mag, d_lg, per * R, cfg->w_log_mag != 0.f},
        {out->lin_mag, d_lin, per * R, cfg->w_lin_mag != 0.f},
        {out->l1, d_l1, per, true},
        {out->l2, d_l2, per, true}};
    for (const auto& c : copies) {
      if (!c.host || c.count == 0) continue;
      if (c.on) HIPCHK(hipMemcpyAsync(c.host, c.dev, sizeof(double) * c.count, hipMemcpyDeviceToHost, st));
      else std::fill(c.host, c.host + c.count, 0.0);
    }
    HIPCHK(hipStreamSynchronize(st));
  });
}

int dsn_mrstft_loss(dsn_ctx* ctx, const float* reals, const float* decoded, int B, int n, int L,
                    const DsnMrstftConfig* cfg, const DsnMrstftOut* out, void* stream) {
  return mrstft_call(ctx, reals, decoded, nullptr, false, B, n, L, cfg, out, stream);
}

int dsn_mrstft_loss_ragged(dsn_ctx* ctx, const float* reals, const float* decoded, const int32_t* lens, int B, int n,
                           int L, const DsnMrstftConfig* cfg, const DsnMrstftOut* out, void* stream) {
  return mrstft_call(ctx, reals, decoded, lens, true, B, n, L, cfg, out, stream);
}

// Development hook: copy `count` floats of the named workspace buffer to host memory.
int dsn_debug_read(dsn_ctx* ctx, const char* name, float* host, int64_t count) {
  return guarded(ctx, [&] {
    auto it = ctx->ws.find(name);
    if (it == ctx->ws.end()) fail(DSN_EINVAL, "no workspace buffer '%s'", name);
    if ((size_t)count * sizeof(float) > it->second.second) fail(DSN_EINVAL, "buffer '%s' smaller than request", name);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(host, it->second.first, sizeof(float) * count, hipMemcpyDeviceToHost));
  });
}

int dsn_enable_graphs(dsn_ctx* ctx, int enable) {
  if (!ctx) return DSN_EINVAL;
  ctx->use_graphs = enable != 0;
  return DSN_OK;
}

int64_t dsn_workspace_bytes(const dsn_ctx* ctx) { return ctx ? ctx->ws_bytes() : 0; }

int dsn_profile_begin(dsn_ctx* ctx) {
  return guarded(ctx, [&] {
    for (auto& r : ctx->prof) {
      (void)hipEventDestroy(r.a);
      (void)hipEventDestroy(r.b);
    }
    ctx->prof.clear();
    ctx->profiling = true;
  });
}

int dsn_profile_end(dsn_ctx* ctx, double* gemm_ms, double* gemm_flops, int64_t* gemm_launches) {
  return guarded(ctx, [&] {
    HIPCHK(hipDeviceSynchronize());
    double ms = 0, fl = 0;
    int64_t n_gemm = 0;
    ctx->hbm_ms = ctx->hbm_bytes = 0;
    ctx->hbm_launches = 0;
    ctx->prof_rows.clear();
    std::map<std::string, size_t> row_of;
    for (auto& r : ctx->prof) {
      float t = 0;
      HIPCHK(hipEventElapsedTime(&t, r.a, r.b));
      if (r.gemm) {
        ms += t;
        fl += r.flops;
        ++n_gemm;
      }
      if (r.hbm_bound) {
        ctx->hbm_ms += t;
        ctx->hbm_bytes += r.hbm_bytes;
        ++ctx->hbm_launches;
      }
      auto it = row_of.find(r.tag);
      if (it == row_of.end()) {
        it = row_of.emplace(r.tag, ctx->prof_rows.size()).first;
        ctx->prof_rows.push_back(ProfRow());
        ctx->prof_rows.back().name = r.tag;
      }
      ProfRow& row = ctx->prof_rows[it->second];
      row.ms += t;
      row.flops += r.flops;
      row.bytes += r.hbm_bytes;
      ++row.launches;
      (void)hipEventDestroy(r.a);
      (void)hipEventDestroy(r.b);
    }
    if (gemm_ms) *gemm_ms = ms;
    if (gemm_flops) *gemm_flops = fl;
    if (gemm_launches) *gemm_launches = n_gemm;
    ctx->prof.clear();
    ctx->profiling = false;
  });
}

int dsn_profile_hbm(dsn_ctx* ctx, double* ms, double* bytes, int64_t* launches) {
  if (!ctx) return DSN_EINVAL;
  if (ms) *ms = ctx->hbm_ms;
  if (bytes) *bytes = ctx->hbm_bytes;
  if (launches) *launches = ctx->hbm_launches;
  return DSN_OK;
}

int dsn_profile_rows(dsn_ctx* ctx, int max_rows, char* names, double* ms, double* flops, double* bytes,
                     int64_t* launches) {
  if (!ctx) return DSN_EINVAL;
  const int n = (int)std::min<size_t>(ctx->prof_rows.size(), (size_t)std::max(0, max_rows));
  for (int i = 0; i < n; ++i) {
    const ProfRow& r = ctx->prof_rows[i];
    if (names) {
      strncpy(names + (size_t)i * DSN_PROFILE_NAME_LEN, r.name.c_str(), DSN_PROFILE_NAME_LEN - 1);
      names[(size_t)i * DSN_PROFILE_NAME_LEN + DSN_PROFILE_NAME_LEN - 1] = 0;
    }
    if (ms) ms[i] = r.ms;
    if (flops) flops[i] = r.flops;
    if (bytes) bytes[i] = r.bytes;
    if (launches) launches[i] = r.launches;
  }
  return (int)ctx->prof_rows.size();
}

// Test hook: the plan of one DiT score call, as finalize + dit_forward would decide it now (no context, no HIP call).
int dsn_dit_plan(const dsn_config* cfg, int B, int T, DsnDitPlan* out) {
  if (!cfg || !out || B <= 0 || T <= 0 || cfg->dit_embed_dim <= 0 || cfg->dit_heads <= 0) return DSN_EINVAL;
  const Switches sw = Switches::read();
  *out = dit_plan(*cfg, B, T, dit_fold_ln(*cfg, sw), dit_fold_ln8(*cfg, sw), sw, dit_limits());
  return DSN_OK;
}

// Test hook: one chosen kernel of the implicit-GEMM family on a caller-built descriptor (include/ditsep_hip.h).
int dsn_test_gemm(dsn_ctx* ctx, const DsnTestGemm* t, void* stream) {
  return guarded(ctx, [&] {
    hipStream_t st = (hipStream_t)stream;
    const int P = ctx->P, PL = ctx->PL;
    if (!t || !t->a || !t->w || t->a_numel % 4 != 0) fail(DSN_EINVAL, "test_gemm: operands missing or a_numel %% 4 != 0");
    const long wn = (long)t->N * t->taps * t->Cin;
    op16_t* ap = ctx->wsbuf<op16_t>("tg_a", t->a_numel * P);
    op16_t* wp = ctx->wsbuf<op16_t>("tg_w", wn * P);
    launch_to_planes(t->a, ap, t->a_numel, PL, t->a_numel, st);
    launch_to_planes(t->w, wp, wn, PL, wn, st);
    Packed pk = plain_packed(wp, wn, t->N, t->Cin, t->taps);
    pk.bias = const_cast<float*>(t->bias);
    pk.bias_mod = t->bias ? (t->bias_mod > 0 ? t->bias_mod : t->N) : 1;
    GemmDesc d = ctx->base_desc(ap + t->a_off, t->a_numel, pk, t->B, t->rows_per_b, t->Lin);
    if (t->M > 0) d.M = t->M;
    d.in_stride = t->in_stride;
    d.tap_dil = t->tap_dil;
    d.in_pad = t->in_pad;
    if (t->in_row_elems > 0) d.in_row_elems = t->in_row_elems;
    d.in_bstride = t->in_bstride > 0 ? t->in_bstride : (long)t->Lin * d.in_row_elems;
    d.img_h = t->img_h;
    d.img_w = t->img_w;
    const int n_out = t->swiglu ? t->N / 2 : t->N;
    d.out_row_elems = t->out_row_elems > 0 ? t->out_row_elems : n_out;
    d.out_bstride = t->out_bstride > 0 ? t->out_bstride : (long)t->rows_per_b * d.out_row_elems;
    d.out_off = t->out_off;
    d.out_limit = t->out_limit > 0 ? t->out_limit : d.out_bstride;
    d.bbias = t->bbias;
    d.bbias_stride = t->bbias_stride > 0 ? t->bbias_stride : t->N;
    d.resid = t->resid;
    d.resid_row_elems = t->resid_row_elems > 0 ? t->resid_row_elems : d.out_row_elems;
    d.resid_bstride = t->resid_bstride > 0 ? t->resid_bstride : (long)t->rows_per_b * d.resid_row_elems;
    d.resid_off = t->resid_off;
    d.out_scale = t->out_scale != 0.f ? t->out_scale : 1.f;
    d.f32_op = t->f32_op;
    d.act = t->act;
    d.act_a = t->act_a;
    d.act_b = t->act_b;
    d.act_mod = t->act_mod > 0 ? t->act_mod : t->N;
    d.swiglu = t->swiglu;
    d.gn_stats = t->gn_stats;
    d.gn_stats2 = t->gn_stats2;
    d.gn_nq2 = t->gn_nq2;
    d.gn_qoff2 = t->gn_qoff2;
    d.out_f32 = t->out_f32;
    d.out_planes = reinterpret_cast<op16_t*>(t->out_planes);
    d.out_ps = t->out_ps;
    if (t->sc_a) {
      if (!t->sc_w || t->sc_a_numel % 4 != 0) fail(DSN_EINVAL, "test_gemm: shortcut weight missing or sc_a_numel %% 4 != 0");
      const long sw = (long)t->N * t->sc_Cin;
      op16_t* sap = ctx->wsbuf<op16_t>("tg_sa", t->sc_a_numel * P);
      op16_t* swp = ctx->wsbuf<op16_t>("tg_sw", sw * P);
      launch_to_planes(t->sc_a, sap, t->sc_a_numel, PL, t->sc_a_numel, st);
      launch_to_planes(t->sc_w, swp, sw, PL, sw, st);
      d.sc_A = sap;
      d.sc_W = swp;
      d.sc_bias = t->sc_bias;
      d.sc_Cin = t->sc_Cin;
      d.sc_row_elems = t->sc_row_elems > 0 ? t->sc_row_elems : t->sc_Cin;
      d.sc_bstride = (long)t->rows_per_b * d.sc_row_elems;
    }
    const bool audit = ctx->sw.audit;
    auto check = [&](hipError_t e, const char* what) {
      if (e != hipSuccess) fail(DSN_EHIP, "test_gemm: %s refused or failed: %s (M=%d N=%d Cin=%d taps=%d)", what,
                                hipGetErrorString(e), d.M, d.N, d.Cin, d.taps);
    };
    switch (t->kernel) {
      case DSN_TG_AUTO:
        ctx->run(d, st);  // (audits when DSN_AUDIT is set)
        break;
      case DSN_TG_TILE:
        if (audit) ctx->audit_desc(d, false);
        check(igemm2_launch_cfg(d, PL, t->bm, t->bn, t->nst, t->bk, st), "igemm2 tile");
        break;
      case DSN_TG_V1:
        if (audit) ctx->audit_desc(d, false);
        check(igemm_launch(d, PL, st), "igemm v1");
        break;
      case DSN_TG_PANEL:
        d.panel_rows = t->panel_rows;
        d.panel_wm = t->panel_wm;
        d.cfg_nst = t->nst;
        d.cfg_bk = t->bk;
        if (audit) ctx->audit_desc(d, false);
        check(igemm_panel_launch(d, PL, t->panel_bn, st), "row-panel kernel");
        break;
      case DSN_TG_SKINNY:
        d.ksplit = std::max(t->ksplit, 1);
        d.slab_stride = t->slab_stride;
        if (audit) ctx->audit_desc(d, false);
        check(igemm_skinny_launch(d, PL, st), "skinny kernel");
        break;
      case DSN_TG_HALO:
        if (audit) ctx->audit_desc(d, false);
        check(igemm_halo3x3_launch(d, PL, st), "halo 3x3 kernel");
        break;
      case DSN_TG_SPLITK: {
        if (!t->slabs || t->ksplit < 2 || t->slab_stride <= 0) fail(DSN_EINVAL, "test_gemm: split-K needs slabs, ksplit >= 2");
        GemmDesc g = d;  // the GEMM: raw partial sums only
        g.ksplit = t->ksplit;
        g.slab_stride = t->slab_stride;
        g.out_f32 = t->slabs;
        g.out_planes = nullptr;
        g.gn_stats = g.gn_stats2 = nullptr;
        if (audit) {
          ctx->audit_desc(g, false);
          ctx->audit_desc(d, false);  // (the slab epilogue reads the slabs over the extent g writes)
        }
        check(igemm2_launch_cfg(g, PL, t->bm, t->bn, t->nst, t->bk, st), "igemm2 split-K tile");
        check(igemm_slab_epilogue_launch(d, PL, t->slabs, t->ksplit, t->slab_stride, st), "slab epilogue");
        break;
      }
      default:
        fail(DSN_EINVAL, "test_gemm: unknown kernel %d", t->kernel);
    }
    HIPCHK(hipGetLastError());
  });
}

// Test hook: one launch wrapper of the non-GEMM kernels with the caller's arguments (include/ditsep_hip.h).
int dsn_test_kernel(dsn_ctx* ctx, const DsnTestKernel* t, void* stream) {
  return guarded(ctx, [&] {
    hipStream_t st = (hipStream_t)stream;
    const int P = ctx->P, PL = ctx->PL;
    if (!t) fail(DSN_EINVAL, "test_kernel: null descriptor");
    // fp32 operand -> the engine's operand planes (plane stride = numel)
    auto planes_of = [&](const char* name, const float* src, long n) {
      if (!src || n <= 0 || n % 4 != 0) fail(DSN_EINVAL, "test_kernel: operand %s missing or its numel %% 4 != 0", name);
      op16_t* p = ctx->wsbuf<op16_t>(name, n * P);
      launch_to_planes(src, p, n, PL, n, st);
      return p;
    };
    op16_t* oplanes = reinterpret_cast<op16_t*>(t->out_planes);
    // ATTENTION / QKV_ATTENTION with `lens`: checked on the host (this synchronises the stream), then passed through
    auto checked_lens = [&](const char* who) -> const int* {
      if (!t->lens) return nullptr;
      std::vector<int32_t> h((size_t)t->B);
      HIPCHK(hipStreamSynchronize(st));
      HIPCHK(hipMemcpy(h.data(), t->lens, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost));
      for (int b = 0; b < t->B; ++b)
        if (h[b] < 1 || h[b] > t->S)
          fail(DSN_EINVAL, "test_kernel %s: lens[%d] = %d outside [1, S = %d]", who, b, (int)h[b], t->S);
      return reinterpret_cast<const int*>(t->lens);
    };
    switch (t->kind) {
      case DSN_TK_ATTENTION: {
        if (t->B < 1 || t->S < 1 || t->H < 1) fail(DSN_EINVAL, "test_kernel attention: B, S, H must be positive");
        const long D = (long)t->H * t->dh, n = (long)t->B * t->S * 3 * D;
        if (t->a_numel != n) fail(DSN_EINVAL, "test_kernel attention: a_numel %ld != B*S*3*H*dh = %ld", (long)t->a_numel, n);
        if (!!t->out_fp8 != !!t->out_fp8_scale || (!t->out_fp8 && !oplanes))
          fail(DSN_EINVAL, "test_kernel attention: needs out_planes, or out_fp8 with out_fp8_scale");
        if (t->out_fp8 && D % 32 != 0) fail(DSN_EINVAL, "test_kernel attention: fp8 output needs H*dh %% 32 == 0");
        const int* lens = checked_lens("attention");
        const op16_t* qkv = planes_of("tk_a", t->a, n);
        const hipError_t e = launch_attention_mfma(qkv, n, t->out_fp8 ? reinterpret_cast<op16_t*>(t->out_fp8) : oplanes,
                                                   t->out_ps, PL, t->B, t->S, t->H, t->dh, st, t->out_fp8_scale, lens);
        if (e == hipErrorNotSupported)
          fail(DSN_EINVAL, "test_kernel attention: unsupported head width %d%s", t->dh, lens ? " with lens (64 only)" : "");
        if (e != hipSuccess) fail(DSN_EHIP, "test_kernel attention: launch failed: %s", hipGetErrorString(e));
        break;
      }
      case DSN_TK_QKV_ATTENTION: {
        if (t->B < 1 || t->S < 1 || t->D < 4) fail(DSN_EINVAL, "test_kernel qkv_attention: B, S, D must be positive");
        const long M = (long)t->B * t->S;
        if (t->a_numel != M * t->D || t->w_numel != 3L * t->D * t->D)
          fail(DSN_EINVAL, "test_kernel qkv_attention: a_numel / w_numel do not match [B*S][D] / [3 D][D]");
        if (!t->rope_cos || !t->rope_sin) fail(DSN_EINVAL, "test_kernel qkv_attention: rope_cos / rope_sin [S][32] missing");
        const int* lens = checked_lens("qkv_attention");
        QkvAttnDesc q;
        memset(&q, 0, sizeof q);
        q.A = planes_of("tk_a", t->a, t->a_numel);
        q.W = planes_of("tk_w", t->w, t->w_numel);
        launch_rope_tables(t->rope_cos, t->rope_sin, t->S, 32, st);
        q.bias = t->bias;
        q.rope_cos = t->rope_cos;
        q.rope_sin = t->rope_sin;
        q.out = t->out_fp8 ? nullptr : oplanes;
        q.out8 = t->out_fp8;
        q.out8_scale = t->out_fp8_scale;
        q.M = (int)M;
        q.D = t->D;
        q.H = t->H;
        q.S = t->S;
        q.ipp = t->ipp;
        q.q_scale = 0.125f;
        const hipError_t e = qkv_attention_launch(q, PL, st, lens);
        if (e != hipSuccess)
          fail(DSN_EHIP, "test_kernel qkv_attention: refused or failed: %s (D=%d H=%d S=%d ipp=%d planes=%d)",
               hipGetErrorString(e), t->D, t->H, t->S, t->ipp, P);
        break;
      }
      case DSN_TK_RESIDUAL_NORM: {
        if (!t->x || t->rows < 1 || t->D < 4 || t->D % 4 != 0 || t->D > 4096)
          fail(DSN_EINVAL, "test_kernel residual_norm: needs x, rows >= 1, D %% 4 == 0, D <= 4096 (D=%d)", t->D);
        if (t->nslab < 0 || t->nslab > 8 || (t->nslab > 0 && !t->slabs))
          fail(DSN_EINVAL, "test_kernel residual_norm: nslab %d outside [0, 8] or slabs missing", t->nslab);
        if (t->do_norm && !t->gamma) fail(DSN_EINVAL, "test_kernel residual_norm: do_norm needs gamma");
        if (!!t->out_fp8 != !!t->out_fp8_scale || (!t->out_fp8 && !oplanes))
          fail(DSN_EINVAL, "test_kernel residual_norm: needs out_planes, or out_fp8 with out_fp8_scale");
        if (t->out_fp8 && t->D % 32 != 0) fail(DSN_EINVAL, "test_kernel residual_norm: fp8 output needs D %% 32 == 0");
        launch_residual_norm(t->x, t->slabs, t->nslab, t->slab_stride, t->bias, t->gamma, t->beta,
                             t->out_fp8 ? reinterpret_cast<op16_t*>(t->out_fp8) : oplanes, t->out_ps, PL, t->rows, t->D,
                             t->eps, t->do_norm, st, t->out_fp8_scale);
        break;
      }
      case DSN_TK_GN_STATS:
      case DSN_TK_GN_APPLY: {
        if (!t->x || t->B < 1 || t->HW < 1 || t->C % 4 != 0 || !gn_groups_fit(t->C, t->C) || t->C > 1024 ||
            t->rstride < t->C || t->rstride % 4 != 0)
          fail(DSN_EINVAL, "test_kernel group norm: unsupported view (C=%d rstride=%d HW=%d)", t->C, t->rstride, t->HW);
        if (t->kind == DSN_TK_GN_STATS) {
          if (!t->out_f32) fail(DSN_EINVAL, "test_kernel gn_stats: out_f32 (the statistics) missing");
          launch_gn_stats(t->x, t->bstride, t->rstride, t->C, t->B, t->HW, t->out_f32, st);
        } else {
          if (!t->stats || !t->gamma || !t->beta || (!t->out_f32 && !oplanes))
            fail(DSN_EINVAL, "test_kernel gn_apply: stats, gamma, beta and an output are required");
          launch_gn_apply(t->x, t->bstride, t->rstride, t->C, t->B, t->HW, t->stats, t->gamma, t->beta, t->eps, t->silu,
                          t->out_f32, oplanes, t->out_ps, PL, st);
        }
        break;
      }
      case DSN_TK_FIR2D: {
        if (!t->x || t->B < 1 || t->C < 4 || t->C % 4 != 0 || t->rstride < t->C || t->rstride % 4 != 0 || t->img_h < 1 ||
            t->img_w < 1 || (!t->up && ((t->img_h | t->img_w) & 1)) || (!t->out_f32 && !oplanes))
          fail(DSN_EINVAL, "test_kernel fir2d: unsupported view (C=%d rstride=%d %d x %d up=%d)", t->C, t->rstride,
               t->img_h, t->img_w, t->up);
        launch_fir2d(t->x, t->bstride, t->rstride, t->C, t->B, t->img_h, t->img_w, t->up, t->add, t->out_f32, oplanes,
                     t->out_ps, PL, st);
        break;
      }
      case DSN_TK_CONV_OUT1: {
        // (the generic kernel reads 8-channel chunks and splits C into 4 quarters of whole float4s)
        if (t->B < 1 || t->L < 1 || t->ktaps < 1 || (t->ktaps & 1) == 0 || t->C < 16 || t->C % 16 != 0 || !t->w ||
            !t->out_f32)
          fail(DSN_EINVAL, "test_kernel conv_out1: needs odd ktaps, C %% 16 == 0, w and out_f32 (C=%d ktaps=%d)", t->C,
               t->ktaps);
        const long n = (long)t->B * t->L * t->C;
        if (t->a_numel != n) fail(DSN_EINVAL, "test_kernel conv_out1: a_numel != B*L*C");
        if (((size_t)(64 + t->ktaps - 1) * (t->C + 4) + (size_t)t->ktaps * t->C + 256) * sizeof(float) > 160 * 1024)
          fail(DSN_EINVAL, "test_kernel conv_out1: C=%d ktaps=%d does not fit in LDS", t->C, t->ktaps);
        const op16_t* a = planes_of("tk_a", t->a, n);
        launch_conv_out1(a, n, PL, t->w, t->out_f32, t->B, t->L, t->C, t->ktaps, t->apply_tanh, st);
        break;
      }
      case DSN_TK_CONV_IN1: {
        if (!t->x || !t->w || t->B < 1 || t->L < 1 || t->C < 1 || t->ktaps < 1 || (t->ktaps & 1) == 0 ||
            (!t->out_f32 && !oplanes))
          fail(DSN_EINVAL, "test_kernel conv_in1: needs wav (x), w, odd ktaps and an output (C=%d ktaps=%d)", t->C, t->ktaps);
        if (t->act != DSN_ACT_NONE && t->act != DSN_ACT_ELU && t->act != DSN_ACT_SNAKE)
          fail(DSN_EINVAL, "test_kernel conv_in1: unsupported activation %d", t->act);
        if (t->act == DSN_ACT_SNAKE && (!t->act_a || !t->act_b)) fail(DSN_EINVAL, "test_kernel conv_in1: Snake needs act_a / act_b");
        launch_conv_in1(t->x, t->w, t->bias, t->B, t->L, t->C, t->ktaps, t->out_f32, oplanes, t->out_ps, PL, t->act,
                        t->act_a, t->act_b, st);
        break;
      }
      case DSN_TK_RU_FUSED: {
        if (t->B < 1 || t->L < 1) fail(DSN_EINVAL, "test_kernel ru_fused: B and L must be positive (B=%d L=%d)", t->B, t->L);
        const long n = (long)t->B * t->L * 128;
        if (t->a_numel != n || t->w_numel != 128L * 7 * 128 || t->w2_numel != 128L * 128)
          fail(DSN_EINVAL, "test_kernel ru_fused: a_numel / w_numel / w2_numel do not match [B][L][128] / [128][7*128] / "
                           "[128][128]");
        if (!t->x || !t->bias || !t->bias2) fail(DSN_EINVAL, "test_kernel ru_fused: x, bias or bias2 missing");
        if (oplanes && t->out_ps < n) fail(DSN_EINVAL, "test_kernel ru_fused: out_ps %ld < B*L*128", (long)t->out_ps);
        RuDesc d;
        memset(&d, 0, sizeof d);
        d.A = planes_of("tk_a", t->a, n);
        d.a_ps = n;
        d.W7 = planes_of("tk_w", t->w, t->w_numel);
        d.w7_ps = t->w_numel;
        d.W1 = planes_of("tk_w2", t->w2, t->w2_numel);
        d.w1_ps = t->w2_numel;
        d.X = t->x;
        d.b7 = t->bias;
        d.b1 = t->bias2;
        d.out_f32 = t->out_f32;
        d.out_planes = oplanes;
        d.out_ps = t->out_ps;
        d.act_mid = t->act;
        d.mid_a = t->act_a;
        d.mid_b = t->act_b;
        d.act_out = t->act_out;
        d.out_a = t->out_act_a;
        d.out_b = t->out_act_b;
        d.S = t->B;
        d.L = t->L;
        d.dil = t->dil;
        const hipError_t e = ru_fused_launch(d, PL, ctx->sw.ru_v1, st);
        if (e != hipSuccess)
          fail(DSN_EHIP, "test_kernel ru_fused: refused or failed: %s (S=%d L=%d dil=%d act %d / %d)", hipGetErrorString(e),
               t->B, t->L, t->dil, t->act, t->act_out);
        break;
      }
      // ---- the sampler's kernels between two score calls: fp32 tensors passed through, every refusal before the launch
      case DSN_TK_PC_PRIOR:
      case DSN_TK_PC_CORRECTOR:
      case DSN_TK_PC_PREDICTOR:
      case DSN_TK_MIX_PRIOR:
      case DSN_TK_MIX_CORRECTOR:
      case DSN_TK_MIX_PREDICTOR:
      case DSN_TK_SB_UPDATE:
      case DSN_TK_REPEAT_SOURCES: {
        static const char* const names[] = {"pc_prior", "pc_corrector", "", "pc_predictor", "", "mix_prior",
                                            "mix_corrector", "mix_predictor", "sb_update", "repeat_sources"};
        const char* nm = names[t->kind - DSN_TK_PC_PRIOR];
        const int k = t->kind;
        if (t->B < 1 || t->n < 1 || t->D < 1 || t->T < 1)
          fail(DSN_EINVAL, "test_kernel %s: B, n, D, T must be positive (B=%d n=%d D=%d T=%d)", nm, t->B, t->n, t->D, t->T);
        const bool mix = k == DSN_TK_MIX_PRIOR || k == DSN_TK_MIX_CORRECTOR || k == DSN_TK_MIX_PREDICTOR;
        if (mix && t->n > 4) fail(DSN_EINVAL, "test_kernel %s: n = %d sources, the kernel holds at most 4", nm, t->n);
        auto need = [&](const void* p, const char* what) {
          if (!p) fail(DSN_EINVAL, "test_kernel %s: %s missing", nm, what);
        };
        need(t->x, "x");
        const bool wants_y = k == DSN_TK_PC_PRIOR || k == DSN_TK_PC_PREDICTOR || k == DSN_TK_MIX_PRIOR ||
                             k == DSN_TK_REPEAT_SOURCES;
        const bool wants_sc = k == DSN_TK_PC_CORRECTOR || k == DSN_TK_PC_PREDICTOR || k == DSN_TK_MIX_CORRECTOR ||
                              k == DSN_TK_MIX_PREDICTOR || k == DSN_TK_SB_UPDATE;
        const bool wants_z = k != DSN_TK_SB_UPDATE && k != DSN_TK_REPEAT_SOURCES;
        const bool wants_xm = k == DSN_TK_PC_PREDICTOR || k == DSN_TK_MIX_PREDICTOR;
        if (wants_y) need(t->y, "y");
        if (wants_sc) need(t->score, "score");
        if (wants_z) need(t->z, "z");
        if (wants_xm) need(t->xmean, "xmean");
        const int B = t->B, n = t->n, D = t->D, T = t->T;
        switch (k) {
          case DSN_TK_PC_PRIOR: launch_pc_prior(t->y, t->mean_full, t->z, t->x, t->stdT, B, n, D, T, st); break;
          case DSN_TK_PC_CORRECTOR:
            launch_pc_corrector(t->x, t->xmean, t->score, t->z, t->step, t->gain, t->norms, t->snr, B, n, D, T, st);
            break;
          case DSN_TK_PC_PREDICTOR:
            launch_pc_predictor(t->x, t->xmean, t->y, t->score, t->z, t->theta, t->dt, t->G, t->g, t->em, B, n, D, T, st);
            break;
          case DSN_TK_MIX_PRIOR: launch_mix_prior(t->y, t->z, t->x, t->smix, t->s1, t->s2, B, n, D, T, st); break;
          case DSN_TK_MIX_CORRECTOR:
            launch_mix_corrector(t->x, t->xmean, t->score, t->z, t->smix, t->s1, t->s2, t->snr, B, n, D, T, st);
            break;
          case DSN_TK_MIX_PREDICTOR:
            launch_mix_predictor(t->x, t->xmean, t->score, t->z, t->smix, t->lam, t->dt, t->g, t->sqdt, t->em, B, n, D, T,
                                 st);
            break;
          case DSN_TK_SB_UPDATE:
            launch_sb_update(t->x, t->score, t->third_is_y ? t->y : t->z, t->w_prev, t->w_est, t->w3, t->third_is_y, B, n,
                             D, T, st);
            break;
          default: launch_repeat_sources(t->y, t->x, B, n, D, T, st); break;
        }
        break;
      }
      case DSN_TK_PC_ITEM_NORMS: {
        if (t->B < 1 || t->count < 1)
          fail(DSN_EINVAL, "test_kernel pc_item_norms: B and count must be positive (B=%d count=%ld)", t->B, (long)t->count);
        if (!t->x || !t->out_f32) fail(DSN_EINVAL, "test_kernel pc_item_norms: x or out_f32 missing");
        launch_pc_item_norms(t->x, (long)t->count, t->B, t->out_f32, st);
        break;
      }
      case DSN_TK_SIGMA_MIX: {
        if (t->B < 1 || t->L < 1) fail(DSN_EINVAL, "test_kernel sigma_mix: B and L must be positive (B=%d L=%d)", t->B, t->L);
        if (t->avg_len < 1) fail(DSN_EINVAL, "test_kernel sigma_mix: avg_len %d < 1", t->avg_len);
        if (!t->y || !t->out_f32) fail(DSN_EINVAL, "test_kernel sigma_mix: y or out_f32 missing");
        launch_sigma_mix(t->y, t->out_f32, t->B, t->L, t->avg_len, st);
        break;
      }
      case DSN_TK_VAE_SAMPLE: {
        if (t->B < 1 || t->D < 1 || t->T < 1)
          fail(DSN_EINVAL, "test_kernel vae_sample: B, D, T must be positive (B=%d D=%d T=%d)", t->B, t->D, t->T);
        if (!t->x || !t->z || !t->out_f32) fail(DSN_EINVAL, "test_kernel vae_sample: x (encoder output), z or out_f32 missing");
        launch_vae_sample(t->x, t->z, t->out_f32, t->B, t->D, t->T, st);
        break;
      }
      case DSN_TK_CODEC_TAIL_ZERO: {
        if (t->B < 1 || t->L < 1 || t->rep < 1 || t->mul < 1 || !t->lens)
          fail(DSN_EINVAL, "test_kernel codec_tail_zero: B, L, rep, mul must be positive and lens (the frame counts) given");
        if (oplanes && t->out_ps < (long)t->B * t->L * t->C)
          fail(DSN_EINVAL, "test_kernel codec_tail_zero: out_ps %ld < B*L*C", (long)t->out_ps);
        std::vector<int32_t> h((size_t)cdiv(t->B, t->rep));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(h.data(), t->lens, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < h.size(); ++i)
          if (h[i] < 0 || (long)h[i] * t->mul > t->L)
            fail(DSN_EINVAL, "test_kernel codec_tail_zero: frames[%d] = %d: %ld rows outside [0, L = %d]", (int)i,
                 (int)h[i], (long)h[i] * t->mul, t->L);
        const char* why = launch_codec_tail_zero(oplanes, t->out_ps, P, t->x, t->out_f32, t->B, t->L, t->C,
                                                 reinterpret_cast<const int*>(t->lens), t->rep, t->mul, st);
        if (why) fail(DSN_EINVAL, "test_kernel codec_tail_zero: %s (C=%d)", why, t->C);
        break;
      }
      case DSN_TK_RANDN:
      case DSN_TK_RAND_UNIFORM: {
        const char* nm = t->kind == DSN_TK_RANDN ? "randn" : "rand_uniform";
        if (t->count < 1) fail(DSN_EINVAL, "test_kernel %s: count %ld must be positive", nm, (long)t->count);
        if (!t->out_f32) fail(DSN_EINVAL, "test_kernel %s: out_f32 missing", nm);
        if (t->kind == DSN_TK_RANDN) launch_randn(t->out_f32, (long)t->count, t->seed, t->offset, st);
        else launch_rand_uniform(t->out_f32, (long)t->count, t->seed, t->offset, t->lo, t->hi, st);
        break;
      }
      // ---- load-time weight preparation, the per-call movers and the feature kernels: tensors passed through
      case DSN_TK_WN_SCALE: {
        if (t->rows < 1 || t->count < 1)
          fail(DSN_EINVAL, "test_kernel wn_scale: rows and count must be positive (rows=%d count=%ld)", t->rows, (long)t->count);
        if (!t->x || !t->gamma || !t->out_f32) fail(DSN_EINVAL, "test_kernel wn_scale: x (v), gamma (g) or out_f32 missing");
        launch_wn_scale(t->x, t->gamma, t->out_f32, t->rows, (long)t->count, st);
        break;
      }
      case DSN_TK_PACK_WEIGHT: {
        static const char* const modes[] = {"linear", "linear_swiglu", "conv", "convt", "conv2d", "nin"};
        const int m = t->mode, N = t->N, K = t->K;
        if (m < PACK_LINEAR || m > PACK_NIN) fail(DSN_EINVAL, "test_kernel pack_weight: unknown mode %d", m);
        if (N < 1 || K < 1) fail(DSN_EINVAL, "test_kernel pack_weight %s: N and K must be positive (N=%d K=%d)", modes[m], N, K);
        if (!t->x || !oplanes) fail(DSN_EINVAL, "test_kernel pack_weight %s: x (the source) or out_planes missing", modes[m]);
        if (t->out_ps < (long)N * K) fail(DSN_EINVAL, "test_kernel pack_weight %s: out_ps %ld < N*K", modes[m], (long)t->out_ps);
        const bool linear = m == PACK_LINEAR || m == PACK_LINEAR_SWIGLU;
        if (t->colscale && !linear) fail(DSN_EINVAL, "test_kernel pack_weight %s: colscale is read by the linear modes only", modes[m]);
        if (t->scale && m != PACK_CONV && m != PACK_CONVT)
          fail(DSN_EINVAL, "test_kernel pack_weight %s: scale is read by conv and convt only", modes[m]);
        long need = (long)N * K;  // floats of the source the index map reaches
        if (m == PACK_LINEAR_SWIGLU && N % 32 != 0)
          fail(DSN_EINVAL, "test_kernel pack_weight linear_swiglu: N %% 32 != 0 (N=%d)", N);
        if (!linear && m != PACK_NIN) {
          if (t->Cin < 1 || t->Cout < 1 || t->kw < 1)
            fail(DSN_EINVAL, "test_kernel pack_weight %s: Cin, Cout, kw must be positive (Cin=%d Cout=%d kw=%d)", modes[m],
                 t->Cin, t->Cout, t->kw);
          need = (long)t->Cout * t->Cin * t->kw;
        }
        if (m == PACK_CONV && (N != t->Cout || K != t->kw * t->Cin))
          fail(DSN_EINVAL, "test_kernel pack_weight conv: needs N = Cout, K = kw*Cin (N=%d K=%d)", N, K);
        if (m == PACK_CONVT) {
          if (t->stride < 1 || t->kw != 2 * t->stride)
            fail(DSN_EINVAL, "test_kernel pack_weight convt: kw != 2*stride (kw=%d stride=%d)", t->kw, t->stride);
          if (N != t->stride * t->Cout || K != 2 * t->Cin)
            fail(DSN_EINVAL, "test_kernel pack_weight convt: needs N = stride*Cout, K = 2*Cin (N=%d K=%d)", N, K);
        }
        if (m == PACK_CONV2D && (t->stride < t->Cin || N < t->Cout || K != t->kw * t->stride))
          fail(DSN_EINVAL, "test_kernel pack_weight conv2d: needs stride (padded Cin) >= Cin, N >= Cout, K = kw*stride "
                           "(N=%d K=%d stride=%d)", N, K, t->stride);
        if (t->count != need)
          fail(DSN_EINVAL, "test_kernel pack_weight %s: count %ld != the %ld floats the mode reads", modes[m], (long)t->count, need);
        launch_pack_weight(t->x, t->scale, oplanes, t->out_ps, PL, m, N, K, t->Cin, t->Cout, t->kw, t->stride, st,
                           t->colscale);
        break;
      }
      case DSN_TK_PACK_BIAS_SWIGLU: {
        if (t->N < 1 || t->N % 32 != 0) fail(DSN_EINVAL, "test_kernel pack_bias_swiglu: N %% 32 != 0 or N < 1 (N=%d)", t->N);
        if (!t->x || !t->out_f32) fail(DSN_EINVAL, "test_kernel pack_bias_swiglu: x (the bias) or out_f32 missing");
        launch_pack_bias_swiglu(t->x, t->out_f32, t->N, st);
        break;
      }
      case DSN_TK_PACK_WEIGHT_FP8: {
        if (t->N < 1 || t->K < 1) fail(DSN_EINVAL, "test_kernel pack_weight_fp8: N and K must be positive (N=%d K=%d)", t->N, t->K);
        if (t->K % 32 != 0) fail(DSN_EINVAL, "test_kernel pack_weight_fp8: K %% 32 != 0 (K=%d)", t->K);
        if (t->mode != PACK_LINEAR && t->mode != PACK_LINEAR_SWIGLU)
          fail(DSN_EINVAL, "test_kernel pack_weight_fp8: mode %d is neither linear nor linear_swiglu", t->mode);
        if (t->mode == PACK_LINEAR_SWIGLU && t->N % 32 != 0)
          fail(DSN_EINVAL, "test_kernel pack_weight_fp8 linear_swiglu: N %% 32 != 0 (N=%d)", t->N);
        if (!t->x || !t->out_fp8 || !t->out_fp8_scale)
          fail(DSN_EINVAL, "test_kernel pack_weight_fp8: x (the source), out_fp8 or out_fp8_scale missing");
        if (((uintptr_t)t->x | (uintptr_t)t->colscale) & 15 || (uintptr_t)t->out_fp8 & 3)
          fail(DSN_EINVAL, "test_kernel pack_weight_fp8: x / colscale must be 16-byte and out_fp8 4-byte aligned");
        launch_pack_weight_fp8(t->x, t->out_fp8, t->out_fp8_scale, t->N, t->K, t->mode == PACK_LINEAR_SWIGLU, st, t->colscale);
        break;
      }
      case DSN_TK_PACKED_ROW_SUM: {
        if (t->N < 1 || t->K < 1) fail(DSN_EINVAL, "test_kernel packed_row_sum: N and K must be positive (N=%d K=%d)", t->N, t->K);
        if (!t->in_planes || !t->out_f32) fail(DSN_EINVAL, "test_kernel packed_row_sum: in_planes or out_f32 missing");
        if (t->in_ps < (long)t->N * t->K) fail(DSN_EINVAL, "test_kernel packed_row_sum: in_ps %ld < N*K", (long)t->in_ps);
        launch_packed_row_sum(reinterpret_cast<const op16_t*>(t->in_planes), t->in_ps, PL, t->N, t->K, t->out_f32, st);
        break;
      }
      case DSN_TK_FP8_ROW_SUM: {
        if (t->N < 1 || t->K < 1) fail(DSN_EINVAL, "test_kernel fp8_row_sum: N and K must be positive (N=%d K=%d)", t->N, t->K);
        if (t->K % 32 != 0) fail(DSN_EINVAL, "test_kernel fp8_row_sum: K %% 32 != 0 (K=%d)", t->K);
        if (!t->in_fp8 || !t->in_fp8_scale || !t->out_f32)
          fail(DSN_EINVAL, "test_kernel fp8_row_sum: in_fp8, in_fp8_scale or out_f32 missing");
        if ((uintptr_t)t->in_fp8 & 3) fail(DSN_EINVAL, "test_kernel fp8_row_sum: in_fp8 must be 4-byte aligned");
        launch_fp8_row_sum(t->in_fp8, t->in_fp8_scale, t->N, t->K, t->out_f32, st);
        break;
      }
      case DSN_TK_BIAS_PLUS_WBETA: {
        if (t->N < 1 || t->K < 1) fail(DSN_EINVAL, "test_kernel bias_plus_wbeta: N and K must be positive (N=%d K=%d)", t->N, t->K);
        if (!t->x || !t->beta || !t->out_f32) fail(DSN_EINVAL, "test_kernel bias_plus_wbeta: x (W), beta or out_f32 missing");
        launch_bias_plus_wbeta(t->x, t->beta, t->bias, t->N, t->K, t->out_f32, st);
        break;
      }
      case DSN_TK_SNAKE_PARAMS: {
        if (t->C < 1) fail(DSN_EINVAL, "test_kernel snake_params: C must be positive (C=%d)", t->C);
        if (!t->act_a || !t->act_b || !t->out_f32 || !t->out2_f32)
          fail(DSN_EINVAL, "test_kernel snake_params: act_a (alpha), act_b (beta), out_f32 or out2_f32 missing");
        launch_snake_params(t->act_a, t->act_b, t->out_f32, t->out2_f32, t->C, st);
        break;
      }
      case DSN_TK_PACK_TOKENS: {
        if (t->B < 1 || t->T < 1 || t->C0 < 1 || t->C1 < 0)
          fail(DSN_EINVAL, "test_kernel pack_tokens: B, T, C0 must be positive and C1 >= 0 (B=%d T=%d C0=%d C1=%d)", t->B,
               t->T, t->C0, t->C1);
        if (!t->x || (t->C1 > 0) != !!t->y)
          fail(DSN_EINVAL, "test_kernel pack_tokens: x (src0) missing, or y (src1) does not go with C1 = %d", t->C1);
        if (!t->out_f32 && !oplanes) fail(DSN_EINVAL, "test_kernel pack_tokens: out_f32 and out_planes both missing");
        if (oplanes && t->out_ps < (long)t->B * t->T * (t->C0 + t->C1))
          fail(DSN_EINVAL, "test_kernel pack_tokens: out_ps %ld < B*T*(C0+C1)", (long)t->out_ps);
        launch_pack_tokens(t->x, t->C0, t->y, t->C1, t->B, t->T, t->out_f32, oplanes, t->out_ps, PL, st);
        break;
      }
      case DSN_TK_WIN_PACK_TOKENS: {
        if (t->B < 1 || t->T < 1 || t->C0 < 1 || t->C1 < 0 || t->R < 1 || t->Tsrc < 1)
          fail(DSN_EINVAL, "test_kernel win_pack_tokens: B, T, C0, R, Tsrc must be positive and C1 >= 0 (B=%d T=%d C0=%d "
               "C1=%d R=%d Tsrc=%d)", t->B, t->T, t->C0, t->C1, t->R, t->Tsrc);
        if (!t->x || (t->C1 > 0) != !!t->y || !t->wtab)
          fail(DSN_EINVAL, "test_kernel win_pack_tokens: x (src0) or wtab missing, or y (src1) does not go with C1 = %d",
               t->C1);
        if (!t->out_f32 && !oplanes) fail(DSN_EINVAL, "test_kernel win_pack_tokens: out_f32 and out_planes both missing");
        if (oplanes && t->out_ps < (long)t->B * t->T * (t->C0 + t->C1))
          fail(DSN_EINVAL, "test_kernel win_pack_tokens: out_ps %ld < B*T*(C0+C1)", (long)t->out_ps);
        std::vector<int32_t> h((size_t)t->B * 3);
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(h.data(), t->wtab, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost));
        for (int b = 0; b < t->B; ++b) {
          const int r = h[3 * b], s = h[3 * b + 1], l = h[3 * b + 2];
          if (r < 0 || r >= t->R || s < 0 || l < 0 || l > t->T || (long)s + l > t->Tsrc)
            fail(DSN_EINVAL, "test_kernel win_pack_tokens: wtab[%d] = (%d, %d, %d) outside R = %d, Tsrc = %d, T = %d", b, r,
                 s, l, t->R, t->Tsrc, t->T);
        }
        launch_win_pack_tokens(t->x, t->C0, t->y, t->C1, reinterpret_cast<const int*>(t->wtab), t->B, t->T, t->Tsrc,
                               t->out_f32, oplanes, t->out_ps, PL, st);
        break;
      }
      case DSN_TK_WIN_BLEND_TOKENS: {
        if (t->B < 1 || t->T < 1 || t->C < 4 || t->C % 4 != 0 || t->rows < 1)
          fail(DSN_EINVAL, "test_kernel win_blend_tokens: B, T, rows must be positive and C a positive multiple of 4 "
               "(B=%d T=%d rows=%d C=%d)", t->B, t->T, t->rows, t->C);
        if (!t->x || !t->ftab || !t->fw || !t->out_f32)
          fail(DSN_EINVAL, "test_kernel win_blend_tokens: x (window tokens), ftab, fw or out_f32 missing");
        if (((uintptr_t)t->x | (uintptr_t)t->out_f32) & 15)
          fail(DSN_EINVAL, "test_kernel win_blend_tokens: x / out_f32 must be 16-byte aligned");
        std::vector<int32_t> h((size_t)t->rows * 4);
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(h.data(), t->ftab, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost));
        for (int f = 0; f < t->rows; ++f)
          for (int k = 0; k < 4; k += 2) {
            const int w = h[4 * f + k], o = h[4 * f + k + 1];
            if (w >= t->B || (w >= 0 && (o < 0 || o >= t->T)))
              fail(DSN_EINVAL, "test_kernel win_blend_tokens: ftab[%d] names window %d offset %d outside B = %d, T = %d",
                   f, w, o, t->B, t->T);
          }
        launch_win_blend_tokens(t->x, reinterpret_cast<const int*>(t->ftab), t->fw, t->out_f32, t->rows, t->C, t->T, st);
        break;
      }
      case DSN_TK_UNPACK_TOKENS: {
        if (t->B < 1 || t->C < 1 || t->T < 1)
          fail(DSN_EINVAL, "test_kernel unpack_tokens: B, C, T must be positive (B=%d C=%d T=%d)", t->B, t->C, t->T);
        if (!t->x || !t->out_f32) fail(DSN_EINVAL, "test_kernel unpack_tokens: x or out_f32 missing");
        launch_unpack_tokens(t->x, t->out_f32, t->B, t->C, t->T, st);
        break;
      }
      case DSN_TK_COPY_ROWS: {
        if (t->rows < 1 || t->C < 1) fail(DSN_EINVAL, "test_kernel copy_rows: rows and C must be positive (rows=%d C=%d)", t->rows, t->C);
        if (t->C % 4 != 0 || t->dst_stride % 4 != 0 || t->dst_stride < t->C)
          fail(DSN_EINVAL, "test_kernel copy_rows: C %% 4 != 0, dst_stride %% 4 != 0 or dst_stride < C (C=%d dst_stride=%ld)",
               t->C, (long)t->dst_stride);
        if (!t->x || !t->out_f32) fail(DSN_EINVAL, "test_kernel copy_rows: x or out_f32 missing");
        if (((uintptr_t)t->x | (uintptr_t)t->out_f32) & 15) fail(DSN_EINVAL, "test_kernel copy_rows: x / out_f32 must be 16-byte aligned");
        launch_copy_rows(t->x, t->out_f32, t->rows, t->C, (long)t->dst_stride, st);
        break;
      }
      case DSN_TK_TO_PLANES: {
        if (t->count < 1 || t->count % 4 != 0)
          fail(DSN_EINVAL, "test_kernel to_planes: count %% 4 != 0 or count < 1 (count=%ld)", (long)t->count);
        if (!t->x || !oplanes) fail(DSN_EINVAL, "test_kernel to_planes: x or out_planes missing");
        if (t->out_ps < t->count || t->out_ps % 4 != 0)
          fail(DSN_EINVAL, "test_kernel to_planes: out_ps %ld < count or out_ps %% 4 != 0", (long)t->out_ps);
        if ((uintptr_t)t->x & 15 || (uintptr_t)oplanes & 7) fail(DSN_EINVAL, "test_kernel to_planes: x must be 16-byte, out_planes 8-byte aligned");
        launch_to_planes(t->x, oplanes, t->out_ps, PL, (long)t->count, st);
        break;
      }
      case DSN_TK_ZERO_TAIL: {
        if (t->B < 1 || t->n < 1 || t->D < 1 || t->T < 1)
          fail(DSN_EINVAL, "test_kernel zero_tail: B, n, D, T must be positive (B=%d n=%d D=%d T=%d)", t->B, t->n, t->D, t->T);
        if (!t->x || !t->lens) fail(DSN_EINVAL, "test_kernel zero_tail: x or lens missing");
        launch_zero_tail(t->x, reinterpret_cast<const int*>(t->lens), t->B, t->n, t->D, t->T, st);
        break;
      }
      case DSN_TK_VAE_SAMPLE_RAGGED: {
        if (t->B < 1 || t->D < 1 || t->T < 1)
          fail(DSN_EINVAL, "test_kernel vae_sample_ragged: B, D, T must be positive (B=%d D=%d T=%d)", t->B, t->D, t->T);
        if (!t->x || !t->z || !t->lens || !t->out_f32)
          fail(DSN_EINVAL, "test_kernel vae_sample_ragged: x (encoder output), z, lens (frames) or out_f32 missing");
        launch_vae_sample_ragged(t->x, t->z, reinterpret_cast<const int*>(t->lens), t->out_f32, t->B, t->D, t->T, st);
        break;
      }
      case DSN_TK_TIMESTEP_FEATURES:
      case DSN_TK_NCSN_FOURIER: {
        const char* nm = t->kind == DSN_TK_NCSN_FOURIER ? "ncsn_fourier" : "timestep_features";
        if (t->B < 1 || t->half < 1) fail(DSN_EINVAL, "test_kernel %s: B and half must be positive (B=%d half=%d)", nm, t->B, t->half);
        if (!t->x || !t->w || !oplanes) fail(DSN_EINVAL, "test_kernel %s: x (t), w or out_planes missing", nm);
        if (t->out_ps < 2L * t->B * t->half) fail(DSN_EINVAL, "test_kernel %s: out_ps %ld < 2*B*half", nm, (long)t->out_ps);
        if (t->kind == DSN_TK_NCSN_FOURIER) launch_ncsn_fourier(t->x, t->w, t->B, t->half, oplanes, t->out_ps, PL, st);
        else launch_timestep_features(t->x, t->w, t->B, t->half, oplanes, t->out_ps, PL, st);
        break;
      }
      case DSN_TK_ROPE_TABLES: {
        if (t->S < 1 || t->dh < 2 || (t->dh & 1))
          fail(DSN_EINVAL, "test_kernel rope_tables: S must be positive and dh (the rotary width) even (S=%d dh=%d)", t->S, t->dh);
        if (!t->rope_cos || !t->rope_sin) fail(DSN_EINVAL, "test_kernel rope_tables: rope_cos or rope_sin missing");
        launch_rope_tables(t->rope_cos, t->rope_sin, t->S, t->dh, st);
        break;
      }
      case DSN_TK_NCSN_PACK:
      case DSN_TK_NCSN_OUTPUT: {
        const bool pack = t->kind == DSN_TK_NCSN_PACK;
        const char* nm = pack ? "ncsn_pack" : "ncsn_output";
        if (t->B < 1 || t->n < 1 || t->H < 1 || t->T < 1)
          fail(DSN_EINVAL, "test_kernel %s: B, n, H, T must be positive (B=%d n=%d H=%d T=%d)", nm, t->B, t->n, t->H, t->T);
        if (t->Wp < t->T) fail(DSN_EINVAL, "test_kernel %s: Wp %d < T %d", nm, t->Wp, t->T);
        if (!t->x || !t->y) fail(DSN_EINVAL, "test_kernel %s: x or y missing", nm);
        if (pack) {
          if (t->Cp < t->n + 1) fail(DSN_EINVAL, "test_kernel ncsn_pack: Cp %d < n + 1", t->Cp);
          if (!t->out_f32 && !oplanes) fail(DSN_EINVAL, "test_kernel ncsn_pack: out_f32 and out_planes both missing");
          if (oplanes && t->out_ps < (long)t->B * t->H * t->Wp * t->Cp)
            fail(DSN_EINVAL, "test_kernel ncsn_pack: out_ps %ld < B*H*Wp*Cp", (long)t->out_ps);
          launch_ncsn_pack(t->x, t->y, t->B, t->n, t->H, t->T, t->Wp, t->Cp, t->out_f32, oplanes, t->out_ps, PL, st);
        } else {
          if (t->cin < 1 || t->Cp < t->cin) fail(DSN_EINVAL, "test_kernel ncsn_output: Cp %d < cin %d, or cin < 1", t->Cp, t->cin);
          if (!t->w || !t->bias || !t->out_f32) fail(DSN_EINVAL, "test_kernel ncsn_output: w, bias or out_f32 missing");
          launch_ncsn_output(t->x, t->Cp, t->y, t->w, t->bias, t->cin, t->n, t->B, t->H, t->T, t->Wp, t->out_f32, st);
        }
        break;
      }
      default:
        fail(DSN_EINVAL, "test_kernel: unknown kind %d", t->kind);
    }
    HIPCHK(hipGetLastError());
  });
}

// Development hook: time `iters` back-to-back launches of the implicit-GEMM kernel on random operands.
int dsn_bench_igemm(dsn_ctx* ctx, int B, int Lin, int Cin, int N, int taps, int tap_dil, int in_pad, int ksplit,
                    int variant, int iters, double* ms_out) {
  return guarded(ctx, [&] {
    const int P = ctx->P, PL = ctx->PL;
    const long an = (long)B * Lin * Cin, wn = (long)N * taps * Cin, on = (long)B * Lin * N;
    float* af = ctx->wsbuf<float>("b_af", an);
    float* wf = ctx->wsbuf<float>("b_wf", wn);
    op16_t* ap = ctx->wsbuf<op16_t>("b_a", an * P);
    op16_t* wp = ctx->wsbuf<op16_t>("b_w", wn * P);
    float* out = ctx->wsbuf<float>("b_o", on * (ksplit > 1 ? ksplit : 1));
    launch_randn(af, an, 1, 0, nullptr);
    launch_randn(wf, wn, 2, 0, nullptr);
    launch_to_planes(af, ap, an, PL, an, nullptr);
    launch_to_planes(wf, wp, wn, PL, wn, nullptr);
    const Packed pk = plain_packed(wp, wn, N, Cin, taps);
    GemmDesc d = ctx->base_desc(ap, an, pk, B, Lin, Lin);
    d.tap_dil = tap_dil;
    d.in_pad = in_pad;
    d.out_f32 = out;
    d.ksplit = ksplit;
    d.slab_stride = on;
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    auto launch = [&] {
      d.m_fast = (variant & 0x40) ? 1 : 0;
      if (variant & 0x20) {
        d.panel_rows = (variant >> 8) & 0xfff;
        d.panel_wm = (variant & 0x80) ? 2 : 0;     // 8-wave variants; low bits then pick the ring (nst, BK 64 flag)
        if (variant & 0x80) {
          d.cfg_nst = variant & 0xf;
          d.cfg_bk = (variant & 0x10) ? 64 : 32;
        }
        hipError_t e2 = igemm_panel_launch(d, PL, (variant >> 20) & 0x3ff, nullptr);
        if (e2 != hipSuccess) fail(DSN_EHIP, "bench panel launch: %s", hipGetErrorString(e2));
        return;
      }
      hipError_t e = variant == 1 ? igemm_launch(d, PL, nullptr)
                                  : igemm2_launch_cfg(d, PL, (variant >> 8) & 0xfff, (variant >> 20) & 0x3ff,
                                                      variant & 0xf, (variant & 0x10) ? 64 : 32, nullptr);
      if (e != hipSuccess) fail(DSN_EHIP, "bench launch: %s", hipGetErrorString(e));
    };
    launch();
    launch();
    HIPCHK(hipEventRecord(e0, nullptr));
    for (int i = 0; i < iters; ++i) launch();
    HIPCHK(hipEventRecord(e1, nullptr));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    if (ms_out) *ms_out = ms / iters;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  });
}

}  // extern "C"
