// NCSN++ latent score network inside dsn_ctx (included by engine.hip inside the struct body).
// reference: LatentScoreModelNCSNpp src/models/diffsep/score_models.py:140-186,
//            NCSNpp src/models/diffsep/ncsnpp.py:48-478, blocks ncsnpp_utils/layerspp.py:37-328.

struct NcsnRes {
  float *g0 = nullptr, *b0 = nullptr, *g1 = nullptr, *b1 = nullptr;
  Packed conv0, conv1, conv2;
  bool has_conv2 = false, up = false, down = false;
  int cin = 0, cout = 0, dense_off = 0;
};
struct NcsnAttn {
  float *g = nullptr, *b = nullptr;
  Packed qkv, out;
  int c = 0;
};
struct NcsnHead {  // GroupNorm + conv3x3 -> pyramid channels
  float *g = nullptr, *b = nullptr;
  Packed conv;
  int c = 0;
};
// channels-last image view: element (item, row, ch) at item*bs + row*rs + coff + ch
struct CatStats {  // GroupNorm partials of a concat buffer [h_prev | skip], filled by the two producers' epilogues
  float* slot = nullptr;
  int nq = 0;      // quads per row of the whole concatenation
  int parts = 0;   // bit 0: the slice at channel 0 has been written with partials, bit 1: the other slice
};
struct View {
  float* f = nullptr;
  op16_t* p = nullptr;
  long pps = 0;  // plane stride of p
  int C = 0, rs = 0, coff = 0;
  long bs = 0;
  CatStats* cat = nullptr;  // set on channel slices of a concat buffer (and on the whole buffer)
};

static constexpr int NCS_GN_SLOTS = 96;
int ncs_gn_slot = 0;
float* ncs_fourier_w = nullptr;
Packed ncs_lin1, ncs_lin2, ncs_dense_all, ncs_conv_in;
std::vector<NcsnRes> ncs_res;     // in module order
std::vector<NcsnAttn> ncs_attn;
std::vector<Packed> ncs_combine;
std::vector<NcsnHead> ncs_heads;
float *ncs_out_w = nullptr, *ncs_out_b = nullptr;
int ncs_dense_total = 0;
int ncs_cp = 32;  // padded channel count of the (n_src+1)-channel input / input pyramid

Packed pack_conv2d(const std::string& prefix, int taps, hipStream_t st) {
  const DevTensor& w = get(prefix + "weight");
  if (w.shape.size() != 4 || w.shape[2] * w.shape[3] != taps) fail(DSN_EINVAL, "%s: expected %d-tap conv", prefix.c_str(), taps);
  const int Cout = (int)w.shape[0], Cin = (int)w.shape[1];
  Packed p;
  p.N = (Cout + 3) / 4 * 4;
  p.Cin = (Cin + 31) / 32 * 32;
  p.taps = taps;
  p.K = taps * p.Cin;
  p.ps = (long)p.N * p.K;
  p.w = (op16_t*)dmalloc(sizeof(op16_t) * p.ps * P);
  launch_pack_weight(w.p, nullptr, p.w, p.ps, PL, PACK_CONV2D, p.N, p.K, Cin, Cout, taps, p.Cin, st);
  const DevTensor& b = get(prefix + "bias");
  if (p.N == Cout) {
    p.bias = b.p;
  } else {
    p.bias = (float*)dmalloc(sizeof(float) * p.N);
    HIPCHK(hipMemsetAsync(p.bias, 0, sizeof(float) * p.N, st));
    HIPCHK(hipMemcpyAsync(p.bias, b.p, sizeof(float) * Cout, hipMemcpyDeviceToDevice, st));
  }
  p.bias_mod = p.N;
  return p;
}

void finalize_ncsnpp(hipStream_t st) {
  const std::string bp = "score_model.backbone.";
  const std::string mp = bp + "all_modules.";
  const int nf = cfg.ncsn_nf, levels = cfg.ncsn_n_levels, nrb = cfg.ncsn_num_res_blocks;
  if (nf % 32 != 0 || levels < 1 || levels > 4) fail(DSN_EINVAL, "NCSN++: nf must be a multiple of 32, 1..4 levels");
  if (cfg.ncsn_image_size != cfg.latent_dim) fail(DSN_EINVAL, "NCSN++: image_size must equal latent_dim");
  ncs_cp = 32;
  const int ch_in = cfg.n_src + 1;
  auto M = [&](int i) { return mp + std::to_string(i) + "."; };
  ncs_fourier_w = get(M(0) + "W").p;
  ncs_lin1 = pack_linear(M(1) + "weight", M(1) + "bias", false, st);
  ncs_lin2 = pack_linear(M(2) + "weight", M(2) + "bias", false, st);
  ncs_conv_in = pack_conv2d(M(3), 9, st);
  ncs_res.clear();
  ncs_attn.clear();
  ncs_combine.clear();
  ncs_heads.clear();
  int i = 4;
  std::vector<std::pair<std::string, int>> dense;  // (prefix, cout) in res order
  auto add_res = [&](int cin, int cout, bool up, bool down) {
    NcsnRes r;
    const std::string p = M(i);
    r.cin = cin;
    r.cout = cout;
    r.up = up;
    r.down = down;
    r.g0 = get(p + "GroupNorm_0.weight").p;
    r.b0 = get(p + "GroupNorm_0.bias").p;
    r.g1 = get(p + "GroupNorm_1.weight").p;
    r.b1 = get(p + "GroupNorm_1.bias").p;
    r.conv0 = pack_conv2d(p + "Conv_0.", 9, st);
    r.conv1 = pack_conv2d(p + "Conv_1.", 9, st);
    r.has_conv2 = cin != cout || up || down;
    if (r.has_conv2) r.conv2 = pack_conv2d(p + "Conv_2.", 1, st);
    r.dense_off = ncs_dense_total;
    ncs_dense_total += cout;
    dense.push_back({p + "Dense_0.", cout});
    ncs_res.push_back(r);
    ++i;
  };
  auto add_attn = [&](int c) {
    if (c != 64 && c != 128 && c != 256) fail(DSN_EINVAL, "NCSN++ attention width %d unsupported (64/128/256)", c);
    NcsnAttn a;
    const std::string p = M(i);
    a.c = c;
    a.g = get(p + "GroupNorm_0.weight").p;
    a.b = get(p + "GroupNorm_0.bias").p;
    // fused q|k|v projection: rows [0,C) = NIN_0^T, [C,2C) = NIN_1^T, [2C,3C) = NIN_2^T
    a.qkv.N = 3 * c;
    a.qkv.K = a.qkv.Cin = c;
    a.qkv.taps = 1;
    a.qkv.ps = (long)3 * c * c;
    a.qkv.w = (op16_t*)dmalloc(sizeof(op16_t) * a.qkv.ps * P);
    a.qkv.bias = (float*)dmalloc(sizeof(float) * 3 * c);
    a.qkv.bias_mod = 3 * c;
    for (int k = 0; k < 3; ++k) {
      const std::string np = p + "NIN_" + std::to_string(k) + ".";
      // pack each [C][C] block into its rows of both planes
      for (int pl_i = 0; pl_i < 1; ++pl_i) (void)pl_i;
      launch_pack_weight(get(np + "W").p, nullptr, a.qkv.w + (long)k * c * c, a.qkv.ps, PL, PACK_NIN, c, c, c, c, 1, 1, st);
      HIPCHK(hipMemcpyAsync(a.qkv.bias + k * c, get(np + "b").p, sizeof(float) * c, hipMemcpyDeviceToDevice, st));
    }
    a.out.N = c;
    a.out.K = a.out.Cin = c;
    a.out.taps = 1;
    a.out.ps = (long)c * c;
    a.out.w = (op16_t*)dmalloc(sizeof(op16_t) * a.out.ps * P);
    launch_pack_weight(get(p + "NIN_3.W").p, nullptr, a.out.w, a.out.ps, PL, PACK_NIN, c, c, c, c, 1, 1, st);
    a.out.bias = get(p + "NIN_3.b").p;
    a.out.bias_mod = c;
    ncs_attn.push_back(a);
    ++i;
  };
  ncs_dense_total = 0;
  std::vector<int> hs_c{nf};
  int in_ch = nf;
  for (int lv = 0; lv < levels; ++lv) {
    const int res = cfg.ncsn_image_size >> lv;
    for (int k = 0; k < nrb; ++k) {
      const int out_ch = nf * cfg.ncsn_ch_mult[lv];
      add_res(in_ch, out_ch, false, false);
      in_ch = out_ch;
      if (res == cfg.ncsn_attn_resolution) add_attn(in_ch);
      hs_c.push_back(in_ch);
    }
    if (lv != levels - 1) {
      add_res(in_ch, in_ch, false, true);
      ncs_combine.push_back(pack_conv2d(M(i) + "Conv_0.", 1, st));
      ++i;
      hs_c.push_back(in_ch);
    }
  }
  add_res(in_ch, in_ch, false, false);
  add_attn(in_ch);
  add_res(in_ch, in_ch, false, false);
  for (int lv = levels - 1; lv >= 0; --lv) {
    const int res = cfg.ncsn_image_size >> lv;
    for (int k = 0; k < nrb + 1; ++k) {
      const int out_ch = nf * cfg.ncsn_ch_mult[lv];
      add_res(in_ch + hs_c.back(), out_ch, false, false);
      hs_c.pop_back();
      in_ch = out_ch;
    }
    if (res == cfg.ncsn_attn_resolution) add_attn(in_ch);
    NcsnHead hd;
    hd.c = in_ch;
    hd.g = get(M(i) + "weight").p;
    hd.b = get(M(i) + "bias").p;
    ++i;
    hd.conv = pack_conv2d(M(i), 9, st);
    ++i;
    ncs_heads.push_back(hd);
    if (lv != 0) add_res(in_ch, in_ch, true, false);
  }
  // all Dense_0 layers batched into one [sum Cout][4 nf] GEMM
  {
    const int K = 4 * nf;
    float* wcat = (float*)dmalloc(sizeof(float) * (long)ncs_dense_total * K);
    float* bcat = (float*)dmalloc(sizeof(float) * ncs_dense_total);
    long row = 0;
    for (auto& dn : dense) {
      const DevTensor& w = get(dn.first + "weight");
      if (w.numel != (long)dn.second * K) fail(DSN_EINVAL, "%s: bad Dense_0 shape", dn.first.c_str());
      HIPCHK(hipMemcpyAsync(wcat + row * K, w.p, sizeof(float) * w.numel, hipMemcpyDeviceToDevice, st));
      HIPCHK(hipMemcpyAsync(bcat + row, get(dn.first + "bias").p, sizeof(float) * dn.second, hipMemcpyDeviceToDevice, st));
      row += dn.second;
    }
    Packed& p = ncs_dense_all;
    p.N = ncs_dense_total;
    p.K = p.Cin = K;
    p.taps = 1;
    p.ps = (long)p.N * K;
    p.w = (op16_t*)dmalloc(sizeof(op16_t) * p.ps * P);
    launch_pack_weight(wcat, nullptr, p.w, p.ps, PL, PACK_LINEAR, p.N, K, K, p.N, 1, 1, st);
    p.bias = bcat;
    p.bias_mod = p.N;
  }
  const DevTensor& ow = get(bp + "output_layer.weight");
  if (ow.numel != (long)cfg.n_src * ch_in) fail(DSN_EINVAL, "output_layer shape mismatch");
  ncs_out_w = ow.p;
  ncs_out_b = get(bp + "output_layer.bias").p;
}

// --- building blocks -------------------------------------------------------------------
View new_view(const std::string& name, int B, int HW, int C, bool need_f32 = true, bool need_planes = true) {
  View v;
  v.C = v.rs = C;
  v.bs = (long)HW * C;
  v.pps = (long)B * HW * C;
  if (need_f32) v.f = wsbuf<float>(name + "_f", v.pps);
  if (need_planes) v.p = wsbuf<op16_t>(name + "_p", v.pps * P);
  return v;
}
View slice(const View& base, int coff, int C) const {
  View v = base;
  v.coff = base.coff + coff;
  v.C = C;
  return v;
}
// 2-D conv GEMM over a planes view; output described by `out` (either member may be null)
GemmDesc conv_desc(const View& in, const Packed& w, int B, int H, int W) {
  GemmDesc d = base_desc(in.p + in.coff, in.pps, w, B, H * W, H * W);
  d.in_bstride = in.bs;
  d.in_row_elems = in.rs;
  if (w.taps == 9) {
    d.img_h = H;
    d.img_w = W;
  }
  return d;
}
void set_out(GemmDesc& d, const View& out, bool f32, bool planes) {
  d.out_bstride = out.bs;
  d.out_row_elems = out.rs;
  d.out_off = out.coff;
  d.out_limit = out.bs;
  d.out_f32 = f32 ? out.f : nullptr;
  d.out_planes = planes ? out.p : nullptr;
  d.out_ps = out.pps;
}
void set_resid(GemmDesc& d, const View& r) {
  d.resid = r.f;
  d.resid_bstride = r.bs;
  d.resid_row_elems = r.rs;
  d.resid_off = r.coff;
}
// every GroupNorm of a forward pass has its own statistics slot: slice partials [B][HW/64][C/4][2] written with plain
// stores by the stats kernel / the producing GEMM's epilogue (no atomics, nothing to zero), sized for the largest
// (slices x quads) of the pass
long ncs_slot_floats = 0;
float* gn_slot(int B) {
  if (ncs_gn_slot >= NCS_GN_SLOTS) fail(DSN_EINVAL, "too many GroupNorm calls in one pass");
  return wsbuf<float>("ncs_stats", (long)NCS_GN_SLOTS * ncs_slot_floats) + (long)(ncs_gn_slot++) * ncs_slot_floats;
}
// ask the GEMM that produces `C` channels per row to accumulate that tensor's GroupNorm statistics
float* gn_in_epilogue(GemmDesc& d, int C, int B, int HW) {
  if (HW % 64 != 0 || d.ksplit > 1) return nullptr;
  d.gn_stats = gn_slot(B);
  return d.gn_stats;
}
// Statistics of the tensors written in this pass, keyed by (fp32 address, channels) -- a concat buffer and its
// first slice share the address: filled by the producing GEMM's
// epilogue (track_output) or by the first GroupNorm that had to run the stats kernel; a second GroupNorm of the
// same tensor (pyramid head + up-sampling block) reuses them.
std::map<std::pair<const float*, int>, float*> ncs_stats_of;
void track_output(GemmDesc& d, const View& out, int B, int HW) {
  if (!out.f) return;
  float* s = gn_in_epilogue(d, out.C, B, HW);
  if (s) ncs_stats_of[{out.f + out.coff, out.C}] = s;
  else ncs_stats_of.erase({out.f + out.coff, out.C});
  if (out.cat && out.C < out.rs) {  // a channel slice of a concat buffer: partials also in the concatenation's layout
    const int bit = out.coff == 0 ? 1 : 2;
    if (s && out.coff % 4 == 0) {
      if (!out.cat->slot) out.cat->slot = gn_slot(B);
      d.gn_stats2 = out.cat->slot;
      d.gn_nq2 = out.cat->nq;
      d.gn_qoff2 = out.coff / 4;
      out.cat->parts |= bit;
    } else {
      out.cat->parts &= ~bit;
    }
  }
}
// stats != null: already accumulated by the producer
void group_norm(const View& x, const float* gamma, const float* beta, int B, int HW, bool silu, float* of, op16_t* op,
                long ops, hipStream_t st, float* stats = nullptr, bool tracked = true) {
  // tracked = false: a scratch tensor that every block reuses (its producer hands `stats` over directly)
  if (!stats && tracked) {
    auto it = ncs_stats_of.find({x.f + x.coff, x.C});
    if (it != ncs_stats_of.end()) stats = it->second;
  }
  // the whole concat buffer, both slices written with partials by their producers' epilogues
  if (!stats && tracked && x.cat && x.C == x.rs && x.coff == 0 && x.cat->parts == 3) stats = x.cat->slot;
  if (!stats) {
    stats = gn_slot(B);
    launch_gn_stats(x.f + x.coff, x.bs, x.rs, x.C, B, HW, stats, st);
    if (tracked) ncs_stats_of[{x.f + x.coff, x.C}] = stats;
  }
  launch_gn_apply(x.f + x.coff, x.bs, x.rs, x.C, B, HW, stats, gamma, beta, 1e-6f, silu ? 1 : 0, of, op, ops, PL, st);
}

// ResnetBlockBigGANpp: x (H x W) -> out (H' x W'), out may be a channel slice of a concat buffer
void ncs_resblock(const NcsnRes& r, const View& x, const View& out, const float* dense, int B, int H, int W,
                  hipStream_t st) {
  const int Ho = r.up ? 2 * H : (r.down ? H / 2 : H), Wo = r.up ? 2 * W : (r.down ? W / 2 : W);
  const long rows_i = (long)B * H * W, rows_o = (long)B * Ho * Wo;
  View a0 = new_view("ncs_a0", B, Ho * Wo, r.cin, false, true);
  View xs = x;  // shortcut source (planes)
  if (!r.up && !r.down) {
    group_norm(x, r.g0, r.b0, B, H * W, true, nullptr, a0.p, a0.pps, st);
  } else {
    float* tmp = wsbuf<float>("ncs_a0f", rows_i * r.cin);
    group_norm(x, r.g0, r.b0, B, H * W, true, tmp, nullptr, 0, st);
    launch_fir2d(tmp, (long)H * W * r.cin, r.cin, r.cin, B, H, W, r.up ? 1 : 0, nullptr, nullptr, a0.p, a0.pps, PL, st);
    View xr = new_view("ncs_xr", B, Ho * Wo, r.cin, false, true);
    launch_fir2d(x.f + x.coff, x.bs, x.rs, r.cin, B, H, W, r.up ? 1 : 0, nullptr, nullptr, xr.p, xr.pps, PL, st);
    xs = xr;
  }
  View h1 = new_view("ncs_h1", B, Ho * Wo, r.cout, true, false);
  View a1 = new_view("ncs_a1", B, Ho * Wo, r.cout, false, true);
  float* h1_stats = nullptr;
  bool gn_done = false;
  {
    GemmDesc d = conv_desc(a0, r.conv0, B, Ho, Wo);
    set_out(d, h1, true, false);
    d.bbias = dense + r.dense_off;
    d.bbias_stride = ncs_dense_total;
    h1_stats = gn_in_epilogue(d, r.cout, B, Ho * Wo);   // GroupNorm_1's statistics come out of this epilogue
    // h1 has one consumer, GroupNorm_1 -> SiLU -> Conv_1: where the halo kernel runs this conv in one resident round
    // its workgroups finish the GroupNorm themselves and write a1 from their accumulators (h1 is never stored).
    // DSN_NO_GN_FIN keeps the separate pass.
    if (!sw.no_gn_fin && h1_stats && P == 1 && (long)cdiv((long)B * Ho * Wo, 128) * cdiv(r.cout, 128) > 32) {
      GemmDesc f = d;
      f.out_f32 = nullptr;
      f.gnf_out = a1.p;
      f.gnf_gamma = r.g1;
      f.gnf_beta = r.b1;
      f.gnf_eps = 1e-6f;
      f.gnf_silu = 1;
      if (igemm_halo3x3_gnfin_ok(f, PL)) {
        f.gnf_sync = gnf_counters(Ho * Wo / igemm_halo3x3_tile(f, PL), (long)B * cdiv(r.cout, 128), st);
        f.gnf_err = fin_err_dev;
        d = f;
        gn_done = true;
      } else if (igemm2_gnfin_ok(f, PL)) {
        // 128-pixel images (level 2): igemm2's 128 x 64 tile holds a whole image -- finished inside the workgroup
        f.cfg_bm = 128;
        f.cfg_bn = 64;
        f.cfg_nst = 3;
        f.cfg_bk = 64;
        d = f;
        gn_done = true;
      }
    }
    run(d, st);
  }
  if (!gn_done) group_norm(h1, r.g1, r.b1, B, Ho * Wo, true, nullptr, a1.p, a1.pps, st, h1_stats, false);
  View sc;
  // NIN shortcut (Conv_2, 1x1 over the raw block input): where the halo kernel runs Conv_1 it accumulates the shortcut
  // into the same tile first (GemmDesc::sc_A) -- no launch, no fp32 round trip of Conv_2's output
  bool sc_fused = false;
  if (r.has_conv2 && P == 1 && r.conv2.taps == 1 && r.conv2.Cin % 32 == 0 && r.conv2.N == r.cout &&
      (long)cdiv(rows_o, 128) * cdiv(r.cout, 128) > 32) {
    GemmDesc probe = conv_desc(a1, r.conv1, B, Ho, Wo);
    sc_fused = igemm_halo3x3_eligible(probe, PL);
  }
  if (r.has_conv2 && !sc_fused) {
    sc = new_view("ncs_sc", B, Ho * Wo, r.cout, true, false);
    GemmDesc d = conv_desc(xs, r.conv2, B, Ho, Wo);
    set_out(d, sc, true, false);
    run(d, st);
  }
  {
    GemmDesc d = conv_desc(a1, r.conv1, B, Ho, Wo);
    set_out(d, out, out.f != nullptr, out.p != nullptr);
    if (sc_fused) {
      d.sc_A = xs.p + xs.coff;
      d.sc_W = r.conv2.w;
      d.sc_bias = r.conv2.bias;
      d.sc_Cin = r.conv2.Cin;
      d.sc_row_elems = xs.rs;
      d.sc_bstride = xs.bs;
    } else
    set_resid(d, r.has_conv2 ? sc : x);
    d.out_scale = 0.70710678118654752f;
    track_output(d, out, B, Ho * Wo);
    run(d, st);
  }
  (void)rows_o;
}

// AttnBlockpp, in place on `x` (single head of width C over all H*W positions)
void ncs_attention(const NcsnAttn& a, const View& x, int B, int HW, hipStream_t st) {
  View n = new_view("ncs_an", B, HW, a.c, false, true);
  group_norm(x, a.g, a.b, B, HW, false, nullptr, n.p, n.pps, st);
  const long rows = (long)B * HW;
  op16_t* qkv = wsbuf<op16_t>("ncs_qkv", rows * 3 * a.c * P);
  {
    GemmDesc d = base_desc(n.p, n.pps, a.qkv, 1, (int)rows, (int)rows);
    d.out_planes = qkv;
    d.out_ps = rows * 3 * a.c;
    d.qkv_D = a.c;
    d.q_scale = 1.f / sqrtf((float)a.c);
    run(d, st);
  }
  {
    const hipError_t e = launch_attention_mfma(qkv, rows * 3 * a.c, n.p, n.pps, PL, B, HW, 1, a.c, st);
    if (e == hipErrorNotSupported) fail(DSN_EINVAL, "unsupported attention width %d", a.c);
    if (e != hipSuccess) fail(DSN_EHIP, "ncsnpp attention launch failed (%d keys, width %d): %s", HW, a.c, hipGetErrorString(e));
  }
  {
    GemmDesc d = base_desc(n.p, n.pps, a.out, B, HW, HW);
    set_out(d, x, x.f != nullptr, x.p != nullptr);
    set_resid(d, x);
    d.out_scale = 0.70710678118654752f;
    track_output(d, x, B, HW);   // x is rewritten in place: its statistics are replaced with it
    run(d, st);
  }
}

// t [rows] -> Dense_0(silu(temb)) of every res-block, fp32 [rows][ncs_dense_total]
// (GaussianFourierProjection -> Linear -> SiLU -> Linear, ncsnpp.py:331-345; the per-block SiLU + Dense_0 batched)
void ncs_time_dense(const float* t, int rows, float* out, hipStream_t st) {
  const int nf = cfg.ncsn_nf;
  op16_t* FF = wsbuf<op16_t>("ncs_ff", (long)rows * 2 * nf * P);
  op16_t* E1 = wsbuf<op16_t>("ncs_e1", (long)rows * 4 * nf * P);
  op16_t* E2 = wsbuf<op16_t>("ncs_e2", (long)rows * 4 * nf * P);
  launch_ncsn_fourier(t, ncs_fourier_w, rows, nf, FF, (long)rows * 2 * nf, PL, st);
  GemmDesc d = base_desc(FF, (long)rows * 2 * nf, ncs_lin1, rows, 1, 1);
  d.out_planes = E1;
  d.out_ps = (long)rows * 4 * nf;
  d.act = DSN_ACT_SILU;
  run(d, st);
  GemmDesc e = base_desc(E1, (long)rows * 4 * nf, ncs_lin2, rows, 1, 1);
  e.out_planes = E2;
  e.out_ps = (long)rows * 4 * nf;
  e.act = DSN_ACT_SILU;
  run(e, st);
  GemmDesc f = base_desc(E2, (long)rows * 4 * nf, ncs_dense_all, rows, 1, 1);
  f.out_f32 = out;
  run(f, st);
}

// xt [B,n,64,T], t [B], mix [B,1,64,T] -> score token-major [B*T][n*64] in ws "sc"
float* ncsnpp_forward(const float* xt, const float* t, const float* mix, int B, int T, hipStream_t st) {
  const int n = cfg.n_src, nf = cfg.ncsn_nf, levels = cfg.ncsn_n_levels, nrb = cfg.ncsn_num_res_blocks;
  const int H0 = cfg.ncsn_image_size;
  const int mll = cfg.ncsn_max_latent_length;
  const int W0 = (T + mll - 1) / mll * mll;
  if (W0 % (1 << (levels - 1)) != 0) fail(DSN_EINVAL, "latent frames %d not divisible by 2^(levels-1)", W0);
  const int ch_in = n + 1;
  float* SC = wsbuf<float>("sc", (long)B * T * n * H0);
  ncs_gn_slot = 0;
  ncs_stats_of.clear();
  {  // slot size: level-0 slices x the widest tensor's quads (a concat of two of the widest feature maps)
    int cm = 1;
    for (int l = 0; l < levels; ++l) cm = std::max(cm, cfg.ncsn_ch_mult[l]);
    ncs_slot_floats = (long)B * cdiv((long)H0 * W0, 64) * (2L * nf * cm / 4) * 2;
    (void)wsbuf<float>("ncs_stats", (long)NCS_GN_SLOTS * ncs_slot_floats);
  }
  // ---- time embedding: all res-block Dense_0(silu(temb)) in one GEMM (once per sampler pass: time_cache) ----
  const float* DB = time_cache.find(t, B);
  if (!DB) {
    float* tmp = wsbuf<float>("ncs_dense", (long)B * ncs_dense_total);
    ncs_time_dense(t, B, tmp, st);
    DB = tmp;
  }
  // ---- concat buffers of the up path: CB[u] = [h_prev | skip] ----
  struct Lv { int H, W, C; };
  std::vector<Lv> lv(levels);
  for (int l = 0; l < levels; ++l) lv[l] = {H0 >> l, W0 >> l, nf * cfg.ncsn_ch_mult[l]};
  // skip tensors hs[] in creation order: (level, channels)
  std::vector<std::pair<int, int>> hs;
  hs.push_back({0, nf});
  for (int l = 0; l < levels; ++l) {
    for (int k = 0; k < nrb; ++k) hs.push_back({l, lv[l].C});
    if (l != levels - 1) hs.push_back({l + 1, lv[l].C});
  }
  const int nhs = (int)hs.size();
  // up block u consumes hs[nhs-1-u]; its h_prev has in_ch channels
  std::vector<View> CB(nhs);
  std::vector<int> cb_ch(nhs);
  std::vector<CatStats> cats(nhs);   // (views hold pointers into it: sized once, never resized)
  {
    int in_ch = lv[levels - 1].C, u = 0;
    for (int l = levels - 1; l >= 0; --l)
      for (int k = 0; k < nrb + 1; ++k, ++u) {
        const int cs = hs[nhs - 1 - u].second;
        CB[u] = new_view("ncs_cb" + std::to_string(u), B, lv[l].H * lv[l].W, in_ch + cs);
        cats[u].nq = (in_ch + cs) / 4;
        CB[u].cat = &cats[u];
        cb_ch[u] = in_ch;
        in_ch = lv[l].C;
      }
  }
  auto hs_view = [&](int i) { const int u = nhs - 1 - i; return slice(CB[u], cb_ch[u], hs[i].second); };

  // ---- input + input pyramid ----
  View xin = new_view("ncs_xin", B, H0 * W0, ncs_cp);
  launch_ncsn_pack(xt, mix, B, n, H0, T, W0, ncs_cp, xin.f, xin.p, xin.pps, PL, st);
  int ri = 0, ai = 0, ci = 0, hi = 0;
  {
    GemmDesc d = conv_desc(xin, ncs_conv_in, B, H0, W0);
    const View o = hs_view(0);
    set_out(d, o, true, true);
    track_output(d, o, B, H0 * W0);
    run(d, st);
  }
  View pyr_in = xin;
  int cur = 0;  // index of the newest hs entry
  for (int l = 0; l < levels; ++l) {
    const int H = lv[l].H, W = lv[l].W;
    for (int k = 0; k < nrb; ++k) {
      const View o = hs_view(cur + 1);
      ncs_resblock(ncs_res[ri++], hs_view(cur), o, DB, B, H, W, st);
      if (H == cfg.ncsn_attn_resolution) ncs_attention(ncs_attn[ai++], o, B, H * W, st);
      ++cur;
    }
    if (l != levels - 1) {
      View hd = new_view("ncs_hd", B, (H / 2) * (W / 2), lv[l].C, true, false);
      ncs_resblock(ncs_res[ri++], hs_view(cur), hd, DB, B, H, W, st);
      View pn = new_view("ncs_pyr" + std::to_string(l + 1), B, (H / 2) * (W / 2), ncs_cp);
      launch_fir2d(pyr_in.f, pyr_in.bs, pyr_in.rs, ncs_cp, B, H, W, 0, nullptr, pn.f, pn.p, pn.pps, PL, st);
      pyr_in = pn;
      {  // Combine (sum): conv1x1(input pyramid) + h
        GemmDesc d = conv_desc(pyr_in, ncs_combine[ci++], B, H / 2, W / 2);
        const View o = hs_view(cur + 1);
        set_out(d, o, true, true);
        set_resid(d, hd);
        track_output(d, o, B, (H / 2) * (W / 2));
        run(d, st);
      }
      ++cur;
    }
  }
  // ---- middle ----
  const int Hm = lv[levels - 1].H, Wm = lv[levels - 1].W, Cm = lv[levels - 1].C;
  View hm = new_view("ncs_hm", B, Hm * Wm, Cm);
  ncs_resblock(ncs_res[ri++], hs_view(cur), hm, DB, B, Hm, Wm, st);
  ncs_attention(ncs_attn[ai++], hm, B, Hm * Wm, st);
  ncs_resblock(ncs_res[ri++], hm, slice(CB[0], 0, Cm), DB, B, Hm, Wm, st);
  // ---- up path ----
  float* pyramid = nullptr;
  int u = 0;
  for (int l = levels - 1; l >= 0; --l) {
    const int H = lv[l].H, W = lv[l].W, C = lv[l].C;
    View h = new_view("ncs_hup" + std::to_string(l), B, H * W, C);
    for (int k = 0; k < nrb + 1; ++k, ++u) {
      const bool last = k == nrb;
      const View o = last ? h : slice(CB[u + 1], 0, C);
      ncs_resblock(ncs_res[ri++], CB[u], o, DB, B, H, W, st);
    }
    if (H == cfg.ncsn_attn_resolution) ncs_attention(ncs_attn[ai++], h, B, H * W, st);
    {  // progressive output_skip head: conv3x3(silu(GN(h))) -> pyramid channels
      const NcsnHead& hd = ncs_heads[hi++];
      View a = new_view("ncs_pa", B, H * W, C, false, true);
      group_norm(h, hd.g, hd.b, B, H * W, true, nullptr, a.p, a.pps, st);
      const int Np = hd.conv.N;
      float* ph = wsbuf<float>("ncs_ph" + std::to_string(l), (long)B * H * W * Np);
      GemmDesc d = conv_desc(a, hd.conv, B, H, W);
      d.out_f32 = ph;
      run(d, st);
      if (!pyramid) {
        pyramid = ph;
      } else {
        float* pn = wsbuf<float>("ncs_pyo" + std::to_string(l), (long)B * H * W * Np);
        launch_fir2d(pyramid, (long)(H / 2) * (W / 2) * Np, Np, Np, B, H / 2, W / 2, 1, ph, pn, nullptr, 0, PL, st);
        pyramid = pn;
      }
    }
    if (l != 0) ncs_resblock(ncs_res[ri++], h, slice(CB[u], 0, C), DB, B, H, W, st);
  }
  launch_ncsn_output(pyramid, ncs_heads[0].conv.N, t, ncs_out_w, ncs_out_b, ch_in, n, B, H0, T, W0, SC, st);
  return SC;
}
