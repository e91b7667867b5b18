// Sinc resampling of a ragged batch (dsn_resample): x [B][C][L] -> out [B][C or 1][Lout], the polyphase filter of
// resample_plan.h walked over its non-zero taps only.  Restated in float64 in tests/resample_restatement.py.
//
// One launch.  A workgroup owns RS_TILES_PER_WG consecutive tiles of RS_TILE output samples of one (item, channel)
// and keeps the compact taps c [n][stride] and k0 [n] in LDS for all of them; `stride` is S made odd, so lanes on
// neighbouring phases read different banks.  Per tile it stages the input span the tile needs -- every input sample
// comes from HBM once, as 16-byte loads where the row's alignment allows, zeros where the span leaves [0, lens[b]);
// with downmix the C channels are averaged in fp32 on the way in, (x_0 + .. + x_{C-1}) / C in that order -- and lane i
// forms output j = j0 + i (+ 256, ..): phase p = j mod n, frame m = j / n, one product and S - 1 fused multiply-adds in tap
// order, one coalesced store.  Past an item's own ceil(n lens[b] / o) samples the row is written as zero, and nothing
// at or past lens[b] is read.  Plain C++: no atomics, two calls give identical bits.  Global indices are 64-bit.
#include "../../include/ditsep_hip.h"
#include "kernels.h"

namespace {

constexpr int RSPB = 256;
constexpr int RS_TILE = 1024;        // output samples of one tile
constexpr int RS_TILES_PER_WG = 4;   // consecutive tiles one workgroup walks with the tables loaded once
// The LDS budget of a launch, in 4-byte words: what a kernel may take as dynamic LDS without opting in to more (64 KB).
// A plan whose table, k0 and tile span together exceed it is refused (resample_lds_refusal).
constexpr long RS_LDS_WORDS = 16384;
static_assert(RS_TILE % RSPB == 0, "a tile is whole rounds of the workgroup");

struct ResampleShape {
  int C, L, Cout, Lout;    // input channels and row length; output channels (1 with downmix) and row length
  int o, n, width, S;
  int stride;              // words per table row in LDS and in `taps`
  int kmin, kspan;         // min k0, and max k0 + S - min k0: the taps any phase touches, as a span of input
  int downmix, vec;        // vec: the 16-byte path may be taken (aligned base; with downmix, L % 4 == 0)
};

__device__ __forceinline__ float rs_load(const ResampleShape& q, const float* __restrict__ row, long i, int len) {
  if (i < 0 || i >= len) return 0.f;
  if (!q.downmix) return row[i];
  float s = row[i];
  for (int ch = 1; ch < q.C; ++ch) s += row[(long)ch * q.L + i];
  return s / (float)q.C;
}

__global__ void __launch_bounds__(RSPB) resample_kernel(const ResampleShape q, const float* __restrict__ x,
                                                        const int* __restrict__ lens,
                                                        const float* __restrict__ taps,
                                                        const int* __restrict__ k0, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  const int tabw = (q.n * q.stride + 3) & ~3, nq = (q.n + 3) & ~3;
  float* s_c = rs_lds;
  int* s_k0 = reinterpret_cast<int*>(rs_lds + tabw);
  float* s_x = rs_lds + tabw + nq;   // (16-byte aligned)
  const int tid = threadIdx.x;
  const int b = blockIdx.y / q.Cout, c = blockIdx.y % q.Cout;
  const int len = lens ? lens[b] : q.L;
  const long Lb = ((long)q.n * len + q.o - 1) / q.o;   // this item's output samples
  const long rowoff = ((long)b * q.C + (q.downmix ? 0 : c)) * q.L;
  const float* row = x + rowoff;
  float* dst = out + ((long)b * q.Cout + c) * q.Lout;

  for (int i = tid; i < q.n * q.stride; i += RSPB) s_c[i] = taps[i];
  for (int i = tid; i < q.n; i += RSPB) s_k0[i] = k0[i];

  for (int t = 0; t < RS_TILES_PER_WG; ++t) {
    const long j0 = ((long)blockIdx.x * RS_TILES_PER_WG + t) * RS_TILE;
    if (j0 >= q.Lout) break;   // (uniform)
    if (j0 >= Lb) {            // (uniform) the whole tile lies past the item's end
      for (int r = 0; r < RS_TILE / RSPB; ++r) {
        const long j = j0 + tid + r * RSPB;
        if (j < q.Lout) dst[j] = 0.f;
      }
      continue;
    }
    const long j1 = j0 + RS_TILE < Lb ? j0 + RS_TILE : Lb;
    const long m0 = j0 / q.n, m1 = (j1 - 1) / q.n;
    const long g0 = m0 * q.o + q.kmin - q.width;                 // first input sample a lane of this tile may read
    const int count = (int)(m1 - m0) * q.o + q.kspan;            // .. and how many follow it
    // s_x[0] is input sample g0 - lead: with `vec` that is a multiple of 4 floats from the (aligned) base
    const int lead = q.vec ? (int)(((rowoff + g0) % 4 + 4) % 4) : 0;
    const long gs = g0 - lead;
    const int quads = (count + lead + 3) >> 2;
    __syncthreads();   // the tables are in; the previous tile's lanes are done with s_x
    for (int v = tid; v < quads; v += RSPB) {
      const long i = gs + 4L * v;
      float4 f;
      if (q.vec && i >= 0 && i + 3 < len) {
        f = *reinterpret_cast<const float4*>(row + i);
        if (q.downmix) {
          for (int ch = 1; ch < q.C; ++ch) {
            const float4 a = *reinterpret_cast<const float4*>(row + (long)ch * q.L + i);
            f.x += a.x, f.y += a.y, f.z += a.z, f.w += a.w;
          }
          const float cf = (float)q.C;
          f.x /= cf, f.y /= cf, f.z /= cf, f.w /= cf;
        }
      } else {
        f.x = rs_load(q, row, i, len);
        f.y = rs_load(q, row, i + 1, len);
        f.z = rs_load(q, row, i + 2, len);
        f.w = rs_load(q, row, i + 3, len);
      }
      *reinterpret_cast<float4*>(s_x + 4 * v) = f;
    }
    __syncthreads();
    for (int r = 0; r < RS_TILE / RSPB; ++r) {
      const long j = j0 + tid + r * RSPB;
      if (j >= q.Lout) break;
      float acc = 0.f;
      if (j < Lb) {
        const long m = j / q.n;
        const int p = (int)(j - m * q.n);
        const float* cp = s_c + p * q.stride;
        const float* xp = s_x + (int)(m - m0) * q.o + (s_k0[p] - q.kmin) + lead;
        acc = cp[0] * xp[0];   // (not 0 + ..: a lone tap of 1 hands -0.0 through)
        for (int s = 1; s < q.S; ++s) acc = fmaf(cp[s], xp[s], acc);
      }
      dst[j] = acc;
    }
  }
}

}  // namespace

// LDS words (floats) one launch takes: the table, k0 and the widest span of a tile, each rounded to 16 bytes
long resample_lds_words(int o, int n, int stride, int kspan) {
  const long tabw = ((long)n * stride + 3) & ~3L, nq = ((long)n + 3) & ~3L;
  // a tile of T outputs touches at most (T - 1) / n + 1 frame boundaries; + 3 lead-in, + 3 to a whole quad
  const long span = ((long)(RS_TILE - 1) / n + 1) * o + kspan + 8;
  return tabw + nq + span;
}

const char* resample_lds_refusal(int o, int n, int stride, int kspan, char* buf, size_t bufsz) {
  const long need = resample_lds_words(o, n, stride, kspan);
  if (need <= RS_LDS_WORDS) return nullptr;
  snprintf(buf, bufsz, "the plan (orig %d, new %d) needs %ld words of LDS -- a table of %ld, %d first taps and the span "
           "of a %d-sample tile -- more than the kernel's %ld", o, n, need, (long)n * stride, n, RS_TILE, RS_LDS_WORDS);
  return buf;
}

void launch_resample(const float* x, const int* lens, const float* taps, const int* k0, float* out, int B, int C,
                     int L, int Lout, int o, int n, int width, int S, int stride, int kmin, int kspan, int downmix,
                     hipStream_t s) {
  const bool aligned = ((uintptr_t)x & 15) == 0;
  const ResampleShape q{C, L, downmix ? 1 : C, Lout, o, n, width, S, stride, kmin, kspan, downmix ? 1 : 0,
                        aligned && (!downmix || C == 1 || L % 4 == 0) ? 1 : 0};
  const long per = (long)RS_TILE * RS_TILES_PER_WG;
  const dim3 grid((unsigned)((Lout + per - 1) / per), (unsigned)((long)B * q.Cout));
  const size_t lds = sizeof(float) * (size_t)resample_lds_words(o, n, stride, kspan);
  hipLaunchKernelGGL(resample_kernel, grid, dim3(RSPB), lds, s, q, x, lens, taps, k0, out);
}
