// Ragged batches through the codec: the rows of a padded item past its own end are written as zero between two
// layers, so that every convolution reads there what it reads past the end of the item run alone (its zero padding).
// ELU(0) = SnakeBeta(0) = 0, so a zeroed tail is zero in the activated operand planes as well.
#include "kernels.h"

#include <algorithm>

namespace {

constexpr int TZ_TPB = 256;
constexpr int TZ_ELEMS = 8192;  // elements of one item a workgroup covers: TZ_ELEMS / C whole rows (at least one)

inline int tz_rows_per_block(int C) { return C >= TZ_ELEMS ? 1 : TZ_ELEMS / C; }

// Workgroup (x, s) owns rows [x * rpb, (x + 1) * rpb) of item s; the part of them at or past the item's valid row count
// is one contiguous span of every destination ([S][L][C] row-major), which the threads clear with 16-byte stores, lane i
// next to lane i + 1.  A workgroup with no tail row returns after one scalar load.  valid is clamped to [0, L]: the
// kernel stays inside the buffers whatever the device array holds.
__global__ __launch_bounds__(TZ_TPB) void codec_tail_zero_kernel(op16_t* __restrict__ planes, long ps, int n_planes,
                                                                 float* __restrict__ xf, float* __restrict__ out, int L,
                                                                 int C, int rpb, const int* __restrict__ frames, int rep,
                                                                 int mul) {
  const int s = blockIdx.y;
  const long valid = min(max((long)frames[s / rep] * mul, 0L), (long)L);
  const long r0 = (long)blockIdx.x * rpb;
  const long ra = max(r0, valid), rb = min(r0 + rpb, (long)L);
  if (ra >= rb) return;
  const long e0 = ((long)s * L + ra) * C;
  const int n8 = (int)(((rb - ra) * C) >> 3);  // 8-element chunks of the span (C % 8 == 0)
  const int tid = threadIdx.x;
  if (planes) {
    const op16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int p = 0; p < n_planes; ++p) {
      op16x8* d = reinterpret_cast<op16x8*>(planes + p * ps + e0);
      for (int i = tid; i < n8; i += TZ_TPB) d[i] = z;
    }
  }
  const f32x4 zf = {0.f, 0.f, 0.f, 0.f};
  if (xf) {
    f32x4* d = reinterpret_cast<f32x4*>(xf + e0);
    for (int i = tid; i < 2 * n8; i += TZ_TPB) d[i] = zf;
  }
  if (out) {
    f32x4* d = reinterpret_cast<f32x4*>(out + e0);
    for (int i = tid; i < 2 * n8; i += TZ_TPB) d[i] = zf;
  }
}

// vae_sample_kernel (kernels.hip) with y[s, :, t] = 0 for t >= frames[s]
__global__ void vae_sample_ragged_kernel(const float* __restrict__ enc, const float* __restrict__ noise,
                                         const int* __restrict__ frames, float* __restrict__ y, int D, int T,
                                         long total) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int t = (int)(i % T);
    const long sc = i / T;
    const int c = (int)(sc % D);
    const long s = sc / D;
    float v = 0.f;
    if (t < frames[s]) {
      const float* row = enc + (s * T + t) * (2L * D);
      const float mean = row[c], scale = row[D + c];
      const float sp = scale > 20.f ? scale : log1pf(expf(scale));
      v = noise[i] * (sp + 1e-4f) + mean;
    }
    y[i] = v;
  }
}

}  // namespace

const char* launch_codec_tail_zero(op16_t* planes, long ps, int n_planes, float* xf, float* out, int S, int L, int C,
                                   const int* frames, int rep, int mul, hipStream_t st) {
  if (S < 1 || L < 1 || rep < 1 || mul < 1 || !frames) return "S, L, rep, mul must be positive and frames non-null";
  if (C < 8 || C % 8 != 0) return "C must be a positive multiple of 8 (16-byte stores)";
  if (S > 65535) return "more than 65535 items";
  if (planes && (n_planes < 1 || n_planes > 2 || (n_planes > 1 && ps % 8 != 0))) return "1 or 2 planes, plane stride a multiple of 8";
  if (((uintptr_t)planes | (uintptr_t)xf | (uintptr_t)out) & 15) return "destinations must be 16-byte aligned";
  if (!planes && !xf && !out) return nullptr;
  const int rpb = tz_rows_per_block(C);
  hipLaunchKernelGGL(codec_tail_zero_kernel, dim3(cdiv(L, rpb), S), dim3(TZ_TPB), 0, st, planes, ps, n_planes, xf, out, L,
                     C, rpb, frames, rep, mul);
  return nullptr;
}

void launch_vae_sample_ragged(const float* enc, const float* noise, const int* frames, float* y, int S, int D, int T,
                              hipStream_t st) {
  const long total = (long)S * D * T;
  const int grid = (int)std::min<long>((total + 255) / 256, 1 << 16);
  hipLaunchKernelGGL(vae_sample_ragged_kernel, dim3(grid), dim3(256), 0, st, enc, noise, frames, y, D, T, total);
}
