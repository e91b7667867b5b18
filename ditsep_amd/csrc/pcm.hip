// WAV payloads to fp32 and back, and the reference's output gain (dsn_pcm_decode, dsn_pcm_encode,
// dsn_pcm_encode_frames, dsn_scale_output).
// Restated in numpy in tests/pcm_restatement.py.
//
//   pcm_decode_kernel   one launch for a mixed batch.  A workgroup owns one tile of PCM_TILE frames of one item, whatever
//                       its encoding and channel count.  It stages the tile's byte range -- frames of 1 to 48 bytes from
//                       an arbitrary byte offset -- through LDS with 16-byte loads aligned down in the buffer and guarded
//                       by nbytes (byte loads for a chunk that crosses the buffer's end, or from an unaligned buffer), so
//                       every payload byte comes from HBM once and no lane issues a byte-wide global load on the way.
//                       Lane i then unpacks frames 4 i .. 4 i + 3 from LDS (two or three dword reads and a funnel shift
//                       per sample: a sample may straddle dwords) and stores them as one 16-byte store per output row
//                       where the row's alignment allows.  Frames at or past the item's end, and the channels past its
//                       own, are written as zero without touching LDS.
//   pcm_encode_kernel   a workgroup owns one tile of PCM_TILE payload samples of one row (a row's channels interleaved;
//                       the mono call has one): loads coalesced per channel, quantisation, the
//                       tile's byte image in LDS at the 16-byte phase of its place in the buffer; then the bytes up to
//                       the first 16-byte boundary one by one, whole aligned 16-byte stores, and the rest one by one.
//                       Nothing outside the tile's own bytes is written: neighbouring rows share dwords.
//   scale_*_kernel      sums (fp64, exact products, per thread in stride order, a fixed tree, one plain store per tile),
//                       one thread per row adding the tile sums in index order and forming alpha, and the product.
//                       A thread's samples are the same on the 16-byte and on the scalar load path, so a row gives the
//                       bits it gives alone.
// The only atomics are the integer clipped counts.  Index arithmetic is 64-bit.
#include "../../include/ditsep_hip.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int PCPB = 256;
constexpr int PCM_TILE = 1024;     // frames (decode) or samples (encode) of one workgroup: 4 per lane
constexpr int SCALE_TILE = 4096;   // samples one workgroup of the gain's sum launch adds up
static_assert(PCM_TILE == 4 * PCPB, "a lane converts four consecutive frames");
static_assert(SCALE_TILE % (4 * PCPB) == 0, "a tile is whole rounds of four samples per lane");
// dynamic LDS of the decode launch: the widest tile, up to 15 bytes of lead-in, and the two dwords a funnel shift may
// read past a sample's first
inline size_t decode_lds_bytes(int max_frame_bytes) { return (size_t)PCM_TILE * max_frame_bytes + 32; }
static_assert((size_t)PCM_TILE * DSN_PCM_MAX_FRAME_BYTES + 32 <= 65536, "the widest tile fits the LDS of one launch");

// the sample whose first byte is byte p of the LDS image
__device__ __forceinline__ float pcm_sample(const unsigned* __restrict__ lds, int p, int enc) {
  const int i = p >> 2, sh = (p & 3) * 8;
  const unsigned long long lo = ((unsigned long long)lds[i + 1] << 32) | lds[i];
  const unsigned v = (unsigned)(lo >> sh);
  switch (enc) {
    case DSN_PCM_U8: return (float)((int)(v & 0xffu) - 128) * 0x1p-7f;
    case DSN_PCM_S16: return (float)(short)(v & 0xffffu) * 0x1p-15f;
    case DSN_PCM_S24: return (float)((int)(v << 8) >> 8) * 0x1p-23f;
    case DSN_PCM_S32: return (float)(int)v * 0x1p-31f;   // (the conversion rounds to nearest even; the product is exact)
    case DSN_PCM_F32: return __uint_as_float(v);
    default: {
      unsigned long long d = lo >> sh;
      if (sh) d |= (unsigned long long)lds[i + 2] << (64 - sh);
      const double x = __longlong_as_double((long long)d);
      return x != x ? __uint_as_float(0x7fc00000u) : (float)x;
    }
  }
}

// grid (x: tiles of Lmax, y: item)
__global__ void __launch_bounds__(PCPB) pcm_decode_kernel(const unsigned char* __restrict__ bytes, long nbytes,
                                                          const PcmItem* __restrict__ items, int downmix,
                                                          float* __restrict__ out, int Cout, int Lmax, int vec_in,
                                                          int vec_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned pcm_lds[];
  const int b = blockIdx.y, tid = threadIdx.x;
  const PcmItem it = items[b];
  const long f0 = (long)blockIdx.x * PCM_TILE;
  const int C = it.channels, w = pcm_sample_bytes(it.enc), fb = C * w;
  const long left = (long)it.frames - f0;
  const int nf = left <= 0 ? 0 : left < PCM_TILE ? (int)left : PCM_TILE;   // (uniform) frames of this tile
  int lead = 0;
  if (nf > 0) {
    const long s = it.offset + f0 * fb, e = s + (long)nf * fb;   // the tile's bytes: inside [0, nbytes) by the host check
    const long a = s & ~15L;
    lead = (int)(s - a);
    const int chunks = (int)((e - a + 15) >> 4);
    for (int v = tid; v < chunks; v += PCPB) {
      const long g = a + 16L * v;
      uint4 q;
      if (vec_in && g + 16 <= nbytes) {
        q = *reinterpret_cast<const uint4*>(bytes + g);
      } else {
        unsigned r[4] = {0u, 0u, 0u, 0u};
        for (int k = 0; k < 16; ++k)
          if (g + k < nbytes) r[k >> 2] |= (unsigned)bytes[g + k] << (8 * (k & 3));
        q = make_uint4(r[0], r[1], r[2], r[3]);
      }
      reinterpret_cast<uint4*>(pcm_lds)[v] = q;
    }
  }
  __syncthreads();
  const int fl = 4 * tid;
  const long f = f0 + fl;
  if (f >= Lmax) return;
  for (int c = 0; c < Cout; ++c) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (downmix || c < C) {
      for (int k = 0; k < 4; ++k) {
        if (fl + k >= nf) break;
        const int p = lead + (fl + k) * fb;
        if (!downmix) {
          v[k] = pcm_sample(pcm_lds, p + c * w, it.enc);
        } else {
          float s = pcm_sample(pcm_lds, p, it.enc);
          if (C > 1) {
            for (int ch = 1; ch < C; ++ch) s += pcm_sample(pcm_lds, p + ch * w, it.enc);
            s = s / (float)C;
          }
          v[k] = s;
        }
      }
    }
    float* dst = out + ((long)b * Cout + c) * Lmax + f;
    if (vec_out) {   // (Lmax % 4 == 0: the four samples are inside the row)
      *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      for (int k = 0; k < 4; ++k)
        if (f + k < Lmax) dst[k] = v[k];
    }
  }
}

// grid (x: tiles of C Lmax interleaved samples, y: row); x [R][C][Lmax], row r holds items[r].frames frames of
// items[r].channels channels: payload sample j is channel j % channels of frame j / channels
__global__ void __launch_bounds__(PCPB) pcm_encode_kernel(const float* __restrict__ x,
                                                          const PcmItem* __restrict__ items, int C, int Lmax, int enc,
                                                          unsigned char* __restrict__ bytes,
                                                          unsigned long long* __restrict__ clipped) {
  __shared__ __attribute__((aligned(16))) unsigned char img[PCM_TILE * 4 + 32];
  const int r = blockIdx.y, tid = threadIdx.x;
  const PcmItem it = items[r];
  const long j0 = (long)blockIdx.x * PCM_TILE, total_j = (long)it.frames * it.channels;
  if (j0 >= total_j) return;   // (uniform)
  const int nj = total_j - j0 < PCM_TILE ? (int)(total_j - j0) : PCM_TILE;
  const int w = pcm_sample_bytes(enc);
  unsigned char* dst = bytes + it.offset + j0 * w;
  const int lead = (int)((uintptr_t)dst & 15);
  const float* row = x + (long)r * C * Lmax;
  const float scale = enc == DSN_PCM_S16 ? 32768.f : 8388608.f;
  int clip = 0;
  const long fr0 = j0 / it.channels;                  // (uniform) the tile's first frame ..
  const int c0 = (int)(j0 - fr0 * it.channels);       // .. and the channel it starts in
  for (int j = tid; j < nj; j += PCPB) {
    const int s = c0 + j, df = it.channels == 1 ? s : s / it.channels;
    const float v = row[(long)(s - df * it.channels) * Lmax + fr0 + df];
    unsigned q;
    if (enc == DSN_PCM_F32) {
      q = __float_as_uint(v);
    } else {
      float y = rintf(v * scale);
      if (!(y >= -scale && y <= scale - 1.f)) {   // outside the range, or not finite
        ++clip;
        y = y != y ? 0.f : y < 0.f ? -scale : scale - 1.f;
      }
      q = (unsigned)(int)y;
    }
    const int p = lead + j * w;
    for (int k = 0; k < w; ++k) img[p + k] = (unsigned char)(q >> (8 * k));
  }
  __syncthreads();
  const int total = nj * w;
  int head = (16 - lead) & 15;
  if (head > total) head = total;
  const int mid = (total - head) >> 4, tail = total - head - 16 * mid;
  if (tid < head) dst[tid] = img[lead + tid];
  for (int v = tid; v < mid; v += PCPB)   // (dst + head and img + lead + head are 16-byte aligned)
    *reinterpret_cast<uint4*>(dst + head + 16 * v) = *reinterpret_cast<const uint4*>(img + lead + head + 16 * v);
  if (tid < tail) dst[head + 16 * mid + tid] = img[lead + head + 16 * mid + tid];
  if (enc != DSN_PCM_F32) {
    for (int off = 32; off > 0; off >>= 1) clip += __shfl_down(clip, off, 64);
    if ((tid & 63) == 0 && clip > 0) atomicAdd(&clipped[r], (unsigned long long)clip);
  }
}

// grid (x: tiles, y: row b n + i).  A lane adds samples k0 + 4 tid + {0, 1, 2, 3} (+ 4 PCPB, ..) in that order on
// either load path.
__global__ void __launch_bounds__(PCPB) scale_sum_kernel(const float* __restrict__ mix, const float* __restrict__ sep,
                                                         const int* __restrict__ lens, int n, int Lmax, int tiles,
                                                         double* __restrict__ part, int vec) {
  __shared__ double red[2][PCPB / 64];
  const int row = blockIdx.y, b = row / n, c = blockIdx.x, tid = threadIdx.x;
  const int len = lens ? lens[b] : Lmax;
  const long k0 = (long)c * SCALE_TILE;
  if (k0 >= len) return;   // (uniform)
  const long k1 = k0 + SCALE_TILE < len ? k0 + SCALE_TILE : len;
  const float* m = mix + (long)b * Lmax;
  const float* s = sep + (long)row * Lmax;
  double num = 0.0, den = 0.0;
  for (long k = k0 + 4 * tid; k < k1; k += 4 * PCPB) {
    float mv[4] = {0.f, 0.f, 0.f, 0.f}, sv[4] = {0.f, 0.f, 0.f, 0.f};
    const int cnt = k1 - k < 4 ? (int)(k1 - k) : 4;
    if (vec && cnt == 4) {
      const float4 a = *reinterpret_cast<const float4*>(m + k), e = *reinterpret_cast<const float4*>(s + k);
      mv[0] = a.x, mv[1] = a.y, mv[2] = a.z, mv[3] = a.w;
      sv[0] = e.x, sv[1] = e.y, sv[2] = e.z, sv[3] = e.w;
    } else {
      for (int q = 0; q < cnt; ++q) mv[q] = m[k + q], sv[q] = s[k + q];
    }
    for (int q = 0; q < cnt; ++q) {
      num += (double)mv[q] * (double)sv[q];
      den += (double)sv[q] * (double)sv[q] + 1e-10;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    num += __shfl_down(num, off, 64);
    den += __shfl_down(den, off, 64);
  }
  if ((tid & 63) == 0) red[0][tid >> 6] = num, red[1][tid >> 6] = den;
  __syncthreads();
  if (tid < 2) {
    double t = 0.0;
    for (int q = 0; q < PCPB / 64; ++q) t += red[tid][q];
    part[((long)row * tiles + c) * 2 + tid] = t;
  }
}

// one thread per row: the row's own tiles in index order
__global__ void __launch_bounds__(PCPB) scale_alpha_kernel(const double* __restrict__ part,
                                                           const int* __restrict__ lens, int rows, int n, int Lmax,
                                                           int tiles, float* __restrict__ alpha) {
  const int row = blockIdx.x * PCPB + threadIdx.x;
  if (row >= rows) return;
  const int len = lens ? lens[row / n] : Lmax;
  const int nt = (int)(((long)len + SCALE_TILE - 1) / SCALE_TILE);
  double num = 0.0, den = 0.0;
  for (int c = 0; c < nt; ++c) {
    num += part[((long)row * tiles + c) * 2];
    den += part[((long)row * tiles + c) * 2 + 1];
  }
  alpha[row] = (float)(num / den);
}

// grid (x: groups of 4 PCPB samples, y: row)
__global__ void __launch_bounds__(PCPB) scale_apply_kernel(const float* __restrict__ sep, const int* __restrict__ lens,
                                                           const float* __restrict__ alpha, int n, int Lmax,
                                                           float* __restrict__ out, int vec) {
  const int row = blockIdx.y;
  const long t0 = ((long)blockIdx.x * PCPB + threadIdx.x) * 4;
  if (t0 >= Lmax) return;
  const int len = lens ? lens[row / n] : Lmax;
  const float a = alpha[row];
  const float* s = sep + (long)row * Lmax + t0;
  float* dst = out + (long)row * Lmax + t0;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (vec && t0 + 3 < len) {
    const float4 e = *reinterpret_cast<const float4*>(s);
    v[0] = a * e.x, v[1] = a * e.y, v[2] = a * e.z, v[3] = a * e.w;
  } else {
    for (int k = 0; k < 4; ++k)
      if (t0 + k < len) v[k] = a * s[k];
  }
  if (vec) {   // (Lmax % 4 == 0: the four samples are inside the row)
    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int k = 0; k < 4; ++k)
      if (t0 + k < Lmax) dst[k] = v[k];
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

long scale_output_tiles(int L) { return ((long)L + SCALE_TILE - 1) / SCALE_TILE; }

void launch_pcm_decode(const unsigned char* bytes, long nbytes, const PcmItem* items, int B, int downmix, float* out,
                       int Cout, int Lmax, int max_frame_bytes, hipStream_t s) {
  const dim3 grid((unsigned)(((long)Lmax + PCM_TILE - 1) / PCM_TILE), (unsigned)B);
  const int vec_in = aligned16(bytes), vec_out = aligned16(out) && Lmax % 4 == 0;
  hipLaunchKernelGGL(pcm_decode_kernel, grid, dim3(PCPB), decode_lds_bytes(max_frame_bytes), s, bytes, nbytes, items,
                     downmix ? 1 : 0, out, Cout, Lmax, vec_in, vec_out);
}

void launch_pcm_encode(const float* x, const PcmItem* items, int R, int C, int Lmax, int enc, unsigned char* bytes,
                       unsigned long long* clipped, hipStream_t s) {
  const dim3 grid((unsigned)(((long)C * Lmax + PCM_TILE - 1) / PCM_TILE), (unsigned)R);
  hipLaunchKernelGGL(pcm_encode_kernel, grid, dim3(PCPB), 0, s, x, items, C, Lmax, enc, bytes, clipped);
}

void launch_scale_output(const float* mix, const float* sep, const int* lens, int B, int n, int Lmax, double* part,
                         float* alpha, float* out, hipStream_t s) {
  const int rows = B * n, tiles = (int)scale_output_tiles(Lmax);
  const int vin = aligned16(mix) && aligned16(sep) && Lmax % 4 == 0;
  const int vout = vin && aligned16(out);
  hipLaunchKernelGGL(scale_sum_kernel, dim3((unsigned)tiles, (unsigned)rows), dim3(PCPB), 0, s, mix, sep, lens, n, Lmax,
                     tiles, part, vin);
  hipLaunchKernelGGL(scale_alpha_kernel, dim3((unsigned)((rows + PCPB - 1) / PCPB)), dim3(PCPB), 0, s, part, lens, rows,
                     n, Lmax, tiles, alpha);
  const long per = 4L * PCPB;
  hipLaunchKernelGGL(scale_apply_kernel, dim3((unsigned)((Lmax + per - 1) / per), (unsigned)rows), dim3(PCPB), 0, s, sep,
                     lens, alpha, n, Lmax, out, vout);
}
