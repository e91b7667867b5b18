// Denoising score-matching loss of the OUVE SDE (reference src/diffsep_latent.py:130-187: sample_prior,
// compute_score_loss, compute_score_loss_init_hack_pit) around one score call: perturb -> score network -> reduce ->
// combine.  Restated in float64 in tests/score_loss_restatement.py.
//
// Arithmetic.  Per item, e = exp(-theta t) and sigma = OUVESDE._std(t) are evaluated in fp64 from the fp32 time and
// rounded ONCE to fp32 (the reference evaluates both closed forms in fp32; the single rounding stays within its few
// ulp).  x_t is then formed in fp32 in the reference's order, (e x0 + (1 - e) y) + sigma z, not contracted into FMAs.
// The loss terms (sigma s + z)^2 are formed and summed in fp64 from those fp32 values: per-workgroup partials in
// plain stores, added in a fixed order by the one-workgroup combine kernel -- no atomics, reruns are bit-identical.
//
// PIT variant (t = 1 for every item, x_t = y + sigma z0): the reference's target noise of permutation p in slot s,
// z_p[s] = z0[s] + (y - mean(x0[p(s)])) / sigma, depends on p only through the source j = p(s) that sits in the slot,
// so the n x n table  L[s][j] = mean_{D,T} (sigma score[s] + z0[s] + (y - mean(x0[j])) / sigma)^2  holds every
// permutation's loss, and the reference's stack(dim=1).min(dim=1) -- a minimum per (item, slot) -- is min_j L[s][j]
// (every source occupies every slot in some permutation).  One score call instead of n!.
//
// Ragged batches (tok non-null: tok[b] = 1 + frames[b], the token counts the length-aware attention reads): item b's
// valid elements are [.., :frames[b]] of its rows of stride T.  perturb forms exactly the dense value there, writes
// x_t as zero past the end and reads nothing else there; reduce and combine walk the D frames[b] valid elements of a
// row in (channel, frame) order, chunked from the row's start, and divide by D frames[b]: the same fp64 terms in an
// order that depends on the item's own length only, whatever the padding and the batch around it.
#include "../../include/ditsep_hip.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int LTPB = 256;

__device__ __forceinline__ double loss_decay(const LossSde& q, double t) { return exp(-q.theta * t); }
// sqrt(sigma_min^2 exp(-2 theta t) (exp(2 (theta + logsig) t) - 1) logsig / (theta + logsig))
__device__ __forceinline__ double loss_std(const LossSde& q, double t) {
  const double num =
      q.sigma_min * q.sigma_min * exp(-2.0 * q.theta * t) * (exp(2.0 * (q.theta + q.logsig) * t) - 1.0) * q.logsig;
  return sqrt(num / (q.theta + q.logsig));
}

// fixed-order block sum of one fp64 value per thread; the result is valid in thread 0
__device__ double loss_block_sum(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
  __syncthreads();
  return s;
}

// grid (x: slices of one item's n*D*T elements, y: item)
__global__ void loss_perturb_kernel(const LossSde q, const float* __restrict__ y, const float* __restrict__ x0,
                                    const float* __restrict__ z, const float* __restrict__ t_in, float t_const,
                                    const int* __restrict__ perm, int pit, float* __restrict__ xt,
                                    float* __restrict__ tv, float* __restrict__ sigma, int n, long DT, int T,
                                    const int* __restrict__ tok) {
  const int b = blockIdx.y;
  const float tf = t_in ? t_in[b] : t_const;
  const float e = (float)loss_decay(q, (double)tf);
  const float sg = (float)loss_std(q, (double)tf);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    tv[b] = tf;
    sigma[b] = sg;
  }
  const long per_item = (long)n * DT;
  const float ome = 1.f - e;
  const int fb = tok ? tok[b] - 1 : T;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < per_item; i += (long)gridDim.x * blockDim.x) {
    const int s = (int)(i / DT);
    const long r = i - (long)s * DT;
    const long xi = (long)b * per_item + i;
    if (tok && (int)(r % T) >= fb) {  // past the item's end: zero, and nothing is read
      xt[xi] = 0.f;
      continue;
    }
    const float ym = y[b * DT + r];
    float v;
    if (pit) {
      v = ym + sg * z[xi];
    } else {
      const int src = perm ? perm[b * n + s] : s;
      const float mean = e * x0[((long)b * n + src) * DT + r] + ome * ym;
      v = mean + sg * z[xi];
    }
    xt[xi] = v;
  }
}

// grid (x: chunk of DSN_LOSS_CHUNK elements of a row, y: source slot, z: item)
__global__ void loss_reduce_kernel(const LossSde q, const float* __restrict__ sc, const float* __restrict__ z,
                                   const float* __restrict__ y, const float* __restrict__ x0,
                                   const float* __restrict__ tv, const float* __restrict__ sigma, int pit,
                                   double* __restrict__ part, int n, int D, int T, const int* __restrict__ tok) {
  __shared__ double red[LTPB / 64];
  const int c = blockIdx.x, s = blockIdx.y, b = blockIdx.z;
  const int chunks = gridDim.x;
  const long DT = (long)D * T;
  const int fb = tok ? tok[b] - 1 : T;  // the row's valid frames
  const long DF = (long)D * fb;
  if ((long)c * DSN_LOSS_CHUNK >= DF) return;  // uniform: a chunk past the item's end
  const double sg = (double)sigma[b];
  const double e = (double)(float)loss_decay(q, (double)tv[b]);
  const double ome = (double)(1.f - (float)e);
  const long r0 = (long)c * DSN_LOSS_CHUNK;
  const long r1 = r0 + DSN_LOSS_CHUNK < DF ? r0 + DSN_LOSS_CHUNK : DF;
  const int nj = pit ? n : 1;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (long k = r0 + threadIdx.x; k < r1; k += blockDim.x) {
    const int ch = (int)(k / fb), t = (int)(k - (long)ch * fb);
    const long r = (long)ch * T + t;  // (k itself when fb == T)
    const double sv = (double)sc[((long)b * T + t) * ((long)n * D) + (long)s * D + ch];
    const double base = sg * sv + (double)z[((long)b * n + s) * DT + r];
    if (!pit) {
      acc[0] += base * base;
    } else {
      const double ym = (double)y[b * DT + r];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < nj) {
          const double mean = e * (double)x0[((long)b * n + j) * DT + r] + ome * ym;
          const double v = base + (ym - mean) / sg;
          acc[j] += v * v;
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < nj) {   // (nj is uniform over the workgroup: every thread reaches the same barriers)
      const double v = loss_block_sum(acc[j], red);
      if (threadIdx.x == 0) part[(((long)b * n + s) * nj + j) * chunks + c] = v;
    }
  }
}

__global__ void loss_combine_kernel(const double* __restrict__ part, double* __restrict__ rows,
                                    float* __restrict__ out, int rows_n, int nj, int chunks, int n, int D, int T,
                                    int mean_reduction, const int* __restrict__ tok) {
  __shared__ double red[LTPB / 64];
  double acc = 0.0;
  for (int i = threadIdx.x; i < rows_n; i += blockDim.x) {
    double best = 0.0;
    const int fb = tok ? tok[i / n] - 1 : T, own = tok ? loss_chunks(D, fb) : chunks;  // chunks stays the stride
    const double len = (double)((long)D * fb);
    for (int j = 0; j < nj; ++j) {
      double v = 0.0;
      for (int c = 0; c < own; ++c) v += part[((long)i * nj + j) * chunks + c];
      v /= len;
      if (j == 0 || v < best) best = v;
    }
    rows[i] = best;
    acc += best;
    if (!mean_reduction) out[i] = (float)best;
  }
  if (mean_reduction) {
    acc = loss_block_sum(acc, red);
    if (threadIdx.x == 0) out[0] = (float)(acc / (double)rows_n);
  }
}

}  // namespace

void launch_loss_perturb(const LossSde& q, const float* y, const float* x0, const float* z, const float* t_in,
                         float t_const, const int* perm, int pit, float* xt, float* tv, float* sigma, int B, int n,
                         int D, int T, hipStream_t s, const int* tok) {
  const long DT = (long)D * T, per_item = DT * n;
  long gx = (per_item + 4L * LTPB - 1) / (4L * LTPB);
  if (gx > 256) gx = 256;
  hipLaunchKernelGGL(loss_perturb_kernel, dim3((unsigned)gx, (unsigned)B), dim3(LTPB), 0, s, q, y, x0, z, t_in,
                     t_const, perm, pit, xt, tv, sigma, n, DT, T, tok);
}

void launch_loss_reduce(const LossSde& q, const float* score_tok, const float* z, const float* y, const float* x0,
                        const float* tv, const float* sigma, int pit, double* part, int B, int n, int D, int T,
                        hipStream_t s, const int* tok) {
  hipLaunchKernelGGL(loss_reduce_kernel, dim3((unsigned)loss_chunks(D, T), (unsigned)n, (unsigned)B), dim3(LTPB), 0, s,
                     q, score_tok, z, y, x0, tv, sigma, pit, part, n, D, T, tok);
}

void launch_loss_combine(const double* part, double* rows, float* out, int B, int n, int nj, int chunks, int D, int T,
                         int mean_reduction, hipStream_t s, const int* tok) {
  hipLaunchKernelGGL(loss_combine_kernel, dim3(1), dim3(LTPB), 0, s, part, rows, out, B * n, nj, chunks, n,
                     D, T, mean_reduction, tok);
}
