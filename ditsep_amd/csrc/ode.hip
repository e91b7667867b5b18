// Probability-flow ODE sampler (reference src/sdes/__init__.py:196-281) on the device: an explicit embedded
// Runge-Kutta pair whose Butcher tableau is a parameter, with the step control of scipy 1.15's
// solve_ivp(method="RK45" | "RK23") -- RungeKutta._step_impl / rk_step / _estimate_error_norm and
// select_initial_step / norm of scipy/integrate/_ivp/{rk,common}.py -- restated in tests/ode_restatement.py.
//
// The ODE state y and the stage derivatives K_i are fp64 (scipy integrates in float64); the score network reads the
// fp32 cast of each stage point.  t, h and the controller flags live in OdeCtl (device memory), so one attempt is the
// same launch sequence every time (prep, then per stage: score call + ode_stage_kernel, then ode_control_kernel) and
// can be captured once and replayed; once `done` is set every kernel of an attempt returns at once.  The error norm is
// a fixed-order fp64 sum (per-block partials, one-block finisher): reruns are bit-identical.
//
// Arithmetic is not contracted into FMAs here, so that each fp64 formula rounds as numpy evaluates it.  The two fp32
// steps the sampler shares with the PC sampler -- the prior draw and the noise-free reverse-diffusion step -- run on
// the PC sampler's own kernels (launch_pc_prior, launch_pc_predictor), not on restatements of them.
#include "../../include/ditsep_hip.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int OTPB = 256;

// x[B,n,D,T] linear index -> y[B,1,D,T] index and token-major score [B*T][n*D] index (as pc_index, kernels.hip)
__device__ __forceinline__ void ode_index(long i, int n, int D, int T, long& yi, long& si) {
  const int t = (int)(i % T);
  long r = i / T;
  const int c = (int)(r % D);
  r /= D;
  const int s = (int)(r % n);
  const long b = r / n;
  yi = (b * D + c) * T + t;
  si = (b * T + t) * ((long)n * D) + (long)s * D + c;
}

// g(t)^2 of the OUVE SDE: (sigma_min (sigma_max / sigma_min)^t)^2 * 2 log(sigma_max / sigma_min)
__device__ __forceinline__ double ode_g2(const OdeSde& q, double t) {
  const double sigma = q.sigma_min * pow(q.ratio, t);
  return sigma * sigma * (2.0 * q.logratio);
}

// probability-flow drift: theta (y - x) - 1/2 g^2 s
__device__ __forceinline__ double ode_drift(const OdeSde& q, double half_g2, float ymix, double x, float s) {
  return q.theta * ((double)ymix - x) - half_g2 * (double)s;
}

// fixed-order block sum of one fp64 value per thread; the result is valid in thread 0
__device__ double block_sum(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
  __syncthreads();
  return s;
}

__device__ void write_times(float* tv, int B, double t) {
  if (blockIdx.x == 0)
    for (int b = threadIdx.x; b < B; b += blockDim.x) tv[b] = (float)t;
}

// ---------------------------------------------------------------- controller (one thread)
// scipy RungeKutta._step_impl: at the start of a step min_step is taken at t and h_abs clamped to [min_step, max_step]
__device__ void ctl_set_h(OdeCtl* c) {
  if (c->h_abs < c->min_step) {  // `if h_abs < min_step: return False, self.TOO_SMALL_STEP`
    c->done = 1;
    c->status = DSN_ODE_STEP_TOO_SMALL;
    return;
  }
  double h = c->h_abs * c->direction;
  double t_new = c->t + h;
  if (c->direction * (t_new - c->t_bound) > 0) t_new = c->t_bound;
  h = t_new - c->t;
  c->h = h;
  c->t_new = t_new;
  c->h_abs = fabs(h);
}
__device__ void ctl_begin_step(OdeCtl* c) {
  c->min_step = 10.0 * fabs(nextafter(c->t, c->direction * INFINITY) - c->t);
  if (c->h_abs > c->max_step) c->h_abs = c->max_step;
  else if (c->h_abs < c->min_step) c->h_abs = c->min_step;
  c->step_rejected = 0;
  ctl_set_h(c);
}

// ---------------------------------------------------------------- kernels
// state y0 = x_T exactly: the fp32 prior launch_pc_prior wrote into xs32 (the PC sampler's own kernel, so a seed or
// injected noise gives bit for bit the x_T dsn_pc_sample starts from), widened; tv = t0
__global__ void ode_widen_prior_kernel(const float* __restrict__ xs32, double* __restrict__ y, float* __restrict__ tv,
                                       double t0, int B, long total) {
  write_times(tv, B, t0);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x)
    y[i] = (double)xs32[i];
}

// select_initial_step, first half: f0 = fun(t0, y0) -> K0; partials of sum (y0/scale)^2 and sum (f0/scale)^2,
// scale = atol + |y0| rtol
__global__ void ode_init_f0_kernel(const OdeSde q, const OdeCtl* __restrict__ ctl, const float* __restrict__ ymix,
                                   const float* __restrict__ sc, const double* __restrict__ y, double* __restrict__ K0,
                                   double* __restrict__ part, int n, int D, int T, long total) {
  __shared__ double red[OTPB / 64];
  const double half_g2 = 0.5 * ode_g2(q, ctl->t);
  const double rtol = ctl->rtol, atol = ctl->atol;
  double s0 = 0.0, s1 = 0.0;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    long yi, si;
    ode_index(i, n, D, T, yi, si);
    const double f = ode_drift(q, half_g2, ymix[yi], y[i], sc[si]);
    K0[i] = f;
    const double scale = atol + fabs(y[i]) * rtol;
    const double a = y[i] / scale, b = f / scale;
    s0 += a * a;
    s1 += b * b;
  }
  s0 = block_sum(s0, red);
  s1 = block_sum(s1, red);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = s0;
    part[gridDim.x + blockIdx.x] = s1;
  }
}

// d0, d1 -> h0 (or the caller's first step: then the first step begins here)
__global__ void ode_init_h0_kernel(OdeCtl* __restrict__ ctl, const double* __restrict__ part, int nblk, long total) {
  if (threadIdx.x != 0) return;
  double s0 = 0.0, s1 = 0.0;
  for (int k = 0; k < nblk; ++k) {
    s0 += part[k];
    s1 += part[nblk + k];
  }
  OdeCtl* c = ctl;
  const double rn = sqrt((double)total);
  c->nfev = 1;
  if (c->first_step > 0) {
    c->h_abs = c->first_step;
    ctl_begin_step(c);
    return;
  }
  const double d0 = sqrt(s0) / rn, d1 = sqrt(s1) / rn;
  double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
  const double interval = fabs(c->t_bound - c->t);
  h0 = fmin(h0, interval);
  c->h0 = h0;
  c->d1 = d1;
}

// y1 = y0 + h0 direction f0 (stage point of the extra evaluation), tv = t0 + h0 direction
__global__ void ode_init_y1_kernel(const OdeCtl* __restrict__ ctl, const double* __restrict__ y,
                                   const double* __restrict__ K0, double* __restrict__ xs64, float* __restrict__ xs32,
                                   float* __restrict__ tv, int B, long total) {
  const double hd = ctl->h0 * ctl->direction;
  write_times(tv, B, ctl->t + hd);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const double v = y[i] + hd * K0[i];
    xs64[i] = v;
    xs32[i] = (float)v;
  }
}

// f1 = fun(t0 + h0 direction, y1); partials of sum ((f1 - f0)/scale)^2
__global__ void ode_init_f1_kernel(const OdeSde q, const OdeCtl* __restrict__ ctl, const float* __restrict__ ymix,
                                   const float* __restrict__ sc, const double* __restrict__ y,
                                   const double* __restrict__ K0, const double* __restrict__ xs64,
                                   double* __restrict__ part, int n, int D, int T, long total) {
  __shared__ double red[OTPB / 64];
  const double half_g2 = 0.5 * ode_g2(q, ctl->t + ctl->h0 * ctl->direction);
  const double rtol = ctl->rtol, atol = ctl->atol;
  double s = 0.0;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    long yi, si;
    ode_index(i, n, D, T, yi, si);
    const double f1 = ode_drift(q, half_g2, ymix[yi], xs64[i], sc[si]);
    const double scale = atol + fabs(y[i]) * rtol;
    const double a = (f1 - K0[i]) / scale;
    s += a * a;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// d2 -> h1 -> the first step size; the first step begins
__global__ void ode_init_h1_kernel(OdeCtl* __restrict__ ctl, const double* __restrict__ part, int nblk, long total,
                                   int err_order) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int k = 0; k < nblk; ++k) s += part[k];
  OdeCtl* c = ctl;
  const double h0 = c->h0, d1 = c->d1;
  const double d2 = sqrt(s) / sqrt((double)total) / h0;
  double h1;
  if (d1 <= 1e-15 && d2 <= 1e-15) h1 = fmax(1e-6, h0 * 1e-3);
  else h1 = pow(0.01 / fmax(d1, d2), 1.0 / (double)(err_order + 1));
  const double interval = fabs(c->t_bound - c->t);
  c->h_abs = fmin(fmin(100 * h0, h1), fmin(interval, c->max_step));
  c->nfev = 2;
  ctl_begin_step(c);
}

// first stage point of an attempt: apply the previous attempt's acceptance (y <- y_new, K0 <- f_new), then
// x_1 = y + (K0 a10) h, tv = t + c1 h
__global__ void ode_prep_kernel(const OdeTableau tab, const OdeCtl* __restrict__ ctl, double* __restrict__ y,
                                const double* __restrict__ yn, double* __restrict__ K, double* __restrict__ xs64,
                                float* __restrict__ xs32, float* __restrict__ tv, int B, long total) {
  if (ctl->done) return;
  const double t = ctl->t, h = ctl->h;
  const bool acc = ctl->accept_pending != 0;
  const int S = tab.stages;
  write_times(tv, B, t + tab.c[1] * h);
  double* K0 = K;
  const double* KS = K + (long)S * total;
  const double a10 = tab.a[1][0];
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    double yv, k0;
    if (acc) {
      yv = yn[i];
      k0 = KS[i];
      y[i] = yv;
      K0[i] = k0;
    } else {
      yv = y[i];
      k0 = K0[i];
    }
    const double v = yv + (k0 * a10) * h;
    xs64[i] = v;
    xs32[i] = (float)v;
  }
}

// After the score call of stage `st` (1 .. S): K_st = drift(stage point, score, t_st), then
//   st < S-1 : the next stage point x_{st+1} = y + (sum_{j<=st} K_j a[st+1][j]) h        (fp64 + fp32 copy, tv)
//   st = S-1 : y_new = y + h (sum_{j<S} K_j b_j)                                          (fp64 + fp32 copy, tv = t + h)
//   st = S   : (FSAL f_new) err = (sum_{j<=S} K_j e_j) h, per-block partial of sum (err/scale)^2,
//              scale = atol + max(|y|, |y_new|) rtol
__global__ void ode_stage_kernel(const OdeTableau tab, const OdeSde q, const OdeCtl* __restrict__ ctl, int st,
                                 const float* __restrict__ ymix, const float* __restrict__ sc,
                                 const double* __restrict__ y, double* __restrict__ yn, double* __restrict__ K,
                                 double* __restrict__ xs64, float* __restrict__ xs32, float* __restrict__ tv,
                                 double* __restrict__ part, int B, int n, int D, int T, long total) {
  if (ctl->done) return;
  __shared__ double red[OTPB / 64];
  const int S = tab.stages;
  const double t = ctl->t, h = ctl->h;
  const double ti = st < S ? t + tab.c[st] * h : t + h;
  const double half_g2 = 0.5 * ode_g2(q, ti);
  const double rtol = ctl->rtol, atol = ctl->atol;
  if (st < S - 1) write_times(tv, B, t + tab.c[st + 1] * h);
  else if (st == S - 1) write_times(tv, B, t + h);
  double acc = 0.0;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    long yi, si;
    ode_index(i, n, D, T, yi, si);
    const double xi = st < S ? xs64[i] : yn[i];
    K[(long)st * total + i] = ode_drift(q, half_g2, ymix[yi], xi, sc[si]);
    const double yv = y[i];
    if (st < S) {
      const double* w = st < S - 1 ? tab.a[st + 1] : tab.b;
      double d = 0.0;
      for (int j = 0; j <= st; ++j) d += K[(long)j * total + i] * w[j];
      if (st < S - 1) {
        const double v = yv + d * h;
        xs64[i] = v;
        xs32[i] = (float)v;
      } else {
        const double v = yv + h * d;
        yn[i] = v;
        xs32[i] = (float)v;
      }
    } else {
      double e = 0.0;
      for (int j = 0; j <= S; ++j) e += K[(long)j * total + i] * tab.e[j];
      e = e * h;
      const double scale = atol + fmax(fabs(yv), fabs(yn[i])) * rtol;
      const double r = e / scale;
      acc += r * r;
    }
  }
  if (st == S) {
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
  }
}

// the controller's work for one attempt (scipy RungeKutta._step_impl after rk_step)
__global__ void ode_control_kernel(OdeCtl* __restrict__ ctl, const double* __restrict__ part, int nblk, long total,
                                   int stages, int err_order) {
  if (threadIdx.x != 0) return;
  OdeCtl* c = ctl;
  if (c->done) return;
  double s = 0.0;
  for (int k = 0; k < nblk; ++k) s += part[k];
  const double error_norm = sqrt(s) / sqrt((double)total);
  const double expo = -1.0 / (double)(err_order + 1);
  c->nfev += stages;
  c->attempts += 1;
  if (error_norm < 1) {
    double factor = error_norm == 0 ? 10.0 : fmin(10.0, 0.9 * pow(error_norm, expo));
    if (c->step_rejected) factor = fmin(1.0, factor);
    c->h_abs *= factor;
    c->t = c->t_new;
    c->accept_pending = 1;
    c->accepted += 1;
    if (c->direction * (c->t - c->t_bound) >= 0) {
      c->done = 1;
      c->status = DSN_ODE_FINISHED;
      return;
    }
    ctl_begin_step(c);
  } else {
    c->h_abs *= fmax(0.2, 0.9 * pow(error_norm, expo));
    c->step_rejected = 1;
    c->accept_pending = 0;
    c->rejected += 1;
    ctl_set_h(c);
  }
  if (!c->done && c->attempts >= c->max_attempts) {
    c->done = 1;
    c->status = DSN_ODE_TOO_MANY_ATTEMPTS;
  }
}

// final state as fp32 (the reference's .type(complex64) of solution.y[:, -1]): y, or y_new when the last attempt was
// accepted; tv = t_eps for the denoising score call
__global__ void ode_emit_kernel(const OdeCtl* __restrict__ ctl, const double* __restrict__ y,
                                const double* __restrict__ yn, float* __restrict__ out, float* __restrict__ tv,
                                float t_eps, int B, long total) {
  const bool acc = ctl->accept_pending != 0;
  write_times(tv, B, (double)t_eps);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x)
    out[i] = (float)(acc ? yn[i] : y[i]);
}

}  // namespace

int ode_grid(long total) {
  long g = (total + OTPB - 1) / OTPB;
  return (int)(g < 1 ? 1 : (g > 1024 ? 1024 : g));
}

void launch_ode_prior(const float* ymix, const float* z, double* y, float* xs32, float* tv, float stdT, int B, int n,
                      int D, int T, hipStream_t s) {
  const long total = (long)B * n * D * T;
  launch_pc_prior(ymix, 0, z, xs32, stdT, B, n, D, T, s);
  hipLaunchKernelGGL(ode_widen_prior_kernel, dim3(ode_grid(total)), dim3(OTPB), 0, s, xs32, y, tv, 1.0, B, total);
}
void launch_ode_init_f0(const OdeSde& q, const OdeCtl* ctl, const float* ymix, const float* sc, const double* y,
                        double* K0, double* part, int B, int n, int D, int T, hipStream_t s) {
  const long total = (long)B * n * D * T;
  hipLaunchKernelGGL(ode_init_f0_kernel, dim3(ode_grid(total)), dim3(OTPB), 0, s, q, ctl, ymix, sc, y, K0, part, n, D,
                     T, total);
}
void launch_ode_init_h0(OdeCtl* ctl, const double* part, long total, hipStream_t s) {
  hipLaunchKernelGGL(ode_init_h0_kernel, dim3(1), dim3(64), 0, s, ctl, part, ode_grid(total), total);
}
void launch_ode_init_y1(const OdeCtl* ctl, const double* y, const double* K0, double* xs64, float* xs32, float* tv,
                        int B, long total, hipStream_t s) {
  hipLaunchKernelGGL(ode_init_y1_kernel, dim3(ode_grid(total)), dim3(OTPB), 0, s, ctl, y, K0, xs64, xs32, tv, B,
                     total);
}
void launch_ode_init_f1(const OdeSde& q, const OdeCtl* ctl, const float* ymix, const float* sc, const double* y,
                        const double* K0, const double* xs64, double* part, int B, int n, int D, int T, hipStream_t s) {
  const long total = (long)B * n * D * T;
  hipLaunchKernelGGL(ode_init_f1_kernel, dim3(ode_grid(total)), dim3(OTPB), 0, s, q, ctl, ymix, sc, y, K0, xs64, part,
                     n, D, T, total);
}
void launch_ode_init_h1(OdeCtl* ctl, const double* part, long total, int err_order, hipStream_t s) {
  hipLaunchKernelGGL(ode_init_h1_kernel, dim3(1), dim3(64), 0, s, ctl, part, ode_grid(total), total, err_order);
}
void launch_ode_prep(const OdeTableau& tab, const OdeCtl* ctl, double* y, const double* yn, double* K, double* xs64,
                     float* xs32, float* tv, int B, long total, hipStream_t s) {
  hipLaunchKernelGGL(ode_prep_kernel, dim3(ode_grid(total)), dim3(OTPB), 0, s, tab, ctl, y, yn, K, xs64, xs32, tv, B,
                     total);
}
void launch_ode_stage(const OdeTableau& tab, const OdeSde& q, const OdeCtl* ctl, int stage, const float* ymix,
                      const float* sc, const double* y, double* yn, double* K, double* xs64, float* xs32, float* tv,
                      double* part, int B, int n, int D, int T, hipStream_t s) {
  const long total = (long)B * n * D * T;
  hipLaunchKernelGGL(ode_stage_kernel, dim3(ode_grid(total)), dim3(OTPB), 0, s, tab, q, ctl, stage, ymix, sc, y, yn, K,
                     xs64, xs32, tv, part, B, n, D, T, total);
}
void launch_ode_control(OdeCtl* ctl, const double* part, long total, int stages, int err_order, hipStream_t s) {
  hipLaunchKernelGGL(ode_control_kernel, dim3(1), dim3(64), 0, s, ctl, part, ode_grid(total), total, stages,
                     err_order);
}
void launch_ode_emit(const OdeCtl* ctl, const double* y, const double* yn, float* out, float* tv, float t_eps, int B,
                     long total, hipStream_t s) {
  hipLaunchKernelGGL(ode_emit_kernel, dim3(ode_grid(total)), dim3(OTPB), 0, s, ctl, y, yn, out, tv, t_eps, B, total);
}
