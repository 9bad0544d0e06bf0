// Optimisers on the flat parameter buffer: the default step's Adam (adam_step), the same behind the fp16 loss scaler
// (adam_step_scaled), and the guarded forms: global gradient norm, SGD / Nesterov, Adam / AdamW behind it.  Every piece is written once:
// adam_lines / sgd_lines (one element), opt_walk (the grid-stride walk over the buffers), scaler_rule (the loss scaler's update).
//   grad_norm   two launches, no atomics: one fp32 partial per workgroup (sum of (g * gscale)^2), then one workgroup adds the partials
//               in a fixed order in fp64 and writes the optimiser state {sumsq, norm, coef, nonfinite}.  The grid is a function of
//               `count` alone, so the same buffer gives the same bits.
//   sgd_step    torch.optim.SGD (dampening 0) with the clip coefficient and the skip rule read from the optimiser state
//   adamw_step  torch.optim.Adam (L2 decay) or torch.optim.AdamW (decoupled decay), likewise
// Nothing waits for the host: the update kernels read `coef`, `nonfinite` and the step count from device memory, as adam_scaled_kernel
// reads the loss scaler's state.  A step whose sum of squares is not finite is skipped entirely: parameters, moments,
// momentum buffer and step count stay bit-unchanged and the skipped-steps counter goes up.  That covers every NaN / +-inf gradient
// AND a finite gradient whose scaled square overflows fp32 (|g * gscale| above about 1.8e19): such a step is skipped too.
//
// Optimiser state `ost` (device, 8 floats): {sumsq, norm, coef, nonfinite, steps taken, steps skipped, -, -}.  A fresh state is
// {0, 0, 1, 0, 0, 0, 0, 0}.  With a loss-scaler state (8 floats, see scaler_rule) the two counts live THERE (entries 2 and 4) and
// ost[4], ost[5] are left alone; the scaler's found_inf is raised together with `nonfinite`, so its scale-update rule runs unchanged and
// the norm pass replaces grad_check_kernel's sweep.
#include "common.h"

namespace mednet {

constexpr size_t OPT_MAX_ROWS = 2048;       // memory-bound pass: at most 256 CUs x 8 workgroups, the rest is grid-strided
constexpr size_t ADAM_MAX_ROWS = 8192;      // adam_step / adam_step_scaled: the grid they have always had
constexpr size_t NORM_PER_BLOCK = 4096;     // 256 threads x 4 accumulators x one 16-byte load each
constexpr size_t UPDATE_PER_BLOCK = 1024;   // 256 threads x one 16-byte load per buffer

// the factor every gradient is multiplied by before anything else: 1/world, over the loss scale when a scaler state is given
__device__ __forceinline__ float opt_gscale(float inv_world, const float* __restrict__ sc) { return sc ? inv_world / sc[0] : inv_world; }

__device__ __forceinline__ float sumsq4(f32x4 x, float gscale, float acc) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float s = x[k] * gscale;  // scaled BEFORE it is squared: a loss scale of 2^16 cannot overflow the sum
    acc = fmaf(s, s, acc);
  }
  return acc;
}

// ---------------------------------------------------------------------------------------------- global norm, partial pass
// Elements [0, head) in front of the first 16-byte boundary and the last (count - head) % 4 are read one by one by workgroup 0
// (threads 0..2 and 4..6); the float4s between them are grid-strided, four independent accumulators per thread.
__global__ __launch_bounds__(256) void grad_sumsq_partial_kernel(const float* __restrict__ g, size_t count, float inv_world,
                                                                 const float* __restrict__ sc, float* __restrict__ partial) {
  __shared__ float red[4];
  const float gscale = opt_gscale(inv_world, sc);
  size_t head = ((16 - ((uintptr_t)g & 15)) & 15) >> 2;
  if (head > count) head = count;
  const size_t nvec = (count - head) >> 2, tail = (count - head) & 3;
  const f32x4* __restrict__ gv = reinterpret_cast<const f32x4*>(g + head);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (blockIdx.x == 0) {
    const unsigned t = threadIdx.x;
    if (t < head) {
      const float s = g[t] * gscale;
      a0 = s * s;
    } else if (t >= 4 && t - 4 < tail) {
      const float s = g[head + 4 * nvec + (t - 4)] * gscale;
      a0 = s * s;
    }
  }
  const size_t stride = (size_t)gridDim.x * 256;
  size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (; v + 3 * stride < nvec; v += 4 * stride) {
    const f32x4 x0 = gv[v], x1 = gv[v + stride], x2 = gv[v + 2 * stride], x3 = gv[v + 3 * stride];
    a0 = sumsq4(x0, gscale, a0);
    a1 = sumsq4(x1, gscale, a1);
    a2 = sumsq4(x2, gscale, a2);
    a3 = sumsq4(x3, gscale, a3);
  }
  for (; v < nvec; v += stride) a0 = sumsq4(gv[v], gscale, a0);
  const float s = block_sum<4>((a0 + a1) + (a2 + a3), red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// ---------------------------------------------------------------------------------------------- global norm, finalize
// One workgroup: thread t adds rows t, t + 256, .. in fp64, then the wave tree and the four waves in order.  Every field is ONE
// rounding from the fp64 value.  coef = min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_), 1 when max_norm == 0.
__global__ __launch_bounds__(256) void grad_norm_finalize_kernel(const float* __restrict__ partial, unsigned rows, float max_norm,
                                                                 float* __restrict__ ost, float* __restrict__ sc) {
  __shared__ double red[4];
  double s = 0.0;
  for (unsigned i = threadIdx.x; i < rows; i += 256) s += (double)partial[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double sum = ((red[0] + red[1]) + red[2]) + red[3];
  const double norm = sqrt(sum);
  const float sumsq32 = (float)sum;
  const bool bad = !(fabsf(sumsq32) <= 3.0e38f);  // NaN, inf, or a sum beyond fp32
  ost[0] = sumsq32;
  ost[1] = (float)norm;
  ost[2] = max_norm > 0.f ? (float)fmin(1.0, (double)max_norm / (norm + 1e-6)) : 1.f;
  ost[3] = bad ? 1.f : 0.f;
  if (bad && sc) sc[3] = 1.f;
}

// ---------------------------------------------------------------------------------------------- updates
// does this step run?  (nonfinite of the norm pass, or a found_inf somebody else raised)
__device__ __forceinline__ bool opt_skip(const float* __restrict__ ost, const float* __restrict__ sc) {
  return (ost && ost[3] != 0.f) || (sc && sc[3] != 0.f);
}

template <bool MOM, bool NESTEROV>
__device__ __forceinline__ void sgd_lines(float& p, float g, float& buf, float lr, float mu, float wd, float gscale, float coef) {
  float gr = (g * gscale) * coef;
  if (wd != 0.f) gr = fmaf(wd, p, gr);
  float d = gr;
  if (MOM) {
    buf = fmaf(mu, buf, gr);
    d = NESTEROV ? fmaf(mu, buf, gr) : buf;
  }
  p = fmaf(-lr, d, p);
}

// One element of Adam: L2 decay folded into the gradient, or (DECOUPLED) p *= 1 - lr wd first and no L2 term.  `coef` is the clip
// coefficient; the kernels without a norm pass hand in 1.f, and a product with 1 is exact.
template <bool DECOUPLED>
__device__ __forceinline__ void adam_lines(float& p, float g, float& m, float& v, float lr, float b1, float b2, float eps, float wd,
                                           float bc1, float bc2_sqrt, float gscale, float coef) {
  float gr = (g * gscale) * coef;
  float pi = p;
  if (wd != 0.f) {
    if (DECOUPLED)
      pi = p * (1.f - lr * wd);
    else
      gr = fmaf(wd, p, gr);
  }
  const float mi = b1 * m + (1.f - b1) * gr;
  const float vi = b2 * v + (1.f - b2) * gr * gr;
  m = mi;
  v = vi;
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  p = pi - (lr / bc1) * (mi / denom);
}

// ---------------------------------------------------------------------------------------------- the walk
// The buffers an update rewrites in place: x[0] the parameters, then NB - 1 of {momentum buffer} or {m, v}.
struct OptBufs {
  float* x[3];
};

// Elements [VEC i, VEC i + VEC) of every buffer through `lines(g, e)`, e[j] one element of x[j]: 16-byte loads and stores at VEC = 4.
template <int VEC, int NB, typename F>
__device__ __forceinline__ void opt_item(const OptBufs& b, const float* g, size_t i, F lines) {
  if constexpr (VEC == 4) {
    f32x4 x[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) x[j] = reinterpret_cast<const f32x4*>(b.x[j])[i];
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float e[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) e[j] = x[j][k];
      lines(gv[k], e);
#pragma unroll
      for (int j = 0; j < NB; ++j) x[j][k] = e[j];
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) reinterpret_cast<f32x4*>(b.x[j])[i] = x[j];
  } else {
    float e[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) e[j] = b.x[j][i];
    lines(g[i], e);
#pragma unroll
    for (int j = 0; j < NB; ++j) b.x[j][i] = e[j];
  }
}

// The grid-stride walk of every update kernel (256 threads).  VEC = 4: every pointer is 16-byte aligned, the count % 4 trailing
// elements go to workgroup 0 one by one.  VEC = 1: any alignment.  `lines` is taken BY VALUE (what it captured stays in registers).
template <int VEC, int NB, typename F>
__device__ __forceinline__ void opt_walk(const OptBufs b, const float* g, size_t count, F lines) {
  const size_t stride = (size_t)gridDim.x * 256, n = count / VEC;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) opt_item<VEC, NB>(b, g, i, lines);
  if (VEC == 4 && blockIdx.x == 0 && threadIdx.x < (count & 3)) opt_item<1, NB>(b, g, 4 * n + threadIdx.x, lines);
}

// ---------------------------------------------------------------------------------------------- update kernels
template <int VEC, bool MOM, bool NESTEROV>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                  size_t count, float lr, float mu, float wd, float inv_world,
                                                  const float* __restrict__ ost, const float* __restrict__ sc) {
  if (opt_skip(ost, sc)) return;
  const float coef = ost ? ost[2] : 1.f, gscale = opt_gscale(inv_world, sc);
  constexpr int NB = MOM ? 2 : 1;
  opt_walk<VEC, NB>(OptBufs{{p, buf, nullptr}}, g, count, [=](float gk, float(&e)[NB]) {
    float none = 0.f;
    sgd_lines<MOM, NESTEROV>(e[0], gk, MOM ? e[NB - 1] : none, lr, mu, wd, gscale, coef);
  });
}

// The default step's update (no norm pass, no device state): the bias corrections come from the host entry.
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, size_t count, float lr, float b1, float b2, float eps, float wd,
                                                   float bc1, float bc2_sqrt, float gscale) {
  opt_walk<1, 3>(OptBufs{{p, m, v}}, g, count, [=](float gk, float(&e)[3]) {
    adam_lines<false>(e[0], gk, e[1], e[2], lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale, 1.f);
  });
}

// Adam behind the norm pass (ost: clip coefficient, skip rule, step count) and / or a loss scaler (sc: scale, found_inf, its own step
// count).  The bias correction uses the device-side count of steps actually taken, which a skipped step does not advance.
template <int VEC, bool DECOUPLED>
__device__ __forceinline__ void adam_device_state(float* p, const float* g, float* m, float* v, size_t count, float lr, float b1,
                                                  float b2, float eps, float wd, float inv_world, const float* ost, const float* sc) {
  if (opt_skip(ost, sc)) return;
  const float t = (sc ? sc[2] : ost[4]) + 1.f;
  const float bc1 = 1.f - powf(b1, t), bc2_sqrt = sqrtf(1.f - powf(b2, t));
  const float coef = ost ? ost[2] : 1.f, gscale = opt_gscale(inv_world, sc);
  opt_walk<VEC, 3>(OptBufs{{p, m, v}}, g, count, [=](float gk, float(&e)[3]) {
    adam_lines<DECOUPLED>(e[0], gk, e[1], e[2], lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale, coef);
  });
}

template <int VEC, bool DECOUPLED>
__global__ __launch_bounds__(256) void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, size_t count, float lr, float b1, float b2, float eps,
                                                           float wd, float inv_world, const float* __restrict__ ost,
                                                           const float* __restrict__ sc) {
  adam_device_state<VEC, DECOUPLED>(p, g, m, v, count, lr, b1, b2, eps, wd, inv_world, ost, sc);
}

// ---- fp16 storage: dynamic loss scaling without a host synchronisation (torch.cuda.amp.GradScaler's rule) ---------------
// state[8] (device, fp32): {scale, good steps since the last change, optimizer steps taken, found_inf, steps skipped, -, -, -}.  The loss is
// multiplied by state[0] on the device, so every gradient arrives times `scale`; grad_check raises found_inf if any gradient is not
// finite, adam_scaled divides by the scale and SKIPS the update when found_inf is set, scaler_rule then halves the scale or counts a
// good step and doubles it every `growth_interval` of them.
__global__ __launch_bounds__(256) void grad_check_kernel(const float* __restrict__ g, size_t count, float* __restrict__ state) {
  const size_t stride = (size_t)gridDim.x * 256;
  bool bad = false;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
    const float v = g[i];
    bad |= !(fabsf(v) <= 3.0e38f);  // NaN or +-inf
  }
  if (bad) state[3] = 1.f;  // (every writer stores the same value)
}

// (kept as a kernel of its own over the shared body: its grid, scalar walk and name are the ones adam_step_scaled always launched)
__global__ __launch_bounds__(256) void adam_scaled_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, size_t count, float lr, float b1, float b2, float eps,
                                                          float wd, float inv_world, const float* __restrict__ state) {
  adam_device_state<1, false>(p, g, m, v, count, lr, b1, b2, eps, wd, inv_world, nullptr, state);
}

__device__ __forceinline__ void scaler_rule(float* __restrict__ sc, bool bad, float growth, float backoff, float interval) {
  if (bad) {
    sc[0] = fmaxf(sc[0] * backoff, 1.f);  // never below 1: a persistent NaN (out-of-range labels) must not drive it to 0
    sc[1] = 0.f;
    sc[4] += 1.f;  // skipped steps, for the host to surface
  } else {
    sc[2] += 1.f;
    sc[1] += 1.f;
    if (sc[1] >= interval) {
      sc[0] *= growth;
      sc[1] = 0.f;
    }
  }
  sc[3] = 0.f;
}

__global__ void scaler_update_kernel(float* __restrict__ state, float growth, float backoff, float interval) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  scaler_rule(state, state[3] != 0.f, growth, backoff, interval);
}

// After a guarded update: the scaler's rule when there is a scaler state, otherwise the two counters of the optimiser state.
// `nonfinite` is cleared either way; sumsq / norm / coef stay for the caller to read.
__global__ void optim_state_update_kernel(float* __restrict__ ost, float* __restrict__ sc, float growth, float backoff, float interval) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (sc)
    scaler_rule(sc, sc[3] != 0.f || ost[3] != 0.f, growth, backoff, interval);
  else
    ost[ost[3] != 0.f ? 5 : 4] += 1.f;
  ost[3] = 0.f;
}

}  // namespace mednet

// =================================================================================================== C ABI
using namespace mednet;

static inline bool aligned16(const void* a) { return ((uintptr_t)a & 15) == 0; }

extern "C" size_t mednet_grad_norm_ws_bytes(size_t count) {
  if (count == 0) return 0;
  return (size_t)strided_grid(count, NORM_PER_BLOCK, OPT_MAX_ROWS) * sizeof(float);
}

extern "C" int mednet_grad_norm(const float* g, size_t count, float inv_world, float* scaler_state, float max_norm,
                                float* opt_state, void* ws, size_t ws_bytes, mednet_stream stream) {
  float* sc = scaler_state;  // (may be null; found_inf is raised on a non-finite sum)
  MEDNET_REQUIRE(g && opt_state && ws, MEDNET_E_SHAPE, "grad_norm: null pointer");
  MEDNET_REQUIRE(count > 0, MEDNET_E_SHAPE, "grad_norm: count is 0");
  MEDNET_REQUIRE(max_norm >= 0.f, MEDNET_E_SHAPE, "grad_norm: max_norm %g is negative or NaN", (double)max_norm);
  MEDNET_REQUIRE(ws_bytes >= mednet_grad_norm_ws_bytes(count), MEDNET_E_WORKSPACE, "grad_norm: workspace %zu < %zu bytes", ws_bytes,
                 mednet_grad_norm_ws_bytes(count));
  MEDNET_REQUIRE(((uintptr_t)g & 3) == 0 && ((uintptr_t)ws & 3) == 0, MEDNET_E_SHAPE, "grad_norm: pointer not 4-byte aligned");
  const unsigned rows = strided_grid(count, NORM_PER_BLOCK, OPT_MAX_ROWS);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(grad_sumsq_partial_kernel, dim3(rows), dim3(256), 0, s, g, count, inv_world, (const float*)sc, (float*)ws);
  const int rc = check_launch("grad_norm(partials)");
  if (rc != MEDNET_OK) return rc;
  hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(256), 0, s, (const float*)ws, rows, max_norm, opt_state, sc);
  return check_launch("grad_norm");
}

extern "C" int mednet_sgd_step(float* p, const float* g, float* buf, size_t count, float lr, float momentum, int nesterov,
                               float weight_decay, float inv_world, float* opt_state, float* scaler_state, float growth_factor,
                               float backoff_factor, int growth_interval, mednet_stream stream) {
  MEDNET_REQUIRE(p && g, MEDNET_E_SHAPE, "sgd_step: null pointer");
  MEDNET_REQUIRE(count > 0, MEDNET_E_SHAPE, "sgd_step: count is 0");
  MEDNET_REQUIRE(momentum >= 0.f && momentum < 1.f, MEDNET_E_SHAPE, "sgd_step: momentum %g outside [0, 1)", (double)momentum);
  MEDNET_REQUIRE(lr >= 0.f && weight_decay >= 0.f, MEDNET_E_SHAPE, "sgd_step: negative lr %g or weight_decay %g", (double)lr,
                 (double)weight_decay);
  MEDNET_REQUIRE(!(nesterov && momentum == 0.f), MEDNET_E_SHAPE, "sgd_step: nesterov needs momentum > 0");
  MEDNET_REQUIRE(momentum == 0.f || buf, MEDNET_E_SHAPE, "sgd_step: null pointer (momentum buffer)");
  MEDNET_REQUIRE(opt_state || !scaler_state, MEDNET_E_SHAPE, "sgd_step: null pointer (a scaler state needs the optimiser state)");
  MEDNET_REQUIRE(!scaler_state || growth_interval >= 1, MEDNET_E_SHAPE, "sgd_step: growth_interval %d", growth_interval);
  hipStream_t s = (hipStream_t)stream;
  const bool mom = momentum != 0.f, vec = aligned16(p) && aligned16(g) && (!mom || aligned16(buf));
  const dim3 grid(strided_grid(count, UPDATE_PER_BLOCK, OPT_MAX_ROWS)), block(256);
  const float* ost = opt_state;
  const float* sc = scaler_state;
#define MEDNET_SGD_LAUNCH(V, M, N) \
  hipLaunchKernelGGL((sgd_kernel<V, M, N>), grid, block, 0, s, p, g, buf, count, lr, momentum, weight_decay, inv_world, ost, sc)
  if (vec) {
    if (!mom) MEDNET_SGD_LAUNCH(4, false, false);
    else if (nesterov) MEDNET_SGD_LAUNCH(4, true, true);
    else MEDNET_SGD_LAUNCH(4, true, false);
  } else {
    if (!mom) MEDNET_SGD_LAUNCH(1, false, false);
    else if (nesterov) MEDNET_SGD_LAUNCH(1, true, true);
    else MEDNET_SGD_LAUNCH(1, true, false);
  }
#undef MEDNET_SGD_LAUNCH
  if (opt_state)
    hipLaunchKernelGGL(optim_state_update_kernel, dim3(1), dim3(64), 0, s, opt_state, scaler_state, growth_factor, backoff_factor,
                       (float)growth_interval);
  return check_launch("sgd_step");
}

extern "C" int mednet_adamw_step(float* p, const float* g, float* m, float* v, size_t count, float lr, float beta1, float beta2,
                                 float eps, float weight_decay, int decoupled, float inv_world, float* opt_state, float* scaler_state,
                                 float growth_factor, float backoff_factor, int growth_interval, mednet_stream stream) {
  MEDNET_REQUIRE(p && g && m && v && opt_state, MEDNET_E_SHAPE, "adamw_step: null pointer");
  MEDNET_REQUIRE(count > 0, MEDNET_E_SHAPE, "adamw_step: count is 0");
  MEDNET_REQUIRE(lr >= 0.f && weight_decay >= 0.f, MEDNET_E_SHAPE, "adamw_step: negative lr %g or weight_decay %g", (double)lr,
                 (double)weight_decay);
  MEDNET_REQUIRE(!scaler_state || growth_interval >= 1, MEDNET_E_SHAPE, "adamw_step: growth_interval %d", growth_interval);
  hipStream_t s = (hipStream_t)stream;
  const bool vec = aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v);
  const dim3 grid(strided_grid(count, UPDATE_PER_BLOCK, OPT_MAX_ROWS)), block(256);
  const float* ost = opt_state;
  const float* sc = scaler_state;
#define MEDNET_ADAM_LAUNCH(V, D) \
  hipLaunchKernelGGL((adam_guarded_kernel<V, D>), grid, block, 0, s, p, g, m, v, count, lr, beta1, beta2, eps, weight_decay, inv_world, ost, sc)
  if (vec) {
    if (decoupled) MEDNET_ADAM_LAUNCH(4, true);
    else MEDNET_ADAM_LAUNCH(4, false);
  } else {
    if (decoupled) MEDNET_ADAM_LAUNCH(1, true);
    else MEDNET_ADAM_LAUNCH(1, false);
  }
#undef MEDNET_ADAM_LAUNCH
  hipLaunchKernelGGL(optim_state_update_kernel, dim3(1), dim3(64), 0, s, opt_state, scaler_state, growth_factor, backoff_factor,
                     (float)growth_interval);
  return check_launch("adamw_step");
}

extern "C" int mednet_adam_step_scaled(float* p, const float* g, float* m, float* v, size_t count, float lr, float beta1,
                                       float beta2, float eps, float weight_decay, float inv_world, float* scaler_state,
                                       float growth_factor, float backoff_factor, int growth_interval, mednet_stream stream) {
  MEDNET_REQUIRE(scaler_state != nullptr && growth_interval >= 1, MEDNET_E_SHAPE, "adam_step_scaled: scaler state required");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(strided_grid(count, UPDATE_PER_BLOCK, ADAM_MAX_ROWS)), block(256);
  hipLaunchKernelGGL(grad_check_kernel, grid, block, 0, s, g, count, scaler_state);
  hipLaunchKernelGGL(adam_scaled_kernel, grid, block, 0, s, p, g, m, v, count, lr, beta1, beta2, eps, weight_decay, inv_world,
                     (const float*)scaler_state);
  hipLaunchKernelGGL(scaler_update_kernel, dim3(1), dim3(64), 0, s, scaler_state, growth_factor, backoff_factor,
                     (float)growth_interval);
  return check_launch("adam_step_scaled");
}

extern "C" int mednet_adam_step(float* p, const float* g, float* m, float* v, size_t count, float lr, float beta1,
                                float beta2, float eps, float weight_decay, int step, float grad_scale,
                                mednet_stream stream) {
  MEDNET_REQUIRE(step >= 1, MEDNET_E_SHAPE, "adam_step: step must be >= 1");
  const float bc1 = 1.f - powf(beta1, (float)step);
  const float bc2s = sqrtf(1.f - powf(beta2, (float)step));
  hipLaunchKernelGGL(adam_kernel, dim3(strided_grid(count, UPDATE_PER_BLOCK, ADAM_MAX_ROWS)), dim3(256), 0, (hipStream_t)stream, p, g, m,
                     v, count, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale);
  return check_launch("adam_step");
}
