// Optimizer step of the hot path in three launches: global gradient norm + clip coefficient (Models/SDNetTrainer.py:366,
// torch.nn.utils.clip_grad_norm_) and the Adamax update (:367, torch.optim.Adamax) over ALL trainable tensors at once.
// torch's own path is ~20 multi-tensor launches and three passes over the gradients (norm, scale, update); here the clip
// coefficient stays on the device and is applied inside the update, and embedding rows that the trainer re-pins after every
// step (rows >= tune_partial, :369-373) are left out of the update (their gradients still count in the norm, as in the
// reference).  Tensors are addressed through device tables of pointers; work is cut into chunks of 8192 elements
// (tensor index, start, count), one workgroup per chunk.  All sums run in a fixed order: deterministic.
// A trained encoder may step as a group of its own (opt['bert_optimizer']): one more launch, ruart_adam_step, over its chunks, under the
// same device-resident clip coefficient (the norm runs once over the gradients of both groups).
// The reference's other optimizer confs step the same way: 'ADAM' (Adamax with coupled L2 decay) on ruart_adamax_l2_step, 'SGD' on
// ruart_sgd_step, 'ADAM2' (torch.optim.Adam) on ruart_adam_step with dec = 1.
#include "common.h"
#include "ruart_hip.h"

#define OPT_CHUNK 8192

__global__ __launch_bounds__(256) void gradnorm_partial_kernel(const float* const* __restrict__ grads, const int* __restrict__ c_tensor,
                                                               const int* __restrict__ c_start, const int* __restrict__ c_count,
                                                               float* __restrict__ partial) {
  __shared__ float red[4];
  const int c = blockIdx.x;
  const float* g = grads[c_tensor[c]] + c_start[c];
  const int n = c_count[c];
  float s = 0.f;
  for (int i = threadIdx.x * 4; i < n; i += 1024) {
    if (i + 3 < n) {
      const f32x4_t v = *reinterpret_cast<const f32x4_t*>(g + i);
      s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    } else {
      for (int j = i; j < n; ++j) s += g[j] * g[j];
    }
  }
  s = block_sum<4>(s, red);
  if (threadIdx.x == 0) partial[c] = s;
}

// out[0] = total norm, out[1] = clip coefficient min(1, max_norm / (norm + 1e-6))
__global__ __launch_bounds__(256) void gradnorm_final_kernel(const float* __restrict__ partial, int n, float max_norm,
                                                             const float* __restrict__ extra_sq, float* __restrict__ out) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
  s = block_sum<4>(s, red);
  if (threadIdx.x == 0) {
    if (extra_sq) s += extra_sq[0];           // squared norm of gradients that are not in the chunk list (dp.GradSync.pinned_sq)
    const float norm = sqrtf(s);
    out[0] = norm;
    out[1] = fminf(1.0f, max_norm / (norm + 1e-6f));
  }
}

// torch.optim.Adamax (single-tensor form):  m += (1 - b1) (g - m);  u = max(b2 u, |g| + eps);  p -= clr m / u
__global__ __launch_bounds__(256) void adamax_update_kernel(float* const* __restrict__ params, const float* const* __restrict__ grads,
                                                            float* const* __restrict__ exp_avg, float* const* __restrict__ exp_inf,
                                                            const int* __restrict__ c_tensor, const int* __restrict__ c_start,
                                                            const int* __restrict__ c_count, const float* __restrict__ coef_ptr,
                                                            const float* __restrict__ clr_t, float one_minus_b1, float b2, float eps) {
  const int c = blockIdx.x, t = c_tensor[c], s0 = c_start[c], n = c_count[c];
  const float coef = coef_ptr ? coef_ptr[1] : 1.0f;
  const float clr = clr_t[t];                   // lr / (1 - beta1^step) with the tensor's OWN step count, as torch keeps it
  float* p = params[t] + s0;
  const float* g = grads[t] + s0;
  float* m = exp_avg[t] + s0;
  float* u = exp_inf[t] + s0;
  for (int i = threadIdx.x * 4; i < n; i += 1024) {
    if (i + 3 < n) {
      f32x4_t pv = *reinterpret_cast<f32x4_t*>(p + i), mv = *reinterpret_cast<f32x4_t*>(m + i), uv = *reinterpret_cast<f32x4_t*>(u + i);
      const f32x4_t gv = *reinterpret_cast<const f32x4_t*>(g + i);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float gr = gv[r] * coef;
        mv[r] = mv[r] + one_minus_b1 * (gr - mv[r]);
        uv[r] = fmaxf(uv[r] * b2, fabsf(gr) + eps);
        pv[r] = pv[r] - clr * (mv[r] / uv[r]);
      }
      *reinterpret_cast<f32x4_t*>(p + i) = pv;
      *reinterpret_cast<f32x4_t*>(m + i) = mv;
      *reinterpret_cast<f32x4_t*>(u + i) = uv;
    } else {
      for (int j = i; j < n; ++j) {
        const float gr = g[j] * coef;
        const float mj = m[j] + one_minus_b1 * (gr - m[j]);
        const float uj = fmaxf(u[j] * b2, fabsf(gr) + eps);
        m[j] = mj;
        u[j] = uj;
        p[j] = p[j] - clr * (mj / uj);
      }
    }
  }
}

// torch.optim.Adamax(weight_decay=wd) behind clip_grad_norm_ (the reference's 'ADAM' conf): the decay is coupled, taken from the
// parameter AFTER the clip,  g' = g coef + wd p;  then the rule above on g'.
__global__ __launch_bounds__(256) void adamax_l2_update_kernel(float* const* __restrict__ params, const float* const* __restrict__ grads,
                                                               float* const* __restrict__ exp_avg, float* const* __restrict__ exp_inf,
                                                               const int* __restrict__ c_tensor, const int* __restrict__ c_start,
                                                               const int* __restrict__ c_count, const float* __restrict__ coef_ptr,
                                                               const float* __restrict__ clr_t, float one_minus_b1, float b2, float eps,
                                                               float wd) {
  const int c = blockIdx.x, t = c_tensor[c], s0 = c_start[c], n = c_count[c];
  const float coef = coef_ptr ? coef_ptr[1] : 1.0f;
  const float clr = clr_t[t];
  float* p = params[t] + s0;
  const float* g = grads[t] + s0;
  float* m = exp_avg[t] + s0;
  float* u = exp_inf[t] + s0;
  for (int i = threadIdx.x * 4; i < n; i += 1024) {
    if (i + 3 < n) {
      f32x4_t pv = *reinterpret_cast<f32x4_t*>(p + i), mv = *reinterpret_cast<f32x4_t*>(m + i), uv = *reinterpret_cast<f32x4_t*>(u + i);
      const f32x4_t gv = *reinterpret_cast<const f32x4_t*>(g + i);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float gr = gv[r] * coef + wd * pv[r];
        mv[r] = mv[r] + one_minus_b1 * (gr - mv[r]);
        uv[r] = fmaxf(uv[r] * b2, fabsf(gr) + eps);
        pv[r] = pv[r] - clr * (mv[r] / uv[r]);
      }
      *reinterpret_cast<f32x4_t*>(p + i) = pv;
      *reinterpret_cast<f32x4_t*>(m + i) = mv;
      *reinterpret_cast<f32x4_t*>(u + i) = uv;
    } else {
      for (int j = i; j < n; ++j) {
        const float gr = g[j] * coef + wd * p[j];
        const float mj = m[j] + one_minus_b1 * (gr - m[j]);
        const float uj = fmaxf(u[j] * b2, fabsf(gr) + eps);
        m[j] = mj;
        u[j] = uj;
        p[j] = p[j] - clr * (mj / uj);
      }
    }
  }
}

// torch.optim.SGD (no momentum, no decay) behind clip_grad_norm_:  p -= lr (g coef).  No state tensors.
__global__ __launch_bounds__(256) void sgd_update_kernel(float* const* __restrict__ params, const float* const* __restrict__ grads,
                                                         const int* __restrict__ c_tensor, const int* __restrict__ c_start,
                                                         const int* __restrict__ c_count, const float* __restrict__ coef_ptr, float lr) {
  const int c = blockIdx.x, t = c_tensor[c], s0 = c_start[c], n = c_count[c];
  const float coef = coef_ptr ? coef_ptr[1] : 1.0f;
  float* p = params[t] + s0;
  const float* g = grads[t] + s0;
  for (int i = threadIdx.x * 4; i < n; i += 1024) {
    if (i + 3 < n) {
      f32x4_t pv = *reinterpret_cast<f32x4_t*>(p + i);
      const f32x4_t gv = *reinterpret_cast<const f32x4_t*>(g + i);
#pragma unroll
      for (int r = 0; r < 4; ++r) pv[r] = pv[r] - lr * (gv[r] * coef);
      *reinterpret_cast<f32x4_t*>(p + i) = pv;
    } else {
      for (int j = i; j < n; ++j) p[j] = p[j] - lr * (g[j] * coef);
    }
  }
}

// Adam family of the trained encoder's group (torch.optim.AdamW, and the reference's BertAdam, Models/Bert/optimization.py:129-152), one
// form for both:  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;  p = p dec - a m / (sqrt(v) c + eps).  What differs between the rules,
// the tensors (decay or none, own step count) and the steps (schedule) is the host's: tab[3 t] = {a, dec, c}.
__global__ __launch_bounds__(256) void adam_update_kernel(float* const* __restrict__ params, const float* const* __restrict__ grads,
                                                          float* const* __restrict__ exp_avg, float* const* __restrict__ exp_avg_sq,
                                                          const int* __restrict__ c_tensor, const int* __restrict__ c_start,
                                                          const int* __restrict__ c_count, const float* __restrict__ coef_ptr,
                                                          const float* __restrict__ tab, float b1, float b2, float eps) {
  const int c = blockIdx.x, t = c_tensor[c], s0 = c_start[c], n = c_count[c];
  const float coef = coef_ptr ? coef_ptr[1] : 1.0f;
  const float a = tab[3 * t], dec = tab[3 * t + 1], cs = tab[3 * t + 2];
  const float one_minus_b1 = 1.0f - b1, one_minus_b2 = 1.0f - b2;
  float* p = params[t] + s0;
  const float* g = grads[t] + s0;
  float* m = exp_avg[t] + s0;
  float* v = exp_avg_sq[t] + s0;
  for (int i = threadIdx.x * 4; i < n; i += 1024) {
    if (i + 3 < n) {
      f32x4_t pv = *reinterpret_cast<f32x4_t*>(p + i), mv = *reinterpret_cast<f32x4_t*>(m + i), vv = *reinterpret_cast<f32x4_t*>(v + i);
      const f32x4_t gv = *reinterpret_cast<const f32x4_t*>(g + i);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float gr = gv[r] * coef;
        mv[r] = b1 * mv[r] + one_minus_b1 * gr;
        vv[r] = b2 * vv[r] + one_minus_b2 * gr * gr;
        pv[r] = pv[r] * dec - a * (mv[r] / (sqrtf(vv[r]) * cs + eps));
      }
      *reinterpret_cast<f32x4_t*>(p + i) = pv;
      *reinterpret_cast<f32x4_t*>(m + i) = mv;
      *reinterpret_cast<f32x4_t*>(v + i) = vv;
    } else {
      for (int j = i; j < n; ++j) {
        const float gr = g[j] * coef;
        const float mj = b1 * m[j] + one_minus_b1 * gr;
        const float vj = b2 * v[j] + one_minus_b2 * gr * gr;
        m[j] = mj;
        v[j] = vj;
        p[j] = p[j] * dec - a * (mj / (sqrtf(vj) * cs + eps));
      }
    }
  }
}

extern "C" int ruart_grad_norm_clip(const float* const* grads, const int* c_tensor, const int* c_start, const int* c_count, int n_chunks,
                                    float max_norm, float* partial, float* norm_coef, const float* extra_sq, void* stream) {
  RUART_ENTRY();
  if (n_chunks <= 0 || !grads || !partial || !norm_coef) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(gradnorm_partial_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, grads, c_tensor, c_start, c_count,
                     partial);
  hipLaunchKernelGGL(gradnorm_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, n_chunks, max_norm, extra_sq, norm_coef);
  RUART_CHECK_LAUNCH();
  return 0;
}

extern "C" int ruart_adamax_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_inf,
                                 const int* c_tensor, const int* c_start, const int* c_count, int n_chunks, const float* norm_coef,
                                 const float* clr, float beta1, float beta2, float eps, void* stream) {
  RUART_ENTRY();
  if (n_chunks <= 0 || !clr || !params || !grads || !exp_avg || !exp_inf) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(adamax_update_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg, exp_inf, c_tensor,
                     c_start, c_count, norm_coef, clr, 1.0f - beta1, beta2, eps);
  RUART_CHECK_LAUNCH();
  return 0;
}

extern "C" int ruart_adamax_l2_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_inf,
                                    const int* c_tensor, const int* c_start, const int* c_count, int n_chunks, const float* norm_coef,
                                    const float* clr, float beta1, float beta2, float eps, float weight_decay, void* stream) {
  RUART_ENTRY();
  if (n_chunks <= 0 || !clr || !params || !grads || !exp_avg || !exp_inf || !c_tensor || !c_start || !c_count) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(adamax_l2_update_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg, exp_inf, c_tensor,
                     c_start, c_count, norm_coef, clr, 1.0f - beta1, beta2, eps, weight_decay);
  RUART_CHECK_LAUNCH();
  return 0;
}

extern "C" int ruart_sgd_step(float* const* params, const float* const* grads, const int* c_tensor, const int* c_start, const int* c_count,
                              int n_chunks, const float* norm_coef, float lr, void* stream) {
  RUART_ENTRY();
  if (n_chunks <= 0 || !params || !grads || !c_tensor || !c_start || !c_count) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(sgd_update_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, params, grads, c_tensor, c_start, c_count,
                     norm_coef, lr);
  RUART_CHECK_LAUNCH();
  return 0;
}

extern "C" int ruart_adam_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                               const int* c_tensor, const int* c_start, const int* c_count, int n_chunks, const float* norm_coef,
                               const float* tab, float beta1, float beta2, float eps, void* stream) {
  RUART_ENTRY();
  if (n_chunks <= 0 || !tab || !params || !grads || !exp_avg || !exp_avg_sq || !c_tensor || !c_start || !c_count) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(adam_update_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg, exp_avg_sq, c_tensor,
                     c_start, c_count, norm_coef, tab, beta1, beta2, eps);
  RUART_CHECK_LAUNCH();
  return 0;
}
