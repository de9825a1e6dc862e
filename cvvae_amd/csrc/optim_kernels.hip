// optim_kernels.hip -- the parameter update of a training iteration (cvvae_amd/optim.py, lvdm/modules/ema.py) as multi-tensor passes
// over a LIST of fp32 tensors: the L2 norm of all gradients with the clip coefficient, g <- coef g, AdamW with the coefficient applied
// in flight, the EMA of the weights, and the pack pass of the data-parallel gradient exchange (cvvae_amd/ddp.py: g / world size into
// the slots of one flat bucket).  16-bit networks train on fp32 master weights through adamw_master_kernel: 16-bit g and p, fp32
// master / m / v, the 16-bit parameter rewritten from the new master in the same pass; sumsq_kernel reads fp32 or 16-bit gradients, so
// one norm covers a mixed list (cvvae_mt_sumsq per dtype into one workspace, then cvvae_mt_norm_finish).  gfx950 only.  All of them
// are HBM-bound: plain C++.
//
// Geometry.  The list is cut into chunks of at most CHUNK elements that never straddle two tensors (cvvae_mt_chunk: tensor index,
// first element, length); the tensors' base pointers and per-tensor scalars sit in a second table (cvvae_mt_tensor).  One workgroup
// of 256 threads takes a chunk, workgroup w walking chunks w, w + grid, ...  Inside a chunk group j = elements [8j, 8j + 8) belongs to
// thread j % 256; a group moves as two 16-byte vectors per operand when it is whole and that operand's address is 16-byte aligned,
// element by element otherwise (the tail of a chunk; a tensor that starts 4 bytes into its buffer).  A group of eight 16-bit values is
// one 16-byte vector under the same rule, decided per operand (a view that starts 2 bytes into its buffer goes element by element).
//
// Order of summation (cvvae_mt_grad_norm).  A thread adds the squares of a group in index order, then its groups in index order;
// the 64 lanes of a wave are merged by a butterfly, the four waves through LDS in wave order: ONE partial per chunk.  Stage 2 (one
// workgroup) merges the partials, thread t taking t, t + 256, ... serially, then the same workgroup sum.  Nothing is atomic and the
// grid does not enter: the norm is a function of the values and the list order alone, bit-identical from run to run.
// Longest chain of additions: 8 (CHUNK / 2048 = 4 groups: 7 + 1 each, 32) + 6 + 3 in a chunk, ceil(n_chunks / 256) + 6 + 3 in stage 2.
#include "pass_common.h"

namespace cvvae {
namespace optim {

constexpr int WG = 256;              // threads per workgroup
constexpr int VEC = 8;               // elements per group
constexpr int TILE = WG * VEC;       // elements per workgroup pass: the loss kernels' tile
constexpr int CHUNK = CVVAE_MT_CHUNK;
constexpr int MAX_BLOCKS = 2048;     // grid cap (8 workgroups per CU), as loss_kernels.hip
static_assert(CHUNK % TILE == 0, "a chunk is a whole number of tiles");

// T: the gradients' storage type; the squares and every sum are fp32, so a 16-bit list gives the bits of its fp32 copy
template <typename T>
__global__ __launch_bounds__(WG) void sumsq_kernel(const cvvae_mt_chunk* __restrict__ chunks, const cvvae_mt_tensor* __restrict__ tensors,
                                                   long long n_chunks, float* __restrict__ ws) {
  for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const cvvae_mt_chunk ch = chunks[c];
    const T* g = (const T*)tensors[ch.tensor].g + ch.start;
    float acc = 0.f;
    for (int i = threadIdx.x * VEC; i < ch.n; i += TILE) {
      const int n = (ch.n - i) < VEC ? (ch.n - i) : VEC;
      float f[VEC];
      ld8_n(g + i, n, f);
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < VEC; ++k) s += f[k] * f[k];
      acc += s;
    }
    acc = block_sum(acc);
    __syncthreads();  // frees block_sum's LDS slots for the next chunk
    if (threadIdx.x == 0) ws[c] = acc;
  }
}

// out2[0] = sqrt(sum of the partials), out2[1] = min(1, max_norm / (norm + 1e-6)) with clamp's treatment of NaN: the comparison
// is written out because fminf would drop it
__global__ __launch_bounds__(WG) void norm_final_kernel(const float* __restrict__ ws, long long n_chunks, float max_norm,
                                                        float* __restrict__ out2) {
  float acc = 0.f;
  for (long long i = threadIdx.x; i < n_chunks; i += WG) acc += ws[i];
  acc = block_sum(acc);
  __syncthreads();  // as in sumsq_kernel; a single sum does not need it, it only keeps this kernel's code what it has been
  if (threadIdx.x == 0) {
    const float norm = sqrtf(acc);
    const float c = max_norm / (norm + 1e-6f);
    out2[0] = norm;
    out2[1] = c > 1.f ? 1.f : c;
  }
}

__global__ __launch_bounds__(WG) void scale_kernel(const cvvae_mt_chunk* __restrict__ chunks, const cvvae_mt_tensor* __restrict__ tensors,
                                                   long long n_chunks, const float* __restrict__ coef_dev) {
  const float coef = coef_dev[0];
  for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const cvvae_mt_chunk ch = chunks[c];
    float* g = (float*)tensors[ch.tensor].g + ch.start;
    for (int i = threadIdx.x * VEC; i < ch.n; i += TILE) {
      const int n = (ch.n - i) < VEC ? (ch.n - i) : VEC;
      float f[VEC];
      ld8_n(g + i, n, f);
#pragma unroll
      for (int k = 0; k < VEC; ++k) f[k] = coef * f[k];
      st8_n(g + i, f, n);
    }
  }
}

struct AdamW {
  float beta1, one_minus_beta1, beta2, one_minus_beta2, eps, decay;  // decay = 1 - lr weight_decay
};

__global__ __launch_bounds__(WG) void adamw_kernel(const cvvae_mt_chunk* __restrict__ chunks, const cvvae_mt_tensor* __restrict__ tensors,
                                                   long long n_chunks, AdamW h, const float* __restrict__ coef_dev) {
  const float coef = coef_dev ? coef_dev[0] : 1.f;
  for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const cvvae_mt_chunk ch = chunks[c];
    const cvvae_mt_tensor t = tensors[ch.tensor];
    const float* g = (const float*)t.g + ch.start;
    float* p = (float*)t.p + ch.start;
    float* m = (float*)t.m + ch.start;
    float* v = (float*)t.v + ch.start;
    for (int i = threadIdx.x * VEC; i < ch.n; i += TILE) {
      const int n = (ch.n - i) < VEC ? (ch.n - i) : VEC;
      float fg[VEC], fp[VEC], fm[VEC], fv[VEC];
      ld8_n(g + i, n, fg);
      ld8_n(p + i, n, fp);
      ld8_n(m + i, n, fm);
      ld8_n(v + i, n, fv);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const float G = coef_dev ? coef * fg[k] : fg[k];
        fm[k] = __builtin_fmaf(h.beta1, fm[k], h.one_minus_beta1 * G);
        fv[k] = __builtin_fmaf(h.beta2, fv[k], h.one_minus_beta2 * (G * G));
        const float denom = sqrtf(fv[k]) / t.bias2_sqrt + h.eps;
        fp[k] = fp[k] * h.decay - t.step_size * (fm[k] / denom);
      }
      st8_n(p + i, fp, n);
      st8_n(m + i, fm, n);
      st8_n(v + i, fv, n);
    }
  }
}

// adamw_kernel for a 16-bit parameter: g and p are T, the fp32 master (the `shadow` field) stands in the place of p, and p is
// rewritten as the new master rounded to nearest even.  The element update is adamw_kernel's, expression for expression, so that
// both contract to the same FMAs: master, m and v come out with the bits of adamw_kernel on fp32 copies (tests/test_gpu_master_optim.py)
template <typename T>
__global__ __launch_bounds__(WG) void adamw_master_kernel(const cvvae_mt_chunk* __restrict__ chunks,
                                                          const cvvae_mt_tensor* __restrict__ tensors, long long n_chunks, AdamW h,
                                                          const float* __restrict__ coef_dev) {
  const float coef = coef_dev ? coef_dev[0] : 1.f;
  for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const cvvae_mt_chunk ch = chunks[c];
    const cvvae_mt_tensor t = tensors[ch.tensor];
    const T* g = (const T*)t.g + ch.start;
    T* p = (T*)t.p + ch.start;
    float* w = (float*)t.shadow + ch.start;
    float* m = (float*)t.m + ch.start;
    float* v = (float*)t.v + ch.start;
    for (int i = threadIdx.x * VEC; i < ch.n; i += TILE) {
      const int n = (ch.n - i) < VEC ? (ch.n - i) : VEC;
      float fg[VEC], fp[VEC], fm[VEC], fv[VEC];
      ld8_n(g + i, n, fg);
      ld8_n(w + i, n, fp);
      ld8_n(m + i, n, fm);
      ld8_n(v + i, n, fv);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const float G = coef_dev ? coef * fg[k] : fg[k];
        fm[k] = __builtin_fmaf(h.beta1, fm[k], h.one_minus_beta1 * G);
        fv[k] = __builtin_fmaf(h.beta2, fv[k], h.one_minus_beta2 * (G * G));
        const float denom = sqrtf(fv[k]) / t.bias2_sqrt + h.eps;
        fp[k] = fp[k] * h.decay - t.step_size * (fm[k] / denom);
      }
      st8_n(w + i, fp, n);
      st8_n(m + i, fm, n);
      st8_n(v + i, fv, n);
      st8_n(p + i, fp, n);
    }
  }
}

__global__ __launch_bounds__(WG) void ema_kernel(const cvvae_mt_chunk* __restrict__ chunks, const cvvae_mt_tensor* __restrict__ tensors,
                                                 long long n_chunks, float one_minus_decay) {
  for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const cvvae_mt_chunk ch = chunks[c];
    const cvvae_mt_tensor t = tensors[ch.tensor];
    const float* p = (const float*)t.p + ch.start;
    float* s = (float*)t.shadow + ch.start;
    for (int i = threadIdx.x * VEC; i < ch.n; i += TILE) {
      const int n = (ch.n - i) < VEC ? (ch.n - i) : VEC;
      float fp[VEC], fs[VEC];
      ld8_n(p + i, n, fp);
      ld8_n(s + i, n, fs);
#pragma unroll
      for (int k = 0; k < VEC; ++k) fs[k] = fs[k] - one_minus_decay * (fs[k] - fp[k]);
      st8_n(s + i, fs, n);
    }
  }
}

// shadow <- g / divisor (zeros for a tensor without a gradient: g NULL).  `/` is the correctly rounded fp32 division (hipcc's default;
// the Makefile sets no fast-math flag), as in adamw_kernel.  g and shadow carry no __restrict__: they may be one address.
__global__ __launch_bounds__(WG) void pack_kernel(const cvvae_mt_chunk* __restrict__ chunks, const cvvae_mt_tensor* __restrict__ tensors,
                                                  long long n_chunks, float divisor) {
  for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const cvvae_mt_chunk ch = chunks[c];
    const cvvae_mt_tensor t = tensors[ch.tensor];
    const float* g = t.g ? (const float*)t.g + ch.start : nullptr;
    float* d = (float*)t.shadow + ch.start;
    for (int i = threadIdx.x * VEC; i < ch.n; i += TILE) {
      const int n = (ch.n - i) < VEC ? (ch.n - i) : VEC;
      float f[VEC];
      if (g) {
        ld8_n(g + i, n, f);
#pragma unroll
        for (int k = 0; k < VEC; ++k) f[k] = f[k] / divisor;
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) f[k] = 0.f;
      }
      st8_n(d + i, f, n);
    }
  }
}

static inline int blocks_for(long long n_chunks) { return (int)(n_chunks < MAX_BLOCKS ? n_chunks : MAX_BLOCKS); }

// CVVAE_OK when the launch has something to do, 1 when the list is empty (nothing to launch), else the error
static inline int check_tables(bool dtype_ok, const void* chunks, const void* tensors, int64_t n_chunks) {
  if (n_chunks < 0 || n_chunks > CVVAE_MT_MAX_CHUNKS) return CVVAE_EINVAL;
  if (!dtype_ok) return CVVAE_EUNSUPPORTED;
  if (n_chunks == 0) return 1;
  if (!chunks || !tensors) return CVVAE_EINVAL;
  return CVVAE_OK;
}
// the fp32-only entry points
static inline int check_list(int32_t dtype, const void* chunks, const void* tensors, int64_t n_chunks) {
  return check_tables(dtype == CVVAE_F32, chunks, tensors, n_chunks);
}
static inline bool valid_adamw(double lr, double beta1, double beta2, double eps, double weight_decay) {
  return lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && weight_decay >= 0.0;
}

}  // namespace optim
}  // namespace cvvae

using namespace cvvae;
using namespace cvvae::optim;

extern "C" {

size_t cvvae_mt_workspace_bytes(int64_t n_chunks) {
  if (n_chunks < 0 || n_chunks > CVVAE_MT_MAX_CHUNKS) return 0;
  return (size_t)(n_chunks > 4 ? n_chunks : 4) * sizeof(float);
}

int cvvae_mt_grad_norm(int32_t dtype, const cvvae_mt_chunk* chunks, const cvvae_mt_tensor* tensors, int64_t n_chunks, float max_norm,
                       void* workspace, float* out2, void* stream) {
  if (!workspace || !out2) return CVVAE_EINVAL;
  const int rc = check_list(dtype, chunks, tensors, n_chunks);
  if (rc < 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (rc == 0)
    hipLaunchKernelGGL(sumsq_kernel<float>, dim3(blocks_for(n_chunks)), dim3(WG), 0, s, chunks, tensors, (long long)n_chunks,
                       (float*)workspace);
  hipLaunchKernelGGL(norm_final_kernel, dim3(1), dim3(WG), 0, s, (const float*)workspace, (long long)n_chunks, max_norm, out2);
  return launch_status();
}

int cvvae_mt_scale(int32_t dtype, const cvvae_mt_chunk* chunks, const cvvae_mt_tensor* tensors, int64_t n_chunks, const float* coef_dev,
                   void* stream) {
  if (!coef_dev) return CVVAE_EINVAL;
  const int rc = check_list(dtype, chunks, tensors, n_chunks);
  if (rc != 0) return rc < 0 ? rc : CVVAE_OK;
  hipLaunchKernelGGL(scale_kernel, dim3(blocks_for(n_chunks)), dim3(WG), 0, (hipStream_t)stream, chunks, tensors, (long long)n_chunks,
                     coef_dev);
  return launch_status();
}

int cvvae_mt_adamw(int32_t dtype, const cvvae_mt_chunk* chunks, const cvvae_mt_tensor* tensors, int64_t n_chunks, double lr, double beta1,
                   double beta2, double eps, double weight_decay, const float* coef_dev, void* stream) {
  if (!valid_adamw(lr, beta1, beta2, eps, weight_decay)) return CVVAE_EINVAL;
  const int rc = check_list(dtype, chunks, tensors, n_chunks);
  if (rc != 0) return rc < 0 ? rc : CVVAE_OK;
  const AdamW h{(float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)(1.0 - lr * weight_decay)};
  hipLaunchKernelGGL(adamw_kernel, dim3(blocks_for(n_chunks)), dim3(WG), 0, (hipStream_t)stream, chunks, tensors, (long long)n_chunks, h,
                     coef_dev);
  return launch_status();
}

int cvvae_mt_adamw_master(int32_t dtype, const cvvae_mt_chunk* chunks, const cvvae_mt_tensor* tensors, int64_t n_chunks, double lr,
                          double beta1, double beta2, double eps, double weight_decay, const float* coef_dev, void* stream) {
  if (!valid_adamw(lr, beta1, beta2, eps, weight_decay)) return CVVAE_EINVAL;
  const int rc = check_tables(dtype == CVVAE_BF16 || dtype == CVVAE_F16, chunks, tensors, n_chunks);
  if (rc != 0) return rc < 0 ? rc : CVVAE_OK;
  const AdamW h{(float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)(1.0 - lr * weight_decay)};
  by_dtype16(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(adamw_master_kernel<T>, dim3(blocks_for(n_chunks)), dim3(WG), 0, (hipStream_t)stream, chunks, tensors,
                       (long long)n_chunks, h, coef_dev);
  });
  return launch_status();
}

int cvvae_mt_sumsq(int32_t dtype, const cvvae_mt_chunk* chunks, const cvvae_mt_tensor* tensors, int64_t n_chunks, float* partials,
                   void* stream) {
  if (!partials) return CVVAE_EINVAL;
  const int rc = check_tables(known_dtype(dtype), chunks, tensors, n_chunks);
  if (rc != 0) return rc < 0 ? rc : CVVAE_OK;
  by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(sumsq_kernel<T>, dim3(blocks_for(n_chunks)), dim3(WG), 0, (hipStream_t)stream, chunks, tensors,
                       (long long)n_chunks, partials);
  });
  return launch_status();
}

int cvvae_mt_norm_finish(const float* partials, int64_t n_partials, float max_norm, float* out2, void* stream) {
  if (!partials || !out2 || n_partials < 0 || n_partials > CVVAE_MT_MAX_CHUNKS) return CVVAE_EINVAL;
  hipLaunchKernelGGL(norm_final_kernel, dim3(1), dim3(WG), 0, (hipStream_t)stream, partials, (long long)n_partials, max_norm, out2);
  return launch_status();
}

int cvvae_mt_ema(int32_t dtype, const cvvae_mt_chunk* chunks, const cvvae_mt_tensor* tensors, int64_t n_chunks, float one_minus_decay,
                 void* stream) {
  const int rc = check_list(dtype, chunks, tensors, n_chunks);
  if (rc != 0) return rc < 0 ? rc : CVVAE_OK;
  hipLaunchKernelGGL(ema_kernel, dim3(blocks_for(n_chunks)), dim3(WG), 0, (hipStream_t)stream, chunks, tensors, (long long)n_chunks,
                     one_minus_decay);
  return launch_status();
}

int cvvae_mt_pack(int32_t dtype, const cvvae_mt_chunk* chunks, const cvvae_mt_tensor* tensors, int64_t n_chunks, float divisor,
                  void* stream) {
  if (!(divisor > 0.f) || !(divisor <= 3.402823466e38f)) return CVVAE_EINVAL;
  const int rc = check_list(dtype, chunks, tensors, n_chunks);
  if (rc != 0) return rc < 0 ? rc : CVVAE_OK;
  hipLaunchKernelGGL(pack_kernel, dim3(blocks_for(n_chunks)), dim3(WG), 0, (hipStream_t)stream, chunks, tensors, (long long)n_chunks,
                     divisor);
  return launch_status();
}

}  // extern "C"
