// pass_common.h -- what the element-wise and reduction passes share: 8-element vector access, the 256-thread workgroup sum, the
// softmax passes' row reduction, the GroupNorm record and its merge, the SiLU derivative, and the host side's dtype dispatch.
// gfx950 only.  One definition of each: misc_kernels.hip and disc_kernels.hip must agree on WStat / chan_merge (cvvae_gn_finalize
// merges the records both write), the forward passes of misc_kernels.hip and their adjoints in bwd_kernels.hip on ld8 / st8 and
// the SiLU derivative, and a fix to a store's rounding or a merge's NaN handling belongs in one place.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cvvae.h"

namespace cvvae {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <typename T>
struct Vec8;
template <>
struct Vec8<__bf16> {
  using type = bf16x8;
};
template <>
struct Vec8<_Float16> {
  using type = f16x8;
};

template <typename T>
__device__ __forceinline__ void unpack8(const uint4& u, float (&f)[8]) {
  typename Vec8<T>::type x = __builtin_bit_cast(typename Vec8<T>::type, u);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = (float)x[j];
}
// 8 values rounded once (nearest even) to T
template <typename T>
__device__ __forceinline__ uint4 pack8(const float (&f)[8]) {
  typename Vec8<T>::type x;
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = (T)f[j];
  return __builtin_bit_cast(uint4, x);
}

// 8 consecutive elements <-> fp32 registers, for the 16-bit storage types (one 16-byte access) and for float (two)
template <typename T>
struct Raw8 {
  uint4 a;
};
template <>
struct Raw8<float> {
  uint4 a, b;
};
template <typename T>
__device__ __forceinline__ Raw8<T> ldraw8(const T* p) {
  Raw8<T> r;
  r.a = *reinterpret_cast<const uint4*>(p);
  return r;
}
template <>
__device__ __forceinline__ Raw8<float> ldraw8<float>(const float* p) {
  Raw8<float> r;
  r.a = reinterpret_cast<const uint4*>(p)[0];
  r.b = reinterpret_cast<const uint4*>(p)[1];
  return r;
}
template <typename T>
__device__ __forceinline__ void unraw8(const Raw8<T>& r, float (&f)[8]) {
  unpack8<T>(r.a, f);
}
template <>
__device__ __forceinline__ void unraw8<float>(const Raw8<float>& r, float (&f)[8]) {
  f[0] = __uint_as_float(r.a.x); f[1] = __uint_as_float(r.a.y); f[2] = __uint_as_float(r.a.z); f[3] = __uint_as_float(r.a.w);
  f[4] = __uint_as_float(r.b.x); f[5] = __uint_as_float(r.b.y); f[6] = __uint_as_float(r.b.z); f[7] = __uint_as_float(r.b.w);
}
template <typename T>
__device__ __forceinline__ void ld8(const T* p, float (&f)[8]) {
  unraw8<T>(ldraw8<T>(p), f);
}
template <typename T>
__device__ __forceinline__ void st8(T* p, const float (&f)[8]) {
  *reinterpret_cast<uint4*>(p) = pack8<T>(f);
}
template <>
__device__ __forceinline__ void st8<float>(float* p, const float (&f)[8]) {
  reinterpret_cast<float4*>(p)[0] = make_float4(f[0], f[1], f[2], f[3]);
  reinterpret_cast<float4*>(p)[1] = make_float4(f[4], f[5], f[6], f[7]);
}

template <typename T>
__device__ __forceinline__ bool aligned16(const T* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the partial forms: the first n (<= 8) elements at p.  ld8 / st8 when the group is whole and p is 16-byte aligned, element by
// element otherwise; elements at index >= n read as zero and are not written
template <typename T>
__device__ __forceinline__ void ld8_n(const T* p, int n, float (&f)[8]) {
  if (n == 8 && aligned16(p)) {
    ld8<T>(p, f);
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = (k < n) ? (float)p[k] : 0.f;
  }
}
template <typename T>
__device__ __forceinline__ void st8_n(T* p, const float (&f)[8], int n) {
  if (n == 8 && aligned16(p)) {
    st8<T>(p, f);
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < n) p[k] = (T)f[k];
  }
}

// sum over a workgroup of 256 threads in a fixed order (a butterfly over the 64 lanes of each wave, then the four waves through
// LDS in wave order), valid in thread 0.  No trailing barrier: a caller that sums again in the same kernel puts one behind it.
__device__ __forceinline__ float block_sum(float x) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) x += __shfl_xor(x, m, 64);
  __shared__ float sh[4];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// sum or maximum over a workgroup of whole waves, valid in every thread, through the caller's sh[waves]: the row reduction of the
// softmax passes (misc_kernels.hip forward, bwd_kernels.hip backward)
__device__ __forceinline__ float block_reduce(float v, bool is_max, float* sh) {
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const float o = __shfl_xor(v, off);
    v = is_max ? fmaxf(v, o) : v + o;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh[0];
  for (int i = 1; i < (int)(blockDim.x >> 6); ++i) r = is_max ? fmaxf(r, sh[i]) : r + sh[i];
  return r;
}

// one GroupNorm record (count, mean, sum of squared deviations) and Chan's merge of two of them
struct WStat {
  float n, mean, m2;
};
__device__ __forceinline__ void chan_merge(WStat& a, const WStat& b) {
  if (b.n == 0.f) return;
  const float n = a.n + b.n;
  const float d = b.mean - a.mean;
  const float f = b.n / n;
  a.mean += d * f;
  a.m2 += b.m2 + d * d * a.n * f;
  a.n = n;
}

// d silu(a) / d a
__device__ __forceinline__ float silu_grad_f(float a) {
  const float sg = __builtin_amdgcn_rcpf(1.0f + __expf(-a));
  return sg * (1.0f + a * (1.0f - sg));
}

// ---- host side ----
static inline bool known_dtype(int32_t d) { return d == CVVAE_F16 || d == CVVAE_BF16 || d == CVVAE_F32; }
static inline int launch_status() { return (int)hipGetLastError(); }

// by_dtype(dtype, [&](auto tag) { using T = typename decltype(tag)::type; ... }) runs the body for the element type of a dtype
// code and returns false, having run nothing, for any other code; by_dtype16 knows the two 16-bit types only.  A pair of dtypes
// is two nested calls.
template <typename T>
struct TypeTag {
  using type = T;
};
template <typename F>
static inline bool by_dtype16(int32_t dtype, F&& f) {
  if (dtype == CVVAE_BF16) f(TypeTag<__bf16>{});
  else if (dtype == CVVAE_F16) f(TypeTag<_Float16>{});
  else return false;
  return true;
}
template <typename F>
static inline bool by_dtype(int32_t dtype, F&& f) {
  if (dtype != CVVAE_F32) return by_dtype16(dtype, f);
  f(TypeTag<float>{});
  return true;
}

}  // namespace cvvae
