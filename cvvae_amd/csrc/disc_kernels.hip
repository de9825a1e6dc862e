// disc_kernels.hip -- the non-convolution passes of the 3-D PatchGAN discriminator (cvvae_amd/disc_ops.py) and their adjoints:
// ResnetBlockDown3D's downsample (first frame duplicated when T is odd, then avg_pool3d(2, 2)) and GroupNorm-apply + LeakyReLU
// (or the bare LeakyReLU).  gfx950 only.  All four are HBM- or latency-bound element-wise passes over NDHWC tensors: plain C++,
// fp32 arithmetic, one rounding to the storage dtype, no LDS, no atomics.
//
// Work split.  A lane owns one group of 8 consecutive channels (one 16-byte access for 16-bit types, two for fp32; C % 8 == 0 and
// 16-byte aligned tensors make every group aligned), consecutive lanes take consecutive groups, so a wavefront covers whole lines
// along C, then W.  The grid is capped and strides over the groups; group indices are 64-bit.  Every output element has exactly
// one writer (the adjoint of the pool is a gather), so the results do not depend on the grid: the same inputs give the same bits.
// In-place calls (y == x, gv == gy) are safe because a lane reads its own 8 elements before it writes them and nobody else's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cvvae.h"

namespace cvvae {
namespace disc {

constexpr int WG = 256;            // threads per workgroup
constexpr int VEC = 8;             // elements per lane and trip
constexpr int MAX_BLOCKS = 2048;   // 8 workgroups per CU; the rest of the tensor is reached by the grid stride

template <typename T>
__device__ __forceinline__ void load8(const T* p, float (&f)[VEC]) {
  if constexpr (sizeof(T) == 4) {
    const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
  } else {
    union { uint4 u; T h[VEC]; } v;
    v.u = *reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int j = 0; j < VEC; ++j) f[j] = (float)v.h[j];
  }
}

// 8 values rounded once (nearest even) to T
template <typename T>
__device__ __forceinline__ void store8(T* p, const float (&f)[VEC]) {
  if constexpr (sizeof(T) == 4) {
    reinterpret_cast<float4*>(p)[0] = make_float4(f[0], f[1], f[2], f[3]);
    reinterpret_cast<float4*>(p)[1] = make_float4(f[4], f[5], f[6], f[7]);
  } else {
    union { uint4 u; T h[VEC]; } v;
#pragma unroll
    for (int j = 0; j < VEC; ++j) v.h[j] = (T)f[j];
    *reinterpret_cast<uint4*>(p) = v.u;
  }
}

// group index -> (frame, y, x, channel group) of a [frames][Hd][Wd][cv] tensor.  Only the two outer splits are 64-bit divisions:
// a frame's pixel count and the frame count fit 32 bits (checked on the host).
struct Pos {
  long long frame;
  int y, x, c0;
};
__device__ __forceinline__ Pos decode(long long g, int cv, int Hd, int Wd) {
  const long long pix = g / cv;
  Pos p;
  p.c0 = (int)(g - pix * cv) * VEC;
  p.frame = pix / ((long long)Hd * Wd);
  const unsigned r = (unsigned)(pix - p.frame * ((long long)Hd * Wd));
  p.y = (int)(r / (unsigned)Wd);
  p.x = (int)(r - (unsigned)p.y * (unsigned)Wd);
  return p;
}

// ---------------------------------------------------------------------------------------------------------
// models/discriminator.py:240-243, 250-253:  if T is odd, h = cat([h[:, :, :1], h], 2);  h = avg_pool3d(h, 2, 2).
// Padded frame p is stored frame p (T even) or max(p - 1, 0) (T odd): the duplicate is an index rule, never a tensor.
// ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(WG) void avgpool3d_down_kernel(const T* __restrict__ x, T* __restrict__ y, int Tn, int H, int W, int C,
                                                            int To, int Ho, int Wo, long long ngroups) {
  const int cv = C / VEC, odd = Tn & 1;
  for (long long g = (long long)blockIdx.x * WG + threadIdx.x; g < ngroups; g += (long long)gridDim.x * WG) {
    const Pos o = decode(g, cv, Ho, Wo);
    const long long b = o.frame / To;
    const int to = (int)(o.frame - b * To);
    float s[2][VEC];  // one partial sum per padded frame: ((x00 + x01) + (x10 + x11))
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const int p = 2 * to + dt;
      const int t = odd ? (p > 0 ? p - 1 : 0) : p;
      const T* row0 = x + ((((b * Tn + t) * H + 2 * o.y) * W + 2 * o.x) * (long long)C + o.c0);
      float a[VEC], c[VEC], d[VEC], e[VEC];
      load8<T>(row0, a);
      load8<T>(row0 + C, c);
      load8<T>(row0 + (long long)W * C, d);
      load8<T>(row0 + (long long)W * C + C, e);
#pragma unroll
      for (int j = 0; j < VEC; ++j) s[dt][j] = (a[j] + c[j]) + (d[j] + e[j]);
    }
    float r[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) r[j] = (s[0][j] + s[1][j]) * 0.125f;
    store8<T>(y + g * VEC, r);
  }
}

// the adjoint as a gather: input element (t, y, x) reads the one output element it went into.  0.125 gy; 0.25 gy for frame 0 of an
// odd T (it is both padded frames of output frame 0); 0 for the row / column an odd H / W drops.
template <typename T>
__global__ __launch_bounds__(WG) void avgpool3d_down_bwd_kernel(const T* __restrict__ gy, T* __restrict__ gx, int Tn, int H, int W,
                                                                int C, int To, int Ho, int Wo, long long ngroups) {
  const int cv = C / VEC, odd = Tn & 1;
  for (long long g = (long long)blockIdx.x * WG + threadIdx.x; g < ngroups; g += (long long)gridDim.x * WG) {
    const Pos i = decode(g, cv, H, W);
    const long long b = i.frame / Tn;
    const int t = (int)(i.frame - b * Tn);
    float r[VEC];
    if (i.y < 2 * Ho && i.x < 2 * Wo) {
      const int to = (t + odd) >> 1;
      const float k = (odd && t == 0) ? 0.25f : 0.125f;
      load8<T>(gy + ((((b * To + to) * Ho + (i.y >> 1)) * Wo + (i.x >> 1)) * (long long)C + i.c0), r);
#pragma unroll
      for (int j = 0; j < VEC; ++j) r[j] *= k;
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) r[j] = 0.f;
    }
    store8<T>(gx + g * VEC, r);
  }
}

// ---------------------------------------------------------------------------------------------------------
// Normalize(c) + nn.LeakyReLU(0.2, True) (models/discriminator.py:316-317, 330-331) as one pass over the activation, on the
// (scale, shift) tables of cvvae_gn_stats / cvvae_gn_finalize;  AFFINE = false: the bare LeakyReLU behind the first conv (:302).
// x and y may alias.
// ---------------------------------------------------------------------------------------------------------
template <typename T, bool AFFINE>
__global__ __launch_bounds__(WG) void gn_leaky_apply_kernel(const T* x, const float* __restrict__ scale, const float* __restrict__ shift,
                                                            T* y, long long per_row, int C, float slope, long long ngroups) {
  const int cv = C / VEC;
  for (long long g = (long long)blockIdx.x * WG + threadIdx.x; g < ngroups; g += (long long)gridDim.x * WG) {
    float f[VEC];
    load8<T>(x + g * VEC, f);
    if constexpr (AFFINE) {
      const long long pix = g / cv;
      const long long tab = (pix / per_row) * C + (g - pix * cv) * VEC;
      float sc[VEC], sh[VEC];
      load8<float>(scale + tab, sc);
      load8<float>(shift + tab, sh);
#pragma unroll
      for (int j = 0; j < VEC; ++j) f[j] = __builtin_fmaf(f[j], sc[j], sh[j]);
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) f[j] = f[j] > 0.f ? f[j] : slope * f[j];
    store8<T>(y + g * VEC, f);
  }
}

// gv = y > 0 ? gy : slope gy, the mask taken from the OUTPUT of the activation (slope > 0: y and the pre-activation have the same
// sign, and an in-place LeakyReLU has kept nothing else).  gy and gv may alias.  The last group of a tensor whose length is not a
// multiple of 8 goes element by element.
template <typename T>
__global__ __launch_bounds__(WG) void leaky_bwd_kernel(const T* y, const T* gy, T* gv, long long n, float slope) {
  const long long ngroups = (n + VEC - 1) / VEC;
  for (long long g = (long long)blockIdx.x * WG + threadIdx.x; g < ngroups; g += (long long)gridDim.x * WG) {
    const long long i = g * VEC;
    if (i + VEC <= n) {
      float a[VEC], d[VEC];
      load8<T>(y + i, a);
      load8<T>(gy + i, d);
#pragma unroll
      for (int j = 0; j < VEC; ++j) d[j] = a[j] > 0.f ? d[j] : slope * d[j];
      store8<T>(gv + i, d);
    } else {
      for (long long k = i; k < n; ++k) {
        const float d = (float)gy[k];
        gv[k] = (T)((float)y[k] > 0.f ? d : slope * d);
      }
    }
  }
}

static inline int blocks_for(long long ngroups) {
  const long long b = (ngroups + WG - 1) / WG;
  return (int)(b < MAX_BLOCKS ? b : MAX_BLOCKS);
}

static inline bool known_dtype(int32_t d) { return d == CVVAE_F16 || d == CVVAE_BF16 || d == CVVAE_F32; }

constexpr long long MAX_ELEMS = 1LL << 40;  // what the index arithmetic above holds with room to spare

// element count of the pool's INPUT [B][T][H][W][C], or -1 when a frame's pixels, the frame count or the total leave their range
static inline long long pool_elems(int64_t B, int32_t T, int32_t H, int32_t W, int32_t C) {
  if ((long long)H * W >= (1LL << 31) || B > ((1LL << 31) - 1) / T) return -1;
  const long long pix = (long long)B * T * ((long long)H * W);
  if (pix > MAX_ELEMS / C) return -1;
  return pix * C;
}

}  // namespace disc
}  // namespace cvvae

using namespace cvvae::disc;

#define DISC_BY_DTYPE(CALL) \
  do { \
    if (dtype == CVVAE_F32) { CALL(float); } else if (dtype == CVVAE_F16) { CALL(_Float16); } else { CALL(__bf16); } \
  } while (0)

extern "C" {

int cvvae_avgpool3d_down(int32_t dtype, const void* x, void* y, int64_t B, int32_t T, int32_t H, int32_t W, int32_t C, void* stream) {
  if (!x || !y || B <= 0 || T <= 0 || H < 2 || W < 2 || C <= 0) return CVVAE_EINVAL;
  if (!known_dtype(dtype) || C % VEC) return CVVAE_EUNSUPPORTED;
  if (pool_elems(B, T, H, W, C) < 0) return CVVAE_EUNSUPPORTED;
  const int To = (T + (T & 1)) / 2, Ho = H / 2, Wo = W / 2;
  const long long ngroups = (long long)B * To * Ho * Wo * (C / VEC);
#define CALL(TT) \
  hipLaunchKernelGGL(avgpool3d_down_kernel<TT>, dim3(blocks_for(ngroups)), dim3(WG), 0, (hipStream_t)stream, (const TT*)x, (TT*)y, T, H, \
                     W, C, To, Ho, Wo, ngroups)
  DISC_BY_DTYPE(CALL);
#undef CALL
  return (int)hipGetLastError();
}

int cvvae_avgpool3d_down_bwd(int32_t dtype, const void* gy, void* gx, int64_t B, int32_t T, int32_t H, int32_t W, int32_t C,
                             void* stream) {
  if (!gy || !gx || B <= 0 || T <= 0 || H < 2 || W < 2 || C <= 0) return CVVAE_EINVAL;
  if (!known_dtype(dtype) || C % VEC) return CVVAE_EUNSUPPORTED;
  const long long total = pool_elems(B, T, H, W, C);
  if (total < 0) return CVVAE_EUNSUPPORTED;
  const int To = (T + (T & 1)) / 2, Ho = H / 2, Wo = W / 2;
  const long long ngroups = total / VEC;
#define CALL(TT) \
  hipLaunchKernelGGL(avgpool3d_down_bwd_kernel<TT>, dim3(blocks_for(ngroups)), dim3(WG), 0, (hipStream_t)stream, (const TT*)gy, (TT*)gx, \
                     T, H, W, C, To, Ho, Wo, ngroups)
  DISC_BY_DTYPE(CALL);
#undef CALL
  return (int)hipGetLastError();
}

int cvvae_gn_leaky_apply(int32_t dtype, const void* x, const float* scale, const float* shift, void* y, int64_t rows, int64_t per_row,
                         int32_t C, float slope, void* stream) {
  if (!x || !y || rows <= 0 || per_row <= 0 || C <= 0 || (scale == nullptr) != (shift == nullptr)) return CVVAE_EINVAL;
  if (!known_dtype(dtype) || C % VEC) return CVVAE_EUNSUPPORTED;
  if (rows > MAX_ELEMS / per_row || rows * per_row > MAX_ELEMS / C) return CVVAE_EUNSUPPORTED;
  const long long ngroups = (long long)rows * per_row * (C / VEC);
#define CALL(TT) \
  do { \
    if (scale) \
      hipLaunchKernelGGL((gn_leaky_apply_kernel<TT, true>), dim3(blocks_for(ngroups)), dim3(WG), 0, (hipStream_t)stream, (const TT*)x, \
                         scale, shift, (TT*)y, (long long)per_row, C, slope, ngroups); \
    else \
      hipLaunchKernelGGL((gn_leaky_apply_kernel<TT, false>), dim3(blocks_for(ngroups)), dim3(WG), 0, (hipStream_t)stream, (const TT*)x, \
                         scale, shift, (TT*)y, (long long)per_row, C, slope, ngroups); \
  } while (0)
  DISC_BY_DTYPE(CALL);
#undef CALL
  return (int)hipGetLastError();
}

int cvvae_leaky_bwd(int32_t dtype, const void* y, const void* gy, void* gv, int64_t n_elems, float slope, void* stream) {
  if (!y || !gy || !gv || n_elems <= 0 || !(slope > 0.f)) return CVVAE_EINVAL;
  if (!known_dtype(dtype) || n_elems > MAX_ELEMS) return CVVAE_EUNSUPPORTED;
  const long long ngroups = ((long long)n_elems + VEC - 1) / VEC;
#define CALL(TT) \
  hipLaunchKernelGGL(leaky_bwd_kernel<TT>, dim3(blocks_for(ngroups)), dim3(WG), 0, (hipStream_t)stream, (const TT*)y, (const TT*)gy, \
                     (TT*)gv, (long long)n_elems, slope)
  DISC_BY_DTYPE(CALL);
#undef CALL
  return (int)hipGetLastError();
}

}  // extern "C"
