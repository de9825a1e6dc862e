// lpips_kernels.hip -- the HBM-bound passes around the VGG16 convolutions of the LPIPS perceptual loss (cvvae_amd/lpips.py):
// ScalingLayer + NCHW -> NHWC, ReLU, 2x2 max pooling, the fused ReLU / pooling backward, and the five "lin" heads
// (channel-normalise, squared difference, 1x1 lin, spatial mean) forward and backward.  gfx950 only.
// Every pass reads each tensor once and writes each tensor once, with 16-byte accesses along C; arithmetic is fp32 with one
// rounding to the storage dtype; no atomics (the head's partial sums are merged in index order).
#include "pass_common.h"

namespace cvvae {

// ---------------------------------------------------------------------------------------------------------
// ScalingLayer (lpips.py:67-78) fused with the layout change: [N,3,H,W] -> [N,H,W,Cpad], (x - shift[c]) / scale[c], pad channels 0.
// One thread per (pixel, 8-channel vector): the stores of a wave are one contiguous run.
// ---------------------------------------------------------------------------------------------------------
template <typename TS, typename TD>
__global__ __launch_bounds__(256) void lpips_scale_in_kernel(const TS* __restrict__ in, long long HW, int cv, long long nvec,
                                                             const float* __restrict__ shift, const float* __restrict__ scale,
                                                             TD* __restrict__ out) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= nvec) return;
  const long long pix = v / cv;
  const int vc = (int)(v - pix * cv);
  float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (vc == 0) {
    const long long n = pix / HW, s = pix - n * HW;
#pragma unroll
    for (int c = 0; c < 3; ++c) f[c] = ((float)in[(n * 3 + c) * HW + s] - shift[c]) / scale[c];
  }
  st8<TD>(out + v * 8, f);
}

// the adjoint: NHWC gradient (pixel stride ps) -> [N,3,H,W], g[c] / scale[c]
template <typename TG, typename TD>
__global__ __launch_bounds__(256) void lpips_scale_in_bwd_kernel(const TG* __restrict__ g, long long HW, long long ps, long long npix,
                                                                 const float* __restrict__ scale, TD* __restrict__ out) {
  const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= npix) return;
  const long long n = pix / HW, s = pix - n * HW;
  float f[8];
  ld8<TG>(g + pix * ps, f);
#pragma unroll
  for (int c = 0; c < 3; ++c) out[(n * 3 + c) * HW + s] = (TD)(f[c] / scale[c]);
}

// ---------------------------------------------------------------------------------------------------------
// ReLU (in place allowed) and MaxPool2d(2, 2) on NHWC
// ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void relu_kernel(const T* x, long long nvec, T* out) {
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (long long)gridDim.x * 256) {
    float f[8];
    ld8<T>(x + v * 8, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = f[j] <= 0.f ? 0.f : f[j];  // (NaN stays NaN, as torch.relu's)
    st8<T>(out + v * 8, f);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void maxpool2x2_kernel(const T* __restrict__ x, long long N, int H, int W, int C, T* __restrict__ out) {
  const int cv = C >> 3, Ho = H >> 1, Wo = W >> 1;
  const long long nvec = N * Ho * Wo * cv;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (long long)gridDim.x * 256) {
    const int c0 = (int)(v % cv) * 8;
    long long pix = v / cv;
    const int xo = (int)(pix % Wo);
    pix /= Wo;
    const int yo = (int)(pix % Ho);
    const long long n = pix / Ho;
    float m[8];
    ld8<T>(x + ((n * H + 2 * yo) * W + 2 * xo) * C + c0, m);
#pragma unroll
    for (int d = 1; d < 4; ++d) {
      float f[8];
      ld8<T>(x + ((n * H + 2 * yo + (d >> 1)) * W + 2 * xo + (d & 1)) * C + c0, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) m[j] = (f[j] > m[j] || f[j] != f[j]) ? f[j] : m[j];  // (a NaN anywhere in the window wins, as ATen's)
    }
    st8<T>(out + v * 8, m);
  }
}

// ---------------------------------------------------------------------------------------------------------
// Backward of "ReLU output y, tapped, then pooled":  gx = (g_tap + unpool(g_pool)) * (y > 0).  One thread per 2x2 cell (odd
// extents: the last row / column of cells is partial and receives no pooled gradient) and 8 channels, so y is read once and the
// window's argmax is recomputed instead of stored: the FIRST maximum in row-major scan order (strict >), ATen's tie rule.
// ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void relu_pool_bwd_kernel(const T* __restrict__ y, const T* __restrict__ g_tap,
                                                            const T* __restrict__ g_pool, long long N, int H, int W, int C,
                                                            T* __restrict__ gx) {
  const int cv = C >> 3, Ho = H >> 1, Wo = W >> 1, Hc = (H + 1) >> 1, Wc = (W + 1) >> 1;
  const long long nvec = N * Hc * Wc * cv;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (long long)gridDim.x * 256) {
    const int c0 = (int)(v % cv) * 8;
    long long cell = v / cv;
    const int cx = (int)(cell % Wc);
    cell /= Wc;
    const int cy = (int)(cell % Hc);
    const long long n = cell / Hc;
    float yv[4][8], gv[4][8];
    bool ok[4];
    long long off[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int yy = 2 * cy + (d >> 1), xx = 2 * cx + (d & 1);
      ok[d] = yy < H && xx < W;
      off[d] = ((n * H + yy) * W + xx) * C + c0;
#pragma unroll
      for (int j = 0; j < 8; ++j) yv[d][j] = gv[d][j] = 0.f;
      if (ok[d]) {
        ld8<T>(y + off[d], yv[d]);
        if (g_tap) ld8<T>(g_tap + off[d], gv[d]);
      }
    }
    if (g_pool && cy < Ho && cx < Wo) {  // a whole window: all four positions exist
      float gp[8];
      ld8<T>(g_pool + ((n * Ho + cy) * Wo + cx) * C + c0, gp);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int best = 0;
        float m = yv[0][j];
#pragma unroll
        for (int d = 1; d < 4; ++d)
          if (yv[d][j] > m) { m = yv[d][j]; best = d; }
#pragma unroll
        for (int d = 0; d < 4; ++d) gv[d][j] += (best == d) ? gp[j] : 0.f;
      }
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      if (!ok[d]) continue;
#pragma unroll
      for (int j = 0; j < 8; ++j) gv[d][j] = yv[d][j] > 0.f ? gv[d][j] : 0.f;
      st8<T>(gx + off[d], gv[d]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// LPIPS head of one level (lpips.py:46-64, 141-147).  A pixel's C channels sit in LP = C / 8 lanes of one wave (8 channels = one
// 16-byte load per lane), so both channel reductions (the norms, then the weighted squared difference) are butterflies inside the
// wave: DPP within a 16-lane row, a lane shuffle across rows -- the features are read once and never staged in LDS.
// ---------------------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// sum over aligned groups of LP lanes (LP = 8, 16, 32, 64), delivered in EVERY lane of the group, in a fixed order
template <int LP>
__device__ __forceinline__ float group_sum(float x) {
  x += dpp_f<0xB1>(x);                     // quad_perm [1,0,3,2]: lane ^ 1
  x += dpp_f<0x4E>(x);                     // quad_perm [2,3,0,1]: lane ^ 2
  x += dpp_f<0x141>(x);                    // row_half_mirror: the other quad of each 8 lanes (quads are uniform by now)
  if constexpr (LP >= 16) x += dpp_f<0x140>(x);   // row_mirror: the other half of the 16-lane row
  if constexpr (LP >= 32) x += __shfl_xor(x, 16, 64);
  if constexpr (LP >= 64) x += __shfl_xor(x, 32, 64);
  return x;
}

constexpr float LPIPS_EPS = 1e-10f;

// a x - b y to one rounding of the difference, and EXACTLY 0 for equal operands: p = round(b y) and its exact error ep = b y - p (one
// fma), then (a x - p) - ep.  A plain `a * x - b * y` is contracted into one fma, which keeps the rounding error of the other product:
// identical features then had a non-zero difference, hence a non-zero level value and gradients where the reference computes exact
// zeros.  With equal operands fma(a, x, -p) is that same error ep (it is representable), and the difference is 0.
__device__ __forceinline__ float diff_of_products(float a, float x, float b, float y) {
  const float p = b * y;
  const float ep = __builtin_fmaf(b, y, -p);
  return __builtin_fmaf(a, x, -p) - ep;
}

template <typename T, int LP>
__global__ __launch_bounds__(256) void lpips_head_kernel(const T* __restrict__ f0, const T* __restrict__ f1,
                                                         const float* __restrict__ w, long long HW, float* __restrict__ ws) {
  constexpr int PB = 256 / LP;  // pixels per pass of the workgroup
  constexpr int C = LP * 8;
  const long long n = blockIdx.y;
  const int sub = threadIdx.x / LP, c0 = (threadIdx.x % LP) * 8;
  const float4 w0 = *reinterpret_cast<const float4*>(w + c0), w1 = *reinterpret_cast<const float4*>(w + c0 + 4);
  const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
  float acc = 0.f;
  for (long long p0 = (long long)blockIdx.x * PB; p0 < HW; p0 += (long long)gridDim.x * PB) {  // (workgroup-uniform bounds)
    const long long p = p0 + sub;
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, b[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (p < HW) {
      ld8<T>(f0 + (n * HW + p) * C + c0, a);
      ld8<T>(f1 + (n * HW + p) * C + c0, b);
    }
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s0 = __builtin_fmaf(a[j], a[j], s0);
      s1 = __builtin_fmaf(b[j], b[j], s1);
    }
    s0 = group_sum<LP>(s0);
    s1 = group_sum<LP>(s1);
    const float i0 = 1.0f / (sqrtf(s0 + LPIPS_EPS) + LPIPS_EPS), i1 = 1.0f / (sqrtf(s1 + LPIPS_EPS) + LPIPS_EPS);
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float e = diff_of_products(a[j], i0, b[j], i1);
      d = __builtin_fmaf(wv[j] * e, e, d);
    }
    acc += d;  // (a pixel beyond HW contributes exactly 0)
  }
  // workgroup sum in a fixed order: the wave's 64 lanes, then the four waves
  acc = group_sum<64>(acc);
  __shared__ float sh[4];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) ws[n * gridDim.x + blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// out[n] += (sum of the nblk partials of sample n, in index order) / HW
__global__ __launch_bounds__(64) void lpips_head_final_kernel(const float* __restrict__ ws, int nblk, long long N, float inv_hw,
                                                              float* __restrict__ out) {
  const long long n = (long long)blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
  for (int i = 0; i < nblk; ++i) s += ws[n * nblk + i];
  out[n] += s * inv_hw;
}

// Backward of the head: with u = f / m, m = sqrt(sum f^2 + eps) + eps, e = u0 - u1 and d = sum_c w_c e_c^2,
//   dd/df0_k =  2 w_k e_k / m0 - 2 (sum_c w_c e_c f0_c) f0_k / (m0^2 sqrt(sum f0^2 + eps))     (and the mirrored form for f1)
// times gout[n] / HW.  m, e and the dots are recomputed from the features: one read of f0 / f1, one write per requested side.
template <typename T, int LP>
__global__ __launch_bounds__(256) void lpips_head_bwd_kernel(const T* __restrict__ f0, const T* __restrict__ f1,
                                                             const float* __restrict__ w, const float* __restrict__ gout,
                                                             long long HW, float inv_hw, T* __restrict__ g0, T* __restrict__ g1) {
  constexpr int PB = 256 / LP;
  constexpr int C = LP * 8;
  const long long n = blockIdx.y;
  const int sub = threadIdx.x / LP, c0 = (threadIdx.x % LP) * 8;
  const float4 w0 = *reinterpret_cast<const float4*>(w + c0), w1 = *reinterpret_cast<const float4*>(w + c0 + 4);
  const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
  const float k = 2.0f * gout[n] * inv_hw;
  for (long long p0 = (long long)blockIdx.x * PB; p0 < HW; p0 += (long long)gridDim.x * PB) {
    const long long p = p0 + sub;
    const bool ok = p < HW;
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, b[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const long long off = (n * HW + p) * C + c0;
    if (ok) {
      ld8<T>(f0 + off, a);
      ld8<T>(f1 + off, b);
    }
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s0 = __builtin_fmaf(a[j], a[j], s0);
      s1 = __builtin_fmaf(b[j], b[j], s1);
    }
    s0 = group_sum<LP>(s0);
    s1 = group_sum<LP>(s1);
    const float r0 = sqrtf(s0 + LPIPS_EPS), r1 = sqrtf(s1 + LPIPS_EPS);
    const float i0 = 1.0f / (r0 + LPIPS_EPS), i1 = 1.0f / (r1 + LPIPS_EPS);
    float we[8], d0 = 0.f, d1 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      we[j] = wv[j] * diff_of_products(a[j], i0, b[j], i1);
      d0 = __builtin_fmaf(we[j], a[j], d0);
      d1 = __builtin_fmaf(we[j], b[j], d1);
    }
    d0 = group_sum<LP>(d0);
    d1 = group_sum<LP>(d1);
    if (!ok) continue;
    if (g0) {
      const float q = d0 * i0 * i0 / r0;
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = k * (we[j] * i0 - q * a[j]);
      st8<T>(g0 + off, o);
    }
    if (g1) {
      const float q = d1 * i1 * i1 / r1;
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = k * (q * b[j] - we[j] * i1);
      st8<T>(g1 + off, o);
    }
  }
}

static inline int head_lp(int C) { return (C == 64 || C == 128 || C == 256 || C == 512) ? C / 8 : 0; }
static inline int head_blocks(long long HW, int C, int cap) {
  const long long groups = (HW + 256 / (C / 8) - 1) / (256 / (C / 8));
  return (int)(groups < cap ? groups : cap);
}
constexpr int HEAD_FWD_BLOCKS = 256, HEAD_BWD_BLOCKS = 2048;

}  // namespace cvvae

using namespace cvvae;

static inline unsigned grid_for(long long nvec) {
  long long blocks = (nvec + 255) / 256;
  if (blocks > 256LL * 64) blocks = 256LL * 64;
  return (unsigned)blocks;
}

extern "C" {

int cvvae_lpips_scale_in(int32_t src_dtype, int32_t dst_dtype, const void* in, int64_t N, int32_t H, int32_t W, const float* shift,
                         const float* scale, int32_t Cpad, void* out, void* stream) {
  if (!in || !out || !shift || !scale || N <= 0 || H <= 0 || W <= 0 || Cpad < 8 || Cpad % 8) return CVVAE_EINVAL;
  const long long HW = (long long)H * W, nvec = HW * N * (Cpad / 8);
  if ((nvec + 255) / 256 >= (1LL << 31)) return CVVAE_EUNSUPPORTED;
  const dim3 grid((unsigned)((nvec + 255) / 256));
  hipStream_t s = (hipStream_t)stream;
  bool ok = false;
  by_dtype(dst_dtype, [&](auto td) {
    ok = by_dtype(src_dtype, [&](auto ts) {
      using TS = typename decltype(ts)::type;
      using TD = typename decltype(td)::type;
      hipLaunchKernelGGL((lpips_scale_in_kernel<TS, TD>), grid, dim3(256), 0, s, (const TS*)in, HW, Cpad / 8, nvec, shift, scale, (TD*)out);
    });
  });
  if (!ok) return CVVAE_EINVAL;
  return launch_status();
}

int cvvae_lpips_scale_in_bwd(int32_t g_dtype, int32_t dst_dtype, const void* g, int64_t N, int32_t H, int32_t W, int64_t pix_stride,
                             const float* scale, void* out, void* stream) {
  if (!g || !out || !scale || N <= 0 || H <= 0 || W <= 0 || pix_stride < 8 || pix_stride % 8) return CVVAE_EINVAL;
  const long long HW = (long long)H * W, npix = HW * N;
  if ((npix + 255) / 256 >= (1LL << 31)) return CVVAE_EUNSUPPORTED;
  const dim3 grid((unsigned)((npix + 255) / 256));
  hipStream_t s = (hipStream_t)stream;
  bool ok = false;
  by_dtype(dst_dtype, [&](auto td) {
    ok = by_dtype(g_dtype, [&](auto ts) {
      using TS = typename decltype(ts)::type;
      using TD = typename decltype(td)::type;
      hipLaunchKernelGGL((lpips_scale_in_bwd_kernel<TS, TD>), grid, dim3(256), 0, s, (const TS*)g, HW, (long long)pix_stride, npix, scale,
                         (TD*)out);
    });
  });
  if (!ok) return CVVAE_EINVAL;
  return launch_status();
}

int cvvae_relu(int32_t dtype, const void* x, int64_t n, void* out, void* stream) {
  if (!x || !out || n <= 0 || n % 8) return CVVAE_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long long nvec = n / 8;
  const bool ok = by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(relu_kernel<T>, dim3(grid_for(nvec)), dim3(256), 0, s, (const T*)x, nvec, (T*)out);
  });
  if (!ok) return CVVAE_EINVAL;
  return launch_status();
}

int cvvae_maxpool2x2(int32_t dtype, const void* x, int64_t N, int32_t H, int32_t W, int32_t C, void* out, void* stream) {
  if (!x || !out || N <= 0 || H < 2 || W < 2 || C <= 0 || C % 8) return CVVAE_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long long nvec = (long long)N * (H / 2) * (W / 2) * (C / 8);
  const bool ok = by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(maxpool2x2_kernel<T>, dim3(grid_for(nvec)), dim3(256), 0, s, (const T*)x, (long long)N, H, W, C, (T*)out);
  });
  if (!ok) return CVVAE_EINVAL;
  return launch_status();
}

int cvvae_relu_pool_bwd(int32_t dtype, const void* y, const void* g_tap, const void* g_pool, int64_t N, int32_t H, int32_t W,
                        int32_t C, void* gx, void* stream) {
  if (!y || !gx || (!g_tap && !g_pool) || N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8) return CVVAE_EINVAL;
  if (g_pool && (H < 2 || W < 2)) return CVVAE_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long long nvec = (long long)N * ((H + 1) / 2) * ((W + 1) / 2) * (C / 8);
  const bool ok = by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(relu_pool_bwd_kernel<T>, dim3(grid_for(nvec)), dim3(256), 0, s, (const T*)y, (const T*)g_tap, (const T*)g_pool,
                       (long long)N, H, W, C, (T*)gx);
  });
  if (!ok) return CVVAE_EINVAL;
  return launch_status();
}

size_t cvvae_lpips_head_workspace_bytes(int64_t N, int64_t HW, int32_t C) {
  if (N <= 0 || HW <= 0 || !head_lp(C)) return 0;
  return (size_t)N * head_blocks(HW, C, HEAD_FWD_BLOCKS) * sizeof(float);
}

int cvvae_lpips_head(int32_t dtype, const void* f0, const void* f1, const float* w, int64_t N, int64_t HW, int32_t C, float* out,
                     void* workspace, void* stream) {
  if (!f0 || !f1 || !w || !out || !workspace || N <= 0 || HW <= 0 || C <= 0 || C % 8) return CVVAE_EINVAL;
  const int lp = head_lp(C);
  if (!lp || N > 65535) return CVVAE_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int nblk = head_blocks(HW, C, HEAD_FWD_BLOCKS);
  const dim3 grid((unsigned)nblk, (unsigned)N);
#define CALL_LP(T, LP) \
  hipLaunchKernelGGL((lpips_head_kernel<T, LP>), grid, dim3(256), 0, s, (const T*)f0, (const T*)f1, w, (long long)HW, (float*)workspace)
  const bool ok = by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (lp == 8) CALL_LP(T, 8); else if (lp == 16) CALL_LP(T, 16); else if (lp == 32) CALL_LP(T, 32); else CALL_LP(T, 64);
  });
#undef CALL_LP
  if (!ok) return CVVAE_EINVAL;
  hipLaunchKernelGGL(lpips_head_final_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, s, (const float*)workspace, nblk,
                     (long long)N, 1.0f / (float)HW, out);
  return launch_status();
}

int cvvae_lpips_head_bwd(int32_t dtype, const void* f0, const void* f1, const float* w, const float* gout, int64_t N, int64_t HW,
                         int32_t C, void* g_f0, void* g_f1, void* stream) {
  if (!f0 || !f1 || !w || !gout || (!g_f0 && !g_f1) || N <= 0 || HW <= 0 || C <= 0 || C % 8) return CVVAE_EINVAL;
  const int lp = head_lp(C);
  if (!lp || N > 65535) return CVVAE_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)head_blocks(HW, C, HEAD_BWD_BLOCKS), (unsigned)N);
#define CALL_LP(T, LP) \
  hipLaunchKernelGGL((lpips_head_bwd_kernel<T, LP>), grid, dim3(256), 0, s, (const T*)f0, (const T*)f1, w, gout, (long long)HW, \
                     1.0f / (float)HW, (T*)g_f0, (T*)g_f1)
  const bool ok = by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (lp == 8) CALL_LP(T, 8); else if (lp == 16) CALL_LP(T, 16); else if (lp == 32) CALL_LP(T, 32); else CALL_LP(T, 64);
  });
#undef CALL_LP
  if (!ok) return CVVAE_EINVAL;
  return launch_status();
}

}  // extern "C"
