// metrics_kernels.hip -- per-frame SSE / PSNR / Gaussian-window SSIM of two clips on the 8-bit scale, one pass over both operands
// (include/cvvae.h cvvae_frame_metrics).  gfx950, wave64, no atomics: the same values give the same bits on every run.
//
// A workgroup of 256 threads owns one MT_H x MT_W tile of SSIM map positions of one frame, all three colour channels:
//   1. stage the tile plus the 10-sample halo of both operands into LDS as fp32 ON THE 8-BIT SCALE (a u8 row is 3W interleaved
//      bytes, read as aligned dwords inside the row and byte by byte at its two ends; a float clip is three planes, read with
//      pass_common.h's ld8_n); samples outside the frame are staged as zero and never counted;
//   2. SSE over the samples the tile owns (its MT_H x MT_W block; the last tile of a row / column also owns the halo), fp64;
//   3. per channel: the horizontal 11-tap pass makes the five window rows (x, y, x^2, y^2, xy) in LDS, the vertical pass gives each
//      thread two map positions of one column, the map value is masked to the valid positions and summed;
//   4. butterfly over the 64 lanes, the four waves through LDS in wave order, one (SSIM sum, SSE) partial per workgroup.
// A second launch (one wave per frame) merges the frame's partials in a fixed order and finishes psnr and ssim.
//
// Arithmetic: everything behind the staging is fp64.  The products of two 8-bit-scale fp32 values are exact in fp64, the window
// sums are FMA chains, and E[x^2] - mu^2 is then good to ~1e-13 where fp32 loses three decimals against C2 = 58.5.
// Contraction is off in this file and every FMA is written out, so that x against x gives numerator == denominator bit for bit
// and ssim == 1.0f exactly.
#include <type_traits>

#include "pass_common.h"

#pragma clang fp contract(off)

namespace cvvae {

constexpr int MT_H = 16, MT_W = 32;                      // map positions per tile
constexpr int M_HALO = 10;                               // 11-tap window
constexpr int M_SR = MT_H + M_HALO, M_SC = MT_W + M_HALO;  // staged rows / columns
constexpr int M_SCP = M_SC + 1;                          // LDS row pitch (odd)
constexpr int M_MAX_EXTENT = 1 << 20;                    // H, W
constexpr long long M_MAX_FRAMES = 65535;                // grid.y

struct ClipArg {
  const void* p;
  long long sb, sc, st, sy;
};
struct GaussWin {
  double g[M_HALO + 1];
};
typedef float StagePlane[M_SR][M_SCP];

// the byte cvvae_ncdhw_to_frames_u8 stores for a value held in dtype T (misc_kernels.hip ncdhw_to_frames_u8_kernel, restated here
// operation for operation): clamp, + 1 and * 127.5 as fp32 operations each rounded once to T, then `.to(torch.uint8)`'s truncation.
// tests/test_gpu_metrics_edges.py holds the two to the same bits.
template <typename T>
__device__ __forceinline__ uint8_t unit_to_u8(float x) {
  x = x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x);   // torch.clamp(results, -1.0, 1.0)
  const T a = (T)(x + 1.0f);                         // + 1.0
  const T m = (T)((float)a * 127.5f);                // * 127.5
  return (uint8_t)(float)m;                          // .to(torch.uint8): truncation
}

// a float sample on the 8-bit scale: the byte the scripts' post-processing stores (quantize), or (clamp(x,-1,1) + 1) * 127.5 in fp32
template <typename T>
__device__ __forceinline__ float to_scale8(float x, int quantize) {
  if (quantize) return (float)unit_to_u8<T>(x);
  x = x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x);
  return (x + 1.0f) * 127.5f;
}

// rows [oy0, oy0 + SR) x columns [ox0, ox0 + SC) of frame (b, t) -> s[c][r][x]; zero outside the frame.  ox0 < W always.
template <typename T>
__device__ __forceinline__ void stage_clip(const ClipArg& a, int b, int t, int oy0, int ox0, int H, int W, int SR, int SC,
                                           int quantize, StagePlane* s) {
  const int ncol = min(ox0 + SC, W) - ox0;  // staged columns inside the frame (>= 1)
  if constexpr (std::is_same<T, uint8_t>::value) {
    const uint8_t* base = (const uint8_t*)a.p + (long long)t * a.st + (long long)ox0 * 3;
    const int nvalid = ncol * 3, nbytes = SC * 3;
    constexpr int NDW = (M_SC * 3 + 3 + 3) / 4;  // dwords that cover a row segment at any alignment
    for (int i = threadIdx.x; i < SR * NDW; i += 256) {
      const int r = i / NDW, k = i - r * NDW;
      const int gy = oy0 + r;
      const uint8_t* p0 = base + (long long)(gy < H ? gy : 0) * a.sy;
      const int al = (int)(reinterpret_cast<uintptr_t>(p0) & 3);
      const int j0 = 4 * k - al;  // first byte of this dword, relative to the segment
      const int nv = gy < H ? nvalid : 0;
      uint32_t w = 0;
      if (j0 >= 0 && j0 + 4 <= nv) {
        w = *reinterpret_cast<const uint32_t*>(p0 + j0);  // aligned, wholly inside the row
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (j0 + e >= 0 && j0 + e < nv) w |= (uint32_t)p0[j0 + e] << (8 * e);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = j0 + e;
        if (j >= 0 && j < nbytes) {
          const int px = j / 3;
          s[j - px * 3][r][px] = (float)((w >> (8 * e)) & 255u);
        }
      }
    }
  } else {
    const T* base = (const T*)a.p + (long long)b * a.sb + (long long)t * a.st + ox0;
    const int NG = (SC + 7) / 8;
    for (int i = threadIdx.x; i < 3 * SR * NG; i += 256) {
      const int g = i % NG, cr = i / NG;
      const int r = cr % SR, c = cr / SR;
      const int gy = oy0 + r;
      int n = gy < H ? ncol - 8 * g : 0;
      n = n < 0 ? 0 : (n > 8 ? 8 : n);
      float f[8];
      ld8_n<T>(base + (long long)c * a.sc + (long long)(gy < H ? gy : 0) * a.sy + 8 * g, n, f);  // (n == 0 reads nothing)
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (8 * g + e < SC) s[c][r][8 * g + e] = e < n ? to_scale8<T>(f[e], quantize) : 0.f;
    }
  }
}

template <typename TA, typename TB>
__global__ __launch_bounds__(256) void frame_metrics_tile_kernel(ClipArg A, ClipArg Bv, int T_, int H, int W, int tiles_x, int tiles_y,
                                                                 int halo, int quantize, GaussWin win, double* __restrict__ partials) {
  __shared__ float sA[3][M_SR][M_SCP];
  __shared__ float sB[3][M_SR][M_SCP];
  __shared__ double hb[5][M_SR][MT_W];
  __shared__ double red[2][4];
  const int tile = blockIdx.x, frame = blockIdx.y;
  const int b = frame / T_, t = frame - b * T_;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int oy0 = ty * MT_H, ox0 = tx * MT_W;
  const int SR = MT_H + halo, SC = MT_W + halo;
  stage_clip<TA>(A, b, t, oy0, ox0, H, W, SR, SC, quantize, sA);
  stage_clip<TB>(Bv, b, t, oy0, ox0, H, W, SR, SC, quantize, sB);
  __syncthreads();

  // SSE over the samples this tile owns
  const int own_r = ty == tiles_y - 1 ? SR : MT_H, own_c = tx == tiles_x - 1 ? SC : MT_W;
  double sse = 0.0;
  for (int i = threadIdx.x; i < 3 * SR * SC; i += 256) {
    const int x = i % SC, cr = i / SC;
    const int r = cr % SR, c = cr / SR;
    if (r < own_r && x < own_c && oy0 + r < H && ox0 + x < W) {
      const double d = (double)sA[c][r][x] - (double)sB[c][r][x];
      sse = fma(d, d, sse);
    }
  }

  double ssum = 0.0;
  if (halo) {
    const int VH = H - M_HALO, VW = W - M_HALO;
    const int lx = threadIdx.x & 31, y0 = (threadIdx.x >> 5) * 2;
    for (int c = 0; c < 3; ++c) {
      if (c) __syncthreads();  // the vertical pass of the previous channel has read hb
      for (int i = threadIdx.x; i < M_SR * MT_W; i += 256) {
        const int r = i >> 5, x = i & 31;
        double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
        for (int k = 0; k <= M_HALO; ++k) {
          const double u = (double)sA[c][r][x + k], v = (double)sB[c][r][x + k], w = win.g[k];
          sx = fma(w, u, sx);
          sy = fma(w, v, sy);
          sxx = fma(w, u * u, sxx);  // (u * u, v * v, u * v: exact in fp64)
          syy = fma(w, v * v, syy);
          sxy = fma(w, u * v, sxy);
        }
        hb[0][r][x] = sx;
        hb[1][r][x] = sy;
        hb[2][r][x] = sxx;
        hb[3][r][x] = syy;
        hb[4][r][x] = sxy;
      }
      __syncthreads();
      double m[5][2];
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        double v[M_HALO + 2];
#pragma unroll
        for (int k = 0; k < M_HALO + 2; ++k) v[k] = hb[q][y0 + k][lx];
        double a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int k = 0; k <= M_HALO; ++k) {
          a0 = fma(win.g[k], v[k], a0);
          a1 = fma(win.g[k], v[k + 1], a1);
        }
        m[q][0] = a0;
        m[q][1] = a1;
      }
      const double C1 = 2.55 * 2.55, C2 = 7.65 * 7.65;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        if (oy0 + y0 + e < VH && ox0 + lx < VW) {
          const double mx = m[0][e], my = m[1][e];
          const double xx = mx * mx, yy = my * my, xy = mx * my;
          const double vx = m[2][e] - xx, vy = m[3][e] - yy, cxy = m[4][e] - xy;
          const double num = ((xy + xy) + C1) * ((cxy + cxy) + C2);
          const double den = ((xx + yy) + C1) * ((vx + vy) + C2);
          ssum += num / den;
        }
      }
    }
  }

  // lanes (butterfly), then the four waves in wave order
#pragma unroll
  for (int msk = 1; msk < 64; msk <<= 1) {
    ssum += __shfl_xor(ssum, msk, 64);
    sse += __shfl_xor(sse, msk, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = ssum;
    red[1][threadIdx.x >> 6] = sse;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = partials + ((long long)frame * gridDim.x + tile) * 2;
    o[0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    o[1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  }
}

// one wave per frame: lane l sums partials l, l + 64, ... in index order, then the butterfly
__global__ __launch_bounds__(64) void frame_metrics_finish_kernel(const double* __restrict__ partials, int ntiles, double n_map, double n_samples,
                                                                  double* __restrict__ sse_out, float* __restrict__ psnr, float* __restrict__ ssim) {
  const int frame = blockIdx.x;
  const double* p = partials + (long long)frame * ntiles * 2;
  double ssum = 0.0, sse = 0.0;
  for (int i = threadIdx.x; i < ntiles; i += 64) {
    ssum += p[2 * i];
    sse += p[2 * i + 1];
  }
#pragma unroll
  for (int msk = 1; msk < 64; msk <<= 1) {
    ssum += __shfl_xor(ssum, msk, 64);
    sse += __shfl_xor(sse, msk, 64);
  }
  if (threadIdx.x == 0) {
    sse_out[frame] = sse;
    psnr[frame] = sse == 0.0 ? __builtin_inff() : (float)(10.0 * log10(65025.0 * n_samples / sse));
    if (ssim) ssim[frame] = (float)(ssum / n_map);
  }
}

// ---- host side ----
static inline bool metrics_shape_ok(int64_t B, int64_t T, int64_t H, int64_t W, int32_t want_ssim, int64_t* tiles_x, int64_t* tiles_y) {
  if (B <= 0 || T <= 0 || H <= 0 || W <= 0) return false;
  if (want_ssim && (H <= M_HALO || W <= M_HALO)) return false;
  if (H > M_MAX_EXTENT || W > M_MAX_EXTENT || B > M_MAX_FRAMES || T > M_MAX_FRAMES || B * T > M_MAX_FRAMES) return false;
  const int64_t halo = want_ssim ? M_HALO : 0;
  *tiles_x = (W - halo + MT_W - 1) / MT_W;
  *tiles_y = (H - halo + MT_H - 1) / MT_H;
  return *tiles_x * *tiles_y <= 0x7fffffffLL;
}

template <typename F>
static inline bool by_operand(const cvvae_clip_view* v, F&& f) {
  if (v->layout == CVVAE_CLIP_THWC_U8) {
    f(TypeTag<uint8_t>{});
    return true;
  }
  return by_dtype(v->dtype, f);
}

}  // namespace cvvae

using namespace cvvae;

extern "C" {

size_t cvvae_frame_metrics_workspace_bytes(int32_t B, int32_t T, int32_t H, int32_t W, int32_t want_ssim) {
  int64_t tx, ty;
  if (!metrics_shape_ok(B, T, H, W, want_ssim, &tx, &ty)) return 0;
  return (size_t)((int64_t)B * T * tx * ty * 2 * (int64_t)sizeof(double));
}

int cvvae_frame_metrics(const void* a, const cvvae_clip_view* va, const void* b, const cvvae_clip_view* vb, int32_t B, int32_t T,
                        int32_t H, int32_t W, int32_t quantize, int32_t want_ssim, double* sse, float* psnr, float* ssim,
                        void* workspace, void* stream) {
  if (!a || !b || !va || !vb || !sse || !psnr || !workspace) return CVVAE_EINVAL;
  if (want_ssim && !ssim) return CVVAE_EINVAL;
  if (B <= 0 || T <= 0 || H <= 0 || W <= 0) return CVVAE_EINVAL;
  if ((reinterpret_cast<uintptr_t>(sse) & 7) || (reinterpret_cast<uintptr_t>(workspace) & 7) || (reinterpret_cast<uintptr_t>(psnr) & 3) ||
      (reinterpret_cast<uintptr_t>(ssim) & 3))
    return CVVAE_EINVAL;
  const cvvae_clip_view* views[2] = {va, vb};
  for (const cvvae_clip_view* v : views)
    if (v->sb < 0 || v->sc < 0 || v->st < 0 || v->sy < 0) return CVVAE_EINVAL;
  for (const cvvae_clip_view* v : views) {
    if (v->layout != CVVAE_CLIP_NCTHW && v->layout != CVVAE_CLIP_THWC_U8) return CVVAE_EUNSUPPORTED;
    if (v->layout == CVVAE_CLIP_NCTHW && !known_dtype(v->dtype)) return CVVAE_EUNSUPPORTED;
  }
  for (const cvvae_clip_view* v : views)
    if (v->sy < (int64_t)W * (v->layout == CVVAE_CLIP_THWC_U8 ? 3 : 1)) return CVVAE_EINVAL;
  for (const cvvae_clip_view* v : views)
    if (v->layout == CVVAE_CLIP_THWC_U8 && B != 1) return CVVAE_EUNSUPPORTED;
  int64_t tiles_x, tiles_y;
  if (!metrics_shape_ok(B, T, H, W, want_ssim, &tiles_x, &tiles_y)) return CVVAE_EUNSUPPORTED;

  GaussWin win;
  double wsum = 0.0;
  for (int i = 0; i <= M_HALO; ++i) wsum += (win.g[i] = exp(-(double)((i - 5) * (i - 5)) / 4.5));
  for (int i = 0; i <= M_HALO; ++i) win.g[i] /= wsum;
  const ClipArg A = {a, va->sb, va->sc, va->st, va->sy}, Bv = {b, vb->sb, vb->sc, vb->st, vb->sy};
  const int ntiles = (int)(tiles_x * tiles_y), frames = B * T, halo = want_ssim ? M_HALO : 0;
  hipStream_t s = (hipStream_t)stream;
  double* partials = (double*)workspace;
  by_operand(va, [&](auto ta) {
    using TA = typename decltype(ta)::type;
    by_operand(vb, [&](auto tb) {
      using TB = typename decltype(tb)::type;
      hipLaunchKernelGGL((frame_metrics_tile_kernel<TA, TB>), dim3(ntiles, frames), dim3(256), 0, s, A, Bv, T, H, W, (int)tiles_x,
                         (int)tiles_y, halo, quantize ? 1 : 0, win, partials);
    });
  });
  int rc = launch_status();
  if (rc) return rc;
  const double n_samples = 3.0 * H * W, n_map = want_ssim ? 3.0 * (H - M_HALO) * (W - M_HALO) : 1.0;
  hipLaunchKernelGGL(frame_metrics_finish_kernel, dim3(frames), dim3(64), 0, s, (const double*)partials, ntiles, n_map, n_samples, sse, psnr,
                     want_ssim ? ssim : (float*)nullptr);
  return launch_status();
}

}  // extern "C"
