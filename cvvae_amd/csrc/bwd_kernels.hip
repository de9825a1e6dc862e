// bwd_kernels.hip -- the backward passes of the training path that are not convolutions: the GroupNorm (+ SiLU) backward with and
// without its affine sums, the per-channel sums (bias and GroupNorm-affine gradients), the row-softmax backward, the 2x2 sum (the
// adjoint of the nearest-neighbour upsample), the adjoint of replicate / zero padding and the temporal-attention backward.  No
// encode or decode step launches any of them (cvvae_amd._lib.TRAINING_ONLY_SOURCES).  gfx950 only.
//
// The GroupNorm-backward element, the 8-channel table, the per-channel LDS fold and the finish over the partial tables are written
// ONCE here: cvvae_gn_bwd_input_params and cvvae_channel_sums must agree on d gamma / d beta, and a fix to the FMA contraction or
// to the SiLU derivative belongs in one place.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pass_common.h"

namespace cvvae {

// ---------------------------------------------------------------------------------------------------------
// GroupNorm (+ SiLU) backward -- the frozen-module backward of the training path (cvvae_amd/grad.py) and its trainable form.
//   xh = (x - mean) * rstd = x * rs[c] + nm[c]      (rs = rstd, nm = -mean * rstd: cvvae_gn_finalize with gamma 1, beta 0)
//   a  = xh * gamma[c] + beta[c],  y = act(a)       (the forward value the next conv consumed)
//   gact = gy * act'(a),  gh = gact * gamma[c]      (gradient w.r.t. a and w.r.t. xh)
//   gx = rs * (gh - mean_grp(gh) - xh * mean_grp(gh * xh))  [+ add]
//   d beta[c] = sum gact,  d gamma[c] = sum gact * xh
// Pass 1 (gn_bwd_reduce_kernel) writes, per (row, pixel split, group), sum(gh) and sum(gh * xh); pass 2 (gn_bwd_apply_kernel) sums
// the splits in index order (deterministic) and applies.  Channel quads never straddle a group (C / G a multiple of 4).
// The affine sums alone (chan_sums_kernel) and on the reduction pass (gn_bwd_reduce_kernel<.., PARAMS>) leave one [C][2] table per
// (row, split); chan_sums_final_kernel sums the tables in a fixed order.
// ---------------------------------------------------------------------------------------------------------
struct GnBwdTab {  // the per-channel tables of my 8 channels
  float rs[8], nm[8], ga[8], be[8];
};
// the tables of channels c0 .. c0 + 7 of `row`; those from c0 + n on read as zero (n = 8: all of them are there)
__device__ __forceinline__ void gn_bwd_load_tab(GnBwdTab& t, const float* __restrict__ rs, const float* __restrict__ nm,
                                                const float* __restrict__ gamma, const float* __restrict__ beta, long long row,
                                                int C, int c0, int n = 8) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const bool ok = j < n;
    t.rs[j] = ok ? rs[row * C + c0 + j] : 0.f;
    t.nm[j] = ok ? nm[row * C + c0 + j] : 0.f;
    t.ga[j] = ok ? gamma[c0 + j] : 0.f;
    t.be[j] = ok ? beta[c0 + j] : 0.f;
  }
}

// one element of channel j: xh and gact = gy * act'(a)
__device__ __forceinline__ void gn_bwd_elem(float x, float gy, const GnBwdTab& t, int j, int silu, float& xh, float& gact) {
  xh = __builtin_fmaf(x, t.rs[j], t.nm[j]);
  const float a = __builtin_fmaf(xh, t.ga[j], t.be[j]);
  gact = gy * (silu ? silu_grad_f(a) : 1.0f);
}

// the [C][2] table of a workgroup whose thread pl * cv + v holds the sums s1, s2 of channel vector v over its pixel lane pl:
// channel c sums the pixel lanes of its vector in index order
__device__ __forceinline__ void chan_fold(const float (&s1)[8], const float (&s2)[8], int C, int cv, int ppp, float* __restrict__ o) {
  __shared__ float sh[256][17];
  const int tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sh[tid][j] = s1[j];
    sh[tid][8 + j] = s2[j];
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float a1 = 0.f, a2 = 0.f;
    for (int pl = 0; pl < ppp; ++pl) {
      const int th = pl * cv + (c >> 3);
      if (th < 256) {  // (always, where 256 % cv == 0)
        a1 += sh[th][c & 7];
        a2 += sh[th][8 + (c & 7)];
      }
    }
    o[c * 2] = a1;
    o[c * 2 + 1] = a2;
  }
}

// PARAMS: also the per-channel sums of the affine gradients (the kernel forms gy act'(a) anyway: training the norm costs no extra
// pass over x and gy), one [C][2] table per (row, split) in `wsp`
template <typename T, bool PARAMS = false, int SUB = 4>  // SUB: channels per group-sum slot, as in gn_partial_kernel
__global__ __launch_bounds__(256) void gn_bwd_reduce_kernel(const T* __restrict__ x, const T* __restrict__ gy, long long S, int C,
                                                            int G, int nsplit, const float* __restrict__ rs,
                                                            const float* __restrict__ nm, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, int silu, float* __restrict__ ws,
                                                            float* __restrict__ wsp = nullptr) {
  const int split = blockIdx.x, row = blockIdx.y, tid = threadIdx.x;
  const int cv = C >> 3, ppp = 256 / cv;
  const int myv = tid % cv, mypl = tid / cv;
  const long long per = (S + nsplit - 1) / nsplit;
  const long long p0 = (long long)split * per;
  long long p1 = p0 + per;
  if (p1 > S) p1 = S;
  GnBwdTab t;
  gn_bwd_load_tab(t, rs, nm, gamma, beta, row, C, myv * 8);
  constexpr int NS = 8 / SUB;
  float a1[NS], a2[NS];
#pragma unroll
  for (int h = 0; h < NS; ++h) a1[h] = a2[h] = 0.f;
  float pb[8], pg[8];  // (PARAMS only)
#pragma unroll
  for (int j = 0; j < 8; ++j) pb[j] = pg[j] = 0.f;
  const T* xb = x + (long long)row * S * C + myv * 8;
  const T* gb = gy + (long long)row * S * C + myv * 8;
  // four pixels per trip: their 16-byte loads are issued together (one pixel per trip was latency bound: ~2 TB/s on the
  // million-pixel tensors of a training step); lanes past the end re-read pixel px with a zeroed gradient
  constexpr int U = 4;
  for (long long px = p0 + mypl; px < p1; px += U * ppp) {
    float f[U][8], g[U][8];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool ok = px + u * ppp < p1;
      const long long q = ok ? px + u * ppp : px;
      ld8<T>(xb + q * C, f[u]);
      ld8<T>(gb + q * C, g[u]);
      if (!ok) {
#pragma unroll
        for (int j = 0; j < 8; ++j) g[u][j] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float xh, gact;
        gn_bwd_elem(f[u][j], g[u][j], t, j, silu, xh, gact);
        const float gh = gact * t.ga[j];
        a1[j / SUB] += gh;
        a2[j / SUB] += gh * xh;
        if constexpr (PARAMS) {
          pb[j] += gact;
          pg[j] += gact * xh;
        }
      }
    }
  }
  if constexpr (PARAMS) chan_fold(pb, pg, C, cv, ppp, wsp + ((long long)row * nsplit + split) * C * 2);
  __shared__ float sh1[256][NS], sh2[256][NS];
#pragma unroll
  for (int h = 0; h < NS; ++h) {
    sh1[tid][h] = a1[h];
    sh2[tid][h] = a2[h];
  }
  __syncthreads();
  if (tid < G) {  // group tid: its channel slots (quads / pairs) q, every pixel lane, in index order
    const int qpg = (C / G) / SUB;
    float s1 = 0.f, s2 = 0.f;
    for (int q = tid * qpg; q < (tid + 1) * qpg; ++q)
      for (int pl = 0; pl < ppp; ++pl) {
        const int th = pl * cv + q / NS;
        s1 += sh1[th][q % NS];
        s2 += sh2[th][q % NS];
      }
    float* o = ws + (((long long)row * nsplit + split) * G + tid) * 2;
    o[0] = s1;
    o[1] = s2;
  }
}

template <typename T, int SUB = 4>
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ gy,
                                                           const T* __restrict__ add, T* __restrict__ out, long long S, int C, int G,
                                                           int nsplit, const float* __restrict__ rs, const float* __restrict__ nm,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, int silu,
                                                           const float* __restrict__ ws) {
  const int row = blockIdx.y, tid = threadIdx.x;
  __shared__ float c1[64], c2[64], q1[256], q2[256];
  {  // group g = tid % G, split lane l = tid / G sums splits l, l + lanes, ...; the lanes are then added in index order
    const int lanes = 256 / G, g = tid % G, l = tid / G;
    float s1 = 0.f, s2 = 0.f;
    if (l < lanes)
      for (int sp = l; sp < nsplit; sp += lanes) {
        const float2 o = *reinterpret_cast<const float2*>(ws + (((long long)row * nsplit + sp) * G + g) * 2);
        s1 += o.x;
        s2 += o.y;
      }
    q1[tid] = s1;
    q2[tid] = s2;
    __syncthreads();
    if (tid < G) {
      s1 = 0.f; s2 = 0.f;
      for (int k = 0; k < lanes; ++k) {
        s1 += q1[k * G + tid];
        s2 += q2[k * G + tid];
      }
      const float invd = 1.0f / ((float)(C / G) * (float)S);
      c1[tid] = s1 * invd;
      c2[tid] = s2 * invd;
    }
  }
  __syncthreads();
  const int cv = C >> 3;
  const int myv = tid % cv;  // 256 % cv == 0 and the stride below is a multiple of 256: my channel vector is fixed
  GnBwdTab t;
  gn_bwd_load_tab(t, rs, nm, gamma, beta, row, C, myv * 8);
  const int cpg = C / G;
  constexpr int NS = 8 / SUB;
  float m1[NS], m2[NS];  // the group means of my channel slots
#pragma unroll
  for (int h = 0; h < NS; ++h) {
    m1[h] = c1[(myv * 8 + h * SUB) / cpg];
    m2[h] = c2[(myv * 8 + h * SUB) / cpg];
  }
  const long long nvec = S * cv, base = (long long)row * S * C;
  for (long long v = (long long)blockIdx.x * 256 + tid; v < nvec; v += (long long)gridDim.x * 256) {
    const long long off = base + v * 8;  // v = pixel * cv + myv
    float f[8], g[8], ad[8];
    ld8<T>(x + off, f);
    ld8<T>(gy + off, g);
    if (add) ld8<T>(add + off, ad);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float xh, gact;
      gn_bwd_elem(f[j], g[j], t, j, silu, xh, gact);
      const float gh = gact * t.ga[j];
      const float r = t.rs[j] * (gh - m1[j / SUB] - xh * m2[j / SUB]);
      f[j] = add ? r + ad[j] : r;
    }
    st8<T>(out + off, f);
  }
}

// per-channel sums over pixels, one [C][2] table per (row, split): bias gradients (x = null: sum g in slot 0) and the GroupNorm
// affine gradients (d beta, d gamma)
template <typename T>
__global__ __launch_bounds__(256) void chan_sums_kernel(const T* __restrict__ x, const T* __restrict__ g, long long S, int C,
                                                        long long g_ps, int nsplit, const float* __restrict__ rs,
                                                        const float* __restrict__ nm, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, int silu, float* __restrict__ ws) {
  const int split = blockIdx.x, row = blockIdx.y, tid = threadIdx.x;
  const int cv = (C + 7) >> 3;
  const int ppp = 256 / cv > 0 ? 256 / cv : 1;
  const int myv = tid % cv, mypl = tid / cv;
  const long long per = (S + nsplit - 1) / nsplit;
  const long long p0 = (long long)split * per;
  long long p1 = p0 + per;
  if (p1 > S) p1 = S;
  GnBwdTab t;
  gn_bwd_load_tab(t, rs, nm, gamma, beta, row, C, myv * 8, x != nullptr ? C - myv * 8 : 0);
  float s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
  if (mypl < ppp && myv * 8 < C) {
    // four pixels per trip: their 16-byte loads are issued together (one pixel per trip left ~4 MB in flight on the chip --
    // latency bound at ~2 TB/s); lanes past the end re-read pixel px with a zeroed gradient
    constexpr int U = 4;
    for (long long px = p0 + mypl; px < p1; px += U * ppp) {
      float f[U][8], gg[U][8];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool ok = px + u * ppp < p1;
        const long long q = ok ? px + u * ppp : px;
        ld8<T>(g + ((long long)row * S + q) * g_ps + myv * 8, gg[u]);
        if (x != nullptr) ld8<T>(x + ((long long)row * S + q) * (long long)C + myv * 8, f[u]);
        if (!ok) {
#pragma unroll
          for (int j = 0; j < 8; ++j) gg[u][j] = 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (x != nullptr) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float xh, gact;
            gn_bwd_elem(f[u][j], gg[u][j], t, j, silu, xh, gact);
            s1[j] += gact;
            s2[j] += gact * xh;
          }
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) s1[j] += gg[u][j];
        }
      }
    }
  }
  chan_fold(s1, s2, C, cv, ppp, ws + ((long long)row * nsplit + split) * C * 2);
}

// o1[c], o2[c] (either may be null) = sums over `nparts` [C][2] tables
__global__ __launch_bounds__(256) void chan_sums_final_kernel(const float* __restrict__ ws, int nparts, int C, float* __restrict__ o1,
                                                              float* __restrict__ o2) {
  // a block = 32 channels x 8 part lanes: lane pl sums parts pl, pl + 8, ... (coalesced 256-byte rows), then the 8 lanes are
  // added in index order -- a fixed summation order, hence bit-reproducible
  __shared__ float sh[8][32][2];
  const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  float a1 = 0.f, a2 = 0.f;
  if (c < C) {
    int i = pl;
    for (; i + 24 < nparts; i += 32) {  // four loads in flight, added in index order
      float2 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float2*>(ws + ((long long)(i + 8 * u) * C + c) * 2);
#pragma unroll
      for (int u = 0; u < 4; ++u) { a1 += v[u].x; a2 += v[u].y; }
    }
    for (; i < nparts; i += 8) {
      const float2 v = *reinterpret_cast<const float2*>(ws + ((long long)i * C + c) * 2);
      a1 += v.x;
      a2 += v.y;
    }
  }
  sh[pl][cl][0] = a1;
  sh[pl][cl][1] = a2;
  __syncthreads();
  if (pl == 0 && c < C) {
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      s1 += sh[k][cl][0];
      s2 += sh[k][cl][1];
    }
    if (o1) o1[c] = s1;
    if (o2) o2[c] = s2;
  }
}

static inline int gn_bwd_splits(long long S) {  // >= 512 pixels per split (a 147 k-pixel tensor at 2048 had 72 workgroups for 256 CUs)
  // (up to 1024 splits: a 5-D GroupNorm has ONE row per sample, and 64 workgroups left three quarters of the CUs idle on the
  //  million-pixel tensors of a training step -- 372 us per call, profiles/r4_train_step_kernel_stats_v2.txt)
  const long long n = (S + 511) / 512;
  return (int)(n < 1 ? 1 : (n > 1024 ? 1024 : n));
}

static inline int chan_sums_splits(long long S, int rows, int C) {
  // ~32 pixels per thread (8 trips of 4): a workgroup covers 256 / (C / 8) pixels per step, so wide tensors take short splits
  // (at a fixed 1024 pixels per split a 512-channel tensor gave each thread 256 dependent trips and a 147 k-pixel one 144
  // workgroups for 256 CUs)
  const int cv = (C + 7) >> 3;
  const int ppp = 256 / cv > 0 ? 256 / cv : 1;
  long long per = 32ll * ppp;
  if (per < 128) per = 128;
  long long n = (S + per - 1) / per;
  const long long cap = rows > 0 ? (2048 + rows - 1) / rows : 2048;
  if (n > cap) n = cap;
  return (int)(n < 1 ? 1 : n);
}

template <typename T, int SUB>
static void gn_bwd_launch(const void* x, const void* gy, const void* add, int rows, long long S, int C, int G, const float* rs,
                          const float* nm, const float* gamma, const float* beta, int silu, void* gx, float* ws, hipStream_t s,
                          float* dgamma, float* dbeta) {
  const int nsplit = gn_bwd_splits(S);
  if (dgamma) {  // training the norm: the affine sums ride on the reduction pass (tables behind the group sums in the workspace)
    float* wsp = ws + (long long)rows * nsplit * G * 2;
    hipLaunchKernelGGL((gn_bwd_reduce_kernel<T, true, SUB>), dim3(nsplit, rows), dim3(256), 0, s, (const T*)x, (const T*)gy, S, C, G, nsplit,
                       rs, nm, gamma, beta, silu, ws, wsp);
    hipLaunchKernelGGL(chan_sums_final_kernel, dim3((C + 31) / 32), dim3(256), 0, s, (const float*)wsp, rows * nsplit, C, dbeta, dgamma);
  } else
  hipLaunchKernelGGL((gn_bwd_reduce_kernel<T, false, SUB>), dim3(nsplit, rows), dim3(256), 0, s, (const T*)x, (const T*)gy, S, C, G, nsplit, rs, nm,
                     gamma, beta, silu, ws);
  long long blocks = (S * (C / 8) + 255) / 256;
  if (blocks > 2048) blocks = 2048;  // grid-stride beyond 8 blocks per CU and row
  hipLaunchKernelGGL((gn_bwd_apply_kernel<T, SUB>), dim3((unsigned)blocks, rows), dim3(256), 0, s, (const T*)x, (const T*)gy, (const T*)add,
                     (T*)gx, S, C, G, nsplit, rs, nm, gamma, beta, silu, ws);
}

// the body of cvvae_gn_bwd_input (dgamma = dbeta = null) and of cvvae_gn_bwd_input_params
static int gn_bwd_input(int32_t dtype, const void* x, const void* gy, const void* add, int32_t rows, int64_t S, int32_t C, int32_t groups,
                        const float* rstd, const float* nmean, const float* gamma, const float* beta, int32_t silu, void* gx,
                        float* dgamma, float* dbeta, void* workspace, void* stream) {
  if (!x || !gy || !gx || !rstd || !nmean || !gamma || !beta || !workspace || rows <= 0 || S <= 0 || C <= 0) return CVVAE_EINVAL;
  // 8-channel vectors that tile a 256-thread block; channel quads (or pairs) inside one group
  if (groups <= 0 || groups > 64 || C % groups || (C / groups) % 2 || C % 8 || C > 2048 || 256 % (C / 8)) return CVVAE_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const bool ok = by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    // group sums on channel quads where the groups are made of them, on pairs otherwise (groups of 2 or 6 channels)
    if ((C / groups) % 4 == 0)
      gn_bwd_launch<T, 4>(x, gy, add, rows, S, C, groups, rstd, nmean, gamma, beta, silu, gx, (float*)workspace, s, dgamma, dbeta);
    else
      gn_bwd_launch<T, 2>(x, gy, add, rows, S, C, groups, rstd, nmean, gamma, beta, silu, gx, (float*)workspace, s, dgamma, dbeta);
  });
  if (!ok) return CVVAE_EINVAL;
  return launch_status();
}

// ---------------------------------------------------------------------------------------------------------
// gradient of the row softmax: gs = alpha * p * (gp - sum_j p_j gp_j); columns >= n_valid (up to ld_o) are written as 0
// ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void softmax_bwd_rows_kernel(const T* __restrict__ p, long long ld_p, const float* __restrict__ gp,
                                                               long long ld_g, int n_valid, float alpha, T* __restrict__ out,
                                                               long long ld_o) {
  __shared__ float sh[4];
  const T* pr = p + (long long)blockIdx.x * ld_p;
  const float* gr = gp + (long long)blockIdx.x * ld_g;
  T* orow = out + (long long)blockIdx.x * ld_o;
  float dot = 0.f;
  for (int i = threadIdx.x; i < n_valid; i += 256) dot += (float)pr[i] * gr[i];
  dot = block_reduce(dot, false, sh);
  for (int i = threadIdx.x; i < (int)ld_o; i += 256) orow[i] = (T)(i < n_valid ? alpha * (float)pr[i] * (gr[i] - dot) : 0.f);
}

// gradient of the nearest-neighbour x2 upsample (H and W): out[n][y][x][c] = sum of the 2x2 block of g [n][2H][2W][C]
template <typename T>
__global__ __launch_bounds__(256) void upsample2x_sum_kernel(const T* __restrict__ g, long long N, int H, int W, int C,
                                                             T* __restrict__ out) {
  const int cv = C >> 3;
  const long long nvec = N * H * W * cv;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (long long)gridDim.x * 256) {
    const int c0 = (int)(v % cv) * 8;
    long long pix = v / cv;
    const int xo = (int)(pix % W);
    pix /= W;
    const int yo = (int)(pix % H);
    const long long n = pix / H;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      float f[8];
      ld8<T>(g + (((n * 2 * H + 2 * yo + (d >> 1)) * 2 * W) + 2 * xo + (d & 1)) * C + c0, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += f[j];
    }
    st8<T>(out + ((n * H + yo) * W + xo) * C + c0, acc);
  }
}

// ---------------------------------------------------------------------------------------------------------
// adjoint of replicate / zero padding: gp [B][Tp][Hp][Wp][C] is the gradient w.r.t. the PADDED input (front pads pt, ph, pw);
// out[b][t][y][x] = sum of gp over every padded position that the forward's coordinate map sends to (t, y, x)
// (replicate: clamp -- border elements collect their whole pad region; zero: only the interior copy).  `add` is summed in.
// ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void pad_fold_kernel(const T* __restrict__ gp, int B, int T_, int H, int W, int C, int Tp, int Hp,
                                                       int Wp, int pt, int ph, int pw, int mode_t, int mode_hw,
                                                       const T* __restrict__ add, T* __restrict__ out) {
  const int cv = C >> 3;
  const long long nvec = (long long)B * T_ * H * W * cv;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (long long)gridDim.x * 256) {
    const int c0 = (int)(v % cv) * 8;
    long long pix = v / cv;
    const int x = (int)(pix % W);
    pix /= W;
    const int y = (int)(pix % H);
    pix /= H;
    const int t = (int)(pix % T_);
    const int b = (int)(pix / T_);
    // padded index range [lo, hi] that maps to coordinate c of an axis of length L
    auto range = [](int c, int L, int pf, int Lp, int mode, int& lo, int& hi) {
      lo = hi = c + pf;
      if (mode) {
        if (c == 0) lo = 0;
        if (c == L - 1) hi = Lp - 1;
      }
    };
    int t0, t1, y0, y1, x0, x1;
    range(t, T_, pt, Tp, mode_t, t0, t1);
    range(y, H, ph, Hp, mode_hw, y0, y1);
    range(x, W, pw, Wp, mode_hw, x0, x1);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int tp = t0; tp <= t1; ++tp)
      for (int yp = y0; yp <= y1; ++yp)
        for (int xp = x0; xp <= x1; ++xp) {
          float f[8];
          ld8<T>(gp + ((((long long)b * Tp + tp) * Hp + yp) * Wp + xp) * C + c0, f);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] += f[j];
        }
    const long long off = ((((long long)b * T_ + t) * H + y) * W + x) * C + c0;
    if (add) {
      float f[8];
      ld8<T>(add + off, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += f[j];
    }
    st8<T>(out + off, acc);
  }
}

// ---------------------------------------------------------------------------------------------------------
// backward of cvvae_temporal_attention (MemoryEfficientAttnVideoBlock.attention_t, models/vae_models.py:573-587): per pixel,
// softmax(q k^T * scale) v over the Tn <= 8 frames of a clip.  One wave per pixel, as the forward: pass 1 over the channels forms
// S = q k^T and dP = go v^T (two 8 x 8 tables per lane, reduced over the wave), the softmax and its gradient
// dS = scale * P o (dP - rowsum(P o dP)) are per lane; pass 2 writes dq = dS k, dk = dS^T q, dv = P^T go.
// ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void temporal_attn_bwd_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                                const T* __restrict__ v, const T* __restrict__ go, long long P,
                                                                int Tn, long long S, int C, float scale, T* __restrict__ gq,
                                                                T* __restrict__ gk, T* __restrict__ gv) {
  const long long pix = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);  // over B*S
  if (pix >= P) return;
  const int lane = threadIdx.x & 63;
  const int nv = C >> 3;
  const long long b = pix / S, s = pix - b * S;
  const long long base = (b * Tn * S + s) * C, tstride = S * C;
  float sc[8][8], dp[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) sc[i][j] = dp[i][j] = 0.f;
  for (int vv = lane; vv < nv; vv += 64) {
    float qf[8][8], gf[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < Tn) {
        ld8<T>(q + base + i * tstride + vv * 8, qf[i]);
        ld8<T>(go + base + i * tstride + vv * 8, gf[i]);
      }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < Tn) {
        float kf[8], vf[8];
        ld8<T>(k + base + j * tstride + vv * 8, kf);
        ld8<T>(v + base + j * tstride + vv * 8, vf);
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (i < Tn) {
            float d1 = 0.f, d2 = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              d1 += qf[i][e] * kf[e];
              d2 += gf[i][e] * vf[e];
            }
            sc[i][j] += d1;
            dp[i][j] += d2;
          }
      }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float x = sc[i][j], y = dp[i][j];
#pragma unroll
      for (int off = 32; off; off >>= 1) {
        x += __shfl_xor(x, off);
        y += __shfl_xor(y, off);
      }
      sc[i][j] = x * scale;
      dp[i][j] = y;
    }
  // P (as the forward computes it), then dS in place of dp
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (i < Tn) {
      float mx = -3.0e38f;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < Tn) mx = fmaxf(mx, sc[i][j]);
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < Tn) {
          sc[i][j] = __expf(sc[i][j] - mx);
          sum += sc[i][j];
        }
      const float inv = 1.0f / sum;
      float dot = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        sc[i][j] = (j < Tn) ? sc[i][j] * inv : 0.f;
        dot += sc[i][j] * dp[i][j];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) dp[i][j] = (j < Tn) ? scale * sc[i][j] * (dp[i][j] - dot) : 0.f;
    }
  for (int vv = lane; vv < nv; vv += 64) {
    float qf[8][8], gf[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < Tn) {
        ld8<T>(q + base + i * tstride + vv * 8, qf[i]);
        ld8<T>(go + base + i * tstride + vv * 8, gf[i]);
      }
    float dq[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int e = 0; e < 8; ++e) dq[i][e] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < Tn) {
        float kf[8], dk[8], dv[8];
        ld8<T>(k + base + j * tstride + vv * 8, kf);
#pragma unroll
        for (int e = 0; e < 8; ++e) dk[e] = dv[e] = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (i < Tn) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              dq[i][e] += dp[i][j] * kf[e];
              dk[e] += dp[i][j] * qf[i][e];
              dv[e] += sc[i][j] * gf[i][e];
            }
          }
        st8<T>(gk + base + j * tstride + vv * 8, dk);
        st8<T>(gv + base + j * tstride + vv * 8, dv);
      }
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < Tn) st8<T>(gq + base + i * tstride + vv * 8, dq[i]);
  }
}

}  // namespace cvvae

using namespace cvvae;

extern "C" {

int64_t cvvae_gn_bwd_workspace_bytes(int32_t rows, int32_t groups, int64_t S) {
  if (rows <= 0 || groups <= 0 || S <= 0) return 0;
  return (int64_t)rows * gn_bwd_splits(S) * groups * 2 * (int64_t)sizeof(float);
}

int64_t cvvae_gn_bwd_params_workspace_bytes(int32_t rows, int32_t groups, int64_t S, int32_t C) {
  if (rows <= 0 || groups <= 0 || S <= 0 || C <= 0) return 0;
  return (int64_t)rows * gn_bwd_splits(S) * (groups + C) * 2 * (int64_t)sizeof(float);
}

int cvvae_gn_bwd_input_params(int32_t dtype, const void* x, const void* gy, const void* add, int32_t rows, int64_t S, int32_t C,
                              int32_t groups, const float* rstd, const float* nmean, const float* gamma, const float* beta,
                              int32_t silu, void* gx, float* dgamma, float* dbeta, void* workspace, void* stream) {
  if (!dgamma || !dbeta) return CVVAE_EINVAL;
  return gn_bwd_input(dtype, x, gy, add, rows, S, C, groups, rstd, nmean, gamma, beta, silu, gx, dgamma, dbeta, workspace, stream);
}

int cvvae_gn_bwd_input(int32_t dtype, const void* x, const void* gy, const void* add, int32_t rows, int64_t S, int32_t C,
                       int32_t groups, const float* rstd, const float* nmean, const float* gamma, const float* beta, int32_t silu,
                       void* gx, void* workspace, void* stream) {
  return gn_bwd_input(dtype, x, gy, add, rows, S, C, groups, rstd, nmean, gamma, beta, silu, gx, nullptr, nullptr, workspace, stream);
}

int cvvae_softmax_bwd_rows(int32_t dtype, const void* p, int64_t ld_p, const float* gp, int64_t ld_g, int64_t rows, int32_t n_valid,
                           float alpha, void* gs, int64_t ld_o, void* stream) {
  if (!p || !gp || !gs || rows <= 0 || n_valid <= 0 || ld_p < n_valid || ld_g < n_valid || ld_o < n_valid) return CVVAE_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const bool ok = by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(softmax_bwd_rows_kernel<T>, dim3((unsigned)rows), dim3(256), 0, s, (const T*)p, (long long)ld_p, gp,
                       (long long)ld_g, n_valid, alpha, (T*)gs, (long long)ld_o);
  });
  if (!ok) return CVVAE_EINVAL;
  return launch_status();
}

int cvvae_upsample2x_sum(int32_t dtype, const void* g, int64_t N, int32_t H, int32_t W, int32_t C, void* out, void* stream) {
  if (!g || !out || N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8) return CVVAE_EINVAL;
  long long blocks = ((long long)N * H * W * (C / 8) + 255) / 256;
  if (blocks > 256LL * 64) blocks = 256LL * 64;
  hipStream_t s = (hipStream_t)stream;
  const bool ok = by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(upsample2x_sum_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, s, (const T*)g, (long long)N, H, W, C, (T*)out);
  });
  if (!ok) return CVVAE_EINVAL;
  return launch_status();
}

int64_t cvvae_channel_sums_workspace_bytes(int32_t rows, int64_t S, int32_t C) {
  if (rows <= 0 || S <= 0 || C <= 0) return CVVAE_EINVAL;
  return (int64_t)rows * chan_sums_splits(S, rows, C) * C * 2 * (int64_t)sizeof(float);
}

// x == NULL: sum1[c] = sum over rows x S pixels of g (a bias gradient); else the GroupNorm affine gradients
// sum1 = d beta, sum2 = d gamma with (rstd, -mean*rstd) tables [rows][C] as in cvvae_gn_bwd_input
int cvvae_channel_sums(int32_t dtype, const void* x, const void* g, int64_t g_pix_stride, int32_t rows, int64_t S, int32_t C,
                       const float* rstd, const float* nmean, const float* gamma, const float* beta, int32_t silu, float* sum1,
                       float* sum2, void* workspace, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!g || !sum1 || !workspace || rows <= 0 || S <= 0 || C <= 0 || C % 8 || C > 2048 || g_pix_stride < C || g_pix_stride % 8)
    return CVVAE_EINVAL;
  if (x && (!rstd || !nmean || !gamma || !beta || !sum2 || g_pix_stride != C)) return CVVAE_EINVAL;
  if ((C >> 3) > 256) return CVVAE_EUNSUPPORTED;
  const int nsplit = chan_sums_splits(S, rows, C);
  float* ws = (float*)workspace;
  const bool ok = by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(chan_sums_kernel<T>, dim3(nsplit, rows), dim3(256), 0, stream, (const T*)x, (const T*)g, S, C, g_pix_stride, nsplit,
                       rstd, nmean, gamma, beta, silu, ws);
  });
  if (!ok) return CVVAE_EINVAL;
  int rc = launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(chan_sums_final_kernel, dim3((C + 31) / 32), dim3(256), 0, stream, (const float*)ws, rows * nsplit, C, sum1,
                     sum2);
  return launch_status();
}

int cvvae_pad_fold(int32_t dtype, const void* gp, int32_t B, int32_t T, int32_t H, int32_t W, int32_t C, int32_t pad_t_front,
                   int32_t pad_t_back, int32_t pad_h, int32_t pad_w, int32_t pad_mode_t, int32_t pad_mode_hw, const void* add, void* out,
                   void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!gp || !out || B <= 0 || T <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8) return CVVAE_EINVAL;
  if (pad_t_front < 0 || pad_t_back < 0 || pad_h < 0 || pad_w < 0) return CVVAE_EINVAL;
  const int Tp = T + pad_t_front + pad_t_back, Hp = H + 2 * pad_h, Wp = W + 2 * pad_w;
  long long blocks = ((long long)B * T * H * W * (C / 8) + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  const bool ok = by_dtype(dtype, [&](auto tag) {
    using TY = typename decltype(tag)::type;  // (T is the frame count here)
    hipLaunchKernelGGL(pad_fold_kernel<TY>, dim3((unsigned)blocks), dim3(256), 0, stream, (const TY*)gp, B, T, H, W, C, Tp, Hp, Wp,
                       pad_t_front, pad_h, pad_w, pad_mode_t, pad_mode_hw, (const TY*)add, (TY*)out);
  });
  if (!ok) return CVVAE_EINVAL;
  return launch_status();
}

int cvvae_temporal_attention_bwd(int32_t dtype, const void* q, const void* k, const void* v, const void* go, int32_t B, int32_t Tn,
                                 int64_t S, int32_t C, void* gq, void* gk, void* gv, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!q || !k || !v || !go || !gq || !gk || !gv || B <= 0 || Tn <= 0 || S <= 0 || C <= 0 || C % 8) return CVVAE_EINVAL;
  if (Tn > 8) return CVVAE_EUNSUPPORTED;  // (the windows of the reference's wrapper give T' <= 5; longer sequences: not built)
  const long long P = (long long)B * S;
  const float scale = 1.0f / sqrtf((float)C);
  const unsigned grid = (unsigned)((P + 3) / 4);
  const bool ok = by_dtype(dtype, [&](auto tag) {
    using TY = typename decltype(tag)::type;
    hipLaunchKernelGGL(temporal_attn_bwd_kernel<TY>, dim3(grid), dim3(256), 0, stream, (const TY*)q, (const TY*)k, (const TY*)v,
                       (const TY*)go, P, Tn, (long long)S, C, scale, (TY*)gq, (TY*)gk, (TY*)gv);
  });
  if (!ok) return CVVAE_EINVAL;
  return launch_status();
}

}  // extern "C"
