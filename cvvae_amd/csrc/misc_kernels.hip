// misc_kernels.hip -- the HBM-bound FORWARD kernels around the conv: GroupNorm statistics, LayerNorm, row softmax, transpose,
// temporal attention, NCDHW<->NDHWC, tile blending (the weight packers are in pack_kernels.hip, the backward passes of these
// kernels in bwd_kernels.hip: nothing here runs only in training).  gfx950 only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cvvae.h"
#include "conv_kernel.h"

namespace cvvae {

// ---------------------------------------------------------------------------------------------------------
// GroupNorm statistics.  Stage 1: grid (nsplit, rows); each block reduces a slab of pixels for all channels
// with Welford/Chan updates on 4-channel quads; stage 2 merges the slabs and emits the affine table.
// SUB = channels per statistics slot of a lane's 8 channels: 4 (groups of whole quads), or 2 for groups of 2 or 6 channels
// (GroupNorm(32, 64) of the discriminator) -- the same arithmetic on pairs.
// ---------------------------------------------------------------------------------------------------------
template <typename T, int SUB = 4>
__global__ __launch_bounds__(256) void gn_partial_kernel(const T* __restrict__ x, long long S, int C, long long ps,
                                                         int G, int nsplit, float* __restrict__ ws) {
  const int split = blockIdx.x, row = blockIdx.y;
  const int cv = C >> 3;         // 16-byte channel vectors per pixel
  const int ppp = 256 / cv;      // pixels per pass
  const int tid = threadIdx.x;
  const int myv = tid % cv, mypl = tid / cv;
  const long long per = (S + nsplit - 1) / nsplit;
  const long long p0 = (long long)split * per;
  long long p1 = p0 + per;
  if (p1 > S) p1 = S;
  constexpr int NS = 8 / SUB;  // slots per lane
  WStat st[NS];
#pragma unroll
  for (int h = 0; h < NS; ++h) st[h] = {0.f, 0.f, 0.f};
  if (tid < cv * ppp) {
    const T* base = x + ((long long)row * S) * ps + myv * 8;
    long long px = p0 + mypl;
    // main loop: 8 independent 16-byte loads in flight per thread, then an exact two-pass (sum, then squared
    // deviations) over the 32 values of each channel quad held in registers, and ONE Chan merge per batch
    constexpr int U = 8;
    for (; px + (long long)(U - 1) * ppp < p1; px += (long long)U * ppp) {
      Raw8<T> u[U];
#pragma unroll
      for (int i = 0; i < U; ++i) u[i] = ldraw8<T>(base + (px + (long long)i * ppp) * ps);
      float f[U][8];
#pragma unroll
      for (int i = 0; i < U; ++i) unraw8<T>(u[i], f[i]);
#pragma unroll
      for (int h = 0; h < NS; ++h) {
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < U; ++i) {
          if constexpr (SUB == 4)
            sum += (f[i][h * 4 + 0] + f[i][h * 4 + 1]) + (f[i][h * 4 + 2] + f[i][h * 4 + 3]);
          else
            sum += f[i][h * 2 + 0] + f[i][h * 2 + 1];
        }
        const float mb = sum * (1.0f / (SUB * U));
        float m2b = 0.f;
#pragma unroll
        for (int i = 0; i < U; ++i)
#pragma unroll
          for (int j = 0; j < SUB; ++j) {
            const float d = f[i][h * SUB + j] - mb;
            m2b += d * d;
          }
        WStat q = {(float)(SUB * U), mb, m2b};
        chan_merge(st[h], q);
      }
    }
    for (; px < p1; px += ppp) {
      float f[8];
      ld8<T>(base + px * ps, f);
#pragma unroll
      for (int h = 0; h < NS; ++h) {
        if constexpr (SUB == 4) {
          const float a = f[h * 4 + 0], b = f[h * 4 + 1], c = f[h * 4 + 2], d = f[h * 4 + 3];
          const float mb = (a + b + c + d) * 0.25f;
          const float m2b = (a - mb) * (a - mb) + (b - mb) * (b - mb) + (c - mb) * (c - mb) + (d - mb) * (d - mb);
          WStat q = {4.f, mb, m2b};
          chan_merge(st[h], q);
        } else {
          const float a = f[h * 2 + 0], b = f[h * 2 + 1];
          const float mb = (a + b) * 0.5f;
          const float m2b = (a - mb) * (a - mb) + (b - mb) * (b - mb);
          WStat q = {2.f, mb, m2b};
          chan_merge(st[h], q);
        }
      }
    }
  }
  __shared__ WStat sh[256 * NS];
#pragma unroll
  for (int h = 0; h < NS; ++h) sh[tid * NS + h] = st[h];
  __syncthreads();
  // More than 64 pixel lanes (C < 32): fold the lanes pairwise first.  One thread merging 256 lanes in a row rounds the running mean
  // 256 times; with the mean 40 sigma from zero that alone is more than the 2e-5 sigma the statistics are held to (measured 3.7e-5
  // at C = 8, tests/test_gpu_pass_edges.py; a third of the allowance at 32 lanes), the tree rounds it 8 times.  64 lanes or fewer
  // keep the loop below, and their results bit for bit.
  int npl = ppp;
  if (ppp > 64) {
    for (; npl > 1; npl = (npl + 1) >> 1) {
      const int half = (npl + 1) >> 1;  // lane pl < npl - half takes lane pl + half: writers and partners are disjoint
      if (mypl + half < npl) {
#pragma unroll
        for (int h = 0; h < NS; ++h) chan_merge(sh[tid * NS + h], sh[(tid + half * cv) * NS + h]);
      }
      __syncthreads();
    }
  }
  if (tid < G) {
    const int cpg = C / G;        // channels per group (multiple of SUB)
    const int qpg = cpg / SUB;    // slots (quads / pairs) per group
    WStat acc = {0.f, 0.f, 0.f};
    const int q0 = tid * qpg;     // first slot index (over channels) of this group
    for (int pl = 0; pl < npl; ++pl)
      for (int q = q0; q < q0 + qpg; ++q) {
        const int v = q / NS, h = q % NS;
        chan_merge(acc, sh[(pl * cv + v) * NS + h]);
      }
    float* o = ws + (((long long)row * nsplit + split) * G + tid) * 3;
    o[0] = acc.n;
    o[1] = acc.mean;
    o[2] = acc.m2;
  }
}

__global__ __launch_bounds__(256) void gn_finalize_kernel(const float* __restrict__ ws, int nsplit, int G, int C, float eps,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float* __restrict__ scale, float* __restrict__ shift) {
  const int row = blockIdx.x, tid = threadIdx.x;
  __shared__ float s_mean[64], s_rstd[64];
  // 8 lanes per group (G <= 32)
  const int g = tid >> 3, l8 = tid & 7;
  WStat acc = {0.f, 0.f, 0.f};
  if (g < G) {
    for (int s = l8; s < nsplit; s += 8) {
      const float* o = ws + (((long long)row * nsplit + s) * G + g) * 3;
      WStat q = {o[0], o[1], o[2]};
      chan_merge(acc, q);
    }
  }
#pragma unroll
  for (int off = 1; off < 8; off <<= 1) {
    WStat q;
    q.n = __shfl_xor(acc.n, off);
    q.mean = __shfl_xor(acc.mean, off);
    q.m2 = __shfl_xor(acc.m2, off);
    chan_merge(acc, q);
  }
  if (g < G && l8 == 0) {
    s_mean[g] = acc.mean;
    s_rstd[g] = rsqrtf(acc.m2 / acc.n + eps);
  }
  __syncthreads();
  const int cpg = C / G;
  for (int c = tid; c < C; c += 256) {
    const int gg = c / cpg;
    const float sc = gamma[c] * s_rstd[gg];
    scale[(long long)row * C + c] = sc;
    shift[(long long)row * C + c] = beta[c] - s_mean[gg] * sc;
  }
}

// Finalize for the statistics fused into the conv epilogue: grid (G, rows); the block merges the `slabs` records of
// its (row, group) -- ws[(row*G + g)*slabs + s] = (n, mean, M2), contiguous -- in a fixed order (thread-strided, then a Chan tree)
// and writes the affine table of the group's channels.
// frames > 1: per-FRAME statistics (the per-frame GroupNorm of the attention blocks) from the records of a per-frame producer
// (kT = 1 convs: one-frame tiles in frame-major order): table row = sample * frames + frame, merging that frame's slabs / frames
// consecutive records.
__global__ __launch_bounds__(256) void gn_finalize_slabs_kernel(const float* __restrict__ ws, long long slabs_total, int G, int C,
                                                                float eps, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float* __restrict__ scale,
                                                                float* __restrict__ shift, int frames) {
  const int g = blockIdx.x, tid = threadIdx.x;
  const int orow = blockIdx.y;                      // output table row
  const int row = orow / frames, fr = orow - row * frames;
  const long long slabs = slabs_total / frames;
  const float* base = ws + (((long long)row * G + g) * slabs_total + (long long)fr * slabs) * 3;  // my (row, group, frame) records
  WStat acc = {0.f, 0.f, 0.f};
  // keep 8 independent loads in flight per thread and merge them in index order afterwards (the merge order, hence the
  // result, does not depend on the batching); a wave's loads cover 768 contiguous bytes
  constexpr int U = 8;
  long long s = tid;
  for (; s + (long long)(U - 1) * 256 < slabs; s += (long long)U * 256) {
    WStat q[U];
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const float* o = base + (s + (long long)i * 256) * 3;
      q[i].n = o[0];
      q[i].mean = o[1];
      q[i].m2 = o[2];
    }
#pragma unroll
    for (int i = 0; i < U; ++i) chan_merge(acc, q[i]);
  }
  for (; s < slabs; s += 256) {
    const float* o = base + s * 3;
    WStat q = {o[0], o[1], o[2]};
    chan_merge(acc, q);
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    WStat q;
    q.n = __shfl_xor(acc.n, off);
    q.mean = __shfl_xor(acc.mean, off);
    q.m2 = __shfl_xor(acc.m2, off);
    // both partners must end with the same value: merge in a fixed (lower lane first) order
    WStat lo = (tid & off) ? q : acc, hi = (tid & off) ? acc : q;
    chan_merge(lo, hi);
    acc = lo;
  }
  __shared__ WStat sh[4];
  if ((tid & 63) == 0) sh[tid >> 6] = acc;
  __syncthreads();
  WStat t = sh[0];
  chan_merge(t, sh[1]);
  chan_merge(t, sh[2]);
  chan_merge(t, sh[3]);
  const float mean = t.mean, rstd = rsqrtf(t.m2 / t.n + eps);
  const int cpg = C / G;
  for (int c = g * cpg + tid; c < (g + 1) * cpg; c += 256) {
    const float sc = gamma[c] * rstd;
    scale[(long long)orow * C + c] = sc;
    shift[(long long)orow * C + c] = beta[c] - mean * sc;
  }
}

// ---------------------------------------------------------------------------------------------------------
// GroupNorm-apply (+ SiLU) pass: the conv prologue's arithmetic (gn_affine + silu_f of conv_kernel.h), once per element
// ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void gn_silu_apply_kernel(const T* __restrict__ x, long long S, int C, long long ps,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            int silu, T* __restrict__ out, long long nvec) {
  const int cv = C >> 3;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < nvec; g += (long long)gridDim.x * 256) {
    const long long pix = g / cv;
    const int c0 = (int)(g - pix * cv) * 8;
    const long long row = pix / S;
    float f[8];
    ld8<T>(x + pix * ps + c0, f);
    const float4 a0 = *reinterpret_cast<const float4*>(scale + row * C + c0), a1 = *reinterpret_cast<const float4*>(scale + row * C + c0 + 4);
    const float4 b0 = *reinterpret_cast<const float4*>(shift + row * C + c0), b1 = *reinterpret_cast<const float4*>(shift + row * C + c0 + 4);
    const float sc[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w}, sh[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = gn_affine(f[j], sc[j], sh[j]);
      f[j] = silu ? silu_f(v) : v;
    }
    st8<T>(out + pix * C + c0, f);
  }
}

// ---------------------------------------------------------------------------------------------------------
// LayerNorm over C per pixel: one wave per pixel, C multiple of 8 (any: a lane strides over the row's 8-channel vectors)
// ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void layernorm_kernel(const T* __restrict__ x, long long P, int C, float eps,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        T* __restrict__ out) {
  const long long pix = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pix >= P) return;
  const int lane = threadIdx.x & 63;
  const int nv = C >> 3;
  float sum = 0.f;
  for (int v = lane; v < nv; v += 64) {
    float f[8];
    ld8<T>(x + pix * C + v * 8, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) sum += f[j];
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) sum += __shfl_xor(sum, off);
  const float mean = sum / (float)C;
  float var = 0.f;
  for (int v = lane; v < nv; v += 64) {
    float f[8];
    ld8<T>(x + pix * C + v * 8, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) var += (f[j] - mean) * (f[j] - mean);
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) var += __shfl_xor(var, off);
  const float rstd = rsqrtf(var / (float)C + eps);
  for (int v = lane; v < nv; v += 64) {
    float f[8];
    ld8<T>(x + pix * C + v * 8, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (f[j] - mean) * rstd * gamma[v * 8 + j] + beta[v * 8 + j];
    st8<T>(out + pix * C + v * 8, f);
  }
}

// ---------------------------------------------------------------------------------------------------------
// row softmax: fp32 scores -> T probabilities; one block per row
// ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ s, int n_valid, long long ld_s,
                                                           T* __restrict__ p, long long ld_p) {
  __shared__ float sh[4];
  const float* sr = s + (long long)blockIdx.x * ld_s;
  T* pr = p + (long long)blockIdx.x * ld_p;
  float mx = -3.0e38f;
  for (int i = threadIdx.x; i < n_valid; i += 256) mx = fmaxf(mx, sr[i]);
  mx = block_reduce(mx, true, sh);
  float sum = 0.f;
  for (int i = threadIdx.x; i < n_valid; i += 256) sum += __expf(sr[i] - mx);
  sum = block_reduce(sum, false, sh);
  const float inv = 1.0f / sum;
  for (int i = threadIdx.x; i < (int)ld_p; i += 256) pr[i] = (T)(i < n_valid ? __expf(sr[i] - mx) * inv : 0.f);
}

// ---------------------------------------------------------------------------------------------------------
// transpose of 2-byte elements, 32x32 LDS tiles
// ---------------------------------------------------------------------------------------------------------
template <typename E>  // E = uint16_t (fp16 / bf16 elements) or uint32_t (float)
__global__ __launch_bounds__(256) void transpose16_kernel(const E* __restrict__ in, int R, int C, long long ld_in,
                                                          long long bs_in, E* __restrict__ out, long long ld_out,
                                                          long long bs_out) {
  __shared__ E t[32][33];
  const E* ib = in + (long long)blockIdx.z * bs_in;
  E* ob = out + (long long)blockIdx.z * bs_out;
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = r0 + ty + k * 8, c = c0 + tx;
    t[ty + k * 8][tx] = (r < R && c < C) ? ib[(long long)r * ld_in + c] : (E)0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = c0 + ty + k * 8, r = r0 + tx;
    if (c < C && r < R) ob[(long long)c * ld_out + r] = t[tx][ty + k * 8];
  }
}

// ---------------------------------------------------------------------------------------------------------
// temporal attention over T <= 8 frames per pixel, directly on NDHWC: token (b, t, s) lives at
// ((b*T + t)*S + s)*C.  One wave per pixel (b, s).
// ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void temporal_attn_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                            const T* __restrict__ v, long long P, int Tn, long long S,
                                                            int C, float scale, T* __restrict__ out) {
  const long long pix = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);  // over B*S
  if (pix >= P) return;
  const int lane = threadIdx.x & 63;
  const int nv = C >> 3;  // 16-byte vectors per token
  const long long b = pix / S, s = pix - b * S;
  const long long base = (b * Tn * S + s) * C;  // token 0 of this pixel
  const long long tstride = S * C;
  const T* qb = q + base;
  const T* kb = k + base;
  const T* vb = v + base;
  float sc[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) sc[i][j] = 0.f;
  for (int vv = lane; vv < nv; vv += 64) {
    float qf[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < Tn) ld8<T>(qb + i * tstride + vv * 8, qf[i]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j < Tn) {
        float kf[8];
        ld8<T>(kb + j * tstride + vv * 8, kf);
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (i < Tn) {
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) d += qf[i][e] * kf[e];
            sc[i][j] += d;
          }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float x = sc[i][j];
#pragma unroll
      for (int off = 32; off; off >>= 1) x += __shfl_xor(x, off);
      sc[i][j] = x * scale;
    }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
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
#pragma unroll
      for (int j = 0; j < 8; ++j) sc[i][j] = (j < Tn) ? sc[i][j] * inv : 0.f;
    }
  }
  for (int vv = lane; vv < nv; vv += 64) {
    float o[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int e = 0; e < 8; ++e) o[i][e] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j < Tn) {
        float vf[8];
        ld8<T>(vb + j * tstride + vv * 8, vf);
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (i < Tn) {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[i][e] += sc[i][j] * vf[e];
          }
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < Tn) st8<T>(out + base + i * tstride + vv * 8, o[i]);
  }
}

// General frame count (T' > 8: en_de_n_frames_a_time = None or > 28): one wave per (pixel, query frame), online softmax over
// the key frames, a lane owns up to 4 x 8 channels (C <= 2048).  Same arithmetic as above: fp32 scores / probabilities /
// accumulation, one rounding at the store.
template <typename T>
__global__ __launch_bounds__(256) void temporal_attn_general_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                                    const T* __restrict__ v, long long P, int Tn, long long S,
                                                                    int C, float scale, T* __restrict__ out) {
  const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);  // over B*S*Tn
  if (wid >= P * Tn) return;
  const int lane = threadIdx.x & 63;
  const int nv = C >> 3;
  const long long pix = wid / Tn;
  const int i = (int)(wid - pix * Tn);
  const long long b = pix / S, s = pix - b * S;
  const long long base = (b * Tn * S + s) * C;
  const long long tstride = S * C;
  float qf[4][8], o[4][8];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int vv = lane + u * 64;
#pragma unroll
    for (int e = 0; e < 8; ++e) { qf[u][e] = 0.f; o[u][e] = 0.f; }
    if (vv < nv) ld8<T>(q + base + i * tstride + vv * 8, qf[u]);
  }
  float mx = -3.0e38f, sum = 0.f;
  for (int j = 0; j < Tn; ++j) {
    float d = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int vv = lane + u * 64;
      if (vv < nv) {
        float kf[8];
        ld8<T>(k + base + j * tstride + vv * 8, kf);
#pragma unroll
        for (int e = 0; e < 8; ++e) d += qf[u][e] * kf[e];
      }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) d += __shfl_xor(d, off);
    d *= scale;
    const float nmx = fmaxf(mx, d);
    const float corr = __expf(mx - nmx), pj = __expf(d - nmx);
    sum = sum * corr + pj;
    mx = nmx;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int vv = lane + u * 64;
      if (vv < nv) {
        float vf[8];
        ld8<T>(v + base + j * tstride + vv * 8, vf);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[u][e] = o[u][e] * corr + pj * vf[e];
      }
    }
  }
  const float inv = 1.0f / sum;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int vv = lane + u * 64;
    if (vv < nv) {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[u][e] *= inv;
      st8<T>(out + base + i * tstride + vv * 8, o[u]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// layout at the boundary
// ---------------------------------------------------------------------------------------------------------
template <typename TS, typename TD>
__global__ __launch_bounds__(256) void ncdhw_to_ndhwc_kernel(const TS* __restrict__ in, int C, long long THW, int Cpad,
                                                             long long npix, TD* __restrict__ out) {
  const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;  // over B*T*H*W
  if (pix >= npix) return;
  const long long b = pix / THW, s = pix - b * THW;
  for (int c0 = 0; c0 < Cpad; c0 += 8) {
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + j;
      f[j] = (c < C) ? (float)in[(b * C + c) * THW + s] : 0.f;
    }
    st8<TD>(out + pix * Cpad + c0, f);
  }
}

// [B,C,T,H,W] -> row-packed [B,T,H,W+3,4] (include/cvvae.h, in_overlap): one thread per stored pixel (8 / 16 bytes)
template <typename TS, typename TD>
__global__ __launch_bounds__(256) void ncdhw_to_rowpack_kernel(const TS* __restrict__ in, int C, long long THW, int W, int replicate,
                                                               long long npix_out, TD* __restrict__ out) {
  const long long op = (long long)blockIdx.x * 256 + threadIdx.x;  // over B*T*H*(W+3)
  if (op >= npix_out) return;
  const int Wp = W + 3;
  const long long row = op / Wp;            // over B*T*H
  const int xp = (int)(op - row * Wp);
  int xs = xp - 1;
  bool zero = xp == W + 2;
  if (xs < 0 || xs >= W) {
    if (replicate) xs = xs < 0 ? 0 : W - 1;
    else zero = true;
  }
  const long long TH = THW / W;             // rows per batch item
  const long long b = row / TH, r = row - b * TH;
  TD v[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) v[c] = (TD)((c < C && !zero) ? (float)in[(b * C + c) * THW + r * W + xs] : 0.f);
#pragma unroll
  for (int c = 0; c < 4; ++c) out[op * 4 + c] = v[c];
}

template <typename T>
__global__ __launch_bounds__(256) void ndhwc_to_rowpack_kernel(const T* __restrict__ in, int C, long long ps, int W, int replicate,
                                                               long long npix_out, T* __restrict__ out) {
  const long long op = (long long)blockIdx.x * 256 + threadIdx.x;  // over B*T*H*(W+3)
  if (op >= npix_out) return;
  const int Wp = W + 3;
  const long long row = op / Wp;
  const int xp = (int)(op - row * Wp);
  int xs = xp - 1;
  bool zero = xp == W + 2;
  if (xs < 0 || xs >= W) {
    if (replicate) xs = xs < 0 ? 0 : W - 1;
    else zero = true;
  }
  const T* src = in + (row * W + xs) * ps;
#pragma unroll
  for (int c = 0; c < 4; ++c) out[op * 4 + c] = (c < C && !zero) ? src[c] : (T)0.f;
}

template <typename T>
__global__ __launch_bounds__(256) void ndhwc_to_ncdhw_kernel(const T* __restrict__ in, int C, long long THW, long long ps,
                                                             long long npix, T* __restrict__ out) {
  const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= npix) return;
  const long long b = pix / THW, s = pix - b * THW;
  for (int c = 0; c < C; ++c) out[(b * C + c) * THW + s] = in[pix * ps + c];
}

// ---------------------------------------------------------------------------------------------------------
// pixel pre/post-processing of the inference scripts, on the device (cvvae_inference_video.py:24-38, 47-50).
// The arithmetic is evaluated op by op in the storage dtype, as the script's half tensors do (fp32 op, one rounding each).
// ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void frames_u8_to_ndhwc_kernel(const uint8_t* __restrict__ f, long long npix, int Cpad,
                                                                 T* __restrict__ out) {
  const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= npix) return;
  float v[8];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const T h = (T)(float)f[pix * 3 + c];        // .half()
    const T d = (T)((float)h / 127.5f);          // / 127.5
    v[c] = (float)(T)((float)d - 1.0f);          // - 1.0
  }
#pragma unroll
  for (int c = 3; c < 8; ++c) v[c] = 0.f;
  st8<T>(out + pix * Cpad, v);
  const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int c0 = 8; c0 < Cpad; c0 += 8) st8<T>(out + pix * Cpad + c0, z);
}

template <typename T>
__global__ __launch_bounds__(256) void ncdhw_to_frames_u8_kernel(const T* __restrict__ in, long long thw, uint8_t* __restrict__ f) {
  const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= thw) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float x = (float)in[(long long)c * thw + pix];
    x = x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x);   // torch.clamp(results, -1.0, 1.0)
    const T a = (T)(x + 1.0f);                         // + 1.0
    const T m = (T)((float)a * 127.5f);                // * 127.5
    f[pix * 3 + c] = (uint8_t)(float)m;                // .to(torch.uint8): truncation
  }
}

// ---------------------------------------------------------------------------------------------------------
// one axis of the uint8 antialiased bilinear frame resize (include/cvvae.h cvvae_resize_u8_axis)
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void resize_u8_axis_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, long long n_out,
                                                             int in_size, int out_size, long long inner,
                                                             const int* __restrict__ xmin, const int* __restrict__ xsize,
                                                             const int* __restrict__ w, int ksize, int precision) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;  // over outer * out_size * inner
  if (e >= n_out) return;
  const long long r = e % inner, q = e / inner;
  const int i = (int)(q % out_size);
  const long long o = q / out_size;
  const uint8_t* src = in + (o * in_size + xmin[i]) * inner + r;
  const int* wi = w + (long long)i * ksize;
  int acc = 1 << (precision - 1);
  const int n = xsize[i];
  for (int j = 0; j < n; ++j) acc += wi[j] * (int)src[(long long)j * inner];
  acc >>= precision;
  out[e] = (uint8_t)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
}

// ---------------------------------------------------------------------------------------------------------
// the last layer's spatial taps, gathered from the (3,1,1) conv's per-input-pixel columns (include/cvvae.h cvvae_conv_out_gather)
// ---------------------------------------------------------------------------------------------------------
template <typename T, int CO>
__global__ __launch_bounds__(256) void conv_out_gather_kernel(const float* __restrict__ V, int T_, int H, int W, long long ldv,
                                                              const float* __restrict__ bias, int replicate, long long npix,
                                                              T* __restrict__ out, uint8_t* __restrict__ u8) {
  // XCD-aware block order: consecutive blocks run on different XCDs (8, round-robin), each with its own L2; neighbouring patches
  // share their halo records, so each XCD gets a CONTIGUOUS band of patches
  const long long nblk = gridDim.x, q8 = nblk / 8, bid = blockIdx.x;
  const long long lb = bid < q8 * 8 ? (bid % 8) * q8 + bid / 8 : bid;
  // A block is an 8 x 32 pixel patch.  The 10 x 34 records around it are staged ONCE into LDS with coalesced 16-byte loads (every
  // thread reading its nine neighbours' 12 bytes straight from memory touched nine 128-byte lines per pixel: 3.8 GB fetched for
  // a 0.57 GB V, 0.56 ms); the nine-neighbour sums then come from LDS.  Pixel pitch in LDS: 9*CO + 2 floats (odd: no bank conflicts
  // between the lanes of a row).  Halo pixels outside the frame are staged from the clamped coordinate (replicate padding) or as
  // zeros (zero padding), so the sum below needs no bounds logic.
  constexpr int PW = 34, PH = 10, NV = 9 * CO, PITCH = NV + 2;
  __shared__ float sv[PH * PW * PITCH];
  const int tiles_x = (W + 31) / 32, tiles_y = (H + 7) / 8;
  const int tx = (int)(lb % tiles_x);
  const long long r0 = lb / tiles_x;
  const int ty = (int)(r0 % tiles_y);
  const long long bt = r0 / tiles_y;  // b*T + t
  const int x0 = tx * 32 - 1, y0 = ty * 8 - 1;
  // stage: one thread per (pixel, 16-byte quarter-record): NV = 27 floats = 6.75 quarters -> 7 loads per pixel
  constexpr int QP = (NV + 3) / 4;
  for (int i = threadIdx.x; i < PH * PW * QP; i += 256) {
    const int q = i % QP, pp = i / QP;
    const int px = pp % PW, py = pp / PW;
    int ys = y0 + py, xs = x0 + px;
    const bool outside = ys < 0 || ys >= H || xs < 0 || xs >= W;
    ys = ys < 0 ? 0 : (ys >= H ? H - 1 : ys);
    xs = xs < 0 ? 0 : (xs >= W ? W - 1 : xs);
    float4 v = *reinterpret_cast<const float4*>(V + ((bt * H + ys) * W + xs) * ldv + q * 4);  // (ldv % 4 == 0: 16-byte aligned)
    if (outside && !replicate) v = make_float4(0.f, 0.f, 0.f, 0.f);
    float* d = sv + pp * PITCH + q * 4;
    d[0] = v.x;
    if (q * 4 + 1 < NV) d[1] = v.y;
    if (q * 4 + 2 < NV) d[2] = v.z;
    if (q * 4 + 3 < NV) d[3] = v.w;
  }
  __syncthreads();
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
  const int x = tx * 32 + lx, y = ty * 8 + ly;
  if (x >= W || y >= H) return;
  const long long pix = (bt * H + y) * W + x;
  (void)npix;
  float acc[CO];
#pragma unroll
  for (int c = 0; c < CO; ++c) acc[c] = bias[c];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const float* v = sv + ((ly + dy) * PW + (lx + dx)) * PITCH + (dy * 3 + dx) * CO;
#pragma unroll
      for (int c = 0; c < CO; ++c) acc[c] += v[c];
    }
  const long long thw = (long long)T_ * H * W;
  const long long b = bt / T_, s = pix - b * thw;
#pragma unroll
  for (int c = 0; c < CO; ++c) {
    const T q = (T)acc[c];  // the layer's output, rounded to the model dtype as the stored tensor would be
    if (u8) {
      float xf = (float)q;
      xf = xf < -1.0f ? -1.0f : (xf > 1.0f ? 1.0f : xf);   // torch.clamp(results, -1.0, 1.0)
      const T a = (T)(xf + 1.0f);                            // + 1.0
      const T m = (T)((float)a * 127.5f);                    // * 127.5
      u8[pix * CO + c] = (uint8_t)(float)m;                  // .to(torch.uint8): truncation   ('t h w c', B = 1)
    } else {
      out[(b * CO + c) * thw + s] = q;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// tile blending (in place on b): b[.., :o] = (1-w)*a[.., -o:] + w*b[.., :o], w = i/o in fp32
// ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void blend_kernel(const T* __restrict__ a, int Ha, int Wa, T* __restrict__ b, int Hb,
                                                    int Wb, long long rows, int o, int axis) {
  const long long per_row = axis == 0 ? (long long)o * Wb : (long long)Hb * o;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= rows * per_row) return;
  const long long r = gid / per_row, e = gid - r * per_row;
  int y, x, i;
  long long ai;
  if (axis == 0) {  // blend_v: first o rows of b with last o rows of a
    y = (int)(e / Wb);
    x = (int)(e - (long long)y * Wb);
    i = y;
    ai = (r * Ha + (Ha - o + y)) * (long long)Wa + x;
  } else {          // blend_h: first o columns of b with last o columns of a
    y = (int)(e / o);
    x = (int)(e - (long long)y * o);
    i = x;
    ai = (r * Ha + y) * (long long)Wa + (Wa - o + x);
  }
  const long long bi = (r * Hb + y) * (long long)Wb + x;
  const float w = (float)i / (float)o;
  b[bi] = (T)((1.0f - w) * (float)a[ai] + w * (float)b[bi]);
}

}  // namespace cvvae

using namespace cvvae;

extern "C" {

static int gn_nsplit(int64_t S) {
  int64_t n = (S + 8191) / 8192;  // >= 8192 pixels per block; <= 512 slabs keeps the finalize merge short
  if (n < 1) n = 1;
  if (n > 512) n = 512;
  return (int)n;
}

size_t cvvae_gn_workspace_bytes(int32_t rows, int32_t groups, int64_t S) {
  return (size_t)rows * (size_t)gn_nsplit(S) * (size_t)groups * 3 * sizeof(float);
}

int cvvae_gn_stats(int32_t dtype, const void* x, int32_t rows, int64_t S, int32_t C, int64_t pix_stride, int32_t groups,
                   float eps, const float* gamma, const float* beta, float* scale, float* shift, void* workspace,
                   void* stream) {
  if (!x || !gamma || !beta || !scale || !shift || !workspace || rows <= 0 || S <= 0) return CVVAE_EINVAL;
  if (groups <= 0 || groups > 32 || C % groups || (C / groups) % 2 || C % 8 || C > 2048 || pix_stride % 8) return CVVAE_EUNSUPPORTED;
  const int nsplit = gn_nsplit(S);
  hipStream_t s = (hipStream_t)stream;
  const bool quads = (C / groups) % 4 == 0;  // else pairs: groups of 2 or 6 channels
  const bool ok = by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (quads)
      hipLaunchKernelGGL((gn_partial_kernel<T, 4>), dim3(nsplit, rows), dim3(256), 0, s, (const T*)x, (long long)S, C,
                         (long long)pix_stride, groups, nsplit, (float*)workspace);
    else
      hipLaunchKernelGGL((gn_partial_kernel<T, 2>), dim3(nsplit, rows), dim3(256), 0, s, (const T*)x, (long long)S, C,
                         (long long)pix_stride, groups, nsplit, (float*)workspace);
  });
  if (!ok) return CVVAE_EINVAL;
  hipLaunchKernelGGL(gn_finalize_kernel, dim3(rows), dim3(256), 0, s, (const float*)workspace, nsplit, groups, C, eps, gamma,
                     beta, scale, shift);
  return launch_status();
}

int cvvae_gn_silu_apply(int32_t dtype, const void* x, int32_t rows, int64_t S, int32_t C, int64_t pix_stride,
                        const float* scale, const float* shift, int32_t silu, void* out, void* stream) {
  if (!x || !scale || !shift || !out || rows <= 0 || S <= 0 || C <= 0 || C % 8 || pix_stride < C || pix_stride % 8) return CVVAE_EINVAL;
  const long long nvec = (long long)rows * S * (C / 8);
  long long blocks = (nvec + 255) / 256;
  if (blocks > 256LL * 64) blocks = 256LL * 64;  // grid-stride beyond 64 blocks per CU
  hipStream_t s = (hipStream_t)stream;
  const bool ok = by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(gn_silu_apply_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, s, (const T*)x, (long long)S, C,
                       (long long)pix_stride, scale, shift, silu, (T*)out, nvec);
  });
  if (!ok) return CVVAE_EINVAL;
  return launch_status();
}

int cvvae_gn_finalize(const float* partials, int32_t rows, int64_t slabs, int32_t C, int32_t groups, float eps,
                      const float* gamma, const float* beta, float* scale, float* shift, void* stream) {
  return cvvae_gn_finalize_frames(partials, rows, 1, slabs, C, groups, eps, gamma, beta, scale, shift, stream);
}

int cvvae_gn_finalize_frames(const float* partials, int32_t rows, int32_t frames, int64_t slabs, int32_t C, int32_t groups, float eps,
                             const float* gamma, const float* beta, float* scale, float* shift, void* stream) {
  if (!partials || !gamma || !beta || !scale || !shift || rows <= 0 || frames <= 0 || slabs <= 0 || slabs % frames || groups <= 0 ||
      C <= 0 || C % groups)
    return CVVAE_EINVAL;
  hipLaunchKernelGGL(gn_finalize_slabs_kernel, dim3(groups, rows * frames), dim3(256), 0, (hipStream_t)stream, partials,
                     (long long)slabs, groups, C, eps, gamma, beta, scale, shift, frames);
  return launch_status();
}

int cvvae_layernorm(int32_t dtype, const void* x, int64_t P, int32_t C, float eps, const float* gamma, const float* beta,
                    void* out, void* stream) {
  if (!x || !out || !gamma || !beta || P <= 0 || C <= 0 || C % 8) return CVVAE_EINVAL;
  const int grid = (int)((P + 3) / 4);
  hipStream_t s = (hipStream_t)stream;
  const bool ok = by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(layernorm_kernel<T>, dim3(grid), dim3(256), 0, s, (const T*)x, (long long)P, C, eps, gamma, beta, (T*)out);
  });
  if (!ok) return CVVAE_EINVAL;
  return launch_status();
}

int cvvae_softmax_rows(int32_t dtype, const float* sc, int64_t rows, int32_t n_valid, int64_t ld_s, void* p, int64_t ld_p,
                       void* stream) {
  if (!sc || !p || rows <= 0 || n_valid <= 0 || ld_s < n_valid || ld_p < n_valid) return CVVAE_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const bool ok = by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(softmax_rows_kernel<T>, dim3((unsigned)rows), dim3(256), 0, s, sc, n_valid, (long long)ld_s, (T*)p, (long long)ld_p);
  });
  if (!ok) return CVVAE_EINVAL;
  return launch_status();
}

int cvvae_transpose(int32_t dtype, const void* in, int32_t batch, int32_t R, int32_t C, int64_t ld_in, int64_t bs_in,
                    void* out, int64_t ld_out, int64_t bs_out, void* stream) {
  if (!in || !out || batch <= 0 || R <= 0 || C <= 0) return CVVAE_EINVAL;
  if (dtype == CVVAE_F32)
    hipLaunchKernelGGL(transpose16_kernel<uint32_t>, dim3((C + 31) / 32, (R + 31) / 32, batch), dim3(256), 0, (hipStream_t)stream,
                       (const uint32_t*)in, R, C, (long long)ld_in, (long long)bs_in, (uint32_t*)out, (long long)ld_out,
                       (long long)bs_out);
  else if (dtype == CVVAE_BF16 || dtype == CVVAE_F16)
    hipLaunchKernelGGL(transpose16_kernel<uint16_t>, dim3((C + 31) / 32, (R + 31) / 32, batch), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t*)in, R, C, (long long)ld_in, (long long)bs_in, (uint16_t*)out, (long long)ld_out,
                       (long long)bs_out);
  else
    return CVVAE_EINVAL;
  return launch_status();
}

int cvvae_temporal_attention(int32_t dtype, const void* q, const void* k, const void* v, int32_t B, int32_t T, int64_t S,
                             int32_t C, void* out, void* stream) {
  if (!q || !k || !v || !out || B <= 0 || S <= 0 || T <= 0 || C <= 0 || C % 8) return CVVAE_EINVAL;
  const float scale = 1.0f / sqrtf((float)C);
  const long long P = (long long)B * S;
  hipStream_t s = (hipStream_t)stream;
  if (T > 8) {  // general frame count: one wave per (pixel, query frame)
    if (C > 2048 || P * T >= (1LL << 33)) return CVVAE_EUNSUPPORTED;
    const int gridg = (int)((P * T + 3) / 4);
    const bool ok = by_dtype(dtype, [&](auto tag) {
      using E = typename decltype(tag)::type;  // (T is the frame count here)
      hipLaunchKernelGGL(temporal_attn_general_kernel<E>, dim3(gridg), dim3(256), 0, s, (const E*)q, (const E*)k, (const E*)v, P, T,
                         (long long)S, C, scale, (E*)out);
    });
    if (!ok) return CVVAE_EINVAL;
    return launch_status();
  }
  const int grid = (int)((P + 3) / 4);
  const bool ok = by_dtype(dtype, [&](auto tag) {
    using E = typename decltype(tag)::type;
    hipLaunchKernelGGL(temporal_attn_kernel<E>, dim3(grid), dim3(256), 0, s, (const E*)q, (const E*)k, (const E*)v, P, T, (long long)S,
                       C, scale, (E*)out);
  });
  if (!ok) return CVVAE_EINVAL;
  return launch_status();
}

int cvvae_ncdhw_to_ndhwc(int32_t src_dtype, int32_t dst_dtype, const void* in, int32_t B, int32_t C, int32_t T, int32_t H,
                         int32_t W, int32_t Cpad, void* out, void* stream) {
  if (!in || !out || B <= 0 || C <= 0 || T <= 0 || H <= 0 || W <= 0 || Cpad < C || Cpad % 8) return CVVAE_EINVAL;
  const long long THW = (long long)T * H * W, npix = THW * B;
  const int grid = (int)((npix + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  bool ok = false;
  by_dtype(dst_dtype, [&](auto td) {
    ok = by_dtype(src_dtype, [&](auto ts) {
      using TS = typename decltype(ts)::type;
      using TD = typename decltype(td)::type;
      hipLaunchKernelGGL((ncdhw_to_ndhwc_kernel<TS, TD>), dim3(grid), dim3(256), 0, s, (const TS*)in, C, THW, Cpad, npix, (TD*)out);
    });
  });
  if (!ok) return CVVAE_EINVAL;
  return launch_status();
}

int cvvae_ncdhw_to_rowpack(int32_t src_dtype, int32_t dst_dtype, const void* in, int32_t B, int32_t C, int32_t T, int32_t H,
                           int32_t W, int32_t pad_mode_w, void* out, void* stream) {
  if (!in || !out || B <= 0 || C <= 0 || C > 4 || T <= 0 || H <= 0 || W <= 0 || (pad_mode_w != 0 && pad_mode_w != 1)) return CVVAE_EINVAL;
  const long long THW = (long long)T * H * W, npo = (long long)B * T * H * (W + 3);
  const int grid = (int)((npo + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  // the 16 read-ahead elements behind the last pixel are zeroed (they are only ever multiplied by zero weights)
  const size_t es = dst_dtype == CVVAE_F32 ? 4 : 2;
  hipError_t me = hipMemsetAsync((char*)out + (size_t)npo * 4 * es, 0, 16 * es, s);
  if (me != hipSuccess) return (int)me;
  bool src_ok = false;
  const bool dst_ok = by_dtype16(dst_dtype, [&](auto td) {
    src_ok = by_dtype(src_dtype, [&](auto ts) {
      using TS = typename decltype(ts)::type;
      using TD = typename decltype(td)::type;
      hipLaunchKernelGGL((ncdhw_to_rowpack_kernel<TS, TD>), dim3(grid), dim3(256), 0, s, (const TS*)in, C, THW, W, pad_mode_w, npo,
                         (TD*)out);
    });
  });
  if (!dst_ok) return CVVAE_EUNSUPPORTED;  // (fp32 models keep the channel-padded first layer: no split-precision (3,3,1) instance)
  if (!src_ok) return CVVAE_EINVAL;
  return launch_status();
}

int cvvae_ndhwc_to_rowpack(int32_t dtype, const void* in, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W, int64_t pix_stride,
                           int32_t pad_mode_w, void* out, void* stream) {
  if (!in || !out || B <= 0 || C <= 0 || C > 4 || T <= 0 || H <= 0 || W <= 0 || pix_stride < C || (pad_mode_w != 0 && pad_mode_w != 1))
    return CVVAE_EINVAL;
  if (dtype != CVVAE_F16 && dtype != CVVAE_BF16) return CVVAE_EUNSUPPORTED;
  const long long npo = (long long)B * T * H * (W + 3);
  const int grid = (int)((npo + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  hipError_t me = hipMemsetAsync((char*)out + (size_t)npo * 4 * 2, 0, 16 * 2, s);
  if (me != hipSuccess) return (int)me;
  by_dtype16(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(ndhwc_to_rowpack_kernel<T>, dim3(grid), dim3(256), 0, s, (const T*)in, C, (long long)pix_stride, W, pad_mode_w,
                       npo, (T*)out);
  });
  return launch_status();
}

int cvvae_ndhwc_to_ncdhw(int32_t dtype, const void* in, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W,
                         int64_t pix_stride, void* out, void* stream) {
  if (!in || !out || B <= 0 || C <= 0 || T <= 0 || H <= 0 || W <= 0 || pix_stride < C) return CVVAE_EINVAL;
  const long long THW = (long long)T * H * W, npix = THW * B;
  const int grid = (int)((npix + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  const bool ok = by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(ndhwc_to_ncdhw_kernel<T>, dim3(grid), dim3(256), 0, s, (const T*)in, C, THW, (long long)pix_stride, npix, (T*)out);
  });
  if (!ok) return CVVAE_EINVAL;
  return launch_status();
}

int cvvae_frames_u8_to_ndhwc(int32_t dtype, const uint8_t* frames, int64_t npix, int32_t Cpad, void* out, void* stream) {
  if (!frames || !out || npix <= 0 || Cpad < 8 || Cpad % 8) return CVVAE_EINVAL;
  const int grid = (int)((npix + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  const bool ok = by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(frames_u8_to_ndhwc_kernel<T>, dim3(grid), dim3(256), 0, s, frames, (long long)npix, Cpad, (T*)out);
  });
  if (!ok) return CVVAE_EINVAL;
  return launch_status();
}

int cvvae_ncdhw_to_frames_u8(int32_t dtype, const void* in, int64_t thw, uint8_t* frames, void* stream) {
  if (!in || !frames || thw <= 0) return CVVAE_EINVAL;
  const int grid = (int)((thw + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  const bool ok = by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(ncdhw_to_frames_u8_kernel<T>, dim3(grid), dim3(256), 0, s, (const T*)in, (long long)thw, frames);
  });
  if (!ok) return CVVAE_EINVAL;
  return launch_status();
}

int cvvae_resize_u8_axis(const uint8_t* in, uint8_t* out, int64_t outer, int32_t in_size, int32_t out_size, int64_t inner,
                         const int32_t* xmin, const int32_t* xsize, const int32_t* w, int32_t ksize, int32_t precision, void* stream) {
  if (!in || !out || !xmin || !xsize || !w || outer <= 0 || in_size <= 0 || out_size <= 0 || inner <= 0 || ksize <= 0 || precision < 1 ||
      precision > 22)
    return CVVAE_EINVAL;
  const long long n = (long long)outer * out_size * inner;
  if (n >= (1LL << 31) * 256) return CVVAE_EUNSUPPORTED;
  hipLaunchKernelGGL(resize_u8_axis_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, out, n, in_size, out_size,
                     (long long)inner, xmin, xsize, w, ksize, precision);
  return launch_status();
}

int cvvae_conv_out_gather(int32_t dtype, const float* V, int32_t B, int32_t T, int32_t H, int32_t W, int32_t Cout, int64_t ldv,
                          const float* bias, int32_t pad_mode_hw, void* out_ncdhw, uint8_t* out_u8, void* stream) {
  if (!V || !bias || B <= 0 || T <= 0 || H <= 0 || W <= 0 || ldv < ((9LL * Cout + 3) & ~3LL) || (ldv & 3) || (pad_mode_hw != 0 && pad_mode_hw != 1))
    return CVVAE_EINVAL;
  if ((out_ncdhw != nullptr) == (out_u8 != nullptr)) return CVVAE_EINVAL;
  if (Cout != 3) return CVVAE_EUNSUPPORTED;  // the shipped decoders: RGB
  if (out_u8 && B != 1) return CVVAE_EINVAL;
  const long long npix = (long long)B * T * H * W;
  const long long nblk = (long long)B * T * ((H + 7) / 8) * ((W + 31) / 32);
  if (nblk >= (1LL << 31)) return CVVAE_EUNSUPPORTED;
  const int grid = (int)nblk;
  hipStream_t s = (hipStream_t)stream;
  const bool ok = by_dtype(dtype, [&](auto tag) {
    using E = typename decltype(tag)::type;
    hipLaunchKernelGGL((conv_out_gather_kernel<E, 3>), dim3(grid), dim3(256), 0, s, V, T, H, W, (long long)ldv, bias, pad_mode_hw,
                       npix, (E*)out_ncdhw, out_u8);
  });
  if (!ok) return CVVAE_EUNSUPPORTED;
  return launch_status();
}

int cvvae_blend(int32_t dtype, const void* a, int32_t Ha, int32_t Wa, void* b, int32_t Hb, int32_t Wb, int64_t rows,
                int32_t overlap, int32_t axis, void* stream) {
  if (!a || !b || rows <= 0 || overlap <= 0 || (axis != 0 && axis != 1)) return CVVAE_EINVAL;
  if (axis == 0 && (overlap > Ha || overlap > Hb || Wa != Wb)) return CVVAE_EINVAL;
  if (axis == 1 && (overlap > Wa || overlap > Wb || Ha != Hb)) return CVVAE_EINVAL;
  const long long n = rows * (axis == 0 ? (long long)overlap * Wb : (long long)Hb * overlap);
  const int grid = (int)((n + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  const bool ok = by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(blend_kernel<T>, dim3(grid), dim3(256), 0, s, (const T*)a, Ha, Wa, (T*)b, Hb, Wb, (long long)rows, overlap, axis);
  });
  if (!ok) return CVVAE_EINVAL;
  return launch_status();
}

int cvvae_abi_version(void) { return CVVAE_ABI_VERSION; }

}  // extern "C"
