// disc_kernels.hip -- the non-convolution passes of the 3-D PatchGAN discriminator (cvvae_amd/disc_ops.py) and their adjoints:
// ResnetBlockDown3D's downsample (first frame duplicated when T is odd, then avg_pool3d(2, 2)) and GroupNorm-apply + LeakyReLU
// (or the bare LeakyReLU).  gfx950 only.  All four are HBM- or latency-bound element-wise passes over NDHWC tensors: plain C++,
// fp32 arithmetic, one rounding to the storage dtype, no atomics.  The two *_stats forms (further down) are the same passes that also
// leave the GroupNorm records of the tensor they store; only they use LDS.
//
// Work split.  A lane owns one group of 8 consecutive channels (one 16-byte access for 16-bit types, two for fp32; C % 8 == 0 and
// 16-byte aligned tensors make every group aligned), consecutive lanes take consecutive groups, so a wavefront covers whole lines
// along C, then W.  The grid is capped and strides over the groups; group indices are 64-bit.  Every output element has exactly
// one writer (the adjoint of the pool is a gather), so the results do not depend on the grid: the same inputs give the same bits.
// In-place calls (y == x, gv == gy) are safe because a lane reads its own 8 elements before it writes them and nobody else's.
#include "pass_common.h"

namespace cvvae {
namespace disc {

constexpr int WG = 256;            // threads per workgroup
constexpr int VEC = 8;             // elements per lane and trip
constexpr int MAX_BLOCKS = 2048;   // 8 workgroups per CU; the rest of the tensor is reached by the grid stride

// This file keeps its own 8-element access instead of pass_common.h's ld8 / st8.  The two forms are the same casts in the same
// 16-byte accesses, but the compiler emits different code for the 16-bit kernels behind them, and with ld8 / st8 the records of
// gn_leaky_apply_stats_kernel<16-bit, bare> came out different in their last bits (the tensors themselves did not).
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
// one pooled 8-channel vector: the 8 inputs of output (b, to, oy, ox), summed pairwise in fp32 and scaled by 0.125.  Shared by the plain and
// the statistics kernel, so both round the same fp32 value.
template <typename T>
__device__ __forceinline__ void pool8(const T* __restrict__ x, long long b, int to, int oy, int ox, int c0, int Tn, int H, int W, int C,
                                      float (&r)[VEC]) {
  const int odd = Tn & 1;
  float s[2][VEC];  // one partial sum per padded frame: ((x00 + x01) + (x10 + x11))
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    const int p = 2 * to + dt;
    const int t = odd ? (p > 0 ? p - 1 : 0) : p;
    const T* row0 = x + ((((b * Tn + t) * H + 2 * oy) * W + 2 * ox) * (long long)C + c0);
    float a[VEC], c[VEC], d[VEC], e[VEC];
    load8<T>(row0, a);
    load8<T>(row0 + C, c);
    load8<T>(row0 + (long long)W * C, d);
    load8<T>(row0 + (long long)W * C + C, e);
#pragma unroll
    for (int j = 0; j < VEC; ++j) s[dt][j] = (a[j] + c[j]) + (d[j] + e[j]);
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) r[j] = (s[0][j] + s[1][j]) * 0.125f;
}

template <typename T>
__global__ __launch_bounds__(WG) void avgpool3d_down_kernel(const T* __restrict__ x, T* __restrict__ y, int Tn, int H, int W, int C,
                                                            int To, int Ho, int Wo, long long ngroups) {
  const int cv = C / VEC;
  for (long long g = (long long)blockIdx.x * WG + threadIdx.x; g < ngroups; g += (long long)gridDim.x * WG) {
    const Pos o = decode(g, cv, Ho, Wo);
    const long long b = o.frame / To;
    const int to = (int)(o.frame - b * To);
    float r[VEC];
    pool8<T>(x, b, to, o.y, o.x, o.c0, Tn, H, W, C, r);
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
template <bool AFFINE>
__device__ __forceinline__ void affine_leaky8(float (&f)[VEC], const float (&sc)[VEC], const float (&sh)[VEC], float slope) {
  if constexpr (AFFINE) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) f[j] = __builtin_fmaf(f[j], sc[j], sh[j]);
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) f[j] = f[j] > 0.f ? f[j] : slope * f[j];
}

template <typename T, bool AFFINE>
__global__ __launch_bounds__(WG) void gn_leaky_apply_kernel(const T* x, const float* __restrict__ scale, const float* __restrict__ shift,
                                                            T* y, long long per_row, int C, float slope, long long ngroups) {
  const int cv = C / VEC;
  for (long long g = (long long)blockIdx.x * WG + threadIdx.x; g < ngroups; g += (long long)gridDim.x * WG) {
    float f[VEC];
    load8<T>(x + g * VEC, f);
    float sc[VEC], sh[VEC];
    if constexpr (AFFINE) {
      const long long pix = g / cv;
      const long long tab = (pix / per_row) * C + (g - pix * cv) * VEC;
      load8<float>(scale + tab, sc);
      load8<float>(shift + tab, sh);
    }
    affine_leaky8<AFFINE>(f, sc, sh, slope);
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

// ---------------------------------------------------------------------------------------------------------
// The same two passes with the GroupNorm records of the tensor they STORE (cvvae_gn_leaky_apply_stats, cvvae_avgpool3d_down_stats):
// part[row][group][slab] = (n, mean, M2) of the rounded values, the format cvvae_gn_finalize merges.  Grid (slabs, rows): a workgroup
// owns one contiguous run of one row's pixels, so it never straddles two samples and writes exactly one record per group; no atomics.
// Thread tid = pixel lane * cv + channel vector (cv = C / 8, ppp = WG / cv pixel lanes; threads beyond cv * ppp idle), as in
// gn_partial_kernel: a thread keeps its channel vector for the whole run, hence its statistics slots and, for the affine form, its
// eight table entries.
//
// A lane's 8 channels are 8 / SUB statistics slots of SUB channels: SUB = 2 for groups of 2 or 6 channels (Normalize(64): the lane holds
// four groups), 4 for groups of 4, 12, ... (two), 8 when a group is whole lanes (one slot; a 16-channel group is two lanes).  All slots
// of a lane have seen the same number of pixels k, so one Chan / Welford step per pixel serves them all:  f = 1 / (k + 1),
// mean += (m - mean) f,  M2 += m2 + (m - mean)^2 SUB k f,  (m, m2) the exact two-pass statistics of the SUB new values.
// The slots meet in LDS; group g's thread merges them in a fixed order (pixel lane, then slot): the same inputs give the same bits.
// ---------------------------------------------------------------------------------------------------------
// the value the store leaves in memory
template <typename T>
__device__ __forceinline__ void round8(float (&f)[VEC]) {
  if constexpr (sizeof(T) != 4) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) f[j] = (float)(T)f[j];
  }
}

template <int SUB>
struct LaneStats {
  static constexpr int NS = VEC / SUB;
  float mean[NS], m2[NS], k;
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int h = 0; h < NS; ++h) mean[h] = m2[h] = 0.f;
    k = 0.f;
  }
  __device__ __forceinline__ void add(const float (&f)[VEC]) {
    const float fk = 1.f / (k + 1.f), w = (float)SUB * k * fk;
#pragma unroll
    for (int h = 0; h < NS; ++h) {
      float sum = 0.f;
      if constexpr (SUB == 2) sum = f[h * 2] + f[h * 2 + 1];
      if constexpr (SUB == 4) sum = (f[h * 4] + f[h * 4 + 1]) + (f[h * 4 + 2] + f[h * 4 + 3]);
      if constexpr (SUB == 8) sum = ((f[0] + f[1]) + (f[2] + f[3])) + ((f[4] + f[5]) + (f[6] + f[7]));
      const float mb = sum * (1.0f / SUB);
      float m2b = 0.f;
#pragma unroll
      for (int j = 0; j < SUB; ++j) {
        const float d = f[h * SUB + j] - mb;
        m2b += d * d;
      }
      const float d = mb - mean[h];
      mean[h] += d * fk;
      m2[h] += m2b + d * d * w;
    }
    k += 1.f;
  }
};

// every thread of the workgroup calls this once, after its run: one record per group to rec[g * rec_stride]
template <int SUB>
__device__ __forceinline__ void write_group_records(const LaneStats<SUB>& st, int cv, int ppp, int G, int C, float* rec, long long rec_stride) {
  constexpr int NS = VEC / SUB;
  __shared__ WStat sh[WG * NS];
  const int tid = threadIdx.x;
#pragma unroll
  for (int h = 0; h < NS; ++h) sh[tid * NS + h] = {(float)SUB * st.k, st.mean[h], st.m2[h]};  // k = 0 (idle thread, empty run): merged as nothing
  __syncthreads();
  for (int g = tid; g < G; g += WG) {
    const int spg = C / G / SUB;  // slots per group
    WStat acc = {0.f, 0.f, 0.f};
    for (int pl = 0; pl < ppp; ++pl)
      for (int q = g * spg; q < (g + 1) * spg; ++q) chan_merge(acc, sh[(pl * cv + q / NS) * NS + q % NS]);
    float* o = rec + (long long)g * rec_stride;
    o[0] = acc.n;
    o[1] = acc.mean;
    o[2] = acc.m2;
  }
}

template <typename T, bool AFFINE, int SUB>
__global__ __launch_bounds__(WG) void gn_leaky_apply_stats_kernel(const T* x, const float* __restrict__ scale,
                                                                  const float* __restrict__ shift, T* y, long long per_row, int C,
                                                                  float slope, int G, float* __restrict__ part) {
  const int slabs = gridDim.x, slab = blockIdx.x, row = blockIdx.y;
  const int cv = C / VEC, ppp = WG / cv;
  const int myv = threadIdx.x % cv, mypl = threadIdx.x / cv;
  const long long per = (per_row + slabs - 1) / slabs, p0 = slab * per;
  const long long p1 = p0 + per < per_row ? p0 + per : per_row;
  LaneStats<SUB> st;
  st.init();
  if (mypl < ppp) {
    float sc[VEC], sh[VEC];
    if constexpr (AFFINE) {
      load8<float>(scale + (long long)row * C + myv * VEC, sc);
      load8<float>(shift + (long long)row * C + myv * VEC, sh);
    }
    const long long base = (long long)row * per_row * C + myv * VEC;
    for (long long px = p0 + mypl; px < p1; px += ppp) {
      float f[VEC];
      load8<T>(x + base + px * C, f);
      affine_leaky8<AFFINE>(f, sc, sh, slope);
      round8<T>(f);
      store8<T>(y + base + px * C, f);
      st.add(f);
    }
  }
  write_group_records<SUB>(st, cv, ppp, G, C, part + ((long long)row * G * slabs + slab) * 3, (long long)slabs * 3);
}

template <typename T, int SUB>
__global__ __launch_bounds__(WG) void avgpool3d_down_stats_kernel(const T* __restrict__ x, T* __restrict__ y, int Tn, int H, int W, int C,
                                                                  int To, int Ho, int Wo, int G, float* __restrict__ part) {
  const int slabs = gridDim.x, slab = blockIdx.x, row = blockIdx.y;
  const int cv = C / VEC, ppp = WG / cv;
  const int myv = threadIdx.x % cv, mypl = threadIdx.x / cv;
  const long long frame_pix = (long long)Ho * Wo, per_row = frame_pix * To;
  const long long per = (per_row + slabs - 1) / slabs, p0 = slab * per;
  const long long p1 = p0 + per < per_row ? p0 + per : per_row;
  LaneStats<SUB> st;
  st.init();
  if (mypl < ppp) {
    for (long long px = p0 + mypl; px < p1; px += ppp) {
      const int to = (int)(px / frame_pix);
      const unsigned r = (unsigned)(px - to * frame_pix);
      const int oy = (int)(r / (unsigned)Wo), ox = (int)(r - (unsigned)oy * (unsigned)Wo);
      float f[VEC];
      pool8<T>(x, row, to, oy, ox, myv * VEC, Tn, H, W, C, f);
      round8<T>(f);
      store8<T>(y + ((long long)row * per_row + px) * C + myv * VEC, f);
      st.add(f);
    }
  }
  write_group_records<SUB>(st, cv, ppp, G, C, part + ((long long)row * G * slabs + slab) * 3, (long long)slabs * 3);
}

// ---------------------------------------------------------------------------------------------------------
// Input gradient of a 3x3x3 conv with stride (2,2,2), zero padding 1 and Cin <= 8 (the discriminator's first layer, 3 -> 64), as a
// GATHER over the output gradient:  gx[b,t,h,w,ci] = sum over (kt,kh,kw), co of gy[b,ot,oh,ow,co] W[co,ci,kt,kh,kw],  ot = (t + 1 - kt) / 2
// where t + 1 - kt is even and 0 <= ot < To (oh, ow alike): an even coordinate has one live tap on its axis (k = 1), an odd one two
// (k = 0 and k = 2), so an input pixel reads 1 .. 8 output pixels.  No zero-stuffed tensor, no MFMA tile padded from 3 to 32 columns.
//
// Work split.  A WAVE owns 64 column pairs of one input row (b, t, h): lane j of the chunk computes pixels w = 2j and 2j + 1 from the
// output pixels ow = j (tap kw = 1 for the even pixel, kw = 2 for the odd one) and ow = j + 1 (kw = 0, odd pixel), so
//   * the live (kt, kh) taps are the same for the whole wave (t, h are wave-uniform): no divergence, and the weight reads are
//     same-address LDS broadcasts;
//   * a lane stores its two pixels side by side (2 x 8 channels: 32 contiguous bytes in 16-bit types), consecutive lanes consecutive
//     pairs: full lines;
//   * gy is read in 16-byte vectors along C; neighbouring lanes share ow = j + 1 through the vector cache.
// The weights sit in LDS as fp32 [27][Cout][CI], CI = 4 (Cin <= 4) or 8, staged once per workgroup from the caller's [27][Cout][8] table;
// the grid is capped and the waves stride over the row chunks, so the staging is amortised.  fp32 FMAs in a fixed order (kt, kh, then
// co ascending; per co the kw = 0 product before the kw = 2 one), one rounding at the store, every element one writer: the same inputs
// give the same bits.  Channels >= Cin of the 8-channel result are written as zero.  Row-chunk and element indices are 64-bit.
// ---------------------------------------------------------------------------------------------------------
constexpr int DG_WAVES = WG / 64;
constexpr int DG_MAX_BLOCKS = 1024;
constexpr int DG_MAX_LDS = 64 * 1024;

template <typename T, int CI>
__global__ __launch_bounds__(WG) void conv333_s2_dgrad_small_kernel(const T* __restrict__ gy, long long gy_stride,
                                                                    const float* __restrict__ wtab, T* __restrict__ gx, int Tn, int H,
                                                                    int W, int To, int Ho, int Wo, int Cout, int nchunk,
                                                                    long long nunits) {
  extern __shared__ __attribute__((aligned(16))) float dg_w[];  // [27][Cout][CI]
  for (int i = threadIdx.x; i < 27 * Cout * CI; i += WG) dg_w[i] = wtab[(long long)(i / CI) * VEC + (i % CI)];
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int npairs = (W + 1) >> 1;
  for (long long u = (long long)blockIdx.x * DG_WAVES + wave; u < nunits; u += (long long)gridDim.x * DG_WAVES) {
    const long long row = u / nchunk;                      // (b, t, h) flattened
    const int j = (int)(u - row * nchunk) * 64 + lane;     // column pair
    const long long bt = row / H;
    const int h = (int)(row - bt * H);
    const long long b = bt / Tn;
    const int t = (int)(bt - b * Tn);
    const bool has_a = j < npairs, has_b = j + 1 < Wo;     // (j < npairs implies j < Wo)
    float acc0[CI], acc1[CI];
#pragma unroll
    for (int c = 0; c < CI; ++c) acc0[c] = acc1[c] = 0.f;
    for (int kt = 0; kt < 3; ++kt) {
      const int nt = t + 1 - kt;
      if (nt < 0 || (nt & 1) || (nt >> 1) >= To) continue;
      for (int kh = 0; kh < 3; ++kh) {
        const int nh = h + 1 - kh;
        if (nh < 0 || (nh & 1) || (nh >> 1) >= Ho) continue;
        if (!has_a) continue;
        const T* pa = gy + ((((b * To + (nt >> 1)) * Ho + (nh >> 1)) * (long long)Wo + j) * gy_stride);
        const float* w0 = dg_w + (kt * 9 + kh * 3) * Cout * CI;  // taps kw = 0, 1, 2 follow each other
        const float* w1 = w0 + Cout * CI;
        const float* w2 = w1 + Cout * CI;
        for (int c8 = 0; c8 < Cout; c8 += VEC) {
          float a[VEC], bb[VEC];
          load8<T>(pa + c8, a);
          if (has_b) {
            load8<T>(pa + gy_stride + c8, bb);
          } else {
#pragma unroll
            for (int q = 0; q < VEC; ++q) bb[q] = 0.f;
          }
#pragma unroll
          for (int q = 0; q < VEC; ++q) {
            const int o = (c8 + q) * CI;
#pragma unroll
            for (int c = 0; c < CI; ++c) {
              acc0[c] = __builtin_fmaf(a[q], w1[o + c], acc0[c]);
              acc1[c] = __builtin_fmaf(bb[q], w0[o + c], acc1[c]);
              acc1[c] = __builtin_fmaf(a[q], w2[o + c], acc1[c]);
            }
          }
        }
      }
    }
    if (has_a) {
      float r[VEC];
#pragma unroll
      for (int c = 0; c < VEC; ++c) r[c] = c < CI ? acc0[c < CI ? c : 0] : 0.f;
      T* po = gx + ((row * W + 2 * (long long)j) * VEC);
      store8<T>(po, r);
      if (2 * j + 1 < W) {
#pragma unroll
        for (int c = 0; c < VEC; ++c) r[c] = c < CI ? acc1[c < CI ? c : 0] : 0.f;
        store8<T>(po + VEC, r);
      }
    }
  }
}

static inline int blocks_for(long long ngroups) {
  const long long b = (ngroups + WG - 1) / WG;
  return (int)(b < MAX_BLOCKS ? b : MAX_BLOCKS);
}

constexpr long long MAX_ELEMS = 1LL << 40;  // what the index arithmetic above holds with room to spare

// element count of the pool's INPUT [B][T][H][W][C], or -1 when a frame's pixels, the frame count or the total leave their range
static inline long long pool_elems(int64_t B, int32_t T, int32_t H, int32_t W, int32_t C) {
  if ((long long)H * W >= (1LL << 31) || B > ((1LL << 31) - 1) / T) return -1;
  const long long pix = (long long)B * T * ((long long)H * W);
  if (pix > MAX_ELEMS / C) return -1;
  return pix * C;
}

constexpr int MAX_STAT_C = WG * VEC;  // one thread per channel vector at least
constexpr int MAX_STAT_ROWS = 65535;  // gridDim.y

// 0, or why the statistics forms cannot take (rows, per_row, C, groups)
static inline int stats_args(int64_t rows, int64_t per_row, int32_t C, int32_t groups) {
  if (rows <= 0 || per_row <= 0 || C <= 0 || groups <= 0) return CVVAE_EINVAL;
  if (C % VEC || C > MAX_STAT_C || C % groups || (C / groups) % 2 || groups > WG || rows > MAX_STAT_ROWS) return CVVAE_EUNSUPPORTED;
  return 0;
}

// channels per statistics slot for groups of cpg channels (cpg even)
static inline int sub_for(int cpg) { return cpg % 8 == 0 ? 8 : cpg % 4 == 0 ? 4 : 2; }

}  // namespace disc
}  // namespace cvvae

using namespace cvvae;
using namespace cvvae::disc;

extern "C" {

int cvvae_avgpool3d_down(int32_t dtype, const void* x, void* y, int64_t B, int32_t T, int32_t H, int32_t W, int32_t C, void* stream) {
  if (!x || !y || B <= 0 || T <= 0 || H < 2 || W < 2 || C <= 0) return CVVAE_EINVAL;
  if (!known_dtype(dtype) || C % VEC) return CVVAE_EUNSUPPORTED;
  if (pool_elems(B, T, H, W, C) < 0) return CVVAE_EUNSUPPORTED;
  const int To = (T + (T & 1)) / 2, Ho = H / 2, Wo = W / 2;
  const long long ngroups = (long long)B * To * Ho * Wo * (C / VEC);
  by_dtype(dtype, [&](auto tag) {
    using TT = typename decltype(tag)::type;
    hipLaunchKernelGGL(avgpool3d_down_kernel<TT>, dim3(blocks_for(ngroups)), dim3(WG), 0, (hipStream_t)stream, (const TT*)x, (TT*)y, T, H,
                       W, C, To, Ho, Wo, ngroups);
  });
  return launch_status();
}

int cvvae_avgpool3d_down_bwd(int32_t dtype, const void* gy, void* gx, int64_t B, int32_t T, int32_t H, int32_t W, int32_t C,
                             void* stream) {
  if (!gy || !gx || B <= 0 || T <= 0 || H < 2 || W < 2 || C <= 0) return CVVAE_EINVAL;
  if (!known_dtype(dtype) || C % VEC) return CVVAE_EUNSUPPORTED;
  const long long total = pool_elems(B, T, H, W, C);
  if (total < 0) return CVVAE_EUNSUPPORTED;
  const int To = (T + (T & 1)) / 2, Ho = H / 2, Wo = W / 2;
  const long long ngroups = total / VEC;
  by_dtype(dtype, [&](auto tag) {
    using TT = typename decltype(tag)::type;
    hipLaunchKernelGGL(avgpool3d_down_bwd_kernel<TT>, dim3(blocks_for(ngroups)), dim3(WG), 0, (hipStream_t)stream, (const TT*)gy, (TT*)gx,
                       T, H, W, C, To, Ho, Wo, ngroups);
  });
  return launch_status();
}

int cvvae_gn_leaky_apply(int32_t dtype, const void* x, const float* scale, const float* shift, void* y, int64_t rows, int64_t per_row,
                         int32_t C, float slope, void* stream) {
  if (!x || !y || rows <= 0 || per_row <= 0 || C <= 0 || (scale == nullptr) != (shift == nullptr)) return CVVAE_EINVAL;
  if (!known_dtype(dtype) || C % VEC) return CVVAE_EUNSUPPORTED;
  if (rows > MAX_ELEMS / per_row || rows * per_row > MAX_ELEMS / C) return CVVAE_EUNSUPPORTED;
  const long long ngroups = (long long)rows * per_row * (C / VEC);
  by_dtype(dtype, [&](auto tag) {
    using TT = typename decltype(tag)::type;
    if (scale)
      hipLaunchKernelGGL((gn_leaky_apply_kernel<TT, true>), dim3(blocks_for(ngroups)), dim3(WG), 0, (hipStream_t)stream, (const TT*)x,
                         scale, shift, (TT*)y, (long long)per_row, C, slope, ngroups);
    else
      hipLaunchKernelGGL((gn_leaky_apply_kernel<TT, false>), dim3(blocks_for(ngroups)), dim3(WG), 0, (hipStream_t)stream, (const TT*)x,
                         scale, shift, (TT*)y, (long long)per_row, C, slope, ngroups);
  });
  return launch_status();
}

int cvvae_leaky_bwd(int32_t dtype, const void* y, const void* gy, void* gv, int64_t n_elems, float slope, void* stream) {
  if (!y || !gy || !gv || n_elems <= 0 || !(slope > 0.f)) return CVVAE_EINVAL;
  if (!known_dtype(dtype) || n_elems > MAX_ELEMS) return CVVAE_EUNSUPPORTED;
  const long long ngroups = ((long long)n_elems + VEC - 1) / VEC;
  by_dtype(dtype, [&](auto tag) {
    using TT = typename decltype(tag)::type;
    hipLaunchKernelGGL(leaky_bwd_kernel<TT>, dim3(blocks_for(ngroups)), dim3(WG), 0, (hipStream_t)stream, (const TT*)y, (const TT*)gy,
                       (TT*)gv, (long long)n_elems, slope);
  });
  return launch_status();
}

int64_t cvvae_pass_gn_slabs(int64_t rows, int64_t per_row, int32_t C, int32_t groups) {
  const int bad = stats_args(rows, per_row, C, groups);
  if (bad) return bad;
  // a workgroup's run: at least 16 trips of its WG / (C / 8) pixel lanes, and about MAX_BLOCKS workgroups in all at most
  const int64_t run = 16 * (WG / (C / VEC));
  const int64_t want = (per_row + run - 1) / run, cap = MAX_BLOCKS / rows > 0 ? MAX_BLOCKS / rows : 1;
  return want < cap ? want : cap;
}

#define DISC_BY_SUB(CALL, TT) \
  do { \
    if (sub == 8) { CALL(TT, 8); } else if (sub == 4) { CALL(TT, 4); } else { CALL(TT, 2); } \
  } while (0)

int cvvae_avgpool3d_down_stats(int32_t dtype, const void* x, void* y, int64_t B, int32_t T, int32_t H, int32_t W, int32_t C,
                               int32_t out_groups, float* out_partials, void* stream) {
  if (out_groups < 0) return CVVAE_EINVAL;
  if (out_groups == 0 || !out_partials) return cvvae_avgpool3d_down(dtype, x, y, B, T, H, W, C, stream);
  if (!x || !y || B <= 0 || T <= 0 || H < 2 || W < 2 || C <= 0) return CVVAE_EINVAL;
  if (!known_dtype(dtype) || C % VEC) return CVVAE_EUNSUPPORTED;
  if (pool_elems(B, T, H, W, C) < 0) return CVVAE_EUNSUPPORTED;
  const int To = (T + (T & 1)) / 2, Ho = H / 2, Wo = W / 2;
  const int64_t slabs = cvvae_pass_gn_slabs(B, (int64_t)To * Ho * Wo, C, out_groups);
  if (slabs <= 0) return (int)slabs;
  const int sub = sub_for(C / out_groups);
#define CALL_S(TT, SUB) \
  hipLaunchKernelGGL((avgpool3d_down_stats_kernel<TT, SUB>), dim3((unsigned)slabs, (unsigned)B), dim3(WG), 0, (hipStream_t)stream, \
                     (const TT*)x, (TT*)y, T, H, W, C, To, Ho, Wo, out_groups, out_partials)
  by_dtype(dtype, [&](auto tag) {
    using TT = typename decltype(tag)::type;
    DISC_BY_SUB(CALL_S, TT);
  });
#undef CALL_S
  return launch_status();
}

int cvvae_gn_leaky_apply_stats(int32_t dtype, const void* x, const float* scale, const float* shift, void* y, int64_t rows,
                               int64_t per_row, int32_t C, float slope, int32_t out_groups, float* out_partials, void* stream) {
  if (out_groups < 0) return CVVAE_EINVAL;
  if (out_groups == 0 || !out_partials) return cvvae_gn_leaky_apply(dtype, x, scale, shift, y, rows, per_row, C, slope, stream);
  if (!x || !y || rows <= 0 || per_row <= 0 || C <= 0 || (scale == nullptr) != (shift == nullptr)) return CVVAE_EINVAL;
  if (!known_dtype(dtype) || C % VEC) return CVVAE_EUNSUPPORTED;
  if (rows > MAX_ELEMS / per_row || rows * per_row > MAX_ELEMS / C) return CVVAE_EUNSUPPORTED;
  const int64_t slabs = cvvae_pass_gn_slabs(rows, per_row, C, out_groups);
  if (slabs <= 0) return (int)slabs;
  const int sub = sub_for(C / out_groups);
#define CALL_S(TT, SUB) \
  do { \
    if (scale) \
      hipLaunchKernelGGL((gn_leaky_apply_stats_kernel<TT, true, SUB>), dim3((unsigned)slabs, (unsigned)rows), dim3(WG), 0, \
                         (hipStream_t)stream, (const TT*)x, scale, shift, (TT*)y, (long long)per_row, C, slope, out_groups, out_partials); \
    else \
      hipLaunchKernelGGL((gn_leaky_apply_stats_kernel<TT, false, SUB>), dim3((unsigned)slabs, (unsigned)rows), dim3(WG), 0, \
                         (hipStream_t)stream, (const TT*)x, scale, shift, (TT*)y, (long long)per_row, C, slope, out_groups, out_partials); \
  } while (0)
  by_dtype(dtype, [&](auto tag) {
    using TT = typename decltype(tag)::type;
    DISC_BY_SUB(CALL_S, TT);
  });
#undef CALL_S
  return launch_status();
}

int cvvae_conv333_s2_dgrad_small(int32_t dtype, const void* gy, int64_t gy_pix_stride, const float* w_table, void* gx, int64_t B,
                                 int32_t T, int32_t H, int32_t W, int32_t To, int32_t Ho, int32_t Wo, int32_t Cin, int32_t Cout,
                                 void* stream) {
  if (!gy || !w_table || !gx || B <= 0 || T <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || gy_pix_stride <= 0) return CVVAE_EINVAL;
  // the forward's output extents, from the input's: floor((n + 2 - 3) / 2) + 1
  if (To != (T - 1) / 2 + 1 || Ho != (H - 1) / 2 + 1 || Wo != (W - 1) / 2 + 1) return CVVAE_EINVAL;
  if (!known_dtype(dtype) || Cin > VEC || Cout % VEC || gy_pix_stride % VEC || gy_pix_stride < Cout) return CVVAE_EUNSUPPORTED;
  if (((uintptr_t)gy | (uintptr_t)gx | (uintptr_t)w_table) & 15) return CVVAE_EUNSUPPORTED;
  const int ci = Cin <= 4 ? 4 : 8;
  const long long lds = 27LL * Cout * ci * (long long)sizeof(float);
  if (lds > DG_MAX_LDS) return CVVAE_EUNSUPPORTED;
  if (pool_elems(B, T, H, W, VEC) < 0 || (long long)B * To * Ho * Wo > MAX_ELEMS / gy_pix_stride) return CVVAE_EUNSUPPORTED;
  const int nchunk = (((W + 1) >> 1) + 63) / 64;
  const long long nunits = (long long)B * T * H * nchunk;
  const long long want = (nunits + DG_WAVES - 1) / DG_WAVES;
  const int blocks = (int)(want < DG_MAX_BLOCKS ? want : DG_MAX_BLOCKS);
#define CALL_C(TT, CC) \
  hipLaunchKernelGGL((conv333_s2_dgrad_small_kernel<TT, CC>), dim3(blocks), dim3(WG), (size_t)lds, (hipStream_t)stream, (const TT*)gy, \
                     (long long)gy_pix_stride, w_table, (TT*)gx, T, H, W, To, Ho, Wo, Cout, nchunk, nunits)
  by_dtype(dtype, [&](auto tag) {
    using TT = typename decltype(tag)::type;
    if (ci == 4) { CALL_C(TT, 4); } else { CALL_C(TT, 8); }
  });
#undef CALL_C
  return launch_status();
}

}  // extern "C"
