// pack_kernels.hip -- the writer of the packed weight format that conv_fwd_kernel reads (the format is private to the two):
//   dst[(((nb*nchunks + chunk)*dst_taps + dst_tap0 + tap)*R + r)*512 + lane*8 + j],  R records per tap (1; fp32 sources: 3)
//   = src(co = nb*32 + sigma(lane&31), ci = chunk*16 + (lane>>5)*8 + j, tap)           in the 16-bit form.
// One kernel, pack_kernel<Src, Wr>: a SOURCE answers "value of (co, ci, tap) as fp32" (a strided view with coinciding taps
// summed, or one phase of the upsample-folded 3x3x3 weight), a WRITER turns 16 channels of one tap into the records of the
// storage form (16-bit, split-precision fp32, fast fp32 with bf8 or e3m2 corrections).  gfx950 only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cvvae.h"
#include "conv_kernel.h"

namespace cvvae {

// MFMA row i of a 32-output-channel block carries output channel sigma(i) = i with bits 2 and 3 swapped: the accumulator
// quads 2p, 2p+1 of a lane are then 8 consecutive channels (conv_kernel.h, store tail).
__device__ __forceinline__ int sigma_row(int i) { return (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1); }

// ---- sources.  image(i) selects the i-th weight of a launch; at() is 0 outside [Cout) x [Cin) (the padding of the layout).
// Sums are fp32, from +0.0, in the order written here, and are rounded once by the writer.
template <typename T>
struct StridedSrc {  // element (co, ci, tap) at p[co*s_co + ci*s_ci + tap*s_tap], summed with its fold_n - 1 followers s_fold apart
  const T* p;
  int Cout, Cin, fold_n;
  long long s_co, s_ci, s_tap, s_fold, s_img;
  __device__ void image(int i) { p += (long long)i * s_img; }  // batch item
  __device__ float at(int co, int ci, int tap) const {
    if (co >= Cout || ci >= Cin) return 0.f;
    const T* e = p + (long long)co * s_co + (long long)ci * s_ci + (long long)tap * s_tap;
    if (sizeof(T) == 2 && fold_n <= 1) return (float)e[0];  // a 16-bit element that is not folded is COPIED: its -0.0 stays -0.0
    float a = 0.f;
    for (int f = 0; f < fold_n; ++f) a += (float)e[(long long)f * s_fold];
    return a;
  }
};

// Nearest-2x upsample folded into the conv weights (Upsample3D: F.interpolate(scale (1,2,2)) then a 3x3x3 conv,
// models/vae_blocks3d_sd3.py:342-356, models/vae_models.py:218-229).  Output row 2y+py reads upsampled rows 2y+py-1..2y+py+1
// = stored rows {y-1, y, y} (py = 0) or {y, y, y+1} (py = 1): two stored rows per phase, with the weights of the taps that
// coincide summed.  Same along x.  So phase (py, px) is a 3x2x2 convolution over the stored input with
//   a = 0: ky in {0}      (py = 0) | {0, 1} (py = 1);      a = 1: ky in {1, 2} (py = 0) | {2} (py = 1)
// (likewise b / kx / px); tap = (kt*2 + a)*2 + b.
// tfold: 0 = the three time taps kept (12 taps per phase); 1 = all three summed, 2 = centre tap only (single-frame inputs);
// 3 = taps {0,1} summed, 4 = taps {1,2} summed (the boundary-frame slots of cvvae_pack_weights_upfold_tfolds): 4 taps each
template <typename T>
struct UpfoldSrc {  // p: [Cout, Cin, 3, 3, 3] contiguous
  const T* p;
  int Cout, Cin, tfold, py, px;
  __device__ void image(int i) { py = i >> 1, px = i & 1; }  // phase
  __device__ float at(int co, int ci, int tap) const {
    const int kt = tap >> 2, a = (tap >> 1) & 1, b = tap & 1;
    const int kt_lo = tfold == 0 ? kt : (tfold == 1 || tfold == 3 ? 0 : 1), kt_hi = tfold == 0 ? kt : (tfold == 2 || tfold == 3 ? 1 : 2);
    const int y_lo = a == 0 ? 0 : (py == 0 ? 1 : 2), y_hi = a == 0 ? (py == 0 ? 0 : 1) : 2;
    const int x_lo = b == 0 ? 0 : (px == 0 ? 1 : 2), x_hi = b == 0 ? (px == 0 ? 0 : 1) : 2;
    float acc = 0.f;
    if (co < Cout && ci < Cin) {
      const T* w = p + ((long long)co * Cin + ci) * 27;
      for (int k = kt_lo; k <= kt_hi; ++k)
        for (int ky = y_lo; ky <= y_hi; ++ky)
          for (int kx = x_lo; kx <= x_hi; ++kx) acc += (float)w[k * 9 + ky * 3 + kx];
    }
    return acc;
  }
};

// ---- record writers
// Split-precision records (dtype CVVAE_F32: fp32 source, conv_fwd_kernel<..., XP>): THREE fp16 records per (k16, tap),
//   part 0: Wlo(c)  at k = c            (c = 0..15 of the sub-chunk)      x  B = hi(c)            -> Wlo.hi
//   part 1: Whi(c)  at k = c and c + 8  (c = 0..7)                        x  B = [hi(c) | lo(c)]  -> Whi.hi + Whi.lo
//   part 2: Whi(c)  at k = c-8 and c    (c = 8..15)                       x  B = [hi(c) | lo(c)]
// with Whi = fp16(w), Wlo = fp16(w - Whi); w = the (folded, fp32) source element.  The host pre-scales the weights by a power
// of two (ops.py) so that Wlo stays in fp16's normal range; the conv's alpha undoes it.
__device__ __forceinline__ void xp_store(_Float16* dst, long long rec3, int lane, const float (&w)[16]) {
  // w[0..15]: the 16 channels of the sub-chunk for my output row.  lane >> 5 selects k half of the MFMA A operand.
  const int kh = lane >> 5;
  f16x8 p0, p1, p2;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float a0 = w[kh * 8 + j];
    p0[j] = (_Float16)(a0 - (float)(_Float16)a0);  // Wlo of channel kh*8 + j
    p1[j] = (_Float16)w[j];                        // Whi of channel j      (both k halves)
    p2[j] = (_Float16)w[8 + j];                    // Whi of channel 8 + j  (both k halves)
  }
  *reinterpret_cast<f16x8*>(dst + (rec3 + 0) * 512 + lane * 8) = p0;
  *reinterpret_cast<f16x8*>(dst + (rec3 + 1) * 512 + lane * 8) = p1;
  *reinterpret_cast<f16x8*>(dst + (rec3 + 2) * 512 + lane * 8) = p2;
}

// Fast-fp32 records (dtype CVVAE_F32Q, conv_fwd_kernel<..., XP = 2>): the same three 1-KiB records per (k16, tap), holding
//   [0]: Whi(c) at k = c (c = 0..15)                                        x B = hi(c)  on the fp16 MFMA
//   [1], [2] (only at the FIRST tap of a pair; pairs = taps (0,1), (2,3), ... of every run of `run` taps): bytes 0-15 / 16-31 of
//            a lane's operand of the K = 64 bf8 MFMA: lanes 0-31 bf8(Whi(c)), lanes 32-63 bf8(Wlo(c)), c = 0..15, of tap a in
//            [1] and of tap b in [2] (zero when the run ends on tap a)     x B = [bf8(lo) | bf8(hi)] of taps a, b
__device__ __forceinline__ uint4 xq_half(int kh, const float (&w)[16]) {
  float v[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const float hi = (float)(_Float16)w[j];
    v[j] = kh ? w[j] - hi : hi;
  }
  float a[8], b[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a[j] = v[j];
    b[j] = v[8 + j];
  }
  const uint2 lo = pack8_bf8(a), hi = pack8_bf8(b);
  return make_uint4(lo.x, lo.y, hi.x, hi.y);
}
// e3m2 ("bf6": sign, 3 exponent bits of bias 3, 2 mantissa bits; normals 0.25 .. 28, subnormals k/16), round to nearest even,
// saturating -- the rounding of v_cvt_scalef32_pk32_bf6_f16 (tools/probes/fp6_probe.hip)
__device__ __forceinline__ unsigned enc_e3m2(float v) {
  const unsigned sgn = (__float_as_uint(v) >> 31) << 5;
  const float a = fminf(fabsf(v), 28.0f);
  if (!(a >= 0.25f)) return sgn | (unsigned)(int)rintf(a * 16.0f);  // subnormals (and 0.25 itself from below: code 4)
  int e;
  const float fr = frexpf(a, &e);  // a = fr * 2^e, fr in [0.5, 1)  ->  a = (2 fr) * 2^(e-1)
  int m = (int)rintf((2.0f * fr - 1.0f) * 4.0f), ex = e - 1;
  if (m == 4) {
    m = 0;
    ++ex;
  }
  return sgn | (unsigned)((ex + 3) << 2) | (unsigned)m;
}
// Fast-fp32 records with fp6 corrections (dtype CVVAE_F32Q6, conv_fwd_kernel<..., XP = 3>): [0] as above; [1], [2] = the 32 bytes of a
// lane's operand of the K = 64 bf6 MFMA: lanes 0-31 tap a, lanes 32-63 tap b of the pair (zero when the run ends on tap a), row =
// output channel; 32 six-bit codes, slot 16 i + 8 t + c = channel 8 i + c of term t:  t = 0: Whi (x the activation's lo * 2^11),
// t = 1: Wlo * 2^11 (x the activation's hi) -- both of the magnitude of the weight, so that ONE power of two per lane (2^sh, the
// largest with max |value| 2^sh <= 28) puts them into e3m2's range; bytes 0-23 = the codes, byte 24 = the lane's E8M0 block scale
// 127 - sh - 11 (it also undoes the 2^11 of either term).
__device__ __forceinline__ void xq6_lane(const float (&w)[16], uint4& q1, uint4& q2) {
  float v[32];
  float mx = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const float hi = (float)(_Float16)w[j];
    const int sl = 16 * (j >> 3) + (j & 7);
    v[sl] = hi;
    v[sl + 8] = (w[j] - hi) * 2048.0f;
    mx = fmaxf(mx, fmaxf(fabsf(v[sl]), fabsf(v[sl + 8])));
  }
  int sh = 0;
  if (mx > 0.f) {
    int e;
    (void)frexpf(28.0f / mx, &e);
    sh = e - 1;  // floor(log2(28 / mx))
    sh = sh < -100 ? -100 : (sh > 100 ? 100 : sh);
  }
  const float mul = ldexpf(1.0f, sh);
  unsigned d[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    const unsigned long long c = enc_e3m2(v[i] * mul);
    const int bit = 6 * i, dw = bit >> 5, o = bit & 31;
    d[dw] |= (unsigned)(c << o);
    if (o > 26) d[dw + 1] |= (unsigned)(c >> (32 - o));
  }
  q1 = make_uint4(d[0], d[1], d[2], d[3]);
  q2 = make_uint4(d[4], d[5], (unsigned)(127 - sh - 11), 0u);
}
__device__ __forceinline__ void xq_store(_Float16* dst, long long rec3, int lane, const float (&wa)[16], const float (&wb)[16],
                                         bool pair_start, bool has_b, bool q6) {
  const int kh = lane >> 5;
  f16x8 p0;
#pragma unroll
  for (int j = 0; j < 8; ++j) p0[j] = (_Float16)wa[kh * 8 + j];
  uint4 q1 = make_uint4(0, 0, 0, 0), q2 = make_uint4(0, 0, 0, 0);
  if (pair_start && q6) {
    if (kh == 0) xq6_lane(wa, q1, q2);
    else if (has_b) xq6_lane(wb, q1, q2);
    else q2 = make_uint4(0u, 0u, 127u, 0u);
  } else if (pair_start) {
    q1 = xq_half(kh, wa);
    if (has_b) q2 = xq_half(kh, wb);
  }
  *reinterpret_cast<f16x8*>(dst + (rec3 + 0) * 512 + lane * 8) = p0;
  *reinterpret_cast<uint4*>(dst + (rec3 + 1) * 512 + lane * 8) = q1;
  *reinterpret_cast<uint4*>(dst + (rec3 + 2) * 512 + lane * 8) = q2;
}

template <typename T>
struct Write16 {  // one record per tap: the lane's 8 channels, rounded once to T
  T* dst;
  template <class Src>
  __device__ void operator()(const Src& src, int co, int chunk, int tap, long long rec, int lane) const {
    typename Tr<T>::v8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (T)src.at(co, chunk * 16 + (lane >> 5) * 8 + j, tap);
    *reinterpret_cast<typename Tr<T>::v8*>(dst + rec * 512 + lane * 8) = v;
  }
};
struct Write32 {  // three records per tap from the 16 fp32 channels of the chunk
  _Float16* dst;
  int qrun;  // 0 = split-precision (three fp16 MFMAs) records; > 0 = fast-fp32 records with tap pairs inside runs of qrun taps
  bool q6;   // ... with e3m2 instead of bf8 corrections
  template <class Src>
  __device__ void operator()(const Src& src, int co, int chunk, int tap, long long rec, int lane) const {
    float w[16], wb[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j] = src.at(co, chunk * 16 + j, tap);
    if (qrun == 0) return xp_store(dst, rec * 3, lane, w);
    const int tr = tap % qrun;
    const bool start = (tr & 1) == 0, has_b = start && tr + 1 < qrun;
#pragma unroll
    for (int j = 0; j < 16; ++j) wb[j] = has_b ? src.at(co, chunk * 16 + j, tap + 1) : 0.f;
    xq_store(dst, rec * 3, lane, w, wb, start, has_b, q6);
  }
};

// One thread per (lane, tap, k16 chunk, 32-row block) of an image; grid.y = the images of the launch (batch items, or the four
// upsample phases).  This launch fills taps [dst_tap0, dst_tap0 + taps) of a layout with dst_taps taps per k16
// record group (the time-fold slots); a plain packer passes dst_taps = taps, dst_tap0 = 0.
struct PackGeom {
  int taps, nchunks, dst_taps, dst_tap0;
  long long nlanes, d_img;  // threads per image; 2-byte elements between the packed images
};
template <class Src, class Wr>
__global__ void pack_kernel(Src src, Wr wr, PackGeom g) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= g.nlanes) return;
  src.image(blockIdx.y);
  wr.dst += (long long)blockIdx.y * g.d_img;
  const int lane = (int)(gid & 63);
  long long f = gid >> 6;
  const int tap = (int)(f % g.taps);
  f /= g.taps;
  const int chunk = (int)(f % g.nchunks);  // k16 index
  const int nb = (int)(f / g.nchunks);
  const int co = nb * 32 + sigma_row(lane & 31);
  wr(src, co, chunk, tap, ((long long)nb * g.nchunks + chunk) * g.dst_taps + g.dst_tap0 + tap, lane);
}

}  // namespace cvvae

using namespace cvvae;

static bool f32_source(int32_t dtype) { return dtype == CVVAE_F32 || dtype == CVVAE_F32Q || dtype == CVVAE_F32Q6; }
static int records_per_tap(int32_t dtype) { return f32_source(dtype) ? 3 : 1; }

// pack_kernel over the source make(tag of the source's element type) and the writer of `dtype`; CVVAE_EINVAL for a dtype that has neither
template <class Make>
static int pack_launch(int32_t dtype, void* dst, int qrun, int images, const PackGeom& g, void* stream, Make make) {
  const dim3 grid((unsigned)((g.nlanes + 255) / 256), images);
  auto run = [&](auto sr, auto wr) {
    hipLaunchKernelGGL((pack_kernel<decltype(sr), decltype(wr)>), grid, dim3(256), 0, (hipStream_t)stream, sr, wr, g);
  };
  if (f32_source(dtype)) {  // three records per (k16, tap); one thread per record TRIPLE
    run(make(TypeTag<float>{}), Write32{(_Float16*)dst, qrun, dtype == CVVAE_F32Q6});
  } else if (!by_dtype16(dtype, [&](auto tag) {
               using T = typename decltype(tag)::type;
               run(make(tag), Write16<T>{(T*)dst});
             })) {
    return CVVAE_EINVAL;
  }
  return launch_status();
}

static int pack_impl(int32_t dtype, const void* src, int32_t batch, int64_t s_batch, int32_t Cout_src, int32_t Cin_src,
                     int32_t taps, int64_t s_co, int64_t s_ci, int64_t s_tap, int32_t fold_n, int64_t s_fold, int32_t Cin_pad,
                     int32_t kchunk, void* dst, int64_t d_batch_bytes, void* stream, int32_t dst_taps, int32_t dst_tap0) {
  if (!src || !dst || Cout_src <= 0 || Cin_src <= 0 || taps <= 0 || kchunk <= 0 || kchunk % 16 || Cin_pad % kchunk ||
      Cin_pad < Cin_src || fold_n < 1)
    return CVVAE_EINVAL;
  // the packed layout is the same for every kernel family: [Cout/32][Cin_pad/16][tap][64 lanes][8] (k16-major);
  // kchunk only states the granularity Cin_pad was rounded to (the K-chunk of the consuming kernel instance)
  const int nb = (Cout_src + 31) / 32, nchunks = Cin_pad / 16;
  // fast-fp32 pairs stay inside a run of kH*kW taps (the kernel walks 3-tap time kernels as time groups of kH*kW steps):
  // 27 / 54 (time-fold slots) / 9 -> runs of 9, 12 / 24 / 4 -> runs of 4 (the folded-upsample phases come through upfold_launch)
  int qrun = 0;
  if (dtype == CVVAE_F32Q || dtype == CVVAE_F32Q6) {
    qrun = taps % 9 == 0 ? 9 : (taps % 4 == 0 ? 4 : 0);
    if (!qrun || dst_taps % qrun || dst_tap0 % qrun) return CVVAE_EUNSUPPORTED;  // (1x1x1 weights: use CVVAE_F32)
  }
  const PackGeom g = {taps, nchunks, dst_taps, dst_tap0, (long long)nb * nchunks * taps * 64, (long long)(d_batch_bytes / 2)};
  return pack_launch(dtype, dst, qrun, batch, g, stream, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return StridedSrc<T>{(const T*)src, Cout_src, Cin_src, fold_n, s_co, s_ci, s_tap, s_fold, s_batch};
  });
}

static int upfold_launch(int32_t dtype, const void* src, int32_t Cout, int32_t Cin, int32_t Cin_pad, int32_t tfold, void* dst,
                         int32_t dst_taps, int32_t dst_tap0, void* stream) {
  const int nb = (Cout + 31) / 32, nchunks = Cin_pad / 16, ntap = tfold ? 4 : 12;
  // (runs of 4 taps = the 2x2 spatial taps of one time tap: pairs (0,1), (2,3))
  const int qrun = dtype == CVVAE_F32Q || dtype == CVVAE_F32Q6 ? 4 : 0;
  const PackGeom g = {ntap, nchunks, dst_taps, dst_tap0, (long long)nb * nchunks * ntap * 64,
                      (long long)(cvvae_packed_weight_bytes(Cout, Cin_pad, dst_taps * records_per_tap(dtype)) / 2)};
  return pack_launch(dtype, dst, qrun, 4, g, stream, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return UpfoldSrc<T>{(const T*)src, Cout, Cin, tfold, 0, 0};
  });
}

extern "C" {

size_t cvvae_packed_weight_bytes(int32_t Cout, int32_t Cin, int32_t taps) {
  const size_t co = (size_t)((Cout + 31) / 32) * 32;
  return co * (size_t)Cin * (size_t)taps * 2 + WEIGHT_TAIL_BYTES;  // + read-ahead tail for the prefetch ring
}

int cvvae_pack_weights_fold(int32_t dtype, const void* src, int32_t Cout_src, int32_t Cin_src, int32_t taps, int64_t s_co,
                            int64_t s_ci, int64_t s_tap, int32_t fold_n, int64_t s_fold, int32_t Cin_pad, int32_t kchunk,
                            void* dst, void* stream) {
  return pack_impl(dtype, src, 1, 0, Cout_src, Cin_src, taps, s_co, s_ci, s_tap, fold_n, s_fold, Cin_pad, kchunk, dst, 0, stream,
                   taps, 0);
}

int cvvae_pack_weights(int32_t dtype, const void* src, int32_t Cout_src, int32_t Cin_src, int32_t taps, int64_t s_co,
                       int64_t s_ci, int64_t s_tap, int32_t Cin_pad, int32_t kchunk, void* dst, void* stream) {
  return cvvae_pack_weights_fold(dtype, src, Cout_src, Cin_src, taps, s_co, s_ci, s_tap, 1, 0, Cin_pad, kchunk, dst, stream);
}

int cvvae_pack_weights_batched(int32_t dtype, const void* src, int32_t batch, int64_t s_batch, int32_t Cout_src,
                               int32_t Cin_src, int32_t taps, int64_t s_co, int64_t s_ci, int64_t s_tap, int32_t Cin_pad,
                               int32_t kchunk, void* dst, int64_t dst_batch_stride, void* stream) {
  if (dtype == CVVAE_F32Q || dtype == CVVAE_F32Q6) return CVVAE_EUNSUPPORTED;  // per-item (attention) weights are 1x1: they stay in the three-MFMA form
  if (batch <= 0 || dst_batch_stride % 16 ||
      (size_t)dst_batch_stride < cvvae_packed_weight_bytes(Cout_src, Cin_pad, taps * records_per_tap(dtype)))
    return CVVAE_EINVAL;
  return pack_impl(dtype, src, batch, s_batch, Cout_src, Cin_src, taps, s_co, s_ci, s_tap, 1, 0, Cin_pad, kchunk, dst,
                   dst_batch_stride, stream, taps, 0);
}

// Time-fold slots.  A 3-tap time kernel at a clip boundary reads the SAME stored frame through two or three of its taps
// (replicate padding: CausalConv3d front 2, Conv3d(padding_mode="replicate") 1+1 -- vae_blocks3d_sd3.py:16-104,
// vae_models.py:266-328): W0.x + W1.x = (W0+W1).x.  The packed buffer therefore carries, after the 3 original time slots
// (taps [0, 3*nsp)), the slots W0+W1, W1+W2 and W0+W1+W2 (fp32 sums, rounded once), nsp taps each: 6*nsp taps per record
// group.  conv_fwd_kernel picks, per output frame, the slots whose input frames are distinct (conv_kernel.h, "time folds").
int cvvae_pack_weights_tfolds(int32_t dtype, const void* src, int32_t Cout_src, int32_t Cin_src, int32_t nsp, int64_t s_co,
                              int64_t s_ci, int64_t s_tap, int32_t Cin_pad, int32_t kchunk, void* dst, void* stream) {
  if (nsp <= 0) return CVVAE_EINVAL;
  const int es = dtype >= CVVAE_F32 ? 4 : 2;  // bytes per source element
  const char* sp = (const char*)src;
  auto slot = [&](const void* from, int taps, int fold_n, int tap0) {
    return pack_impl(dtype, from, 1, 0, Cout_src, Cin_src, taps, s_co, s_ci, s_tap, fold_n, nsp * s_tap, Cin_pad, kchunk, dst, 0,
                     stream, 6 * nsp, tap0);
  };
  int rc = slot(src, 3 * nsp, 1, 0);
  if (!rc) rc = slot(sp, nsp, 2, 3 * nsp);
  if (!rc) rc = slot(sp + (long long)nsp * s_tap * es, nsp, 2, 4 * nsp);
  if (!rc) rc = slot(sp, nsp, 3, 5 * nsp);
  return rc;
}

// the four folded 3x2x2 phase kernels of cvvae_pack_weights_upfold with the time-fold slots appended: 24 taps per phase
int cvvae_pack_weights_upfold_tfolds(int32_t dtype, const void* src, int32_t Cout, int32_t Cin, int32_t Cin_pad, void* dst,
                                     void* stream) {
  if (!src || !dst || Cout <= 0 || Cin <= 0 || Cin_pad < Cin || Cin_pad % 16) return CVVAE_EINVAL;
  int rc = upfold_launch(dtype, src, Cout, Cin, Cin_pad, 0, dst, 24, 0, stream);
  if (!rc) rc = upfold_launch(dtype, src, Cout, Cin, Cin_pad, 3, dst, 24, 12, stream);
  if (!rc) rc = upfold_launch(dtype, src, Cout, Cin, Cin_pad, 4, dst, 24, 16, stream);
  if (!rc) rc = upfold_launch(dtype, src, Cout, Cin, Cin_pad, 1, dst, 24, 20, stream);
  return rc;
}

int cvvae_pack_weights_upfold(int32_t dtype, const void* src, int32_t Cout, int32_t Cin, int32_t Cin_pad, int32_t tfold,
                              void* dst, void* stream) {
  if (!src || !dst || Cout <= 0 || Cin <= 0 || Cin_pad < Cin || Cin_pad % 16 || tfold < 0 || tfold > 2) return CVVAE_EINVAL;
  return upfold_launch(dtype, src, Cout, Cin, Cin_pad, tfold, dst, tfold ? 4 : 12, 0, stream);
}

}  // extern "C"
