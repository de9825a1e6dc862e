// loss_kernels.hip -- the passes of the training loss around the networks (cvvae_amd/loss.py): a deterministic map-reduce to one
// fp32 scalar (pixel terms, KL, the GAN terms, the gradient norms of the adaptive weight) and its adjoint, over two operand
// sources -- a strided view, a contiguous run, or the frame-mapped clip of the constraint losses' "random" / "mean" 2-D targets --
// and the diagonal-Gaussian posterior (sample + KL) forward and backward.  gfx950 only.  All of them are HBM- or latency-bound:
// plain C++.  Every kernel numbers its elements by their LOGICAL index and visits them through walk(), which fixes the order of
// summation; a source only says where the value of a logical index lives, so the sum is a function of the logical values alone:
// the same inputs give the same bits on every run, and so do a strided view and its contiguous copy at any alignment, and a
// frame-mapped clip and its materialised target.
#include "pass_common.h"

namespace cvvae {
namespace loss {

constexpr int WG = 256;              // threads per workgroup
constexpr int VEC = 8;               // elements per group
constexpr int TILE = WG * VEC;       // elements per workgroup pass
constexpr int MAX_BLOCKS = 2048;     // stage-1 grid cap = stage-2's serial depth x 256
constexpr int MAX_BLOCKS_BWD = 65536;  // the adjoints' grid cap (nothing reads their grid back)

// Order of summation.  Elements are numbered by their logical index i (outer dimensions slowest, the inner run fastest).  Group
// g = elements [8g, 8g + 8) belongs to thread g % 256 of tile g / 256; workgroup w walks tiles w, w + grid, ...; the last group
// may hold n < 8 elements.  walk() calls f(i, n) for each group of the calling thread, in that order.  A reducing kernel adds a
// group's 8 terms first, in index order, and its groups serially; block_sum merges the 64 lanes of a wave by a butterfly and the
// four waves through LDS in wave order, and stage 2 (reduce_final_kernel, one workgroup) merges the per-workgroup partials the
// same way.  The grid is a function of the element count alone and nothing is atomic.  (The kernels' lambdas are always_inline:
// inlined together with walk, before any optimisation, they compile as the loop bodies they are; left to the inliner's own time
// the fp32 instantiations held up to 10 more VGPRs.)
template <typename F>
__device__ __forceinline__ void walk(long long total, F&& f) {
  const long long ntiles = (total + TILE - 1) / TILE;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long i = (t * WG + threadIdx.x) * VEC;
    if (i >= total) continue;
    f(i, (total - i) < VEC ? (int)(total - i) : VEC);
  }
}

// ---------------------------------------------------------------------------------------------------------
// Operand sources: load(i, n, f) puts the n (<= 8) values of logical indices [i, i + n) into f (the rest of f is zero or unused).
// A group is read with 16-byte loads when it lies inside one inner run and its address is 16-byte aligned, element by element
// otherwise (the head and tail of a run whose length or base is not a multiple of 8 elements).  GRAD: the operand can take the
// adjoint's gradient, contiguous over the logical index.
// ---------------------------------------------------------------------------------------------------------
// a contiguous run
template <typename T>
struct Run {
  using type = T;
  static constexpr bool GRAD = true;
  const T* p;
  __device__ __forceinline__ void load(long long i, int n, float (&f)[VEC]) const { ld8_n<T>(p + i, n, f); }
};

// up to three outer dimensions (slowest first) with one operand's element strides, and the inner run
struct View {
  long long n1, n2, L, s0, s1, s2;
  __device__ __forceinline__ long long offset(long long row, long long j) const {
    const long long i2 = row % n2, r = row / n2;
    return (r / n1) * s0 + (r % n1) * s1 + i2 * s2 + j;
  }
};

// a strided view; OPTIONAL: a null p is an absent operand, which reads as zeros
template <typename T, bool OPTIONAL = false>
struct Strided {
  using type = T;
  static constexpr bool GRAD = true;
  const T* p;
  View v;
  __device__ __forceinline__ void load(long long i, int n, float (&f)[VEC]) const {
    if (OPTIONAL && !p) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) f[k] = 0.f;
      return;
    }
    const long long row = i / v.L, j = i - row * v.L;
    if (n == VEC && j + VEC <= v.L) {
      ld8_n<T>(p + v.offset(row, j), VEC, f);
      return;
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      f[k] = 0.f;
      if (k < n) {
        const long long r = (i + k) / v.L;
        f[k] = (float)p[v.offset(r, (i + k) - r * v.L)];
      }
    }
  }
};

// a frame-mapped clip (cvvae_frame_map): the 2-D target of the constraint losses, rows x frames_out x HW, whose frame t' is a frame
// of the clip picked through a table (GATHER) or the mean of `group` consecutive frames (GROUP_MEAN) -- read from the clip in
// place.  The table travels in the kernel arguments (of the kernels over this source only).
struct FrameMap {
  int mode, group;
  long long frames_out, HW, row_stride, frame_stride;
  float inv_group;
  int index[CVVAE_FMAP_MAX_FRAMES];
};

template <typename T>
struct Frames {
  using type = T;
  static constexpr bool GRAD = false;
  const T* clip;
  FrameMap m;
  // the n (<= 8) target values at position j of frame tf of row r, which lie inside that frame's run
  __device__ __forceinline__ void run(long long r, long long tf, long long j, int n, float (&f)[VEC]) const {
    const T* base = clip + r * m.row_stride + j;
    if (m.mode == CVVAE_FMAP_GATHER) {
      ld8_n<T>(base + (long long)m.index[tf] * m.frame_stride, n, f);
      return;
    }
    if (tf == 0) {
      ld8_n<T>(base, n, f);
      return;
    }
    const long long s = 1 + (tf - 1) * m.group;
    ld8_n<T>(base + s * m.frame_stride, n, f);
    for (int q = 1; q < m.group; ++q) {
      float c[VEC];
      ld8_n<T>(base + (s + q) * m.frame_stride, n, c);
#pragma unroll
      for (int k = 0; k < VEC; ++k) f[k] += c[k];
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) f[k] = __fmul_rn(f[k], m.inv_group);  // (its own rounding: never contracted into the term's a - b)
  }
  __device__ __forceinline__ void load(long long i, int n, float (&f)[VEC]) const {
    const long long fr = i / m.HW, j = i - fr * m.HW;
    if (n == VEC && j + VEC <= m.HW) {
      const long long r = fr / m.frames_out;
      run(r, fr - r * m.frames_out, j, VEC, f);
      return;
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      f[k] = 0.f;
      if (k < n) {
        const long long fk = (i + k) / m.HW, r = fk / m.frames_out;
        float one[VEC];
        run(r, fk - r * m.frames_out, (i + k) - fk * m.HW, 1, one);
        f[k] = one[0];
      }
    }
  }
};

// aten::softplus (beta 1, threshold 20) and its derivative
__device__ __forceinline__ float softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float softplus_grad(float x) {
  if (x > 20.f) return 1.f;
  const float z = expf(x);
  return z / (z + 1.f);
}

__device__ __forceinline__ float term(int op, float a, float b) {
  switch (op) {
    case CVVAE_RED_ABS_DIFF: return fabsf(a - b);
    case CVVAE_RED_SQ_DIFF: { const float d = a - b; return d * d; }
    case CVVAE_RED_SQ: return a * a;
    case CVVAE_RED_IDENT: return a;
    case CVVAE_RED_HINGE_NEG: return fmaxf(1.f - a, 0.f);
    case CVVAE_RED_HINGE_POS: return fmaxf(1.f + a, 0.f);
    case CVVAE_RED_SOFTPLUS_NEG: return softplus(-a);
    default: return softplus(a);
  }
}

// d f_op / d a (two-operand ops: d / d b is its negative).  sign(0) = 0; the hinges' sub-gradient is relu's strict inequality
__device__ __forceinline__ float term_grad(int op, float a, float b) {
  switch (op) {
    case CVVAE_RED_ABS_DIFF: { const float d = a - b; return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }
    case CVVAE_RED_SQ_DIFF: return 2.f * (a - b);
    case CVVAE_RED_SQ: return 2.f * a;
    case CVVAE_RED_IDENT: return 1.f;
    case CVVAE_RED_HINGE_NEG: return (1.f - a) > 0.f ? -1.f : 0.f;
    case CVVAE_RED_HINGE_POS: return (1.f + a) > 0.f ? 1.f : 0.f;
    case CVVAE_RED_SOFTPLUS_NEG: return -softplus_grad(-a);
    default: return softplus_grad(a);
  }
}

// stage 1: ws[workgroup] = the workgroup's sum of f_op(a, b)
template <typename SA, typename SB>
__global__ __launch_bounds__(WG) void reduce_partial_kernel(int op, const SA a, const SB b, long long total, float* __restrict__ ws) {
  float acc = 0.f;
  walk(total, [&](long long i, int n) __attribute__((always_inline)) {
    float fa[VEC], fb[VEC];
    a.load(i, n, fa);
    b.load(i, n, fb);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < VEC; ++k) s += (k < n) ? term(op, fa[k], fb[k]) : 0.f;
    acc += s;
  });
  acc = block_sum(acc);
  if (threadIdx.x == 0) ws[blockIdx.x] = acc;
}

// stage 2: out = scale * (the nblk partials, thread t taking t, t + 256, ... serially, then the workgroup sum)
__global__ __launch_bounds__(WG) void reduce_final_kernel(const float* __restrict__ ws, int nblk, float scale, float* __restrict__ out) {
  float acc = 0.f;
  for (int i = threadIdx.x; i < nblk; i += WG) acc += ws[i];
  acc = block_sum(acc);
  if (threadIdx.x == 0) out[0] = scale * acc;
}

// adjoint: ga = coef f_op'(a, b) and gb = -ga, each where asked for (gb: where b's source can take one)
template <typename SA, typename SB>
__global__ __launch_bounds__(WG) void reduce_bwd_kernel(int op, const SA a, const SB b, long long total, const float* __restrict__ coef_dev,
                                                        typename SA::type* __restrict__ ga, typename SB::type* __restrict__ gb) {
  const float coef = coef_dev[0];
  walk(total, [&](long long i, int n) __attribute__((always_inline)) {
    float fa[VEC], fb[VEC], g[VEC];
    a.load(i, n, fa);
    b.load(i, n, fb);
#pragma unroll
    for (int k = 0; k < VEC; ++k) g[k] = coef * term_grad(op, fa[k], fb[k]);
    if (ga) st8_n<typename SA::type>(ga + i, g, n);
    if (SB::GRAD && gb) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) g[k] = -g[k];
      st8_n<typename SB::type>(gb + i, g, n);
    }
  });
}

// ---------------------------------------------------------------------------------------------------------
// DiagonalGaussianDistribution (lvdm/modules/distributions/distributions.py:24-52) in one pass: moments [B][2C][S] chunked at
// channel C into mean and logvar, logvar clamped to [-30, 20], z = mean + exp(0.5 logvar) * noise (noise NULL: z = mean), and the
// partial sums of mean^2 + var - 1 - logvar.  Rows are the B samples, the inner run the C * S values of one chunk.
// ---------------------------------------------------------------------------------------------------------
constexpr float LOGVAR_MIN = -30.f, LOGVAR_MAX = 20.f;

template <typename T>
__global__ __launch_bounds__(WG) void gauss_reg_kernel(const T* __restrict__ mom, const T* __restrict__ noise, T* __restrict__ z,
                                                       long long CS, long long total, float* __restrict__ ws) {
  const View vm{1, 1 << 30, CS, 0, 0, 2 * CS};  // row b of the mean chunk starts at b * 2CS (n2 only has to exceed B)
  const Strided<T> mean{mom, vm}, logvar{mom + CS, vm};
  float acc = 0.f;
  walk(total, [&](long long i, int n) __attribute__((always_inline)) {
    float m[VEC], lv[VEC], e[VEC], o[VEC];
    mean.load(i, n, m);
    logvar.load(i, n, lv);
    if (noise) Run<T>{noise}.load(i, n, e);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float l = fminf(fmaxf(lv[k], LOGVAR_MIN), LOGVAR_MAX);
      o[k] = noise ? __builtin_fmaf(expf(0.5f * l), e[k], m[k]) : m[k];
      s += (k < n) ? (m[k] * m[k] + expf(l) - 1.f - l) : 0.f;
    }
    st8_n<T>(z + i, o, n);
    acc += s;
  });
  acc = block_sum(acc);
  if (threadIdx.x == 0) ws[blockIdx.x] = acc;
}

// adjoint:  d mean = g_z + coef mean;  d logvar = (g_z noise 0.5 std + coef 0.5 (var - 1)) [-30 <= logvar_raw <= 20]
template <typename T>
__global__ __launch_bounds__(WG) void gauss_reg_bwd_kernel(const T* __restrict__ mom, const T* __restrict__ noise,
                                                           const T* __restrict__ gz, const float* __restrict__ coef_dev,
                                                           T* __restrict__ gmom, long long CS, long long total) {
  const float coef = coef_dev[0];
  const View vm{1, 1 << 30, CS, 0, 0, 2 * CS};
  const Strided<T> mean{mom, vm}, logvar{mom + CS, vm};
  walk(total, [&](long long i, int n) __attribute__((always_inline)) {
    float m[VEC], lv[VEC], e[VEC], g[VEC], dm[VEC], dl[VEC];
    mean.load(i, n, m);
    logvar.load(i, n, lv);
#pragma unroll
    for (int k = 0; k < VEC; ++k) e[k] = g[k] = 0.f;
    if (gz) {
      Run<T>{gz}.load(i, n, g);
      if (noise) Run<T>{noise}.load(i, n, e);
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const bool in = lv[k] >= LOGVAR_MIN && lv[k] <= LOGVAR_MAX;
      const float l = fminf(fmaxf(lv[k], LOGVAR_MIN), LOGVAR_MAX);
      dm[k] = __builtin_fmaf(coef, m[k], g[k]);
      dl[k] = in ? (g[k] * e[k] * 0.5f * expf(0.5f * l) + coef * 0.5f * (expf(l) - 1.f)) : 0.f;
    }
    // element i = (b, r) of a chunk lands at b * 2CS + r (mean) and b * 2CS + CS + r (logvar)
    const long long row = i / CS, r = i - row * CS;
    if (n == VEC && r + VEC <= CS) {
      st8_n<T>(gmom + row * 2 * CS + r, dm, VEC);
      st8_n<T>(gmom + row * 2 * CS + CS + r, dl, VEC);
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        if (k >= n) continue;
        const long long rw = (i + k) / CS, rr = (i + k) - rw * CS;
        gmom[rw * 2 * CS + rr] = (T)dm[k];
        gmom[rw * 2 * CS + CS + rr] = (T)dl[k];
      }
    }
  });
}

// ---- host side ----
static inline long long blocks_capped(long long total, long long cap) {
  const long long tiles = (total + TILE - 1) / TILE;
  return tiles < cap ? tiles : cap;
}
static inline int blocks_for(long long total) { return (int)blocks_capped(total, MAX_BLOCKS); }      // forward: stage 2 reads them
static inline int blocks_bwd(long long total) { return (int)blocks_capped(total, MAX_BLOCKS_BWD); }  // adjoints

// element count of a shape, or <= 0 when it is malformed / beyond what the index arithmetic holds
static inline long long shape_total(const cvvae_reduce_shape* s, bool two) {
  if (!s) return 0;
  long long total = 1;
  for (int d = 0; d < 3; ++d) {
    if (s->n[d] <= 0 || s->sa[d] < 0 || (two && s->sb[d] < 0)) return 0;
    if (s->n[d] > (1LL << 40) / total) return -1;
    total *= s->n[d];
  }
  if (s->L <= 0) return 0;
  if (s->L > (1LL << 40) / total) return -1;
  return total * s->L;
}
static inline int total_status(long long total) { return total == 0 ? CVVAE_EINVAL : (total < 0 ? CVVAE_EUNSUPPORTED : 0); }

// the two operands' views of a shape
struct Views {
  View a, b;
};
static inline Views shape_views(const cvvae_reduce_shape* s) {
  return {{s->n[1], s->n[2], s->L, s->sa[0], s->sa[1], s->sa[2]}, {s->n[1], s->n[2], s->L, s->sb[0], s->sb[1], s->sb[2]}};
}

static inline bool known_op(int32_t op) { return op >= CVVAE_RED_ABS_DIFF && op <= CVVAE_RED_SOFTPLUS_POS; }
static inline bool two_operands(int32_t op) { return op == CVVAE_RED_ABS_DIFF || op == CVVAE_RED_SQ_DIFF; }

// a frame map as the kernels take it -> 0 and the element count of the target, or the status to return (nothing was launched)
static inline int frame_map_args(const cvvae_frame_map* fm, FrameMap* m, long long* total) {
  if (!fm) return CVVAE_EINVAL;
  if (fm->mode != CVVAE_FMAP_GATHER && fm->mode != CVVAE_FMAP_GROUP_MEAN) return CVVAE_EINVAL;
  if (fm->rows <= 0 || fm->frames_in <= 0 || fm->frames_out <= 0 || fm->HW <= 0) return CVVAE_EINVAL;
  if (fm->frames_out > CVVAE_FMAP_MAX_FRAMES) return CVVAE_EUNSUPPORTED;
  // a stride of a dimension of extent 1 is never multiplied by anything but 0
  if (fm->frames_in > 1 && fm->frame_stride < fm->HW) return CVVAE_EINVAL;
  if (fm->HW > (1LL << 40) / fm->frames_in || fm->frame_stride > (1LL << 40) / fm->frames_in) return CVVAE_EUNSUPPORTED;
  if (fm->rows > 1 && fm->row_stride < (fm->frames_in - 1) * fm->frame_stride + fm->HW) return CVVAE_EINVAL;
  if (fm->rows > 1 && fm->row_stride > (1LL << 40) / fm->rows) return CVVAE_EUNSUPPORTED;
  if (fm->frames_out * fm->HW > (1LL << 40) / fm->rows) return CVVAE_EUNSUPPORTED;
  m->mode = fm->mode;
  m->group = 1;
  m->inv_group = 1.0f;
  if (fm->mode == CVVAE_FMAP_GATHER) {
    if (!fm->index) return CVVAE_EINVAL;
    for (long long t = 0; t < fm->frames_out; ++t) {
      if (fm->index[t] < 0 || fm->index[t] >= fm->frames_in) return CVVAE_EINVAL;
      m->index[t] = fm->index[t];
    }
  } else {
    if (fm->group < 1 || fm->frames_in != 1 + (fm->frames_out - 1) * (long long)fm->group) return CVVAE_EINVAL;
    m->group = fm->group;
    m->inv_group = 1.0f / (float)fm->group;
  }
  m->frames_out = fm->frames_out;
  m->HW = fm->HW;
  m->row_stride = fm->rows > 1 ? fm->row_stride : 0;
  m->frame_stride = fm->frames_in > 1 ? fm->frame_stride : 0;
  *total = fm->rows * fm->frames_out * fm->HW;
  return 0;
}

// the Gaussian passes' extents -> 0 and the chunk / element counts, or the status to return; `pointers`: none of them is NULL
static inline int gauss_args(bool pointers, int32_t dtype, int64_t B, int64_t C, int64_t S, long long* CS, long long* total) {
  if (!pointers || B <= 0 || C <= 0 || S <= 0) return CVVAE_EINVAL;
  if (!known_dtype(dtype)) return CVVAE_EUNSUPPORTED;
  if (B >= (1 << 30) || C > (1LL << 40) / S || C * S > (1LL << 40) / B) return CVVAE_EUNSUPPORTED;
  *CS = (long long)C * S;
  *total = *CS * B;
  return 0;
}

// f(TA tag, TB tag) for a pair of dtype codes
template <typename F>
static inline void by_dtypes(int32_t dtype_a, int32_t dtype_b, F&& f) {
  by_dtype(dtype_a, [&](auto ta) { by_dtype(dtype_b, [&](auto tb) { f(ta, tb); }); });
}

// stage 1 through partials(nblk, ws), then stage 2: out = scale * the sum
template <typename F>
static inline int reduce_to(long long total, void* workspace, float scale, float* out, hipStream_t s, F&& partials) {
  const int nblk = blocks_for(total);
  partials(nblk, (float*)workspace);
  hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(WG), 0, s, (const float*)workspace, nblk, scale, out);
  return launch_status();
}

}  // namespace loss
}  // namespace cvvae

using namespace cvvae;
using namespace cvvae::loss;

extern "C" {

size_t cvvae_reduce_workspace_bytes(const cvvae_reduce_shape* shape) {
  const long long total = shape_total(shape, false);
  if (total <= 0) return 0;
  return (size_t)blocks_for(total) * sizeof(float);
}

int cvvae_reduce_sum(int32_t op, int32_t dtype_a, const void* a, int32_t dtype_b, const void* b, const cvvae_reduce_shape* shape,
                     void* workspace, float* out, void* stream) {
  if (!a || !shape || !workspace || !out) return CVVAE_EINVAL;
  if (!known_op(op) || !known_dtype(dtype_a) || (b && !known_dtype(dtype_b))) return CVVAE_EUNSUPPORTED;
  const bool two = two_operands(op);
  if (two != (b != nullptr)) return CVVAE_EINVAL;
  const long long total = shape_total(shape, two);
  if (const int rc = total_status(total)) return rc;
  if (!b) dtype_b = CVVAE_F32;
  const Views v = shape_views(shape);
  hipStream_t s = (hipStream_t)stream;
  return reduce_to(total, workspace, 1.0f, out, s, [&](int nblk, float* ws) {
    by_dtypes(dtype_a, dtype_b, [&](auto ta, auto tb) {
      using TA = typename decltype(ta)::type;
      using TB = typename decltype(tb)::type;
      hipLaunchKernelGGL((reduce_partial_kernel<Strided<TA>, Strided<TB, true>>), dim3(nblk), dim3(WG), 0, s, op,
                         Strided<TA>{(const TA*)a, v.a}, Strided<TB, true>{(const TB*)b, v.b}, total, ws);
    });
  });
}

int cvvae_reduce_sum_bwd(int32_t op, int32_t dtype_a, const void* a, int32_t dtype_b, const void* b, const cvvae_reduce_shape* shape,
                         const float* coef_dev, void* ga, void* gb, void* stream) {
  if (!a || !shape || !coef_dev || (!ga && !gb)) return CVVAE_EINVAL;
  if (!known_op(op) || !known_dtype(dtype_a) || (b && !known_dtype(dtype_b))) return CVVAE_EUNSUPPORTED;
  const bool two = two_operands(op);
  if (two != (b != nullptr) || (gb && !two)) return CVVAE_EINVAL;
  const long long total = shape_total(shape, two);
  if (const int rc = total_status(total)) return rc;
  if (!b) dtype_b = CVVAE_F32;
  const Views v = shape_views(shape);
  by_dtypes(dtype_a, dtype_b, [&](auto ta, auto tb) {
    using TA = typename decltype(ta)::type;
    using TB = typename decltype(tb)::type;
    hipLaunchKernelGGL((reduce_bwd_kernel<Strided<TA>, Strided<TB, true>>), dim3(blocks_bwd(total)), dim3(WG), 0, (hipStream_t)stream, op,
                       Strided<TA>{(const TA*)a, v.a}, Strided<TB, true>{(const TB*)b, v.b}, total, coef_dev, (TA*)ga, (TB*)gb);
  });
  return launch_status();
}

size_t cvvae_reduce_frames_workspace_bytes(const cvvae_frame_map* map) {
  FrameMap m{};
  long long total = 0;
  if (frame_map_args(map, &m, &total) != 0) return 0;
  return (size_t)blocks_for(total) * sizeof(float);
}

int cvvae_reduce_sum_frames(int32_t op, int32_t dtype_a, const void* a, int32_t dtype_b, const void* clip, const cvvae_frame_map* map,
                            void* workspace, float* out, void* stream) {
  if (!a || !clip || !map || !workspace || !out) return CVVAE_EINVAL;
  if (!two_operands(op) || !known_dtype(dtype_a) || !known_dtype(dtype_b)) return CVVAE_EUNSUPPORTED;
  FrameMap m{};
  long long total = 0;
  if (const int rc = frame_map_args(map, &m, &total)) return rc;
  hipStream_t s = (hipStream_t)stream;
  return reduce_to(total, workspace, 1.0f, out, s, [&](int nblk, float* ws) {
    by_dtypes(dtype_a, dtype_b, [&](auto ta, auto tb) {
      using TA = typename decltype(ta)::type;
      using TB = typename decltype(tb)::type;
      hipLaunchKernelGGL((reduce_partial_kernel<Run<TA>, Frames<TB>>), dim3(nblk), dim3(WG), 0, s, op, Run<TA>{(const TA*)a},
                         Frames<TB>{(const TB*)clip, m}, total, ws);
    });
  });
}

int cvvae_reduce_sum_frames_bwd(int32_t op, int32_t dtype_a, const void* a, int32_t dtype_b, const void* clip, const cvvae_frame_map* map,
                                const float* coef_dev, void* ga, void* stream) {
  if (!a || !clip || !map || !coef_dev || !ga) return CVVAE_EINVAL;
  if (!two_operands(op) || !known_dtype(dtype_a) || !known_dtype(dtype_b)) return CVVAE_EUNSUPPORTED;
  FrameMap m{};
  long long total = 0;
  if (const int rc = frame_map_args(map, &m, &total)) return rc;
  by_dtypes(dtype_a, dtype_b, [&](auto ta, auto tb) {
    using TA = typename decltype(ta)::type;
    using TB = typename decltype(tb)::type;
    hipLaunchKernelGGL((reduce_bwd_kernel<Run<TA>, Frames<TB>>), dim3(blocks_bwd(total)), dim3(WG), 0, (hipStream_t)stream, op,
                       Run<TA>{(const TA*)a}, Frames<TB>{(const TB*)clip, m}, total, coef_dev, (TA*)ga, (TB*)nullptr);
  });
  return launch_status();
}

int cvvae_gauss_reg(int32_t dtype, const void* moments, const void* noise, void* z, int64_t B, int64_t C, int64_t S, void* workspace,
                    float* kl_sum, void* stream) {
  long long CS = 0, total = 0;
  if (const int rc = gauss_args(moments && z && workspace && kl_sum, dtype, B, C, S, &CS, &total)) return rc;
  hipStream_t s = (hipStream_t)stream;
  return reduce_to(total, workspace, 0.5f, kl_sum, s, [&](int nblk, float* ws) {
    by_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL(gauss_reg_kernel<T>, dim3(nblk), dim3(WG), 0, s, (const T*)moments, (const T*)noise, (T*)z, CS, total, ws);
    });
  });
}

int cvvae_gauss_reg_bwd(int32_t dtype, const void* moments, const void* noise, const void* g_z, const float* coef_kl_dev,
                        void* g_moments, int64_t B, int64_t C, int64_t S, void* stream) {
  long long CS = 0, total = 0;
  if (const int rc = gauss_args(moments && coef_kl_dev && g_moments, dtype, B, C, S, &CS, &total)) return rc;
  by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(gauss_reg_bwd_kernel<T>, dim3(blocks_bwd(total)), dim3(WG), 0, (hipStream_t)stream, (const T*)moments,
                       (const T*)noise, (const T*)g_z, coef_kl_dev, (T*)g_moments, CS, total);
  });
  return launch_status();
}

}  // extern "C"
