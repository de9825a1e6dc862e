// panel_kernels.hip -- the arithmetic of the training engines' log_images as one pass (include/cvvae.h cvvae_recon_panels): two
// NCTHW clips x and xrec, read in place through their strides and once each, give the four [(B T),3,H,W] panels
//   inputs = x,  reconstructions = xrec,
//   diff = 2 * clamp(0.5 * |clamp(xrec,-1,1) - x|, 0, 1) - 1,  diff_boost = 2 * clamp(f * 0.5 * |...|, 0, 1) - 1.
// gfx950, HBM bound: 2 reads and 4 writes per element, no LDS, no atomics.
//
// A thread owns one item of one row (b, c, t, y): item 0 is the scalar head, the elements in front of the first 16-byte boundary of
// the OUTPUT row (output rows start at r * W elements, so an odd W moves the boundary from row to row); item k >= 1 is the k-th group
// of V = 16 / sizeof(T) elements behind it, the last one cut at the row's end.  A whole group is stored with one 16-byte store per
// panel, and loaded with one 16-byte load per clip where that clip's address is aligned too (a row crop or an odd stride leaves the
// loads element by element and the stores whole).  Head, tail and groups run the same per-element code.
//
// Arithmetic: every operation of the eager expression is done in fp32 and rounded once to the clips' dtype T where eager torch
// stores a tensor of that dtype -- the subtraction, 0.5 *, f *, 2 * and - 1; clamp and abs are exact.  The scalar f multiplies in
// fp32 (torch's opmath for a Python scalar against a device tensor).  Contraction is off: f * h, 2 * v and v - 1 stay three
// roundings.  NaN is outside the contract.  The 8-element helpers of pass_common.h are restated here for V elements (4 for float).
#include "pass_common.h"

#pragma clang fp contract(off)

namespace cvvae {

constexpr int P_MAX_EXTENT = 1 << 20;        // H, W, B * T: the element count stays far inside int64
constexpr long long P_MAX_BLOCKS = 1 << 20;  // grid cap; the kernel strides over the items

struct PanelClip {
  const void* p;
  long long sb, sc, st, sy;
};

template <typename T>
struct PVec {
  static constexpr int N = 16 / (int)sizeof(T);
  typedef T type __attribute__((ext_vector_type(16 / sizeof(T))));
};

template <typename T>
__device__ __forceinline__ float rnd(float v) { return (float)(T)v; }

// the first n (<= V) elements at p: one 16-byte load when the group is whole and p is 16-byte aligned, element by element otherwise
template <typename T>
__device__ __forceinline__ void p_ld(const T* p, int n, T (&v)[PVec<T>::N]) {
  constexpr int V = PVec<T>::N;
  if (n == V && aligned16(p)) {
    const typename PVec<T>::type u = *reinterpret_cast<const typename PVec<T>::type*>(p);
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = u[k];
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = (k < n) ? p[k] : (T)0.f;
  }
}
template <typename T>
__device__ __forceinline__ void p_st(T* p, const T (&v)[PVec<T>::N], int n) {
  constexpr int V = PVec<T>::N;
  if (n == V && aligned16(p)) {
    typename PVec<T>::type u;
#pragma unroll
    for (int k = 0; k < V; ++k) u[k] = v[k];
    *reinterpret_cast<typename PVec<T>::type*>(p) = u;
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k)
      if (k < n) p[k] = v[k];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void recon_panels_kernel(PanelClip X, PanelClip R, int T_, int H, int W, int G, long long items, float boost,
                                                           T* __restrict__ o_in, T* __restrict__ o_rec, T* __restrict__ o_diff,
                                                           T* __restrict__ o_boost) {
  constexpr int V = PVec<T>::N;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
    const long long row = i / G;  // output row: ((b * T + t) * 3 + c) * H + y
    const int k = (int)(i - row * G);
    const int y = (int)(row % H);
    const long long fc = row / H;
    const int c = (int)(fc % 3);
    const long long f = fc / 3;
    const int t = (int)(f % T_);
    const long long b = f / T_;
    const long long o = row * W;
    // elements in front of the output row's first 16-byte boundary
    const int mis = (int)(reinterpret_cast<uintptr_t>(o_in + o) & 15) / (int)sizeof(T);
    const int head = min(W, (V - mis) & (V - 1));
    const int e0 = k == 0 ? 0 : head + (k - 1) * V;
    const int n = k == 0 ? head : min(V, W - e0);
    if (n <= 0) continue;
    const T* px = (const T*)X.p + b * X.sb + c * X.sc + t * X.st + y * X.sy + e0;
    const T* pr = (const T*)R.p + b * R.sb + c * R.sc + t * R.st + y * R.sy + e0;
    T xv[V], rv[V], dv[V], bv[V];
    p_ld<T>(px, n, xv);
    p_ld<T>(pr, n, rv);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float x = (float)xv[e], r = (float)rv[e];
      const float cl = fminf(fmaxf(r, -1.0f), 1.0f);      // torch.clamp(xrec, -1.0, 1.0)
      const float d = fabsf(rnd<T>(cl - x));                // torch.abs(... - x)
      float h = rnd<T>(0.5f * d);                           // 0.5 * ...
      h = fminf(fmaxf(h, 0.0f), 1.0f);                      // diff.clamp_(0, 1.0)
      dv[e] = (T)(rnd<T>(2.0f * h) - 1.0f);                 // 2.0 * diff - 1.0
      float g = rnd<T>(boost * h);                          // diff_boost_factor * diff
      g = fminf(fmaxf(g, 0.0f), 1.0f);                      // torch.clamp(..., 0.0, 1.0)
      bv[e] = (T)(rnd<T>(2.0f * g) - 1.0f);                 // 2.0 * ... - 1
    }
    p_st<T>(o_in + o + e0, xv, n);
    p_st<T>(o_rec + o + e0, rv, n);
    p_st<T>(o_diff + o + e0, dv, n);
    p_st<T>(o_boost + o + e0, bv, n);
  }
}

}  // namespace cvvae

using namespace cvvae;

extern "C" {

int cvvae_recon_panels(const void* x, const cvvae_clip_view* vx, const void* xrec, const cvvae_clip_view* vr, int32_t B, int32_t T,
                       int32_t H, int32_t W, float boost, void* inputs, void* reconstructions, void* diff, void* diff_boost,
                       void* stream) {
  if (!x || !xrec || !vx || !vr || !inputs || !reconstructions || !diff || !diff_boost) return CVVAE_EINVAL;
  if (B <= 0 || T <= 0 || H <= 0 || W <= 0) return CVVAE_EINVAL;
  const cvvae_clip_view* views[2] = {vx, vr};
  for (const cvvae_clip_view* v : views)
    if (v->sb < 0 || v->sc < 0 || v->st < 0 || v->sy < 0) return CVVAE_EINVAL;
  for (const cvvae_clip_view* v : views)
    if (v->layout != CVVAE_CLIP_NCTHW || !known_dtype(v->dtype)) return CVVAE_EUNSUPPORTED;
  if (vx->dtype != vr->dtype) return CVVAE_EUNSUPPORTED;
  for (const cvvae_clip_view* v : views)
    if (v->sy < (int64_t)W) return CVVAE_EINVAL;
  const uintptr_t esz = vx->dtype == CVVAE_F32 ? 4 : 2;
  const void* ptrs[6] = {x, xrec, inputs, reconstructions, diff, diff_boost};
  for (const void* p : ptrs)
    if (reinterpret_cast<uintptr_t>(p) & (esz - 1)) return CVVAE_EINVAL;
  if (H > P_MAX_EXTENT || W > P_MAX_EXTENT || (int64_t)B * T > P_MAX_EXTENT) return CVVAE_EUNSUPPORTED;

  const PanelClip X = {x, vx->sb, vx->sc, vx->st, vx->sy}, R = {xrec, vr->sb, vr->sc, vr->st, vr->sy};
  const long long rows = (long long)B * T * 3 * H;
  hipStream_t s = (hipStream_t)stream;
  by_dtype(vx->dtype, [&](auto tag) {
    using E = typename decltype(tag)::type;
    constexpr int V = PVec<E>::N;
    const int G = (W + V - 1) / V + 1;  // the head, then the groups behind it (the head shortens the row by < V elements)
    const long long items = rows * G;
    long long blocks = (items + 255) / 256;
    if (blocks > P_MAX_BLOCKS) blocks = P_MAX_BLOCKS;
    hipLaunchKernelGGL(recon_panels_kernel<E>, dim3((unsigned)blocks), dim3(256), 0, s, X, R, T, H, W, G, items, boost, (E*)inputs,
                       (E*)reconstructions, (E*)diff, (E*)diff_boost);
  });
  return launch_status();
}

}  // extern "C"
