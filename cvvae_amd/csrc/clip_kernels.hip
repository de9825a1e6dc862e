// clip_kernels.hip -- the training data side's per-sample transform as one pass (include/cvvae.h cvvae_clip_from_frames_u8): decoded
// uint8 frames [T_in][H][W][3] -> one slot [3][T_out][oh][ow] of the training batch, in [-1, 1]:
//   frame selection (frame_index), separable resampling of ONLY the crop window (caller-built tap tables, cvvae_amd/data.py),
//   ((v / 255) - 0.5) * 2, one rounding to the slot's dtype, the [T,H,W,C] -> [C,T,H,W] move.
// gfx950; no atomics, one writer per output element.
//
// A workgroup of 256 threads owns one frame, R output rows and 64 output columns.  It works through its rows in batches whose input
// rows fit the LDS stage of `cap` rows (the host picks R so that a tile is one batch; the loop only makes the kernel independent of
// that estimate):
//   horizontal: thread (x = tid & 63, wave = tid >> 6) resamples column x of one (input row, channel) per step straight from the
//               frame's bytes -- the lanes of a wave read bytes 3 * scale apart in one row, which the vector cache serves -- and writes
//               the fp32 value to stage[row][c][x] (consecutive dwords: no bank conflict);
//   vertical:   thread (4 columns, one (output row, channel) per step) reads float4s from the stage (64 consecutive dwords per 16
//               lanes: conflict-free for ds_read_b128), runs the tap chain, normalises and stores 4 elements with one store where the
//               address is aligned to it and the row has them, element by element otherwise.
// Arithmetic (the contract): each pass is acc = w0 * s0, then acc = fma(wj, sj, acc) in tap order, fp32; the division is IEEE.
// Contraction is off, so the subtraction and the doubling stay their own roundings.  The value of an output element depends on the
// frame's bytes and the table entries alone, not on the tile it falls in.
//
// The tables are trusted for the VALUES; for memory safety every frame, row and column index is clamped into the frame and every
// stage index into the stage, which changes nothing for tables that stay inside [y_lo, y_hi) x [x_lo, x_hi).
#include "pass_common.h"

#pragma clang fp contract(off)

namespace cvvae {

constexpr int CL_TILE_W = 64;             // output columns per workgroup
constexpr int CL_STAGE_ROW = 3 * CL_TILE_W;  // floats per staged input row
constexpr int CL_MAX_ROWS = 64;           // 64 rows * 768 B = 48 KiB: three workgroups share a CU's 160 KiB
constexpr int CL_MAX_EXTENT = 1 << 20;    // H, W, oh, ow
constexpr int CL_MAX_FRAMES = 65535;      // grid z

struct ClipArgs {
  const uint8_t* frames;
  long long in_st, in_sy;  // bytes
  int T_in, H, W;
  const int32_t* frame_index;
  const int32_t *ymin, *ysize;
  const float* yw;
  int kh, oh;
  const int32_t *xmin, *xsize;
  const float* xw;
  int kw, ow;
  long long sc, st, sy;  // elements
  int R, cap;
};

__device__ __forceinline__ int cl_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ float cl_norm(float v) { return (__fdiv_rn(v, 255.0f) - 0.5f) * 2.0f; }

template <typename T>
__global__ __launch_bounds__(256) void clip_from_frames_kernel(ClipArgs a, T* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float stage[];  // [rows <= cap][3][64]
  typedef T V4 __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x;
  const int t = blockIdx.z;
  const int x0 = blockIdx.y * CL_TILE_W;
  const int r_begin = blockIdx.x * a.R, r_end = min(r_begin + a.R, a.oh);
  const int fi = cl_clamp(a.frame_index ? a.frame_index[t] : t, 0, a.T_in - 1);
  const uint8_t* src = a.frames + (long long)fi * a.in_st;

  // the horizontal pass's column of this thread
  const int hl = tid & 63, hx = x0 + hl;
  int hmin = 0, hn = 0;
  if (hx < a.ow) {
    hmin = a.xmin[hx];
    hn = cl_clamp(a.xsize[hx], 0, a.kw);
  }
  const float* hw = a.xw + (long long)min(hx, a.ow - 1) * a.kw;
  // the vertical pass's four columns
  const int vl = (tid & 15) * 4, vx = x0 + vl;
  const int vn = min(4, a.ow - vx);

  for (int r = r_begin; r < r_end;) {
    // the batch [r, r + n): its input rows [lo, hi) fit the stage (all of this is uniform over the workgroup)
    const int lo = cl_clamp(a.ymin[r], 0, a.H - 1);
    int hi = lo + 1, n = 0;
    for (; r + n < r_end; ++n) {
      const int b = a.ymin[r + n];
      const int e = b + cl_clamp(a.ysize[r + n], 0, a.kh);
      if (n > 0 && (b < lo || e > lo + a.cap)) break;
      hi = max(hi, min(e, lo + a.cap));
    }
    hi = min(hi, a.H);
    const int rows = hi - lo;  // 1 .. cap

    for (int item = tid >> 6; item < rows * 3; item += 4) {
      const int row = item / 3, c = item - row * 3;
      float acc = 0.f;
      if (hn > 0) {
        const uint8_t* p = src + (long long)(lo + row) * a.in_sy + c;
        acc = hw[0] * (float)p[3 * cl_clamp(hmin, 0, a.W - 1)];
        for (int j = 1; j < hn; ++j) acc = __fmaf_rn(hw[j], (float)p[3 * cl_clamp(hmin + j, 0, a.W - 1)], acc);
      }
      stage[item * CL_TILE_W + hl] = acc;
    }
    __syncthreads();

    if (vn > 0) {
      for (int item = tid >> 4; item < n * 3; item += 16) {
        const int ry = item / 3, c = item - ry * 3;
        const int y = r + ry;
        const int first = a.ymin[y] - lo;
        const int nt = cl_clamp(a.ysize[y], 0, a.kh);
        const float* w = a.yw + (long long)y * a.kh;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (nt > 0) {
          const float* sp = stage + c * CL_TILE_W + vl;
          const float w0 = w[0];
          const float4 s0 = *reinterpret_cast<const float4*>(sp + cl_clamp(first, 0, rows - 1) * CL_STAGE_ROW);
          acc[0] = w0 * s0.x; acc[1] = w0 * s0.y; acc[2] = w0 * s0.z; acc[3] = w0 * s0.w;
          for (int j = 1; j < nt; ++j) {
            const float wj = w[j];
            const float4 s = *reinterpret_cast<const float4*>(sp + cl_clamp(first + j, 0, rows - 1) * CL_STAGE_ROW);
            acc[0] = __fmaf_rn(wj, s.x, acc[0]); acc[1] = __fmaf_rn(wj, s.y, acc[1]);
            acc[2] = __fmaf_rn(wj, s.z, acc[2]); acc[3] = __fmaf_rn(wj, s.w, acc[3]);
          }
        }
        T* p = out + c * a.sc + t * a.st + y * a.sy + vx;
        if (vn == 4 && (reinterpret_cast<uintptr_t>(p) & (4 * sizeof(T) - 1)) == 0) {
          V4 v;
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = (T)cl_norm(acc[k]);
          *reinterpret_cast<V4*>(p) = v;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k < vn) p[k] = (T)cl_norm(acc[k]);
        }
      }
    }
    __syncthreads();
    r += n;
  }
}

}  // namespace cvvae

using namespace cvvae;

extern "C" {

int cvvae_clip_from_frames_u8(const uint8_t* frames, const cvvae_clip_view* vin, int32_t T_in, int32_t H, int32_t W,
                              const int32_t* frame_index, int32_t T_out, const int32_t* ymin, const int32_t* ysize, const float* yw,
                              int32_t kh, int32_t oh, const int32_t* xmin, const int32_t* xsize, const float* xw, int32_t kw, int32_t ow,
                              int32_t y_lo, int32_t y_hi, int32_t x_lo, int32_t x_hi, void* out, const cvvae_clip_view* vout,
                              void* stream) {
  if (!frames || !vin || !ymin || !ysize || !yw || !xmin || !xsize || !xw || !out || !vout) return CVVAE_EINVAL;
  if (T_in <= 0 || H <= 0 || W <= 0 || T_out <= 0 || oh <= 0 || ow <= 0) return CVVAE_EINVAL;
  if (kh < 1 || kw < 1) return CVVAE_EINVAL;
  if (vin->st < 0 || vin->sy < 0 || vout->sc < 0 || vout->st < 0 || vout->sy < 0) return CVVAE_EINVAL;
  if (vin->layout != CVVAE_CLIP_THWC_U8 || vout->layout != CVVAE_CLIP_NCTHW || !known_dtype(vout->dtype)) return CVVAE_EUNSUPPORTED;
  if (vin->sy < 3 * (int64_t)W || vout->sy < (int64_t)ow) return CVVAE_EINVAL;
  const uintptr_t esz = vout->dtype == CVVAE_F32 ? 4 : 2;
  if (reinterpret_cast<uintptr_t>(out) & (esz - 1)) return CVVAE_EINVAL;
  if (y_lo < 0 || y_hi > H || y_lo >= y_hi || x_lo < 0 || x_hi > W || x_lo >= x_hi) return CVVAE_EINVAL;
  if (H > CL_MAX_EXTENT || W > CL_MAX_EXTENT || oh > CL_MAX_EXTENT || ow > CL_MAX_EXTENT || T_out > CL_MAX_FRAMES)
    return CVVAE_EUNSUPPORTED;
  // R output rows read about (R - 1) * (input rows per output row) + kh + 1 input rows; the largest R whose rows fit the stage
  if (kh > CL_MAX_ROWS) return CVVAE_EUNSUPPORTED;
  const int64_t span = (int64_t)y_hi - y_lo;
  int R = 16, cap = 0;
  for (;; R >>= 1) {
    const int64_t need = ((R - 1) * span + oh - 1) / oh + kh + 1;
    if (need <= CL_MAX_ROWS || R == 1) {
      cap = (int)(need < CL_MAX_ROWS ? need : CL_MAX_ROWS);
      break;
    }
  }

  ClipArgs a;
  a.frames = frames; a.in_st = vin->st; a.in_sy = vin->sy; a.T_in = T_in; a.H = H; a.W = W;
  a.frame_index = frame_index;
  a.ymin = ymin; a.ysize = ysize; a.yw = yw; a.kh = kh; a.oh = oh;
  a.xmin = xmin; a.xsize = xsize; a.xw = xw; a.kw = kw; a.ow = ow;
  a.sc = vout->sc; a.st = vout->st; a.sy = vout->sy; a.R = R; a.cap = cap;
  const dim3 grid((unsigned)((oh + R - 1) / R), (unsigned)((ow + CL_TILE_W - 1) / CL_TILE_W), (unsigned)T_out);
  const size_t lds = (size_t)cap * CL_STAGE_ROW * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  by_dtype(vout->dtype, [&](auto tag) {
    using E = typename decltype(tag)::type;
    hipLaunchKernelGGL(clip_from_frames_kernel<E>, grid, dim3(256), lds, s, a, (E*)out);
  });
  return launch_status();
}

}  // extern "C"
