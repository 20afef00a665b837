// Attention maps (README "Attention Visualization"): the attention weights the forward materialises and drops -- the
// RPN-level rows of dana.py:142-146 and the RoI-level rows of dana.py:273-277 -- reduced to one map per (box, shot) on
// the device, and the two image-side kernels that turn a map into the README's overlay.
//
//   attn_box_mean_kernel   out[p][j][k] = mean over the rows r of box j's rectangle of attn[p][r][k]
//   heatmap_upsample_kernel  cv2.resize(INTER_LINEAR) of a [gh][gw] map to [S][S] (the tap convention of pipeline.hip)
//   heatmap_render_kernel  upsample, per-map min-max normalisation, 256-entry colour table, blend with the prepared image
//
// The cell rectangle of a box (attention.cell_rect is the same rule in Python, tested on hand-worked boxes): on a
// (gh, gw) grid of `cell`-pixel cells
//   x_lo = clamp(floor(x1 / cell), 0, gw - 1)    x_hi = clamp(floor(x2 / cell), x_lo, gw - 1)
// and the same for y with gh: never empty, never outside the grid, whatever the box holds (a NaN coordinate lands on
// cell 0: fmaxf / fminf return their other operand).
#include "common.h"
#include "../../include/dana_hip.h"
#include <float.h>
#include <limits.h>

namespace {

constexpr int BM_THREADS = 64;  // one wave per (problem, box, column chunk); a chunk is BM_THREADS * VEC columns

__device__ __forceinline__ int cell_lo(float v, float inv_cell, int n) {
  return (int)fminf(fmaxf(floorf(v * inv_cell), 0.f), (float)(n - 1));
}
__device__ __forceinline__ int cell_hi(float v, float inv_cell, int lo, int n) {
  return (int)fminf(fmaxf(floorf(v * inv_cell), (float)lo), (float)(n - 1));
}

constexpr int BM_UNROLL = 8;    // rows in flight per lane

template <int VEC>
struct RowVec {
  float v[VEC];
};
template <int VEC>
__device__ __forceinline__ RowVec<VEC> load_row(const float* r) {
  RowVec<VEC> t;
  if constexpr (VEC == 4) {
    const float4 q = *reinterpret_cast<const float4*>(r);  // (c0 + 3 < ld: ld % 4 == 0 and c0 < K <= ld)
    t.v[0] = q.x;
    t.v[1] = q.y;
    t.v[2] = q.z;
    t.v[3] = q.w;
  } else {
    t.v[0] = r[0];
  }
  return t;
}

// Lanes run along the K columns (VEC = 4: one float4 per lane and row, ld % 4 == 0 and a 16-byte aligned base), the
// rectangle's rows are walked in row-major order by every lane alike: a fixed order, two runs give the same bits. The
// sum is kept in float64 (exact for up to 2^29 fp32 terms of one binade; rounded once, at the end).
// mode 0: rows_b == gh * gw, the rectangle comes from boxes[(p / group)][j]; mode 1 (RoI level): rows_b == n * gh * gw,
// box j owns rows j * gh * gw .. + gh * gw and the rectangle is the whole grid (boxes is not read).
template <int VEC>
__global__ void __launch_bounds__(BM_THREADS)
attn_box_mean_kernel(const float* __restrict__ attn, const float* __restrict__ boxes, float* __restrict__ out, int rows_b,
                     long ld, int K, int n, int gh, int gw, int group, int mode, float inv_cell) {
  const int p = blockIdx.z, j = blockIdx.y;
  const int c0 = (blockIdx.x * BM_THREADS + threadIdx.x) * VEC;
  if (c0 >= K) return;
  int x_lo = 0, x_hi = gw - 1, y_lo = 0, y_hi = gh - 1;
  long base = 0;
  if (mode == 0) {
    const float* b = boxes + ((long)(p / group) * n + j) * 4;
    x_lo = cell_lo(b[0], inv_cell, gw);
    x_hi = cell_hi(b[2], inv_cell, x_lo, gw);
    y_lo = cell_lo(b[1], inv_cell, gh);
    y_hi = cell_hi(b[3], inv_cell, y_lo, gh);
  } else {
    base = (long)j * gh * gw;
  }
  const float* a = attn + ((long)p * rows_b + base) * ld + c0;
  double acc[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v] = 0.0;
  // step i of the walk is cell (y_lo + i / rw, x_lo + i % rw). A wave has nothing to hide a load's latency behind but
  // its own next loads: BM_UNROLL rows are loaded before the first of them is added -- in walk order, so the unrolled loop
  // sums exactly what the plain one would.
  const int rw = x_hi - x_lo + 1, nrow = rw * (y_hi - y_lo + 1);
  const long first = (long)y_lo * gw + x_lo;
  int i = 0;
  for (; i + BM_UNROLL <= nrow; i += BM_UNROLL) {
    RowVec<VEC> t[BM_UNROLL];
#pragma unroll
    for (int u = 0; u < BM_UNROLL; ++u) t[u] = load_row<VEC>(a + (first + (long)((i + u) / rw) * gw + (i + u) % rw) * ld);
#pragma unroll
    for (int u = 0; u < BM_UNROLL; ++u)
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] += (double)t[u].v[v];
  }
  for (; i < nrow; ++i) {
    const RowVec<VEC> t = load_row<VEC>(a + (first + (long)(i / rw) * gw + i % rw) * ld);
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] += (double)t.v[v];
  }
  const double inv_n = 1.0 / (double)nrow;
  float* o = out + ((long)p * n + j) * K + c0;
#pragma unroll
  for (int v = 0; v < VEC; ++v)
    if (c0 + v < K) o[v] = (float)(acc[v] * inv_n);
}

// cv2.resize(INTER_LINEAR), the convention of pipeline.hip's linear_tap: sample position (d + 0.5) * scale - 0.5,
// s = floor, s < 0 -> (0, 0), s >= n - 1 -> (n - 1, 0). The position stays in double until the fraction is taken (cv2
// rounds it to float first: up to 2.4e-7 of a cell at 7 -> 320, which a map's numbers need not carry).
struct Tap {
  int s0, s1;
  float a0, a1;
};
__device__ __forceinline__ Tap linear_tap(int d, double scale, int n) {
  const double pos = ((double)d + 0.5) * scale - 0.5;
  int s = (int)floor(pos);
  float f = (float)(pos - (double)s);
  if (s < 0) {
    s = 0;
    f = 0.f;
  }
  if (s >= n - 1) {
    s = n - 1;
    f = 0.f;
  }
  Tap t;
  t.s0 = s;
  t.s1 = min(s + 1, n - 1);
  t.a0 = 1.f - f;
  t.a1 = f;
  return t;
}
__device__ __forceinline__ float sample_map(const float* __restrict__ m, int gh, int gw, int y, int x, double scale_y,
                                            double scale_x) {
  const Tap tx = linear_tap(x, scale_x, gw), ty = linear_tap(y, scale_y, gh);
  const float* r0 = m + (long)ty.s0 * gw;
  const float* r1 = m + (long)ty.s1 * gw;
  const float h0 = r0[tx.s0] * tx.a0 + r0[tx.s1] * tx.a1;
  const float h1 = r1[tx.s0] * tx.a0 + r1[tx.s1] * tx.a1;
  return h0 * ty.a0 + h1 * ty.a1;
}

__global__ void __launch_bounds__(256)
heatmap_upsample_kernel(const float* __restrict__ maps, float* __restrict__ out, long total, int gh, int gw, int size,
                        double scale_y, double scale_x) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long pix = (long)size * size;
  const long m = i / pix;
  const int q = (int)(i - m * pix);
  out[i] = sample_map(maps + m * gh * gw, gh, gw, q / size, q % size, scale_y, scale_x);
}

// `bpm` workgroups per map. Each reduces ITS map's gh * gw entries to (min, max) itself -- a few hundred floats, cheaper
// than a second launch and a round trip through memory -- then colours its share of the S * S pixels:
//   t = (v - min) / (max - min) (0 for a constant map), entry round(255 t) of table[256][3] (RGB bytes),
//   out[y][x][c] = round((1 - alpha) * clamp(image[2 - c][y][x] + mean[2 - c], 0, 255) + alpha * table[c])
// (image: BGR planes, mean-subtracted, as the model is fed; out: RGB interleaved).
__global__ void __launch_bounds__(256)
heatmap_render_kernel(const float* __restrict__ maps, const float* __restrict__ images,
                      const unsigned char* __restrict__ table, unsigned char* __restrict__ out, int bpm, int gh, int gw,
                      int size, double scale_y, double scale_x, float alpha, float mean_b, float mean_g, float mean_r) {
  __shared__ float s_lo[256], s_hi[256];
  const long m = blockIdx.x / bpm;
  const int part = blockIdx.x % bpm, tid = threadIdx.x;
  const float* mp = maps + m * gh * gw;
  float lo = FLT_MAX, hi = -FLT_MAX;
  for (int i = tid; i < gh * gw; i += 256) {
    const float v = mp[i];
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  s_lo[tid] = lo;
  s_hi[tid] = hi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      s_lo[tid] = fminf(s_lo[tid], s_lo[tid + o]);
      s_hi[tid] = fmaxf(s_hi[tid], s_hi[tid + o]);
    }
    __syncthreads();
  }
  lo = s_lo[0];
  hi = s_hi[0];
  const float inv = hi > lo ? 1.f / (hi - lo) : 0.f;
  const int pix = size * size;
  const float* im = images + m * 3 * (long)pix;
  unsigned char* op = out + m * 3 * (long)pix;
  const float mean[3] = {mean_r, mean_g, mean_b};  // by OUTPUT channel (RGB)
  for (int q = part * 256 + tid; q < pix; q += bpm * 256) {
    const float v = sample_map(mp, gh, gw, q / size, q % size, scale_y, scale_x);
    const float t = fminf(fmaxf((v - lo) * inv, 0.f), 1.f);
    const int e = (int)(t * 255.f + 0.5f);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float px = fminf(fmaxf(im[(long)(2 - c) * pix + q] + mean[c], 0.f), 255.f);
      const float b = (1.f - alpha) * px + alpha * (float)table[e * 3 + c];
      op[(long)q * 3 + c] = (unsigned char)(fminf(fmaxf(b, 0.f), 255.f) + 0.5f);
    }
  }
}

}  // namespace

extern "C" {

int dana_attn_box_mean(const float* attn, const float* boxes, float* out, int n_problems, int rows_b, long ld, int k, int n,
                       int gh, int gw, int group, int mode, float cell, dana_stream_t stream) {
  DANA_CHECK_ARG(n_problems > 0 && n_problems <= 65535 && n > 0 && n <= 65535 && k > 0 && gh > 0 && gw > 0 && group > 0 &&
                     (long)gh * gw <= INT_MAX,
                 "dana_attn_box_mean: bad shape problems=%d n=%d k=%d grid=%dx%d group=%d", n_problems, n, k, gh, gw, group);
  DANA_CHECK_ARG(mode == 0 || mode == 1, "dana_attn_box_mean: mode %d (0: box rectangles, 1: per-box row blocks)", mode);
  DANA_CHECK_ARG(ld >= k, "dana_attn_box_mean: ld %ld < k %d", ld, k);
  DANA_CHECK_ARG(mode == 0 ? (long)gh * gw == rows_b : (long)n * gh * gw == rows_b,
                 "dana_attn_box_mean: rows_b %d is not %s%d x %d", rows_b, mode ? "n x " : "", gh, gw);
  DANA_CHECK_ARG(mode == 1 || (n_problems % group == 0 && cell > 0.f),
                 "dana_attn_box_mean: %d problems in groups of %d, cell %g", n_problems, group, (double)cell);
  DANA_CHECK_ARG(attn && out && (boxes || mode == 1), "dana_attn_box_mean: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const float inv_cell = mode == 0 ? 1.f / cell : 1.f;
  if (ld % 4 == 0 && ((uintptr_t)attn & 15) == 0) {
    const dim3 grid(dana_ceil_div(k, BM_THREADS * 4), n, n_problems);
    attn_box_mean_kernel<4><<<grid, BM_THREADS, 0, s>>>(attn, boxes, out, rows_b, ld, k, n, gh, gw, group, mode, inv_cell);
  } else {
    const dim3 grid(dana_ceil_div(k, BM_THREADS), n, n_problems);
    attn_box_mean_kernel<1><<<grid, BM_THREADS, 0, s>>>(attn, boxes, out, rows_b, ld, k, n, gh, gw, group, mode, inv_cell);
  }
  DANA_CHECK_LAUNCH("dana_attn_box_mean");
  return DANA_OK;
}

int dana_heatmap_upsample(const float* maps, float* out, long n_maps, int gh, int gw, int size, dana_stream_t stream) {
  DANA_CHECK_ARG(n_maps >= 0 && gh > 0 && gw > 0 && size > 0 && (long)gh * gw <= INT_MAX && size <= 32768,
                 "dana_heatmap_upsample: bad shape maps=%ld grid=%dx%d size=%d", n_maps, gh, gw, size);
  if (n_maps == 0) return DANA_OK;
  DANA_CHECK_ARG(maps && out, "dana_heatmap_upsample: null pointer");
  const long total = n_maps * size * size;
  DANA_CHECK_ARG((total + 255) / 256 <= INT_MAX, "dana_heatmap_upsample: %ld output pixels", total);
  heatmap_upsample_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      maps, out, total, gh, gw, size, (double)gh / size, (double)gw / size);
  DANA_CHECK_LAUNCH("dana_heatmap_upsample");
  return DANA_OK;
}

int dana_heatmap_render(const float* maps, const float* images, const unsigned char* table, void* out, long n_maps,
                        int gh, int gw, int size, float alpha, float mean_b, float mean_g, float mean_r,
                        dana_stream_t stream) {
  DANA_CHECK_ARG(n_maps >= 0 && gh > 0 && gw > 0 && size > 0 && (long)gh * gw <= INT_MAX && size <= 32768,
                 "dana_heatmap_render: bad shape maps=%ld grid=%dx%d size=%d", n_maps, gh, gw, size);
  DANA_CHECK_ARG(alpha >= 0.f && alpha <= 1.f, "dana_heatmap_render: alpha %g outside [0, 1]", (double)alpha);
  if (n_maps == 0) return DANA_OK;
  DANA_CHECK_ARG(maps && images && table && out, "dana_heatmap_render: null pointer");
  int bpm = dana_ceil_div((long)size * size, 256 * 8);  // 8 pixels per thread
  if (bpm > 64) bpm = 64;
  DANA_CHECK_ARG(n_maps <= INT_MAX / bpm, "dana_heatmap_render: %ld maps", n_maps);
  heatmap_render_kernel<<<(unsigned)(n_maps * bpm), 256, 0, (hipStream_t)stream>>>(
      maps, images, table, (unsigned char*)out, bpm, gh, gw, size, (double)gh / size, (double)gw / size, alpha, mean_b, mean_g, mean_r);
  DANA_CHECK_LAUNCH("dana_heatmap_render");
  return DANA_OK;
}

}  // extern "C"
