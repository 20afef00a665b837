// View ensembles (test-time augmentation: the same image mirrored and at several scales): the step between a class sweep
// over B * V view images and dana_detect_merge / dana_detect_merge_soft with groups = V. Not in the reference tree; the
// rule is written out in include/dana_hip.h (dana_detect_fold_views) and restated by postprocess.fold_views_numpy.
//
//   fold_kernel<false>  one workgroup per input list p = (i * V + v) * C + c. The list is walked FV_THREADS rows at a
//                       time: a lane maps one row into the frame of the original image (un-mirror, frame test, clip, area
//                       window); the survivors are written in walk order to the same rows of the output buffer the list
//                       occupies in the input (ballot + prefix popcount inside a wave, the waves' totals across them, the
//                       running count across chunks). Lane 0 then writes the list's count and offset at the transposed
//                       index q = (i * C + c) * V + v, which is what puts the V views of one (image, class) side by side.
//
//   fold_kernel<true>   tiled inference (dana_detect_fold_tiles): the same walk for a view that is a WINDOW of the frame. A
//                       lane first tests its row against the tile, applies the seam rule on the unclipped coordinates,
//                       clips to the tile and translates into the (possibly mirrored) frame; then the steps above.
//
// Both kernels are one template, fold_kernel<TILES>: the view fold is the instantiation without the tile steps and compiles
// to what it was. No row leaves its list's rows, nothing is shared between workgroups, no atomics: two runs write the same
// bytes.
// Compiled with -ffp-contract=off: every expression below is one IEEE fp32 operation per written operation.
#include <limits.h>
#include "common.h"
#include "../../include/dana_hip.h"

namespace {

constexpr int FV_THREADS = 256;
constexpr int FV_WAVES = FV_THREADS / 64;

// max(x, 0) and min(x, hi) as selects: a -0 stays -0 and the numpy restatement (np.where) takes the same branch
__device__ __forceinline__ float clip_to(float x, float hi) {
  x = x < 0.f ? 0.f : x;
  return x > hi ? hi : x;
}

// view_table row: 0..4 = fw, fh, flip, area_lo, area_hi; for tiles 5..12 = x_off, y_off, tw, th, lim_x1, lim_y1, lim_x2, lim_y2
template <bool TILES>
__global__ void __launch_bounds__(FV_THREADS)
fold_kernel(const float* __restrict__ dets_in, const int* __restrict__ counts_in, const int* __restrict__ offsets_in,
            int views, int lists_per_view, const float* __restrict__ view_table, int view_stride,
            float* __restrict__ dets_out, int* __restrict__ counts_out, int* __restrict__ offsets_out,
            int* __restrict__ src_row_out) {
  __shared__ int s_wave[FV_WAVES];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int iv = p / lists_per_view, c = p % lists_per_view;
  const int i = iv / views, v = iv % views;
  const int n = max(counts_in[p], 0);
  const long off = offsets_in[p];
  const float* t = view_table + (long)iv * view_stride;
  const float wm1 = t[0] - 1.f, hm1 = t[1] - 1.f;
  const bool flip = t[2] != 0.f;
  const float area_lo = t[3], area_hi = t[4];
  // the tile's row is uniform over the workgroup and read once; the view fold never touches columns 5..12
  float x_off = 0.f, y_off = 0.f, twm1 = 0.f, thm1 = 0.f, lim_x1 = 0.f, lim_y1 = 0.f, lim_x2 = 0.f, lim_y2 = 0.f;
  if (TILES) {
    x_off = t[5], y_off = t[6], twm1 = t[7] - 1.f, thm1 = t[8] - 1.f;
    lim_x1 = t[9], lim_y1 = t[10], lim_x2 = t[11], lim_y2 = t[12];
  }
  int cnt = 0;  // rows kept so far: the same value in every thread
  for (int base = 0; base < n; base += FV_THREADS) {
    const int r = base + tid;
    bool keep = false;
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, score = 0.f;
    if (r < n) {
      const float* d = dets_in + (off + r) * 5;
      x1 = d[0], y1 = d[1], x2 = d[2], y2 = d[3], score = d[4];
      bool in_tile = true;
      if (TILES) {
        in_tile = x1 <= twm1 && y1 <= thm1 && x2 >= 0.f && y2 >= 0.f;                                // (a) touches the tile
        in_tile = in_tile && x1 >= lim_x1 && y1 >= lim_y1 && x2 <= lim_x2 && y2 <= lim_y2;          // (b) seam rule, unclipped
        x1 = clip_to(x1, twm1), x2 = clip_to(x2, twm1), y1 = clip_to(y1, thm1), y2 = clip_to(y2, thm1);  // (c)
        x1 = x1 + x_off, x2 = x2 + x_off, y1 = y1 + y_off, y2 = y2 + y_off;                          // (d)
      }
      if (flip) {
        const float a = wm1 - x2, b = wm1 - x1;
        x1 = a, x2 = b;
      }
      keep = in_tile && x1 <= wm1 && y1 <= hm1 && x2 >= 0.f && y2 >= 0.f;  // (a NaN fails its comparison)
      x1 = clip_to(x1, wm1), x2 = clip_to(x2, wm1);
      y1 = clip_to(y1, hm1), y2 = clip_to(y2, hm1);
      const float area = (x2 - x1 + 1.f) * (y2 - y1 + 1.f);
      keep = keep && area_lo <= area && area < area_hi;
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int total = 0, wbase = 0;
#pragma unroll
    for (int w = 0; w < FV_WAVES; ++w) {
      const int k = s_wave[w];
      if (w < wave) wbase += k;
      total += k;
    }
    if (keep) {
      const long o = off + cnt + wbase + __popcll(m & ((1ull << lane) - 1ull));  // <= off + r: inside the list's rows
      float* d = dets_out + o * 5;
      d[0] = x1, d[1] = y1, d[2] = x2, d[3] = y2, d[4] = score;
      if (src_row_out) src_row_out[o] = r;
    }
    cnt += total;
    __syncthreads();  // s_wave is read before the next chunk writes it
  }
  if (tid == 0) {
    const long q = ((long)i * lists_per_view + c) * views + v;
    counts_out[q] = cnt;
    offsets_out[q] = (int)off;
  }
}

template <bool TILES>
int fold_call(const char* who, int min_stride, const float* dets_in, const int* counts_in, const int* offsets_in, int n_images,
              int views, int lists_per_view, const float* view_table, int view_stride, float* dets_out, int* counts_out,
              int* offsets_out, int* src_row_out, dana_stream_t stream) {
  DANA_CHECK_ARG(n_images >= 0 && views >= 0 && lists_per_view >= 0, "%s: bad shape images=%d views=%d lists=%d", who,
                 n_images, views, lists_per_view);
  if (n_images == 0 || views == 0 || lists_per_view == 0) return DANA_OK;
  DANA_CHECK_ARG((long)n_images * views <= INT_MAX / lists_per_view, "%s: %d x %d x %d lists", who, n_images, views, lists_per_view);
  DANA_CHECK_ARG(view_stride >= min_stride, "%s: view_stride %d < %d (fw, fh, flip, area_lo, area_hi%s)", who, view_stride,
                 min_stride, TILES ? ", x_off, y_off, tw, th, lim_x1, lim_y1, lim_x2, lim_y2" : "");
  DANA_CHECK_ARG(dets_in && counts_in && offsets_in && view_table && dets_out && counts_out && offsets_out, "%s: null pointer", who);
  DANA_CHECK_ARG(dets_out != dets_in, "%s: dets_out must not alias dets_in", who);
  fold_kernel<TILES><<<(unsigned)(n_images * views * lists_per_view), FV_THREADS, 0, (hipStream_t)stream>>>(
      dets_in, counts_in, offsets_in, views, lists_per_view, view_table, view_stride, dets_out, counts_out, offsets_out,
      src_row_out);
  DANA_CHECK_LAUNCH(who);
  return DANA_OK;
}

}  // namespace

extern "C" {

int dana_detect_fold_views(const float* dets_in, const int* counts_in, const int* offsets_in, int n_images, int views,
                           int lists_per_view, const float* view_table, int view_stride, float* dets_out, int* counts_out,
                           int* offsets_out, int* src_row_out, dana_stream_t stream) {
  return fold_call<false>("dana_detect_fold_views", 5, dets_in, counts_in, offsets_in, n_images, views, lists_per_view, view_table,
                          view_stride, dets_out, counts_out, offsets_out, src_row_out, stream);
}

int dana_detect_fold_tiles(const float* dets_in, const int* counts_in, const int* offsets_in, int n_images, int views,
                           int lists_per_view, const float* view_table, int view_stride, float* dets_out, int* counts_out,
                           int* offsets_out, int* src_row_out, dana_stream_t stream) {
  return fold_call<true>("dana_detect_fold_tiles", 13, dets_in, counts_in, offsets_in, n_images, views, lists_per_view, view_table,
                         view_stride, dets_out, counts_out, offsets_out, src_row_out, stream);
}

}  // extern "C"
