// The prediction figure (README images/prediction.jpg; fsod_logger.py:22-34, 56-102; net_utils.py:50-60; utils.py:304-310)
// on the device: prepared images back to RGB bytes, box outlines and labels drawn into them, and the query laid out next
// to its support shots.
//
//   to_rgb_kernel      out[y][x][c] = clamp(round(image[2 - c][y][x] + mean[2 - c]), 0, 255): heatmap_render_kernel's
//                      rounding at alpha = 0 (attention_maps.hip), NaN -> 0
//   draw_boxes_kernel  a tile-binned rasteriser: one workgroup per canvas tile, one launch for every box of every image
//   sheet_kernel       query | pad | columns of side x side shots, each resized with common.h's dana_linear_tap
//
// The pixel rule of draw_boxes (render.boxes_numpy is the same rule in numpy, tested on hand-worked boxes). A row
// (x1, y1, x2, y2, v) of image b:
//   1. c' = c * scale[b] in fp32; a row with a NaN / Inf product or a NaN v is skipped; C = (int)clamp(c', -2^20, 2^20)
//   2. X2 < X1 or Y2 < Y1: skipped
//   3. h = t / 2, g = t - h
//   4. band = [X1 - h, X2 + h] x [Y1 - h, Y2 + h] minus [X1 + g, X2 - g] x [Y1 + g, Y2 - g], inside the canvas
//   5. label bar (labels on): 6 * nchars + 1 wide, 9 high, top-left (X1 - h, Y1 - h - 9), or (X1 - h, Y1 + g) when that
//      would start above the canvas; filled with the box's colour, glyph pixels (5x7 in 6x8 cells, one pixel in from the
//      bar's top-left) black when the colour's luma (299 R + 587 G + 114 B) / 1000 >= 128, white otherwise. A box's bar
//      lies over its own band.
//   6. a pixel takes the colour of the topmost box whose band or bar covers it; a pixel nothing covers is not written.
// Compiled with -ffp-contract=off: the products of step 1 and the label's hundredths are single fp32 operations.
#include "common.h"
#include "../../include/dana_hip.h"
#include <float.h>
#include <limits.h>

namespace {

// ---- to_rgb ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
to_rgb_kernel(const float* __restrict__ images, unsigned char* __restrict__ out, long n_images, long pix, float mean_b,
              float mean_g, float mean_r) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_images * pix) return;
  const long m = i / pix, q = i - m * pix;
  const float* im = images + m * 3 * pix + q;
  const float mean[3] = {mean_r, mean_g, mean_b};  // by OUTPUT channel (RGB)
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float px = fminf(fmaxf(im[(long)(2 - c) * pix] + mean[c], 0.f), 255.f);  // (fmaxf(NaN, 0) = 0)
    out[i * 3 + c] = (unsigned char)(px + 0.5f);
  }
}

// ---- draw_boxes ------------------------------------------------------------------------------------------------------------
constexpr int DB_THREADS = 256;  // 4 waves
constexpr int DB_TW = 64, DB_TH = 16, DB_PX = 4;  // tile; a thread owns DB_PX horizontally adjacent pixels of one tile row
constexpr int DB_CAP = 256;      // boxes in the LDS list (render.LIST_CHUNK): one chunk of rows can always be appended
constexpr int DB_LISTS = 256;    // lists of an image whose counts are scanned at a time
constexpr int DB_MAX_T = 1024;   // thickness bound: coordinates stay far inside int
constexpr int DB_MAX_NUM = 9999; // largest number a label prints (class slot, ground-truth class)
constexpr float DB_COORD = 1048576.f;  // 2^20
static_assert(DB_THREADS == DB_TH * (DB_TW / DB_PX), "one thread per DB_PX pixels of the tile");
static_assert(DB_CAP >= DB_THREADS && DB_LISTS == DB_THREADS, "a chunk of rows fits the list; one count per thread");

struct Hit {
  int x1, y1, x2, y2;  // the truncated corners
  int by;              // the label bar's top row (its left column is x1 - h)
  int nch;             // characters of the label, 0: none
  unsigned col;        // R | G << 8 | B << 16 | (glyphs white) << 24
  unsigned c0, c1;     // the characters, 4 bits each from the low end of c0 (0-9, 10 '.', 11 ' ')
};

struct DrawArgs {
  unsigned char* canvas;
  const float* boxes;
  const int* counts;      // layout form: counts[n_images * lists] and offsets[n_images * lists]
  const int* offsets;
  const int* num_boxes;   // ground-truth form (counts == nullptr): rows b * per_image .. + min(num_boxes[b], per_image)
  const float* scale_dev; // [n_images] or nullptr: `scale`
  const unsigned char* colors;
  const int* color_index; // [n_color_index] or nullptr; a row at or beyond its end takes the class slot
  const unsigned char* font;  // [12][7]: 5 bits per glyph row, bit 4 the left column
  long n_rows, n_color_index;
  int height, width, row_ld, lists, per_image, thickness, use_min_score, n_colors, labels, top_last;
  float scale, min_score;
};

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= FLT_MAX; }  // false for NaN and Inf
__device__ __forceinline__ int trunc_coord(float v) { return (int)fminf(fmaxf(v, -DB_COORD), DB_COORD); }

// the label's characters, 4 bits each: c0 holds the first eight, c1 the rest
__device__ __forceinline__ void put_char(unsigned& c0, unsigned& c1, int& n, unsigned ch) {
  if (n < 8) c0 |= ch << (4 * n);
  else c1 |= ch << (4 * (n - 8));
  ++n;
}
// decimal digits of 0 <= v <= DB_MAX_NUM appended to the text (most significant first)
__device__ __forceinline__ void put_number(unsigned& c0, unsigned& c1, int& n, int v) {
  if (v >= 1000) put_char(c0, c1, n, (unsigned)(v / 1000 % 10));
  if (v >= 100) put_char(c0, c1, n, (unsigned)(v / 100 % 10));
  if (v >= 10) put_char(c0, c1, n, (unsigned)(v / 10 % 10));
  put_char(c0, c1, n, (unsigned)(v % 10));
}
__device__ __forceinline__ int count_digits(int v) { return 1 + (v >= 10) + (v >= 100) + (v >= 1000); }

// Row r of image b (class slot `slot`) -> its Hit; false when the row is skipped or touches nothing of the tile
// [tx0, tx1] x [ty0, ty1] (inclusive, already clipped to the canvas).
__device__ __forceinline__ bool make_hit(const DrawArgs& a, long r, int b, int slot, int tx0, int ty0, int tx1, int ty1,
                                         Hit& hh) {
  if (r < 0 || r >= a.n_rows) return false;  // (a layout that points outside the buffer draws nothing)
  const float* row = a.boxes + r * a.row_ld;
  const float sc = a.scale_dev ? a.scale_dev[b] : a.scale;
  const float fx1 = row[0] * sc, fy1 = row[1] * sc, fx2 = row[2] * sc, fy2 = row[3] * sc, v = row[4];
  if (!(finite_f(fx1) && finite_f(fy1) && finite_f(fx2) && finite_f(fy2)) || v != v) return false;
  const bool gt_form = a.counts == nullptr;
  if (gt_form && v == 0.f) return false;
  if (a.use_min_score && v < a.min_score) return false;
  const int X1 = trunc_coord(fx1), Y1 = trunc_coord(fy1), X2 = trunc_coord(fx2), Y2 = trunc_coord(fy2);
  if (X2 < X1 || Y2 < Y1) return false;
  const int t = a.thickness, h = t / 2, g = t - h;
  int nch = 0, by = 0, number = 0;  // the label's length decides the bar; its characters are made for survivors only
  if (a.labels) {
    number = gt_form ? (int)fminf(fmaxf(v, 0.f), (float)DB_MAX_NUM) : slot;
    nch = count_digits(number) + (gt_form ? 0 : 5);
    by = Y1 - h - 9 >= 0 ? Y1 - h - 9 : Y1 + g;
  }
  // the tile test: the band (outer rectangle touches the tile, and the tile is not wholly inside the inner one) or the bar
  const bool outer = X1 - h <= tx1 && X2 + h >= tx0 && Y1 - h <= ty1 && Y2 + h >= ty0;
  const bool inside = tx0 >= X1 + g && tx1 <= X2 - g && ty0 >= Y1 + g && ty1 <= Y2 - g;
  const bool bar = nch > 0 && X1 - h <= tx1 && X1 - h + 6 * nch >= tx0 && by <= ty1 && by + 8 >= ty0;
  if (!((outer && !inside) || bar)) return false;
  unsigned c0 = 0, c1 = 0;
  if (a.labels) {
    int n = 0;
    put_number(c0, c1, n, number);
    if (!gt_form) {
      const int hund = (int)fminf(fmaxf(v * 100.f + 0.5f, 0.f), 100.f);
      put_char(c0, c1, n, 11u);
      put_char(c0, c1, n, (unsigned)(hund / 100));
      put_char(c0, c1, n, 10u);
      put_char(c0, c1, n, (unsigned)(hund / 10 % 10));
      put_char(c0, c1, n, (unsigned)(hund % 10));
    }
  }
  int ci = r < a.n_color_index ? a.color_index[r] : slot;
  ci %= a.n_colors;
  if (ci < 0) ci += a.n_colors;
  const unsigned R = a.colors[ci * 3], G = a.colors[ci * 3 + 1], B = a.colors[ci * 3 + 2];
  const unsigned white = (299u * R + 587u * G + 114u * B) / 1000u >= 128u ? 0u : 1u;
  hh.x1 = X1;
  hh.y1 = Y1;
  hh.x2 = X2;
  hh.y2 = Y2;
  hh.by = by;
  hh.nch = nch;
  hh.col = R | G << 8 | B << 16 | white << 24;
  hh.c0 = c0;
  hh.c1 = c1;
  return true;
}

// One workgroup per (tile, image). The image's rows are walked in painting order, topmost first (top = "last": from the
// end), DB_THREADS at a time: a lane tests one row against the tile; the survivors are appended to the LDS list in walk
// order (ballot + prefix popcount inside a wave, the waves' totals across them). When a chunk would not fit, the list is
// painted first and emptied. Painting: a thread scans the list for its DB_PX pixels and keeps the FIRST hit of each, so
// a pixel settled by an earlier fill of the list is never repainted. Stores: the touched pixels, once, at the end.
__global__ void __launch_bounds__(DB_THREADS)
draw_boxes_kernel(const DrawArgs a) {
  __shared__ Hit s_hit[DB_CAP];
  __shared__ int s_pref[DB_LISTS + 1];
  __shared__ int s_off[DB_LISTS];
  __shared__ int s_scan[DB_THREADS];
  __shared__ int s_wave[DB_THREADS / 64];
  __shared__ unsigned char s_font[12 * 8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z;
  const int tx0 = blockIdx.x * DB_TW, ty0 = blockIdx.y * DB_TH;
  const int tx1 = min(tx0 + DB_TW, a.width) - 1, ty1 = min(ty0 + DB_TH, a.height) - 1;
  const int px0 = tx0 + (tid % (DB_TW / DB_PX)) * DB_PX, py = ty0 + tid / (DB_TW / DB_PX);
  const int t = a.thickness, h = t / 2, g = t - h;
  if (a.labels && tid < 12 * 7) s_font[tid / 7 * 8 + tid % 7] = a.font[tid];  // (published by the scan's barriers)

  unsigned pending = 0;  // bit k: pixel (px0 + k, py) is on the canvas and nothing has covered it yet
  if (py < a.height)
    for (int k = 0; k < DB_PX; ++k)
      if (px0 + k < a.width) pending |= 1u << k;
  unsigned hit_mask = 0, color[DB_PX] = {0, 0, 0, 0};

  auto paint = [&](int cnt) {
    for (int e = 0; e < cnt && pending; ++e) {
      const Hit q = s_hit[e];  // (every lane reads the same entry: an LDS broadcast)
      const int bx = q.x1 - h;
      const int y_lo = q.nch > 0 ? min(q.y1 - h, q.by) : q.y1 - h, y_hi = q.nch > 0 ? max(q.y2 + h, q.by + 8) : q.y2 + h;
      if (py < y_lo || py > y_hi) continue;
      const bool band_y = py >= q.y1 - h && py <= q.y2 + h, inner_y = py >= q.y1 + g && py <= q.y2 - g;
      const bool bar_y = q.nch > 0 && py >= q.by && py < q.by + 9;
      const int gy = py - q.by - 1;  // glyph row
#pragma unroll
      for (int k = 0; k < DB_PX; ++k) {
        if (!(pending >> k & 1u)) continue;
        const int px = px0 + k;
        unsigned c = q.col & 0xffffffu;
        bool covered = false;
        if (bar_y && px >= bx && px <= bx + 6 * q.nch) {
          covered = true;
          const int gx = px - bx - 1;
          if (gx >= 0 && gy >= 0 && gy < 7) {
            const int cell = gx / 6, colx = gx % 6;
            if (cell < q.nch && colx < 5) {
              const unsigned ch = (cell < 8 ? q.c0 >> (4 * cell) : q.c1 >> (4 * (cell - 8))) & 15u;
              if (ch < 12u && (s_font[ch * 8 + gy] >> (4 - colx) & 1u)) c = (q.col >> 24) ? 0xffffffu : 0u;
            }
          }
        } else if (band_y && px >= q.x1 - h && px <= q.x2 + h) {
          covered = !(inner_y && px >= q.x1 + g && px <= q.x2 - g);
        }
        if (covered) {
          pending &= ~(1u << k);
          hit_mask |= 1u << k;
          color[k] = c;
        }
      }
    }
  };

  const bool layout_form = a.counts != nullptr;
  const int L = a.lists;
  const int n_batches = (L + DB_LISTS - 1) / DB_LISTS;
  int cnt = 0;  // boxes in the list: the same value in every thread
  for (int bi = 0; bi < n_batches; ++bi) {
    const int l0 = (a.top_last ? n_batches - 1 - bi : bi) * DB_LISTS;
    const int nl = min(DB_LISTS, L - l0);
    // counts of lists l0 .. l0 + nl - 1 of this image and their running sum
    int c = 0, off = 0;
    if (tid < nl) {
      const long p = (long)b * L + l0 + tid;
      if (layout_form) {
        c = a.counts[p];
        off = a.offsets[p];
      } else {
        c = min(a.num_boxes[b], a.per_image);
        off = b * a.per_image;
      }
      c = (int)min((long)max(c, 0), a.n_rows);
    }
    s_off[tid] = off;
    s_scan[tid] = c;
    __syncthreads();
    for (int o = 1; o < nl; o <<= 1) {  // (entries at and beyond nl are zero and are not needed)
      const int v = tid >= o ? s_scan[tid - o] : 0;
      __syncthreads();
      s_scan[tid] += v;
      __syncthreads();
    }
    s_pref[tid + 1] = s_scan[tid];
    if (tid == 0) s_pref[0] = 0;
    __syncthreads();
    const int T = s_pref[nl];
    for (int base = 0; base < T; base += DB_THREADS) {
      const int i = base + tid;
      bool keep = false;
      Hit hh;
      if (i < T) {
        const int k = a.top_last ? T - 1 - i : i;
        int lo = 0, hi = nl;  // the list that holds the batch's k-th row: the largest s with s_pref[s] <= k
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (s_pref[mid] <= k) lo = mid;
          else hi = mid;
        }
        keep = make_hit(a, (long)s_off[lo] + (k - s_pref[lo]), b, l0 + lo, tx0, ty0, tx1, ty1, hh);
      }
      const unsigned long long m = __ballot(keep);
      if (lane == 0) s_wave[wave] = __popcll(m);
      __syncthreads();
      int total = 0, wbase = 0;
#pragma unroll
      for (int w = 0; w < DB_THREADS / 64; ++w) {
        const int n = s_wave[w];
        total += n;
        if (w < wave) wbase += n;
      }
      if (cnt + total > DB_CAP) {  // (uniform: every thread computed the same cnt and total)
        paint(cnt);
        cnt = 0;
      }
      __syncthreads();  // painted before the list is overwritten; s_wave read before the next chunk writes it
      if (keep) s_hit[cnt + wbase + __popcll(m & ((1ull << lane) - 1ull))] = hh;
      cnt += total;
      __syncthreads();
    }
  }
  paint(cnt);
  if (hit_mask) {
    unsigned char* o = a.canvas + (((long)b * a.height + py) * a.width + px0) * 3;
#pragma unroll
    for (int k = 0; k < DB_PX; ++k)
      if (hit_mask >> k & 1u) {
        o[k * 3] = (unsigned char)(color[k] & 255u);
        o[k * 3 + 1] = (unsigned char)(color[k] >> 8 & 255u);
        o[k * 3 + 2] = (unsigned char)(color[k] >> 16 & 255u);
      }
  }
}

// ---- sheet -----------------------------------------------------------------------------------------------------------------

// out [n][H][W + cols * (pad + side)][3]: x < W the query; shot s at x = W + pad + (s / rpc) * (side + pad),
// y = (s % rpc) * (side + pad), resized to side x side: per channel, in fp32,
//   h0 = p[y0][x0] * ax0 + p[y0][x1] * ax1, h1 = p[y1][x0] * ax0 + p[y1][x1] * ax1, v = h0 * ay0 + h1 * ay1,
//   byte = (unsigned char)(clamp(v, 0, 255) + 0.5); everything else pad_value.
__global__ void __launch_bounds__(256)
sheet_kernel(const unsigned char* __restrict__ query, const unsigned char* __restrict__ supports,
             unsigned char* __restrict__ out, long total, int H, int W, int S, int hs, int ws, int side, int pad, int rpc,
             int out_w, unsigned char pad_value, double scale_y, double scale_x) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % out_w);
  const long ny = i / out_w;
  const int y = (int)(ny % H);
  const long n = ny / H;
  unsigned char* o = out + i * 3;
  if (x < W) {
    const unsigned char* q = query + ((n * H + y) * W + x) * 3;
    o[0] = q[0];
    o[1] = q[1];
    o[2] = q[2];
    return;
  }
  const int cell = side + pad, xs = x - W - pad;
  const int col = xs >= 0 ? xs / cell : 0, cx = xs >= 0 ? xs % cell : side, row = y / cell, cy = y % cell;
  const int s = col * rpc + row;
  if (cx >= side || cy >= side || row >= rpc || s >= S) {
    o[0] = o[1] = o[2] = pad_value;
    return;
  }
  const DanaTap tx = dana_linear_tap(cx, scale_x, ws), ty = dana_linear_tap(cy, scale_y, hs);
  const unsigned char* p = supports + (n * S + s) * (long)hs * ws * 3;
  const unsigned char* r0 = p + (long)ty.s0 * ws * 3;
  const unsigned char* r1 = p + (long)ty.s1 * ws * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float h0 = (float)r0[tx.s0 * 3 + c] * tx.a0 + (float)r0[tx.s1 * 3 + c] * tx.a1;
    const float h1 = (float)r1[tx.s0 * 3 + c] * tx.a0 + (float)r1[tx.s1 * 3 + c] * tx.a1;
    o[c] = (unsigned char)(fminf(fmaxf(h0 * ty.a0 + h1 * ty.a1, 0.f), 255.f) + 0.5f);
  }
}

}  // namespace

extern "C" {

int dana_render_to_rgb(const float* images, void* out, long n_images, int height, int width, float mean_b, float mean_g,
                       float mean_r, dana_stream_t stream) {
  DANA_CHECK_ARG(n_images >= 0 && height > 0 && width > 0, "dana_render_to_rgb: bad shape images=%ld %dx%d", n_images,
                 height, width);
  if (n_images == 0) return DANA_OK;
  DANA_CHECK_ARG(images && out, "dana_render_to_rgb: null pointer");
  const long pix = (long)height * width;
  DANA_CHECK_ARG(n_images <= (long)INT_MAX * 256 / pix - 1, "dana_render_to_rgb: %ld x %ld pixels", n_images, pix);
  const long total = n_images * pix;
  to_rgb_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(images, (unsigned char*)out, n_images, pix,
                                                                                 mean_b, mean_g, mean_r);
  DANA_CHECK_LAUNCH("dana_render_to_rgb");
  return DANA_OK;
}

int dana_render_draw_boxes(void* canvas, int n_images, int height, int width, const float* boxes, int row_ld, long n_rows,
                           const int* counts, const int* offsets, int lists_per_image, const int* num_boxes,
                           int per_image, const float* scale_dev, float scale, int thickness, int use_min_score,
                           float min_score, const unsigned char* colors, int n_colors, const int* color_index,
                           long n_color_index, const unsigned char* font, int labels, int top_last,
                           dana_stream_t stream) {
  DANA_CHECK_ARG(n_images >= 0 && n_images <= 65535 && height > 0 && width > 0 && height <= 65535 * DB_TH && width <= (1 << 20),  // (grid.y, grid.z <= 65535)
                 "dana_render_draw_boxes: bad canvas images=%d %dx%d", n_images, height, width);
  DANA_CHECK_ARG(row_ld >= 5 && n_rows >= 0 && n_rows <= (1L << 22), "dana_render_draw_boxes: %ld rows of %d floats", n_rows,
                 row_ld);
  DANA_CHECK_ARG(thickness >= 1 && thickness <= DB_MAX_T, "dana_render_draw_boxes: thickness %d outside 1..%d", thickness,
                 DB_MAX_T);
  DANA_CHECK_ARG(n_colors >= 1 && n_colors <= (1 << 24), "dana_render_draw_boxes: %d colours", n_colors);
  DANA_CHECK_ARG(n_color_index >= 0 && (color_index || n_color_index == 0), "dana_render_draw_boxes: %ld colour indices without a pointer",
                 n_color_index);
  if (counts) {
    DANA_CHECK_ARG(offsets && lists_per_image >= 1 && lists_per_image <= DB_MAX_NUM + 1,
                   "dana_render_draw_boxes: layout form needs offsets and 1..%d lists per image, got %d", DB_MAX_NUM + 1,
                   lists_per_image);
  } else {
    DANA_CHECK_ARG(num_boxes && per_image >= 0 && lists_per_image == 1 && (long)n_images * per_image <= n_rows,
                   "dana_render_draw_boxes: ground-truth form needs num_boxes and %d x %d <= %ld rows", n_images, per_image,
                   n_rows);
  }
  if (n_images == 0) return DANA_OK;
  DANA_CHECK_ARG(canvas && colors && (boxes || n_rows == 0) && (font || !labels), "dana_render_draw_boxes: null pointer");
  DrawArgs a;
  a.canvas = (unsigned char*)canvas;
  a.boxes = boxes;
  a.counts = counts;
  a.offsets = offsets;
  a.num_boxes = num_boxes;
  a.scale_dev = scale_dev;
  a.colors = colors;
  a.color_index = color_index;
  a.font = font;
  a.n_rows = n_rows;
  a.n_color_index = color_index ? n_color_index : 0;
  a.height = height;
  a.width = width;
  a.row_ld = row_ld;
  a.lists = lists_per_image;
  a.per_image = per_image;
  a.thickness = thickness;
  a.use_min_score = use_min_score;
  a.n_colors = n_colors;
  a.labels = labels ? 1 : 0;
  a.top_last = top_last ? 1 : 0;
  a.scale = scale;
  a.min_score = min_score;
  const dim3 grid(dana_ceil_div(width, DB_TW), dana_ceil_div(height, DB_TH), n_images);
  draw_boxes_kernel<<<grid, DB_THREADS, 0, (hipStream_t)stream>>>(a);
  DANA_CHECK_LAUNCH("dana_render_draw_boxes");
  return DANA_OK;
}

int dana_render_sheet(const void* query, const void* supports, void* out, int n_images, int height, int width, int n_shots,
                      int shot_h, int shot_w, int side, int pad, int pad_value, dana_stream_t stream) {
  DANA_CHECK_ARG(n_images >= 0 && height > 0 && width > 0 && n_shots >= 0 && shot_h > 0 && shot_w > 0 && side > 0 &&
                     pad >= 0 && side <= 32768 && pad <= 32768 && n_shots <= 65535,
                 "dana_render_sheet: bad shape images=%d %dx%d shots=%d %dx%d side=%d pad=%d", n_images, height, width,
                 n_shots, shot_h, shot_w, side, pad);
  DANA_CHECK_ARG(side <= height, "dana_render_sheet: side %d > height %d", side, height);
  DANA_CHECK_ARG(pad_value >= 0 && pad_value <= 255, "dana_render_sheet: pad_value %d outside 0..255", pad_value);
  if (n_images == 0) return DANA_OK;
  DANA_CHECK_ARG(query && out && (supports || n_shots == 0), "dana_render_sheet: null pointer");
  const int rpc = (height + pad) / (side + pad) > 1 ? (height + pad) / (side + pad) : 1;
  const long cols = (n_shots + rpc - 1) / rpc;
  const long out_w = width + cols * (pad + side);
  DANA_CHECK_ARG(out_w <= INT_MAX && (long)n_images * height <= ((long)INT_MAX * 256 - 256) / out_w,
                 "dana_render_sheet: %d x %d x %ld output pixels", n_images, height, out_w);
  const long total = (long)n_images * height * out_w;
  sheet_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      (const unsigned char*)query, (const unsigned char*)supports, (unsigned char*)out, total, height, width, n_shots,
      shot_h, shot_w, side, pad, rpc, (int)out_w, (unsigned char)pad_value, (double)shot_h / side, (double)shot_w / side);
  DANA_CHECK_LAUNCH("dana_render_sheet");
  return DANA_OK;
}

}  // extern "C"
