// A batch of episodes assembled from a resident image pool: three launches driven by one plan
// (dana_amd/pipeline.py: ImagePool, plan_episode, EpisodeAssembler) in place of pipeline.hip's per-image launches.
//
//   episode_queries_kernel   im_data [B][3][H][W]: inside the plan's copy window the value prep_image_kernel would have
//                            written at prepared pixel (y_s + y, x_s + x), computed straight from the uint8 source; 0
//                            elsewhere. Also im_info [B][3].
//   episode_supports_kernel  fs_loader.py:116-137 composed: each output pixel evaluates the (up to) four prepared-image
//                            pixels its second bilinear reads, then applies it as crop_resize_pad_kernel does.
//   episode_boxes_kernel     fs_loader.py:183-315 + minibatch.py:52-54: gather, scale, shift, clamp, filter, compact.
//
// The arithmetic is pipeline.hip's, expression for expression (the cv2.resize restatement at its head), and this file is
// compiled with -ffp-contract=off like it: the results have the bits of the per-image path.
//
// The pool: one byte buffer of packed uint8 RGB frames; offsets[row] (bytes), meta[row] = (h, w, flipped, box_off, box_cnt).
// The plan: int32 words. Query record (EP_QWORDS, at q_off + b * EP_QWORDS), support record (EP_SWORDS, at
// s_off + n * EP_SWORDS); doubles sit on even words. The box orders of the queries follow the records.
//
// Training-time augmentation (not in the reference tree): the *_aug entry points launch the same three bodies with AUG set.
// They read a third plan section, one augmentation record (EP_AWORDS) per query and per support: a 3x4 colour map applied
// to each source tap before the mean is subtracted, and for queries the visibility threshold of the box filter. The plain
// entry points instantiate the bodies without it (the new kernel arguments come last and are not read): the same
// arithmetic, the same bits.
//
// Composed queries (not in the reference tree either): the *_composed entry points read one more plan section, a header
// (EP_CWORDS) per query followed by a table of max_parts part records (EP_PWORDS) per query. A part is a query record with
// a destination (dy, dx) in the holder and a colour map of its own; later parts paint over earlier ones and hide their
// boxes. A query that is not composed is one part at (0, 0) with the record it always had, and comes out with the bits of
// the plain or the augmented launch. The kernels above are not touched: the two below are kernels of their own.
#include "common.h"
#include "../../include/dana_hip.h"

namespace {

enum { EP_QWORDS = 16, EP_SWORDS = 16, EP_AWORDS = 16, EP_META = 5 };
// query record
enum { Q_ROW = 0, Q_NORDER = 1, Q_SCALE = 2, Q_INV = 4, Q_YS = 6, Q_XS = 7, Q_COPY_H = 8, Q_COPY_W = 9, Q_CLAMP_X = 10,
       Q_CLAMP_Y = 11, Q_CLS = 12, Q_ORDER_OFF = 13, Q_OH = 14, Q_OW = 15 };
// support record (words 14, 15 of both: the prepared size oh, ow; the host's limits come from it, no kernel reads it)
enum { S_ROW = 0, S_INV = 2, S_SX = 4, S_SY = 6, S_X0 = 8, S_Y0 = 9, S_CW = 10, S_CH = 11, S_RW = 12, S_RH = 13,
       S_OH = 14, S_OW = 15 };
// augmentation record: float M[3][4] (rows R, G, B of the distorted pixel, columns r, g, b of the source and the offset),
// float min_visible, flags
enum { A_M = 0, A_MIN_VISIBLE = 12, A_FLAGS = 13, A_HAS_COLOR = 1, A_HAS_VISIBLE = 2 };

// composed section: per query a header, then per query max_parts part records. A part record starts like a query record
// (row, order length, scale, 1 / scale, window start, painted size, clamp limits), then the destination, the word offset of
// its box order, flags, and float M[3][4] (words 28, 29: the prepared size, for the host; no kernel reads them)
enum { EP_CWORDS = 8, EP_PWORDS = 32, EP_MAX_PARTS = 16 };
enum { C_NPARTS = 0, C_CLS = 1, C_MIN_VISIBLE = 2, C_FLAGS = 3 };
enum { P_ROW = 0, P_NORDER = 1, P_SCALE = 2, P_INV = 4, P_YS = 6, P_XS = 7, P_H = 8, P_W = 9, P_CLAMP_X = 10, P_CLAMP_Y = 11,
       P_DY = 12, P_DX = 13, P_ORDER_OFF = 14, P_FLAGS = 15, P_M = 16 };

__device__ __forceinline__ double plan_double(const int* rec, int word) {
  return *reinterpret_cast<const double*>(rec + word);
}

struct Source {
  const unsigned char* im;
  int h, w, flipped;
};
// a row outside the pool, or a table entry that is no image, reads nothing: the caller writes zeros
__device__ __forceinline__ bool source_of(const unsigned char* pool, const long long* offsets, const int* meta, int n_rows,
                                          long pool_bytes, int row, Source& s) {
  if (row < 0 || row >= n_rows) return false;
  const int* m = meta + (long)row * EP_META;
  const long off = offsets[row];
  s.h = m[0];
  s.w = m[1];
  s.flipped = m[2];
  if (s.h <= 0 || s.w <= 0 || off < 0 || off + (long)s.h * s.w * 3 > pool_bytes) return false;
  s.im = pool + off;
  return true;
}

// the colour map of one augmentation record; `on` is false where the record asks for none
struct Colour {
  bool on;
  float m[12];
};
__device__ __forceinline__ Colour colour_of(const int* arec) {
  Colour col;
  col.on = (arec[A_FLAGS] & A_HAS_COLOR) != 0;
#pragma unroll
  for (int k = 0; k < 12; ++k) col.m[k] = col.on ? __int_as_float(arec[A_M + k]) : 0.f;
  return col;
}

// what the source pixel px (RGB) counts as in input channel ci: the byte itself, or row ci of the colour map at it, clamped
// to the range of a byte (so the map cannot move behind the resample). float32, in this order, uncontracted.
template <bool AUG>
__device__ __forceinline__ float source_value(const unsigned char* px, int ci, const Colour& col) {
  if (!AUG || !col.on) return (float)px[ci];
  const float* k = col.m + ci * 4;
  const float d = ((k[0] * (float)px[0] + k[1] * (float)px[1]) + k[2] * (float)px[2]) + k[3];
  return fminf(fmaxf(d, 0.f), 255.f);
}

// prep_image_kernel's value of channel c (BGR) at the prepared pixel whose taps are (tx, ty)
template <bool AUG>
__device__ __forceinline__ float prep_value(const Source& s, const DanaTap& tx, const DanaTap& ty, int c, float mean,
                                            const Colour& col) {
  const int x0 = s.flipped ? s.w - 1 - tx.s0 : tx.s0, x1 = s.flipped ? s.w - 1 - tx.s1 : tx.s1;
  const unsigned char* r0 = s.im + (long)ty.s0 * s.w * 3;
  const unsigned char* r1 = s.im + (long)ty.s1 * s.w * 3;
  const int ci = 2 - c;  // output channel c (BGR) reads input channel 2 - c (RGB)
  const float t00 = source_value<AUG>(r0 + x0 * 3, ci, col) - mean, t01 = source_value<AUG>(r0 + x1 * 3, ci, col) - mean;
  const float t10 = source_value<AUG>(r1 + x0 * 3, ci, col) - mean, t11 = source_value<AUG>(r1 + x1 * 3, ci, col) - mean;
  const float h0 = t00 * tx.a0 + t01 * tx.a1;
  const float h1 = t10 * tx.a0 + t11 * tx.a1;
  return h0 * ty.a0 + h1 * ty.a1;
}

// plan: the query records; aug (AUG only): the queries' augmentation records
template <bool AUG>
__global__ void __launch_bounds__(256)
episode_queries_kernel(const unsigned char* __restrict__ pool, const long long* __restrict__ offsets,
                       const int* __restrict__ meta, int n_rows, long pool_bytes, const int* __restrict__ plan, int B,
                       float m0, float m1, float m2, float* __restrict__ im_data, int H, int W,
                       float* __restrict__ im_info, const int* __restrict__ aug) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long plane = (long)H * W;
  if (i < B) {  // (H, W, im_scale): EpisodeHolders.put_query's row
    im_info[i * 3 + 0] = (float)H;
    im_info[i * 3 + 1] = (float)W;
    im_info[i * 3 + 2] = (float)plan_double(plan + i * EP_QWORDS, Q_SCALE);
  }
  if (i >= (long)B * plane) return;
  const int b = (int)(i / plane);
  const long p = i % plane;
  const int x = (int)(p % W), y = (int)(p / W);
  const int* rec = plan + (long)b * EP_QWORDS;
  float v[3] = {0.f, 0.f, 0.f};
  Source s;
  if (y < rec[Q_COPY_H] && x < rec[Q_COPY_W] &&
      source_of(pool, offsets, meta, n_rows, pool_bytes, rec[Q_ROW], s)) {
    const double inv = plan_double(rec, Q_INV);
    const DanaTap tx = dana_linear_tap(rec[Q_XS] + x, inv, s.w), ty = dana_linear_tap(rec[Q_YS] + y, inv, s.h);
    const float mean[3] = {m0, m1, m2};
    Colour col;
    col.on = false;
    if (AUG) col = colour_of(aug + (long)b * EP_AWORDS);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = prep_value<AUG>(s, tx, ty, c, mean[c], col);
  }
  float* o = im_data + (long)b * 3 * plane + p;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[(long)c * plane] = v[c];
}

// plan: the support records; aug (AUG only): the supports' augmentation records
template <bool AUG>
__global__ void __launch_bounds__(256)
episode_supports_kernel(const unsigned char* __restrict__ pool, const long long* __restrict__ offsets,
                        const int* __restrict__ meta, int n_rows, long pool_bytes, const int* __restrict__ plan, int N,
                        float m0, float m1, float m2, int target, float* __restrict__ out,
                        const int* __restrict__ aug) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long plane = (long)target * target;
  if (i >= (long)N * plane) return;
  const int n = (int)(i / plane);
  const long p = i % plane;
  const int x = (int)(p % target), y = (int)(p / target);
  const int* rec = plan + (long)n * EP_SWORDS;
  float v[3] = {0.f, 0.f, 0.f};
  Source s;
  if (x < rec[S_RW] && y < rec[S_RH] && rec[S_CW] > 0 && rec[S_CH] > 0 &&
      source_of(pool, offsets, meta, n_rows, pool_bytes, rec[S_ROW], s)) {
    // the second resample (crop_resize_pad_kernel): taps into the crop, whose pixels are prepared-image pixels
    const DanaTap tx = dana_linear_tap(x, plan_double(rec, S_SX), rec[S_CW]), ty = dana_linear_tap(y, plan_double(rec, S_SY), rec[S_CH]);
    // the first resample (prep_image_kernel) at the two prepared columns and two prepared rows those taps name
    const double inv = plan_double(rec, S_INV);
    const int x0 = rec[S_X0], y0 = rec[S_Y0];
    const DanaTap px0 = dana_linear_tap(x0 + tx.s0, inv, s.w), px1 = dana_linear_tap(x0 + tx.s1, inv, s.w);
    const DanaTap py0 = dana_linear_tap(y0 + ty.s0, inv, s.h), py1 = dana_linear_tap(y0 + ty.s1, inv, s.h);
    const float mean[3] = {m0, m1, m2};
    Colour col;
    col.on = false;
    if (AUG) col = colour_of(aug + (long)n * EP_AWORDS);  // at each of the (up to) sixteen source taps below
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float h0 = prep_value<AUG>(s, px0, py0, c, mean[c], col) * tx.a0 + prep_value<AUG>(s, px1, py0, c, mean[c], col) * tx.a1;
      const float h1 = prep_value<AUG>(s, px0, py1, c, mean[c], col) * tx.a0 + prep_value<AUG>(s, px1, py1, c, mean[c], col) * tx.a1;
      v[c] = h0 * ty.a0 + h1 * ty.a1;
    }
  }
  float* o = out + (long)n * 3 * plane + p;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[(long)c * plane] = v[c];
}

// one wavefront per image: 64 boxes of the plan's order per pass, kept boxes compacted in order with a ballot.
// AUG: a record with A_HAS_VISIBLE also drops a box of which the shift and the clamp leave less than min_visible of its area
template <bool AUG>
__global__ void __launch_bounds__(64)
episode_boxes_kernel(const float* __restrict__ boxes, long n_boxes_total, const int* __restrict__ meta, int n_rows,
                     const int* __restrict__ plan, int plan_words, int q_off, int max_num_box,
                     float* __restrict__ gt_boxes, long long* __restrict__ num_boxes, float* __restrict__ all_boxes,
                     long long* __restrict__ all_num_boxes, int a_off) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int* rec = plan + q_off + (long)b * EP_QWORDS;
  const int row = rec[Q_ROW];
  long box_off = 0;
  int box_cnt = 0, n_order = rec[Q_NORDER];
  const long order_off = rec[Q_ORDER_OFF];
  if (row >= 0 && row < n_rows) {
    box_off = meta[(long)row * EP_META + 3];
    box_cnt = meta[(long)row * EP_META + 4];
  }
  if (box_off < 0 || box_cnt < 0 || box_off + box_cnt > n_boxes_total) box_cnt = 0;
  if (n_order < 0 || order_off < 0 || order_off + n_order > plan_words) n_order = 0;
  const double scale = plan_double(rec, Q_SCALE);
  const float xs = (float)rec[Q_XS], ys = (float)rec[Q_YS];
  const int clamp_x = rec[Q_CLAMP_X], clamp_y = rec[Q_CLAMP_Y];
  const float cls = (float)rec[Q_CLS];
  bool visible_rule = false;
  float min_visible = 0.f;
  if (AUG) {
    const int* arec = plan + a_off + (long)b * EP_AWORDS;
    visible_rule = (arec[A_FLAGS] & A_HAS_VISIBLE) != 0;
    min_visible = __int_as_float(arec[A_MIN_VISIBLE]);
  }
  float* fs_out = gt_boxes + (long)b * max_num_box * 5;
  float* all_out = all_boxes + (long)b * max_num_box * 5;
  const unsigned long long below = (1ull << lane) - 1ull;
  int n_fs = 0, n_all = 0;  // wave-uniform
  for (int base = 0; base < n_order && (n_fs < max_num_box || n_all < max_num_box); base += 64) {
    const int k = base + lane;
    const int idx = k < n_order ? plan[order_off + k] : -1;
    bool keep = false, pos = false;
    float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    float u[4] = {0.f, 0.f, 0.f, 0.f};  // the shifted row before the clamp
    if (idx >= 0 && idx < box_cnt) {
      const float* src = boxes + (box_off + idx) * 5;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // minibatch.py:53: the product in double, rounded into the float32 array
        float t = (float)((double)src[j] * scale);
        t = t - ((j & 1) ? ys : xs);  // fs_loader.py:215-216, 251-252
        u[j] = t;
        const int lim = (j & 1) ? clamp_y : clamp_x;
        if (lim >= 0) t = fminf(fmaxf(t, 0.f), (float)lim);  // :219-220, :254-255, :281
        v[j] = t;
      }
      v[4] = src[4];
      keep = !(v[0] == v[2] || v[1] == v[3]);  // :294, :306
      if (AUG && visible_rule) {
        const float full = (u[2] - u[0]) * (u[3] - u[1]), seen = (v[2] - v[0]) * (v[3] - v[1]);
        keep = keep && seen >= min_visible * full;
      }
      pos = keep && v[4] == cls;               // :288
    }
    const unsigned long long m_all = __ballot(keep), m_fs = __ballot(pos);
    const int at_all = n_all + __popcll(m_all & below), at_fs = n_fs + __popcll(m_fs & below);
    if (keep && at_all < max_num_box) {
#pragma unroll
      for (int j = 0; j < 5; ++j) all_out[(long)at_all * 5 + j] = v[j];
    }
    if (pos && at_fs < max_num_box) {
#pragma unroll
      for (int j = 0; j < 4; ++j) fs_out[(long)at_fs * 5 + j] = v[j];
      fs_out[(long)at_fs * 5 + 4] = 1.f;  // :291
    }
    n_all += __popcll(m_all);
    n_fs += __popcll(m_fs);
  }
  n_all = min(n_all, max_num_box);
  n_fs = min(n_fs, max_num_box);
  for (int k = n_all * 5 + lane; k < max_num_box * 5; k += 64) all_out[k] = 0.f;
  for (int k = n_fs * 5 + lane; k < max_num_box * 5; k += 64) fs_out[k] = 0.f;
  if (lane == 0) {
    num_boxes[b] = n_fs;
    all_num_boxes[b] = n_all;
  }
}

// a query's part count as the kernels take it: what the header says, within the table the entry point checked
__device__ __forceinline__ int part_count(const int* head, int max_parts) { return min(max(head[C_NPARTS], 0), max_parts); }

// One thread per holder pixel, blockIdx.y = the query: the query's part table goes into LDS once per workgroup, every
// thread walks the rectangles from the last part down to its owner and evaluates episode_queries_kernel's expressions for
// that part's record at prepared pixel (y_s + y - dy, x_s + x - dx). heads: the section's headers; tables: its part records
__global__ void __launch_bounds__(256)
episode_queries_composed_kernel(const unsigned char* __restrict__ pool, const long long* __restrict__ offsets,
                                const int* __restrict__ meta, int n_rows, long pool_bytes, const int* __restrict__ heads,
                                const int* __restrict__ tables, int max_parts, float m0, float m1, float m2,
                                float* __restrict__ im_data, int H, int W, float* __restrict__ im_info) {
  __shared__ __attribute__((aligned(8))) int tab[EP_MAX_PARTS * EP_PWORDS];
  const int b = blockIdx.y;
  const int n_parts = part_count(heads + (long)b * EP_CWORDS, max_parts);
  const int* table = tables + (long)b * max_parts * EP_PWORDS;
  for (int k = threadIdx.x; k < n_parts * EP_PWORDS; k += blockDim.x) tab[k] = table[k];
  __syncthreads();
  const long plane = (long)H * W;
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p == 0) {  // (H, W, im_scale of part 0)
    im_info[b * 3 + 0] = (float)H;
    im_info[b * 3 + 1] = (float)W;
    im_info[b * 3 + 2] = n_parts > 0 ? (float)plan_double(tab, P_SCALE) : 0.f;
  }
  if (p >= plane) return;
  const int x = (int)(p % W), y = (int)(p / W);
  int owner = -1;
  for (int r = n_parts - 1; r >= 0; --r) {
    const int* rec = tab + r * EP_PWORDS;
    const int ry = y - rec[P_DY], rx = x - rec[P_DX];
    if (ry >= 0 && ry < rec[P_H] && rx >= 0 && rx < rec[P_W]) {
      owner = r;
      break;
    }
  }
  float v[3] = {0.f, 0.f, 0.f};
  Source s;
  if (owner >= 0) {
    const int* rec = tab + owner * EP_PWORDS;
    if (source_of(pool, offsets, meta, n_rows, pool_bytes, rec[P_ROW], s)) {
      const double inv = plan_double(rec, P_INV);
      const DanaTap tx = dana_linear_tap(rec[P_XS] + (x - rec[P_DX]), inv, s.w);
      const DanaTap ty = dana_linear_tap(rec[P_YS] + (y - rec[P_DY]), inv, s.h);
      const float mean[3] = {m0, m1, m2};
      Colour col;
      col.on = (rec[P_FLAGS] & A_HAS_COLOR) != 0;
#pragma unroll
      for (int k = 0; k < 12; ++k) col.m[k] = col.on ? __int_as_float(rec[P_M + k]) : 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = prep_value<true>(s, tx, ty, c, mean[c], col);
    }
  }
  float* o = im_data + (long)b * 3 * plane + p;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[(long)c * plane] = v[c];
}

// One wavefront per query: the parts in order, 64 boxes of a part's order per pass; the running counts of the ballot
// compaction carry across passes and parts. A box of part p: u, v as episode_boxes_kernel has them, the output row v moved
// to the part's destination, hidden = the sum over the later parts r of the area their rectangles cover of that row.
__global__ void __launch_bounds__(64)
episode_boxes_composed_kernel(const float* __restrict__ boxes, long n_boxes_total, const int* __restrict__ meta, int n_rows,
                              const int* __restrict__ plan, int plan_words, int c_off, int batch, int max_parts,
                              int max_num_box, float* __restrict__ gt_boxes, long long* __restrict__ num_boxes,
                              float* __restrict__ all_boxes, long long* __restrict__ all_num_boxes) {
  __shared__ float rect[EP_MAX_PARTS * 4];  // D_r = [dx, dx + w - 1] x [dy, dy + h - 1] as floats: x1, y1, x2, y2
  const int b = blockIdx.x, lane = threadIdx.x;
  const int* head = plan + c_off + (long)b * EP_CWORDS;
  const int* table = plan + c_off + (long)batch * EP_CWORDS + (long)b * max_parts * EP_PWORDS;
  const int n_parts = part_count(head, max_parts);
  if (lane < n_parts) {
    const int* rec = table + lane * EP_PWORDS;
    rect[lane * 4 + 0] = (float)rec[P_DX];
    rect[lane * 4 + 1] = (float)rec[P_DY];
    rect[lane * 4 + 2] = (float)(rec[P_DX] + rec[P_W] - 1);
    rect[lane * 4 + 3] = (float)(rec[P_DY] + rec[P_H] - 1);
  }
  __syncthreads();
  const float cls = (float)head[C_CLS];
  const bool visible_rule = (head[C_FLAGS] & A_HAS_VISIBLE) != 0;
  const float min_visible = __int_as_float(head[C_MIN_VISIBLE]);
  float* fs_out = gt_boxes + (long)b * max_num_box * 5;
  float* all_out = all_boxes + (long)b * max_num_box * 5;
  const unsigned long long below = (1ull << lane) - 1ull;
  int n_fs = 0, n_all = 0;  // wave-uniform
  for (int part = 0; part < n_parts; ++part) {
    const int* rec = table + part * EP_PWORDS;
    const int row = rec[P_ROW];
    long box_off = 0;
    int box_cnt = 0, n_order = rec[P_NORDER];
    const long order_off = rec[P_ORDER_OFF];
    if (row >= 0 && row < n_rows) {
      box_off = meta[(long)row * EP_META + 3];
      box_cnt = meta[(long)row * EP_META + 4];
    }
    if (box_off < 0 || box_cnt < 0 || box_off + box_cnt > n_boxes_total) box_cnt = 0;
    if (n_order < 0 || order_off < 0 || order_off + n_order > plan_words) n_order = 0;
    const double scale = plan_double(rec, P_SCALE);
    const float xs = (float)rec[P_XS], ys = (float)rec[P_YS];
    const int clamp_x = rec[P_CLAMP_X], clamp_y = rec[P_CLAMP_Y];
    const float dx = (float)rec[P_DX], dy = (float)rec[P_DY];
    for (int base = 0; base < n_order && (n_fs < max_num_box || n_all < max_num_box); base += 64) {
      const int k = base + lane;
      const int idx = k < n_order ? plan[order_off + k] : -1;
      bool keep = false, pos = false;
      float t[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
      if (idx >= 0 && idx < box_cnt) {
        const float* src = boxes + (box_off + idx) * 5;
        float u[4], v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          // as episode_boxes_kernel: the product in double, rounded into float32, shifted, clamped
          float c = (float)((double)src[j] * scale);
          c = c - ((j & 1) ? ys : xs);
          u[j] = c;
          const int lim = (j & 1) ? clamp_y : clamp_x;
          if (lim >= 0) c = fminf(fmaxf(c, 0.f), (float)lim);
          v[j] = c;
          t[j] = c + ((j & 1) ? dy : dx);
        }
        t[4] = src[4];
        keep = !(v[0] == v[2] || v[1] == v[3]);  // on v: the translation could merge distinct values
        if (visible_rule) {
          float hidden = 0.f;
          for (int r = part + 1; r < n_parts; ++r) {  // wave-uniform records
            const float ox = fmaxf(fminf(t[2], rect[r * 4 + 2]) - fmaxf(t[0], rect[r * 4 + 0]), 0.f);
            const float oy = fmaxf(fminf(t[3], rect[r * 4 + 3]) - fmaxf(t[1], rect[r * 4 + 1]), 0.f);
            hidden = hidden + ox * oy;
          }
          const float full = (u[2] - u[0]) * (u[3] - u[1]), seen = (v[2] - v[0]) * (v[3] - v[1]);
          keep = keep && (seen - hidden) >= min_visible * full;
        }
        pos = keep && t[4] == cls;
      }
      const unsigned long long m_all = __ballot(keep), m_fs = __ballot(pos);
      const int at_all = n_all + __popcll(m_all & below), at_fs = n_fs + __popcll(m_fs & below);
      if (keep && at_all < max_num_box) {
#pragma unroll
        for (int j = 0; j < 5; ++j) all_out[(long)at_all * 5 + j] = t[j];
      }
      if (pos && at_fs < max_num_box) {
#pragma unroll
        for (int j = 0; j < 4; ++j) fs_out[(long)at_fs * 5 + j] = t[j];
        fs_out[(long)at_fs * 5 + 4] = 1.f;
      }
      n_all += __popcll(m_all);
      n_fs += __popcll(m_fs);
    }
  }
  n_all = min(n_all, max_num_box);
  n_fs = min(n_fs, max_num_box);
  for (int k = n_all * 5 + lane; k < max_num_box * 5; k += 64) all_out[k] = 0.f;
  for (int k = n_fs * 5 + lane; k < max_num_box * 5; k += 64) fs_out[k] = 0.f;
  if (lane == 0) {
    num_boxes[b] = n_fs;
    all_num_boxes[b] = n_all;
  }
}

// `count` augmentation records at a_off: on an even word like the other sections, and inside the plan
bool aug_fits(int a_off, long count, int plan_words) {
  return a_off >= 0 && a_off % 2 == 0 && (long)a_off + count * EP_AWORDS <= plan_words;
}

// the composed section at c_off: `batch` headers, then `batch` tables of max_parts part records
bool composed_fits(int c_off, long batch, int max_parts, int plan_words) {
  return c_off >= 0 && (long)c_off + batch * EP_CWORDS + batch * max_parts * EP_PWORDS <= plan_words;
}

}  // namespace

extern "C" {

int dana_episode_queries(const unsigned char* pool, long pool_bytes, const long long* offsets, const int* meta,
                         int n_rows, const int* plan, int plan_words, int q_off, int batch,
                         const float* pixel_means_bgr, float* im_data, int height, int width, float* im_info,
                         dana_stream_t stream) {
  DANA_CHECK_ARG(batch > 0 && height > 0 && width > 0 && n_rows > 0 && pool_bytes > 0, "dana_episode_queries: bad shape");
  DANA_CHECK_ARG(q_off >= 0 && q_off % 2 == 0 && (long)q_off + (long)batch * EP_QWORDS <= plan_words,
                 "dana_episode_queries: the query records do not fit the plan");
  DANA_CHECK_ARG(pool && offsets && meta && plan && pixel_means_bgr && im_data && im_info,
                 "dana_episode_queries: null pointer");
  const long blocks = ((long)batch * height * width + 255) / 256;
  DANA_CHECK_ARG(blocks <= 0x7fffffffL, "dana_episode_queries: too many pixels for one launch");
  episode_queries_kernel<false><<<(int)blocks, 256, 0, (hipStream_t)stream>>>(
      pool, offsets, meta, n_rows, pool_bytes, plan + q_off, batch, pixel_means_bgr[0], pixel_means_bgr[1],
      pixel_means_bgr[2], im_data, height, width, im_info, nullptr);
  DANA_CHECK_LAUNCH("dana_episode_queries");
  return DANA_OK;
}

int dana_episode_queries_aug(const unsigned char* pool, long pool_bytes, const long long* offsets, const int* meta,
                             int n_rows, const int* plan, int plan_words, int q_off, int a_off, int batch,
                             const float* pixel_means_bgr, float* im_data, int height, int width, float* im_info,
                             dana_stream_t stream) {
  DANA_CHECK_ARG(batch > 0 && height > 0 && width > 0 && n_rows > 0 && pool_bytes > 0,
                 "dana_episode_queries_aug: bad shape");
  DANA_CHECK_ARG(q_off >= 0 && q_off % 2 == 0 && (long)q_off + (long)batch * EP_QWORDS <= plan_words,
                 "dana_episode_queries_aug: the query records do not fit the plan");
  DANA_CHECK_ARG(aug_fits(a_off, batch, plan_words),
                 "dana_episode_queries_aug: the augmentation records do not fit the plan");
  DANA_CHECK_ARG(pool && offsets && meta && plan && pixel_means_bgr && im_data && im_info,
                 "dana_episode_queries_aug: null pointer");
  const long blocks = ((long)batch * height * width + 255) / 256;
  DANA_CHECK_ARG(blocks <= 0x7fffffffL, "dana_episode_queries_aug: too many pixels for one launch");
  episode_queries_kernel<true><<<(int)blocks, 256, 0, (hipStream_t)stream>>>(
      pool, offsets, meta, n_rows, pool_bytes, plan + q_off, batch, pixel_means_bgr[0], pixel_means_bgr[1],
      pixel_means_bgr[2], im_data, height, width, im_info, plan + a_off);
  DANA_CHECK_LAUNCH("dana_episode_queries_aug");
  return DANA_OK;
}

int dana_episode_supports(const unsigned char* pool, long pool_bytes, const long long* offsets, const int* meta,
                          int n_rows, const int* plan, int plan_words, int s_off, int n_supports,
                          const float* pixel_means_bgr, int target, float* out_chw, dana_stream_t stream) {
  DANA_CHECK_ARG(n_supports > 0 && target > 0 && n_rows > 0 && pool_bytes > 0, "dana_episode_supports: bad shape");
  DANA_CHECK_ARG(s_off >= 0 && s_off % 2 == 0 && (long)s_off + (long)n_supports * EP_SWORDS <= plan_words,
                 "dana_episode_supports: the support records do not fit the plan");
  DANA_CHECK_ARG(pool && offsets && meta && plan && pixel_means_bgr && out_chw, "dana_episode_supports: null pointer");
  const long blocks = ((long)n_supports * target * target + 255) / 256;
  DANA_CHECK_ARG(blocks <= 0x7fffffffL, "dana_episode_supports: too many pixels for one launch");
  episode_supports_kernel<false><<<(int)blocks, 256, 0, (hipStream_t)stream>>>(
      pool, offsets, meta, n_rows, pool_bytes, plan + s_off, n_supports, pixel_means_bgr[0], pixel_means_bgr[1],
      pixel_means_bgr[2], target, out_chw, nullptr);
  DANA_CHECK_LAUNCH("dana_episode_supports");
  return DANA_OK;
}

int dana_episode_supports_aug(const unsigned char* pool, long pool_bytes, const long long* offsets, const int* meta,
                              int n_rows, const int* plan, int plan_words, int s_off, int a_off, int n_supports,
                              const float* pixel_means_bgr, int target, float* out_chw, dana_stream_t stream) {
  DANA_CHECK_ARG(n_supports > 0 && target > 0 && n_rows > 0 && pool_bytes > 0, "dana_episode_supports_aug: bad shape");
  DANA_CHECK_ARG(s_off >= 0 && s_off % 2 == 0 && (long)s_off + (long)n_supports * EP_SWORDS <= plan_words,
                 "dana_episode_supports_aug: the support records do not fit the plan");
  DANA_CHECK_ARG(aug_fits(a_off, n_supports, plan_words),
                 "dana_episode_supports_aug: the augmentation records do not fit the plan");
  DANA_CHECK_ARG(pool && offsets && meta && plan && pixel_means_bgr && out_chw,
                 "dana_episode_supports_aug: null pointer");
  const long blocks = ((long)n_supports * target * target + 255) / 256;
  DANA_CHECK_ARG(blocks <= 0x7fffffffL, "dana_episode_supports_aug: too many pixels for one launch");
  episode_supports_kernel<true><<<(int)blocks, 256, 0, (hipStream_t)stream>>>(
      pool, offsets, meta, n_rows, pool_bytes, plan + s_off, n_supports, pixel_means_bgr[0], pixel_means_bgr[1],
      pixel_means_bgr[2], target, out_chw, plan + a_off);
  DANA_CHECK_LAUNCH("dana_episode_supports_aug");
  return DANA_OK;
}

int dana_episode_boxes(const float* boxes, long n_boxes_total, const int* meta, int n_rows, const int* plan,
                       int plan_words, int q_off, int batch, int max_num_box, float* gt_boxes, long long* num_boxes,
                       float* all_cls_gt_boxes, long long* all_cls_num_boxes, dana_stream_t stream) {
  DANA_CHECK_ARG(batch > 0 && max_num_box > 0 && n_rows > 0 && n_boxes_total >= 0, "dana_episode_boxes: bad shape");
  DANA_CHECK_ARG(q_off >= 0 && q_off % 2 == 0 && (long)q_off + (long)batch * EP_QWORDS <= plan_words,
                 "dana_episode_boxes: the query records do not fit the plan");
  DANA_CHECK_ARG(meta && plan && gt_boxes && num_boxes && all_cls_gt_boxes && all_cls_num_boxes &&
                     (boxes || n_boxes_total == 0),
                 "dana_episode_boxes: null pointer");
  episode_boxes_kernel<false><<<batch, 64, 0, (hipStream_t)stream>>>(boxes, n_boxes_total, meta, n_rows, plan, plan_words,
                                                                     q_off, max_num_box, gt_boxes, num_boxes,
                                                                     all_cls_gt_boxes, all_cls_num_boxes, 0);
  DANA_CHECK_LAUNCH("dana_episode_boxes");
  return DANA_OK;
}

int dana_episode_boxes_aug(const float* boxes, long n_boxes_total, const int* meta, int n_rows, const int* plan,
                           int plan_words, int q_off, int a_off, int batch, int max_num_box, float* gt_boxes,
                           long long* num_boxes, float* all_cls_gt_boxes, long long* all_cls_num_boxes,
                           dana_stream_t stream) {
  DANA_CHECK_ARG(batch > 0 && max_num_box > 0 && n_rows > 0 && n_boxes_total >= 0, "dana_episode_boxes_aug: bad shape");
  DANA_CHECK_ARG(q_off >= 0 && q_off % 2 == 0 && (long)q_off + (long)batch * EP_QWORDS <= plan_words,
                 "dana_episode_boxes_aug: the query records do not fit the plan");
  DANA_CHECK_ARG(aug_fits(a_off, batch, plan_words),
                 "dana_episode_boxes_aug: the augmentation records do not fit the plan");
  DANA_CHECK_ARG(meta && plan && gt_boxes && num_boxes && all_cls_gt_boxes && all_cls_num_boxes &&
                     (boxes || n_boxes_total == 0),
                 "dana_episode_boxes_aug: null pointer");
  episode_boxes_kernel<true><<<batch, 64, 0, (hipStream_t)stream>>>(boxes, n_boxes_total, meta, n_rows, plan, plan_words,
                                                                    q_off, max_num_box, gt_boxes, num_boxes,
                                                                    all_cls_gt_boxes, all_cls_num_boxes, a_off);
  DANA_CHECK_LAUNCH("dana_episode_boxes_aug");
  return DANA_OK;
}

int dana_episode_queries_composed(const unsigned char* pool, long pool_bytes, const long long* offsets, const int* meta,
                                  int n_rows, const int* plan, int plan_words, int c_off, int max_parts, int batch,
                                  const float* pixel_means_bgr, float* im_data, int height, int width, float* im_info,
                                  dana_stream_t stream) {
  DANA_CHECK_ARG(batch > 0 && height > 0 && width > 0 && n_rows > 0 && pool_bytes > 0,
                 "dana_episode_queries_composed: bad shape");
  DANA_CHECK_ARG(max_parts >= 1 && max_parts <= EP_MAX_PARTS, "dana_episode_queries_composed: a part count outside 1..16");
  DANA_CHECK_ARG(c_off >= 0 && c_off % 2 == 0, "dana_episode_queries_composed: the composed section starts on an odd word");
  DANA_CHECK_ARG(composed_fits(c_off, batch, max_parts, plan_words),
                 "dana_episode_queries_composed: the composed section does not fit the plan");
  DANA_CHECK_ARG(pool && offsets && meta && plan && pixel_means_bgr && im_data && im_info,
                 "dana_episode_queries_composed: null pointer");
  const long blocks = ((long)height * width + 255) / 256;
  DANA_CHECK_ARG(blocks <= 0x7fffffffL && batch <= 65535, "dana_episode_queries_composed: too many pixels for one launch");
  episode_queries_composed_kernel<<<dim3((unsigned)blocks, (unsigned)batch), 256, 0, (hipStream_t)stream>>>(
      pool, offsets, meta, n_rows, pool_bytes, plan + c_off, plan + c_off + (long)batch * EP_CWORDS, max_parts,
      pixel_means_bgr[0], pixel_means_bgr[1], pixel_means_bgr[2], im_data, height, width, im_info);
  DANA_CHECK_LAUNCH("dana_episode_queries_composed");
  return DANA_OK;
}

int dana_episode_boxes_composed(const float* boxes, long n_boxes_total, const int* meta, int n_rows, const int* plan,
                                int plan_words, int c_off, int max_parts, int batch, int max_num_box, float* gt_boxes,
                                long long* num_boxes, float* all_cls_gt_boxes, long long* all_cls_num_boxes,
                                dana_stream_t stream) {
  DANA_CHECK_ARG(batch > 0 && max_num_box > 0 && n_rows > 0 && n_boxes_total >= 0,
                 "dana_episode_boxes_composed: bad shape");
  DANA_CHECK_ARG(max_parts >= 1 && max_parts <= EP_MAX_PARTS, "dana_episode_boxes_composed: a part count outside 1..16");
  DANA_CHECK_ARG(c_off >= 0 && c_off % 2 == 0, "dana_episode_boxes_composed: the composed section starts on an odd word");
  DANA_CHECK_ARG(composed_fits(c_off, batch, max_parts, plan_words),
                 "dana_episode_boxes_composed: the composed section does not fit the plan");
  DANA_CHECK_ARG(meta && plan && gt_boxes && num_boxes && all_cls_gt_boxes && all_cls_num_boxes &&
                     (boxes || n_boxes_total == 0),
                 "dana_episode_boxes_composed: null pointer");
  episode_boxes_composed_kernel<<<batch, 64, 0, (hipStream_t)stream>>>(boxes, n_boxes_total, meta, n_rows, plan, plan_words,
                                                                       c_off, batch, max_parts, max_num_box, gt_boxes,
                                                                       num_boxes, all_cls_gt_boxes, all_cls_num_boxes);
  DANA_CHECK_LAUNCH("dana_episode_boxes_composed");
  return DANA_OK;
}

}  // extern "C"
