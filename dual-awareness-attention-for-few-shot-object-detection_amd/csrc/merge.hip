// Merging detection lists on the device: utils.py:182-204 (generate_pseudo_label: cat the per-shot lists, sort by score,
// one more NMS over the union) and the `max_per_image` cut of a Faster R-CNN test loop (inference.py:70), as one call over
// n_lists independent problems; and the step from a detection list to the gt_boxes / num_boxes tensors a train-mode
// forward takes (fs_loader.py:325), so that pseudo-labels never leave the device.
//
//   merge_scatter_kernel   the `groups` input lists of output list l, concatenated in group order into row l of a padded
//                          frame [n_lists][capacity]; padding rows get score -inf: they sort behind every real row (the sort
//                          is stable and they sit behind them in the frame too), so they can never suppress one
//   dana_sort_desc / dana_gather_boxes / dana_nms over the n_lists frame rows: the sort and NMS of post-processing, unchanged
//   merge_compact_kernel   the kept real rows (the prefix of keep[l] below the list's row count), cut at max_dets, packed in
//                          list order with the source (group, row) of every output row -- dets_compact_kernel's pattern
//   dets_to_gt_kernel      one workgroup per image: ordered compaction of the rows with score > thresh (ballot + popcount
//                          inside a wave, four wave totals through LDS), scaled by im_info[b][2], labelled, zero-padded
//
// Rows are only ever copied (bit for bit); the one arithmetic line is the fp32 multiply of dets_to_gt_kernel, compiled with
// -ffp-contract=off like the other byte-parity kernels.
//
// dana_detect_merge_soft puts two more steps beside the hard NMS (neither is in the reference; both are restated from
// their papers, DESIGN.md "Soft-NMS and box voting"):
//   merge_soft_kernel      Soft-NMS (Bodla et al. 2017), one workgroup per list: the concatenation's boxes, working scores
//                          and live flags stay in LDS for the whole loop. A pass = workgroup argmax of the live working
//                          scores (ties to the lowest concatenation index: shuffle reduction inside a wave, the four wave
//                          winners through LDS), then every thread decays the rows it owns against the picked box. It
//                          writes its emissions in the form merge_compact_kernel reads (sorted_* / order / keep / num_keep),
//                          so the compaction is shared with the hard path.
//   merge_vote_kernel      box voting (Gidaris & Komodakis 2015), one thread per emitted row: the list's concatenation goes
//                          through LDS in 256-row chunks, in order, and the thread adds the voters to five double
//                          accumulators sequentially -- the order is the definition, so the result is reproducible.
// Their arithmetic is one IEEE operation per written operation (fp32 IoU with the exact division; the Gaussian decay and the
// voting sums in double), which postprocess.merge_soft_numpy restates.
#include "common.h"
#include "../../include/dana_hip.h"

namespace {

// dana_nms scans a problem with its column words resident in LDS: (n / 64) * 8 + 528 bytes <= 64 KiB
constexpr int MERGE_MAX_CAPACITY = (64 * 1024 - 128 * 4 - 16) / 8 * 64;
// merge_soft_kernel keeps 21 bytes of a row in LDS (box 16, working score 4, live flag 1), 64 KiB less its static words
constexpr int SOFT_ROW_BYTES = 21;
constexpr int SOFT_MAX_CAPACITY = (64 * 1024 - 64) / SOFT_ROW_BYTES / 64 * 64;  // 3072
constexpr int VOTE_CHUNK = 256;

__global__ void __launch_bounds__(256)
merge_scatter_kernel(const float* __restrict__ dets_in, const int* __restrict__ counts_in,
                     const int* __restrict__ offsets_in, int groups, int capacity, float4* __restrict__ boxes,
                     float* __restrict__ scores, int* __restrict__ src_group, int* __restrict__ src_row,
                     int* __restrict__ n_total) {
  __shared__ unsigned long long s_base;
  const int g = blockIdx.x;
  const long l = blockIdx.y;
  const int* cnt = counts_in + l * groups;
  if (threadIdx.x == 0) s_base = 0;
  __syncthreads();
  // rows of the groups in front of this one (each clamped to the frame: the sum cannot overflow)
  unsigned long long part = 0;
  for (int i = threadIdx.x; i < g; i += blockDim.x) part += (unsigned long long)min(max(cnt[i], 0), capacity);
  if (part) atomicAdd(&s_base, part);
  __syncthreads();
  const int base = (int)min(s_base, (unsigned long long)capacity);
  const int mine = min(max(cnt[g], 0), capacity - base);  // a too-small capacity truncates, it never writes outside the frame
  const long frame = l * capacity;
  const float* src = dets_in + (long)offsets_in[l * groups + g] * 5;
  for (int r = threadIdx.x; r < mine; r += blockDim.x) {
    const float* q = src + (long)r * 5;
    const long at = frame + base + r;
    boxes[at] = make_float4(q[0], q[1], q[2], q[3]);
    scores[at] = q[4];
    src_group[at] = g;
    src_row[at] = r;
  }
  if (g == groups - 1) {
    const int total = base + mine;
    if (threadIdx.x == 0) n_total[l] = total;
    for (int r = total + threadIdx.x; r < capacity; r += blockDim.x) {
      boxes[frame + r] = make_float4(0.f, 0.f, 0.f, 0.f);
      scores[frame + r] = -__builtin_huge_valf();
      src_group[frame + r] = -1;
      src_row[frame + r] = -1;
    }
  }
}

// rows list i emits: its kept positions below its row count (ascending positions: a prefix of keep[i]), or without NMS
// every real row; then the max_dets cut
__device__ __forceinline__ int merged_count(const int* __restrict__ keep, const int* __restrict__ num_keep,
                                            const int* __restrict__ n_total, int i, int capacity, int do_nms, int max_dets) {
  const int nt = n_total[i];
  int lo = nt;
  if (do_nms) {
    const int* k = keep + (long)i * capacity;
    int hi = min(num_keep[i], capacity);
    lo = 0;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (k[mid] < nt)
        lo = mid + 1;
      else
        hi = mid;
    }
  }
  return max_dets > 0 ? min(lo, max_dets) : lo;
}

__global__ void __launch_bounds__(256)
merge_compact_kernel(const float4* __restrict__ sorted_boxes, const float* __restrict__ sorted_scores,
                     const int* __restrict__ order, const int* __restrict__ src_group, const int* __restrict__ src_row,
                     const int* __restrict__ keep, const int* __restrict__ num_keep, const int* __restrict__ n_total,
                     int n_lists, int capacity, int do_nms, int max_dets, float* __restrict__ dets_out,
                     int* __restrict__ group_out, int* __restrict__ row_out, int* __restrict__ counts_out,
                     int* __restrict__ offsets_out) {
  __shared__ int s_off;
  const int l = blockIdx.x;
  if (threadIdx.x == 0) s_off = 0;
  __syncthreads();
  int part = 0;
  for (int i = threadIdx.x; i < l; i += blockDim.x) part += merged_count(keep, num_keep, n_total, i, capacity, do_nms, max_dets);
  if (part) atomicAdd(&s_off, part);  // (integer sum: the same total in any order)
  __syncthreads();
  const int off = s_off;
  const int cnt = merged_count(keep, num_keep, n_total, l, capacity, do_nms, max_dets);
  if (threadIdx.x == 0) {
    counts_out[l] = cnt;
    offsets_out[l] = off;
    if (l == n_lists - 1) offsets_out[n_lists] = off + cnt;
  }
  const long frame = (long)l * capacity;
  const int* k = keep + frame;
  for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
    const int pos = do_nms ? k[i] : i;       // position in the sorted list
    const int j = order[frame + pos];        // ... and in the concatenation
    const float4 bx = sorted_boxes[frame + pos];
    float* o = dets_out + (long)(off + i) * 5;
    o[0] = bx.x;
    o[1] = bx.y;
    o[2] = bx.z;
    o[3] = bx.w;
    o[4] = sorted_scores[frame + pos];
    group_out[off + i] = src_group[frame + j];
    row_out[off + i] = src_row[frame + j];
  }
}

// iou(a, b) with the legacy +1 widths and the exact division (the last branch of nms.hip's iou_suppress): the soft path
// needs the value, not only its side of a threshold
__device__ __forceinline__ float area_p1(float4 a) { return (a.z - a.x + 1.f) * (a.w - a.y + 1.f); }
__device__ __forceinline__ float iou_p1(float4 a, float4 b) {
  const float w = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x) + 1.f, 0.f);
  const float h = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y) + 1.f, 0.f);
  const float inter = w * h;
  return inter / ((area_p1(a) + area_p1(b)) - inter);
}

// does candidate (ta, ia) rank in front of (tb, ib)? Larger working score first, a NaN behind every number, then the lower
// concatenation index: a total order, so the reduction tree gives what a sequential scan gives
__device__ __forceinline__ bool soft_ranks_first(float ta, int ia, float tb, int ib) {
  const bool na = ta != ta, nb = tb != tb;
  if (na != nb) return nb;
  if (!na && ta != tb) return ta > tb;
  return ia < ib;
}

enum { SOFT_LINEAR = 1, SOFT_GAUSSIAN = 2 };

__global__ void __launch_bounds__(256)
merge_soft_kernel(const float4* __restrict__ boxes, const float* __restrict__ scores, const int* __restrict__ n_total,
                  int capacity, int method, float nms_thresh, int inclusive, float sigma, float min_score, int max_dets,
                  float4* __restrict__ sorted_boxes, float* __restrict__ sorted_scores, int* __restrict__ order,
                  int* __restrict__ keep, int* __restrict__ num_keep) {
  extern __shared__ float4 s_rows[];  // box [capacity] | working score [capacity] | live [capacity]
  __shared__ float s_wt[4];
  __shared__ int s_wi[4];
  float4* s_box = s_rows;
  float* s_t = (float*)(s_box + capacity);
  unsigned char* s_live = (unsigned char*)(s_t + capacity);
  const int l = blockIdx.x;
  const long frame = (long)l * capacity;
  const int n = min(max(n_total[l], 0), capacity);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < n; i += 256) {
    s_box[i] = boxes[frame + i];
    s_t[i] = scores[frame + i];
    s_live[i] = 1;
  }
  __syncthreads();
  const int limit = max_dets > 0 ? min(max_dets, n) : n;
  const double dsigma = (double)sigma;
  int emitted = 0;
  while (emitted < limit) {
    // the live row with the largest working score; rows of a thread come in ascending index
    float bt = 0.f;
    int bi = -1;
    for (int i = threadIdx.x; i < n; i += 256) {
      if (!s_live[i]) continue;
      const float t = s_t[i];
      if (bi < 0 || soft_ranks_first(t, i, bt, bi)) {
        bt = t;
        bi = i;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ot = __shfl_xor(bt, o);
      const int oi = __shfl_xor(bi, o);
      if (oi >= 0 && (bi < 0 || soft_ranks_first(ot, oi, bt, bi))) {
        bt = ot;
        bi = oi;
      }
    }
    if (lane == 0) {
      s_wt[wave] = bt;
      s_wi[wave] = bi;
    }
    __syncthreads();
    bt = s_wt[0];
    bi = s_wi[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const float ot = s_wt[w];
      const int oi = s_wi[w];
      if (oi >= 0 && (bi < 0 || soft_ranks_first(ot, oi, bt, bi))) {
        bt = ot;
        bi = oi;
      }
    }
    if (bi < 0) break;  // nothing is live (the same in every thread)
    const float4 pick = s_box[bi];
    if (threadIdx.x == 0) {
      sorted_boxes[frame + emitted] = pick;
      sorted_scores[frame + emitted] = bt;
      order[frame + emitted] = bi;
      keep[frame + emitted] = emitted;
    }
    for (int i = threadIdx.x; i < n; i += 256) {
      if (!s_live[i]) continue;
      if (i == bi) {
        s_live[i] = 0;
        continue;
      }
      const float o = iou_p1(pick, s_box[i]);
      float t = s_t[i];
      if (method == SOFT_LINEAR) {
        if (inclusive ? (o >= nms_thresh) : (o > nms_thresh)) t = t * (1.f - o);
      } else {
        t = (float)((double)t * exp(-(double)(o * o) / dsigma));
      }
      s_t[i] = t;
      if (t < min_score) s_live[i] = 0;
    }
    ++emitted;
    __syncthreads();  // the updates are in LDS, and s_wt / s_wi are free again
  }
  if (threadIdx.x == 0) num_keep[l] = emitted;
}

// grid (n_lists, row blocks): thread k of block (l, y) owns emitted row y*256 + k of list l
__global__ void __launch_bounds__(256)
merge_vote_kernel(const float4* __restrict__ boxes, const float* __restrict__ scores, const int* __restrict__ n_total,
                  int capacity, float vote_thresh, int vote_avg, const int* __restrict__ counts_out,
                  const int* __restrict__ offsets_out, float* __restrict__ dets_out, int* __restrict__ votes_out) {
  __shared__ float4 s_box[VOTE_CHUNK];
  __shared__ float s_score[VOTE_CHUNK];
  const int l = blockIdx.x;
  const int cnt = counts_out[l];
  const int k = blockIdx.y * 256 + threadIdx.x;
  if ((int)(blockIdx.y * 256) >= cnt) return;  // (the whole workgroup)
  const long frame = (long)l * capacity;
  const int n = min(max(n_total[l], 0), capacity);
  const bool mine = k < cnt;
  const long at = (long)offsets_out[l] + k;
  float* o = dets_out + at * 5;
  const float4 me = mine ? make_float4(o[0], o[1], o[2], o[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
  double x1 = 0.0, y1 = 0.0, x2 = 0.0, y2 = 0.0, wsum = 0.0;
  int votes = 0;
  for (int c0 = 0; c0 < n; c0 += VOTE_CHUNK) {
    const int m = min(VOTE_CHUNK, n - c0);
    if ((int)threadIdx.x < m) {
      s_box[threadIdx.x] = boxes[frame + c0 + threadIdx.x];
      s_score[threadIdx.x] = scores[frame + c0 + threadIdx.x];
    }
    __syncthreads();
    if (mine) {
      for (int j = 0; j < m; ++j) {  // ascending concatenation index: the order is the definition
        const float4 b = s_box[j];
        if (iou_p1(me, b) >= vote_thresh) {
          const double s = (double)s_score[j];
          x1 += s * (double)b.x;
          y1 += s * (double)b.y;
          x2 += s * (double)b.z;
          y2 += s * (double)b.w;
          wsum += s;
          ++votes;
        }
      }
    }
    __syncthreads();
  }
  if (!mine) return;
  if (wsum > 0.0) {
    o[0] = (float)(x1 / wsum);
    o[1] = (float)(y1 / wsum);
    o[2] = (float)(x2 / wsum);
    o[3] = (float)(y2 / wsum);
  }
  if (vote_avg) o[4] = (float)(wsum / (double)votes);
  votes_out[at] = votes;
}

__global__ void __launch_bounds__(256)
dets_to_gt_kernel(const float* __restrict__ dets, const int* __restrict__ counts, const int* __restrict__ offsets,
                  const float* __restrict__ im_info, int im_info_stride, const float* __restrict__ labels,
                  float score_thresh, int max_boxes, float* __restrict__ gt_boxes, long long* __restrict__ num_boxes) {
  __shared__ int s_wave[4];
  const int b = blockIdx.x;
  const int cnt = max(counts[b], 0);
  const float* src = dets + (long)offsets[b] * 5;
  const float scale = im_info[(long)b * im_info_stride + 2], label = labels[b];
  float* out = gt_boxes + (long)b * max_boxes * 5;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int written = 0;  // rows passing the threshold so far (the same in every lane)
  for (int r0 = 0; r0 < cnt && written < max_boxes; r0 += 256) {
    const int r = r0 + threadIdx.x;
    const bool pass = r < cnt && src[(long)r * 5 + 4] > score_thresh;
    const unsigned long long m = __ballot(pass);
    if (lane == 0) s_wave[wave] = __builtin_popcountll(m);
    __syncthreads();
    int at = written + __builtin_popcountll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) at += s_wave[w];
    if (pass && at < max_boxes) {
      const float* q = src + (long)r * 5;
      float* o = out + (long)at * 5;
      o[0] = q[0] * scale;
      o[1] = q[1] * scale;
      o[2] = q[2] * scale;
      o[3] = q[3] * scale;
      o[4] = label;
    }
    written += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
  }
  const int n = min(written, max_boxes);
  for (int i = n * 5 + threadIdx.x; i < max_boxes * 5; i += 256) out[i] = 0.f;
  if (threadIdx.x == 0) num_boxes[b] = n;
}

struct MergePlan {
  size_t boxes, scores, src_group, src_row, order, sorted_scores, sorted_boxes, keep, num_keep, n_total, sort_ws, nms_ws, total;
};
MergePlan merge_plan(int n_lists, int capacity) {
  MergePlan p;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    size_t at = o;
    o += dana_align_up(bytes, 256);
    return at;
  };
  const size_t n = (size_t)n_lists * capacity;
  p.boxes = take(n * 16);
  p.scores = take(n * 4);
  p.src_group = take(n * 4);
  p.src_row = take(n * 4);
  p.order = take(n * 4);
  p.sorted_scores = take(n * 4);
  p.sorted_boxes = take(n * 16);
  p.keep = take(n * 4);
  p.num_keep = take((size_t)n_lists * 4);
  p.n_total = take((size_t)n_lists * 4);
  p.sort_ws = take(dana_sort_desc_workspace_bytes(n_lists, capacity));
  p.nms_ws = take(dana_nms_workspace_bytes(capacity, n_lists));
  p.total = o;
  return p;
}

bool merge_shape_ok(int n_lists, int groups, int capacity) {
  return n_lists >= 0 && n_lists <= 65535 && groups > 0 && capacity >= 0 && capacity <= MERGE_MAX_CAPACITY;
}

// what dana_detect_merge_soft adds to a merge (null: dana_detect_merge itself)
struct SoftArgs {
  int method;  // 0 hard, SOFT_LINEAR, SOFT_GAUSSIAN
  float sigma, min_score, vote_thresh;
  int vote_avg;
  int* votes_out;
};

int merge_run(const char* who, const float* dets_in, const int* counts_in, const int* offsets_in, int n_lists, int groups,
              int capacity, int do_nms, float nms_thresh, int nms_inclusive, int max_dets, float* dets_out, int* group_out,
              int* row_out, int* counts_out, int* offsets_out, void* workspace, size_t workspace_bytes, dana_stream_t stream,
              const SoftArgs* soft) {
  const bool soft_loop = soft && soft->method != 0;
  const bool vote = soft && soft->vote_thresh >= 0.f;
  DANA_CHECK_ARG(n_lists >= 0 && n_lists <= 65535 && groups > 0 && capacity >= 0, "%s: bad shape n_lists=%d groups=%d capacity=%d",
                 who, n_lists, groups, capacity);
  DANA_CHECK_ARG(capacity <= MERGE_MAX_CAPACITY, "%s: capacity %d above the %d rows dana_nms takes per problem", who, capacity,
                 MERGE_MAX_CAPACITY);
  DANA_CHECK_ARG(!soft_loop || capacity <= SOFT_MAX_CAPACITY,
                 "%s: capacity %d above the %d rows the soft-NMS kernel holds in LDS (%d bytes per row)", who, capacity,
                 SOFT_MAX_CAPACITY, SOFT_ROW_BYTES);
  DANA_CHECK_ARG(offsets_out && (counts_out || n_lists == 0), "%s: null counts_out / offsets_out", who);
  hipStream_t s = (hipStream_t)stream;
  if (n_lists == 0 || capacity == 0) {
    if ((n_lists && hipMemsetAsync(counts_out, 0, (size_t)n_lists * sizeof(int), s) != hipSuccess) ||
        hipMemsetAsync(offsets_out, 0, (size_t)(n_lists + 1) * sizeof(int), s) != hipSuccess) {
      dana_set_error("%s: memset failed", who);
      return DANA_ERR_HIP;
    }
    return DANA_OK;
  }
  DANA_CHECK_ARG(dets_in && counts_in && offsets_in && dets_out && group_out && row_out && (!vote || soft->votes_out),
                 "%s: null pointer", who);
  const MergePlan p = merge_plan(n_lists, capacity);
  if (!workspace || workspace_bytes < p.total) {
    dana_set_error("%s: workspace %zu < %zu", who, workspace_bytes, p.total);
    return DANA_ERR_WORKSPACE;
  }
  char* ws = (char*)workspace;
  float* boxes = (float*)(ws + p.boxes);
  float* scores = (float*)(ws + p.scores);
  int* src_group = (int*)(ws + p.src_group);
  int* src_row = (int*)(ws + p.src_row);
  int* order = (int*)(ws + p.order);
  float* sorted_scores = (float*)(ws + p.sorted_scores);
  float* sorted_boxes = (float*)(ws + p.sorted_boxes);
  int* keep = (int*)(ws + p.keep);
  int* num_keep = (int*)(ws + p.num_keep);
  int* n_total = (int*)(ws + p.n_total);
  merge_scatter_kernel<<<dim3(groups, n_lists), 256, 0, s>>>(dets_in, counts_in, offsets_in, groups, capacity, (float4*)boxes,
                                                             scores, src_group, src_row, n_total);
  DANA_CHECK_LAUNCH(who);
  if (soft_loop) {
    // the emissions in the form the compaction reads: emission i sits at sorted position i, and all of them are "kept"
    const size_t lds = dana_align_up((size_t)capacity * SOFT_ROW_BYTES, 16);
    merge_soft_kernel<<<n_lists, 256, lds, s>>>((const float4*)boxes, scores, n_total, capacity, soft->method, nms_thresh,
                                                nms_inclusive, soft->sigma, soft->min_score, max_dets, (float4*)sorted_boxes,
                                                sorted_scores, order, keep, num_keep);
    DANA_CHECK_LAUNCH(who);
    do_nms = 1;
  } else {
    int rc = dana_sort_desc(scores, n_lists, capacity, order, sorted_scores, ws + p.sort_ws, p.nms_ws - p.sort_ws, stream);
    if (rc) return rc;
    rc = dana_gather_boxes(boxes, order, n_lists, capacity, capacity, capacity, sorted_boxes, stream);
    if (rc) return rc;
    if (do_nms) {
      rc = dana_nms(sorted_boxes, capacity, n_lists, nms_thresh, nms_inclusive, capacity, keep, capacity, num_keep,
                    ws + p.nms_ws, p.total - p.nms_ws, stream);
      if (rc) return rc;
    }
  }
  merge_compact_kernel<<<n_lists, 256, 0, s>>>((const float4*)sorted_boxes, sorted_scores, order, src_group, src_row, keep,
                                               num_keep, n_total, n_lists, capacity, do_nms, max_dets, dets_out, group_out,
                                               row_out, counts_out, offsets_out);
  DANA_CHECK_LAUNCH(who);
  if (vote) {
    const int rows = max_dets > 0 ? min(max_dets, capacity) : capacity;  // the most rows a list can emit
    merge_vote_kernel<<<dim3(n_lists, (rows + 255) / 256), 256, 0, s>>>((const float4*)boxes, scores, n_total, capacity,
                                                                        soft->vote_thresh, soft->vote_avg, counts_out,
                                                                        offsets_out, dets_out, soft->votes_out);
    DANA_CHECK_LAUNCH(who);
  }
  return DANA_OK;
}

}  // namespace

extern "C" {

size_t dana_detect_merge_workspace_bytes(int n_lists, int groups, int capacity) {
  if (!merge_shape_ok(n_lists, groups, capacity) || n_lists == 0 || capacity == 0) return 0;
  return merge_plan(n_lists, capacity).total;
}

int dana_detect_merge(const float* dets_in, const int* counts_in, const int* offsets_in, int n_lists, int groups,
                      int capacity, int do_nms, float nms_thresh, int nms_inclusive, int max_dets, float* dets_out,
                      int* group_out, int* row_out, int* counts_out, int* offsets_out, void* workspace,
                      size_t workspace_bytes, dana_stream_t stream) {
  return merge_run("dana_detect_merge", dets_in, counts_in, offsets_in, n_lists, groups, capacity, do_nms, nms_thresh,
                   nms_inclusive, max_dets, dets_out, group_out, row_out, counts_out, offsets_out, workspace, workspace_bytes,
                   stream, nullptr);
}

// (the frame, the sort's and the NMS's scratch of dana_detect_merge: method 0 runs that chain, and the soft loop writes its
// emissions into the same frame rows)
size_t dana_detect_merge_soft_workspace_bytes(int n_lists, int groups, int capacity) {
  return dana_detect_merge_workspace_bytes(n_lists, groups, capacity);
}

int dana_detect_merge_soft(const float* dets_in, const int* counts_in, const int* offsets_in, int n_lists, int groups,
                           int capacity, int do_nms, float nms_thresh, int nms_inclusive, int max_dets, int method,
                           float sigma, float min_score, float vote_thresh, int vote_score, float* dets_out, int* group_out,
                           int* row_out, int* votes_out, int* counts_out, int* offsets_out, void* workspace,
                           size_t workspace_bytes, dana_stream_t stream) {
  DANA_CHECK_ARG(method >= 0 && method <= SOFT_GAUSSIAN && (vote_score == 0 || vote_score == 1),
                 "dana_detect_merge_soft: bad method %d (0 hard, 1 linear, 2 gaussian) or vote_score %d (0 id, 1 avg)", method,
                 vote_score);
  DANA_CHECK_ARG(method != SOFT_GAUSSIAN || sigma > 0.f, "dana_detect_merge_soft: sigma %g must be positive", (double)sigma);
  DANA_CHECK_ARG(!(vote_thresh > 1.f) && vote_thresh == vote_thresh, "dana_detect_merge_soft: vote_thresh %g above 1",
                 (double)vote_thresh);
  const SoftArgs soft = {method, sigma, min_score, vote_thresh, vote_score, votes_out};
  return merge_run("dana_detect_merge_soft", dets_in, counts_in, offsets_in, n_lists, groups, capacity, do_nms, nms_thresh,
                   nms_inclusive, max_dets, dets_out, group_out, row_out, counts_out, offsets_out, workspace, workspace_bytes,
                   stream, &soft);
}

int dana_dets_to_gt_boxes(const float* dets, const int* counts, const int* offsets, const float* im_info,
                          int im_info_stride, const float* labels, int B, float score_thresh, int max_boxes,
                          float* gt_boxes, long long* num_boxes, dana_stream_t stream) {
  DANA_CHECK_ARG(B >= 0 && max_boxes >= 0 && im_info_stride >= 3, "dana_dets_to_gt_boxes: bad shape B=%d max_boxes=%d stride=%d",
                 B, max_boxes, im_info_stride);
  if (B == 0) return DANA_OK;
  DANA_CHECK_ARG(counts && offsets && im_info && labels && num_boxes && (gt_boxes || max_boxes == 0) && dets,
                 "dana_dets_to_gt_boxes: null pointer");
  dets_to_gt_kernel<<<B, 256, 0, (hipStream_t)stream>>>(dets, counts, offsets, im_info, im_info_stride, labels, score_thresh,
                                                        max_boxes, gt_boxes, num_boxes);
  DANA_CHECK_LAUNCH("dana_dets_to_gt_boxes");
  return DANA_OK;
}

}  // extern "C"
