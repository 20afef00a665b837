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
#include "common.h"
#include "../../include/dana_hip.h"

namespace {

// dana_nms scans a problem with its column words resident in LDS: (n / 64) * 8 + 528 bytes <= 64 KiB
constexpr int MERGE_MAX_CAPACITY = (64 * 1024 - 128 * 4 - 16) / 8 * 64;

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
  DANA_CHECK_ARG(n_lists >= 0 && n_lists <= 65535 && groups > 0 && capacity >= 0,
                 "dana_detect_merge: bad shape n_lists=%d groups=%d capacity=%d", n_lists, groups, capacity);
  DANA_CHECK_ARG(capacity <= MERGE_MAX_CAPACITY, "dana_detect_merge: capacity %d above the %d rows dana_nms takes per problem",
                 capacity, MERGE_MAX_CAPACITY);
  DANA_CHECK_ARG(offsets_out && (counts_out || n_lists == 0), "dana_detect_merge: null counts_out / offsets_out");
  hipStream_t s = (hipStream_t)stream;
  if (n_lists == 0 || capacity == 0) {
    if ((n_lists && hipMemsetAsync(counts_out, 0, (size_t)n_lists * sizeof(int), s) != hipSuccess) ||
        hipMemsetAsync(offsets_out, 0, (size_t)(n_lists + 1) * sizeof(int), s) != hipSuccess) {
      dana_set_error("dana_detect_merge: memset failed");
      return DANA_ERR_HIP;
    }
    return DANA_OK;
  }
  DANA_CHECK_ARG(dets_in && counts_in && offsets_in && dets_out && group_out && row_out, "dana_detect_merge: null pointer");
  const MergePlan p = merge_plan(n_lists, capacity);
  if (!workspace || workspace_bytes < p.total) {
    dana_set_error("dana_detect_merge: workspace %zu < %zu", workspace_bytes, p.total);
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
  DANA_CHECK_LAUNCH("dana_detect_merge(scatter)");
  int rc = dana_sort_desc(scores, n_lists, capacity, order, sorted_scores, ws + p.sort_ws, p.nms_ws - p.sort_ws, stream);
  if (rc) return rc;
  rc = dana_gather_boxes(boxes, order, n_lists, capacity, capacity, capacity, sorted_boxes, stream);
  if (rc) return rc;
  if (do_nms) {
    rc = dana_nms(sorted_boxes, capacity, n_lists, nms_thresh, nms_inclusive, capacity, keep, capacity, num_keep,
                  ws + p.nms_ws, p.total - p.nms_ws, stream);
    if (rc) return rc;
  }
  merge_compact_kernel<<<n_lists, 256, 0, s>>>((const float4*)sorted_boxes, sorted_scores, order, src_group, src_row, keep,
                                               num_keep, n_total, n_lists, capacity, do_nms, max_dets, dets_out, group_out,
                                               row_out, counts_out, offsets_out);
  DANA_CHECK_LAUNCH("dana_detect_merge(compact)");
  return DANA_OK;
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
