// Proposal recall on the device (dana_amd/evaluate.py, `ProposalRecallEvaluator`): the one-to-one greedy matching of
// proposals and ground truth and the recall counts per IoU threshold, proposal budget and object-size range.
//
// Reference semantics replaced (lib/datasets/imdb.py:137-225, `evaluate_recall`, not code): per image the IoU matrix of the
// first `limit` proposals x the ground-truth boxes inside the area range; repeat { the best-covered object, the proposal
// that covers it best, record the IoU, take both out }; recall = (recorded IoU >= t) / objects. Float64, IoU with the
// `+ 1.` pixel convention and the operation order of voc_eval.py:174-187 (this file is compiled with -ffp-contract=off).
//
// dana_eval_proposal_recall is two launches:
//   1. recall_match_kernel: one workgroup per (unit, limit, area range). Per object the workspace keeps the best candidate
//      still available and its IoU (one wavefront scans the candidates of one object); the used candidates are a bitmap in
//      LDS. A round picks the best object by a block reduction, records the pair, and re-scans only the objects whose best
//      candidate was the one just taken: O(G m) IoUs when few objects share a first choice, never more than G^2 m.
//   2. recall_count_kernel: one thread per (limit, area range, pair) compares the recorded IoU with the thresholds; lanes
//      of a wavefront that count into the same (role, limit, area range, class) cell add once, with a 64-bit integer
//      atomic. Integer sums: the same counts in any order.
#include "common.h"
#include "../../include/dana_hip.h"
#include <limits.h>
#include <math.h>

namespace {

typedef unsigned long long u64;

constexpr int PR_MAX_THR = 16;
constexpr int PR_MAX_LIMITS = 8;
constexpr int PR_MAX_AREA = 8;
constexpr int PR_MAX_CAND = 65536;  // candidates per unit and limit: the bitmap's 8 KB of LDS
constexpr int PR_TAB = 9;           // unit_tab columns
constexpr int PR_DONE = -2;         // best-candidate value of an object that is matched or takes no part

struct RecallWs {
  size_t pair_unit, best, cand, total;
};

inline bool recall_shape_ok(long n_boxes, long n_units, long n_pairs, int n_thr, int n_limits, int n_area) {
  return n_boxes >= 0 && n_units >= 0 && n_pairs >= 0 && n_boxes < (long)INT_MAX && n_units < (long)INT_MAX &&
         n_pairs < (long)INT_MAX && n_thr >= 1 && n_thr <= PR_MAX_THR && n_limits >= 1 && n_limits <= PR_MAX_LIMITS &&
         n_area >= 1 && n_area <= PR_MAX_AREA;
}

inline RecallWs recall_layout(long n_pairs, int n_limits, int n_area) {
  RecallWs L;
  const size_t cells = (size_t)n_limits * n_area * (size_t)n_pairs;
  size_t o = 0;
  L.pair_unit = o, o += dana_align_up((size_t)n_pairs * 4 + 4, 256);
  L.best = o, o += dana_align_up(cells * 8 + 8, 256);
  L.cand = o, o += dana_align_up(cells * 4 + 4, 256);
  L.total = o;
  return L;
}

// voc_eval.py:174-187 / evaluate._iou_matrix(bb, gt): the same operations in the same order
__device__ __forceinline__ double iou_plus1(double bx1, double by1, double bx2, double by2, double gx1, double gy1,
                                            double gx2, double gy2) {
  const double ixmin = fmax(gx1, bx1), iymin = fmax(gy1, by1);
  const double ixmax = fmin(gx2, bx2), iymax = fmin(gy2, by2);
  const double iw = fmax(ixmax - ixmin + 1., 0.), ih = fmax(iymax - iymin + 1., 0.);
  const double inters = iw * ih;
  const double uni = ((bx2 - bx1 + 1.) * (by2 - by1 + 1.) + (gx2 - gx1 + 1.) * (gy2 - gy1 + 1.) - inters);
  return inters / uni;
}

// (value, index) -> the larger value, the lower index among equal values, over the 64 lanes (every lane gets it)
__device__ __forceinline__ void wave_argmax(double& v, int& i) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(i, o);
    if (ov > v || (ov == v && oi < i)) {
      v = ov;
      i = oi;
    }
  }
}

// One wavefront: the best available candidate of one object among rows [0, m) -> (IoU, row), (-inf, -1) when none is
// left. Equal IoUs keep the lowest row: a lane walks its rows upwards and takes only a strictly larger value.
__device__ __forceinline__ void scan_object(const float4* __restrict__ cand, int m, const unsigned* used, float4 gb,
                                            double& best, int& row) {
  const int lane = threadIdx.x & 63;
  const double gx1 = gb.x, gy1 = gb.y, gx2 = gb.z, gy2 = gb.w;
  double bv = -INFINITY;
  int bi = INT_MAX;
  for (int i = lane; i < m; i += 64) {
    if ((used[i >> 5] >> (i & 31)) & 1u) continue;
    const float4 b = cand[i];
    const double v = iou_plus1((double)b.x, (double)b.y, (double)b.z, (double)b.w, gx1, gy1, gx2, gy2);
    if (v > bv) {
      bv = v;
      bi = i;
    }
  }
  wave_argmax(bv, bi);
  best = bv;
  row = bi == INT_MAX ? -1 : bi;
}

__global__ void __launch_bounds__(256)
recall_match_kernel(const float4* __restrict__ boxes, const int* __restrict__ unit_tab, const float4* __restrict__ gt_box,
                    const double* __restrict__ gt_area, const int* __restrict__ gt_order, long g, long n_pairs, int n_cls,
                    const int* __restrict__ limits, const double* __restrict__ area_rng, int n_area,
                    double* ov, int* match, int* pair_unit, double* wbest, int* wcand) {
  // (ov / match / the workspace carry values from one wavefront to another across the barriers: no __restrict__)
  __shared__ unsigned used[PR_MAX_CAND / 32];
  __shared__ double red_v[4];
  __shared__ int red_j[4], red_c[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l = blockIdx.y, a = blockIdx.z;
  const int* tab = unit_tab + (long)blockIdx.x * PR_TAB;
  // the table is the host's; a row that does not fit the buffers is skipped as a whole (block-uniform)
  const long box_off = tab[0];
  int count = tab[1];
  long r0b = tab[2], r0e = tab[3], r1b = tab[4], r1e = tab[5];
  const long pair_off = tab[6];
  const int cls = tab[7], role = tab[8];
  r0b = r0b < 0 ? 0 : (r0b > g ? g : r0b);
  r0e = r0e < r0b ? r0b : (r0e > g ? g : r0e);
  r1b = r1b < 0 ? 0 : (r1b > g ? g : r1b);
  r1e = r1e < r1b ? r1b : (r1e > g ? g : r1e);
  const long n0 = r0e - r0b, G_ = n0 + (r1e - r1b);
  if (G_ == 0 || box_off < 0 || pair_off < 0 || pair_off + G_ > n_pairs || cls < 0 || cls >= n_cls || (role | 1) != 1)
    return;
  const int G = (int)G_;
  count = count < 0 ? 0 : count;
  const int lim = limits[l];
  int m = lim <= 0 ? count : (lim < count ? lim : count);
  m = m > PR_MAX_CAND ? PR_MAX_CAND : m;
  const double a_lo = area_rng[2 * a], a_hi = area_rng[2 * a + 1];
  const long base = ((long)l * n_area + a) * n_pairs + pair_off;
  double* ov_u = ov + base;
  int* match_u = match + base;
  double* best_u = wbest + base;
  int* cand_u = wcand + base;
  const float4* cand = boxes + box_off;

  for (int i = tid; i < (m + 31) >> 5; i += 256) used[i] = 0u;
  if (l == 0 && a == 0)
    for (int j = tid; j < G; j += 256) pair_unit[pair_off + j] = (int)blockIdx.x;
  __syncthreads();

  // every object's first choice (one wavefront per object), or -1 for the objects outside the area range
  for (int j = w; j < G; j += 4) {
    const long pos = j < n0 ? r0b + j : r1b + (j - n0);
    const int gi = gt_order[pos];
    bool in = gi >= 0 && gi < g;
    float4 gb = make_float4(0.f, 0.f, 0.f, 0.f);
    if (in) {
      gb = gt_box[gi];
      const double ar = gt_area ? gt_area[gi]
                                : ((double)gb.z - (double)gb.x + 1.) * ((double)gb.w - (double)gb.y + 1.);
      in = a_lo <= ar && ar <= a_hi;
    }
    if (!in) {  // wave-uniform
      if (lane == 0) {
        ov_u[j] = -1.;
        match_u[j] = -1;
        cand_u[j] = PR_DONE;
      }
      continue;
    }
    double bv;
    int bi;
    scan_object(cand, m, used, gb, bv, bi);
    if (lane == 0) {
      best_u[j] = bv;
      cand_u[j] = bi;
    }
  }
  __syncthreads();

  for (int round = 0; round < G; ++round) {
    // the best-covered object still open: the largest IoU, the lowest position among equals
    double bv = -INFINITY;
    int bj = INT_MAX, bc = -1;
    for (int j = tid; j < G; j += 256) {
      const int c = cand_u[j];
      if (c == PR_DONE) continue;
      const double v = c < 0 ? -INFINITY : best_u[j];
      if (v > bv || bj == INT_MAX) {  // j ascends: a later equal value does not replace an earlier one
        bv = v;
        bj = j;
        bc = c;
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const double xv = __shfl_xor(bv, o);
      const int xj = __shfl_xor(bj, o), xc = __shfl_xor(bc, o);
      if (xj != INT_MAX && (bj == INT_MAX || xv > bv || (xv == bv && xj < bj))) {
        bv = xv;
        bj = xj;
        bc = xc;
      }
    }
    if (lane == 0) {
      red_v[w] = bv;
      red_j[w] = bj;
      red_c[w] = bc;
    }
    __syncthreads();
    bv = red_v[0], bj = red_j[0], bc = red_c[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      const double xv = red_v[k];
      const int xj = red_j[k], xc = red_c[k];
      if (xj != INT_MAX && (bj == INT_MAX || xv > bv || (xv == bv && xj < bj))) {
        bv = xv;
        bj = xj;
        bc = xc;
      }
    }
    if (bj == INT_MAX) break;  // every object is done (block-uniform)
    if (bc < 0) {              // the candidates ran out: what is still open stays unmatched
      for (int j = tid; j < G; j += 256)
        if (cand_u[j] != PR_DONE) {
          ov_u[j] = 0.;
          match_u[j] = -1;
        }
      break;
    }
    if (tid == 0) {
      ov_u[bj] = bv;
      match_u[bj] = bc;
      cand_u[bj] = PR_DONE;
      used[bc >> 5] |= 1u << (bc & 31);
    }
    __syncthreads();
    // the objects that lost their first choice look again
    for (int j0 = w * 64; j0 < G; j0 += 256) {
      const int j = j0 + lane;
      u64 again = __ballot(j < G && cand_u[j] == bc);
      while (again) {
        const int jj = j0 + __ffsll((long long)again) - 1;
        again &= again - 1;
        const long pos = jj < n0 ? r0b + jj : r1b + (jj - n0);
        const float4 gb = gt_box[gt_order[pos]];  // (checked above: an object with a candidate is inside [0, g))
        double v;
        int c;
        scan_object(cand, m, used, gb, v, c);
        if (lane == 0) {
          best_u[jj] = v;
          cand_u[jj] = c;
        }
      }
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256)
recall_count_kernel(const double* __restrict__ ov, const int* __restrict__ pair_unit, const int* __restrict__ unit_tab,
                    const double* __restrict__ thr, int T, int L, int A, long n_pairs, long n_units, int K,
                    long long* __restrict__ hits, long long* __restrict__ npos) {
  const int lane = threadIdx.x & 63;
  const long total = (long)L * A * n_pairs;
  const long first = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)blockDim.x * gridDim.x;
  for (long e0 = first - lane; e0 < total; e0 += stride) {  // a wavefront stays together for the ballots
    const long e = e0 + lane;
    double v = -1.;
    int cell = -1;  // ((role * L + l) * A + a) * K + k
    int l = 0;
    if (e < total) {
      const long pair = e % n_pairs;
      const int la = (int)(e / n_pairs);
      l = la / A;
      const int a = la - l * A;
      const int u = pair_unit[pair];
      if (u >= 0 && u < n_units) {
        const int k = unit_tab[(long)u * PR_TAB + 7], role = unit_tab[(long)u * PR_TAB + 8];
        v = ov[e];
        if (v != -1. && k >= 0 && k < K && (role | 1) == 1) cell = ((role * L + l) * A + a) * K + k;
      }
    }
    u64 open = __ballot(cell >= 0);
    while (open) {
      const int leader = __ffsll((long long)open) - 1;
      const int c = __shfl(cell, leader);
      const bool mine = cell == c;
      const u64 same = __ballot(mine);
      open &= ~same;
      const int cl = __shfl(l, leader);
      const int k = c % K, ra = c / K;             // ra = (role * L + l) * A + a
      const int a = ra % A, role = ra / (A * L);
      if (cl == 0) {
        if (lane == leader) atomicAdd((u64*)&npos[((long)role * A + a) * K + k], (u64)__popcll(same));
      }
      for (int t = 0; t < T; ++t) {
        const u64 hit = __ballot(mine && v >= thr[t]);
        if (hit && lane == leader)
          atomicAdd((u64*)&hits[((((long)role * T + t) * L + cl) * A + a) * K + k], (u64)__popcll(hit));
      }
    }
  }
}

}  // namespace

extern "C" {

size_t dana_eval_proposal_recall_workspace_bytes(long n_boxes, long n_units, long n_pairs, int n_thr, int n_limits,
                                                 int n_area) {
  if (!recall_shape_ok(n_boxes, n_units, n_pairs, n_thr, n_limits, n_area)) return 0;
  return recall_layout(n_pairs, n_limits, n_area).total;
}

int dana_eval_proposal_recall(const float* boxes, const int* unit_tab, long n_units, const float* gt_box,
                              const void* gt_area_, const int* gt_order, long g, long n_pairs, int n_cls,
                              const void* iou_thr_, int n_thr, const int* limits, int n_limits, const void* area_rng_,
                              int n_area, void* ov_, int* match, void* hits_, void* npos_, void* workspace,
                              size_t workspace_bytes, dana_stream_t stream) {
  const double *gt_area = (const double*)gt_area_, *iou_thr = (const double*)iou_thr_;
  const double* area_rng = (const double*)area_rng_;
  double* ov = (double*)ov_;
  long long *hits = (long long*)hits_, *npos = (long long*)npos_;
  DANA_CHECK_ARG(n_thr >= 1 && n_thr <= PR_MAX_THR, "dana_eval_proposal_recall: n_thr=%d outside 1..%d", n_thr, PR_MAX_THR);
  DANA_CHECK_ARG(n_limits >= 1 && n_limits <= PR_MAX_LIMITS, "dana_eval_proposal_recall: n_limits=%d outside 1..%d",
                 n_limits, PR_MAX_LIMITS);
  DANA_CHECK_ARG(n_area >= 1 && n_area <= PR_MAX_AREA, "dana_eval_proposal_recall: n_area=%d outside 1..%d", n_area,
                 PR_MAX_AREA);
  DANA_CHECK_ARG(n_units >= 0 && n_pairs >= 0 && g >= 0 && n_units < (long)INT_MAX && n_pairs < (long)INT_MAX &&
                     g < (long)INT_MAX && n_cls >= 1,
                 "dana_eval_proposal_recall: bad shape n_units=%ld g=%ld n_pairs=%ld n_cls=%d", n_units, g, n_pairs, n_cls);
  DANA_CHECK_ARG((long)2 * n_thr * n_limits * n_area * (long)n_cls < (long)INT_MAX,
                 "dana_eval_proposal_recall: 2 * %d * %d * %d * %d count cells overflow", n_thr, n_limits, n_area, n_cls);
  DANA_CHECK_ARG(iou_thr && limits && area_rng && hits && npos, "dana_eval_proposal_recall: null pointer");
  const bool empty = n_units == 0 || n_pairs == 0;
  const RecallWs L = recall_layout(n_pairs, n_limits, n_area);
  if (!empty) {
    DANA_CHECK_ARG(unit_tab && gt_box && gt_order && ov && match && workspace && g > 0,
                   "dana_eval_proposal_recall: null pointer (or %ld pairs of no ground truth)", n_pairs);
    DANA_CHECK_ARG(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)gt_box & 15) == 0,
                   "dana_eval_proposal_recall: boxes and gt_box are read as float4 and must be 16-byte aligned");
    if (workspace_bytes < L.total) {
      dana_set_error("dana_eval_proposal_recall: workspace too small (%zu < %zu)", workspace_bytes, L.total);
      return DANA_ERR_WORKSPACE;
    }
  }
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(hits, 0, (size_t)2 * n_thr * n_limits * n_area * n_cls * sizeof(long long), st) != hipSuccess ||
      hipMemsetAsync(npos, 0, (size_t)2 * n_area * n_cls * sizeof(long long), st) != hipSuccess) {
    dana_set_error("dana_eval_proposal_recall: hipMemsetAsync failed");
    return DANA_ERR_HIP;
  }
  if (empty) return DANA_OK;
  char* ws = (char*)workspace;
  int* pair_unit = (int*)(ws + L.pair_unit);
  double* wbest = (double*)(ws + L.best);
  int* wcand = (int*)(ws + L.cand);
  const size_t cells = (size_t)n_limits * n_area * (size_t)n_pairs;
  // a pair no unit of the table owns is not counted: unit -1
  if (hipMemsetAsync(pair_unit, 0xff, (size_t)n_pairs * 4, st) != hipSuccess) {
    dana_set_error("dana_eval_proposal_recall: hipMemsetAsync failed");
    return DANA_ERR_HIP;
  }
  recall_match_kernel<<<dim3((unsigned)n_units, (unsigned)n_limits, (unsigned)n_area), 256, 0, st>>>(
      (const float4*)boxes, unit_tab, (const float4*)gt_box, gt_area, gt_order, g, n_pairs, n_cls, limits, area_rng, n_area,
      ov, match, pair_unit, wbest, wcand);
  DANA_CHECK_LAUNCH("dana_eval_proposal_recall (matching)");
  const long total = (long)cells;
  const long blocks = (total + 255) / 256;
  recall_count_kernel<<<(unsigned)(blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks)), 256, 0, st>>>(
      ov, pair_unit, unit_tab, iou_thr, n_thr, n_limits, n_area, n_pairs, n_units, n_cls, hits, npos);
  DANA_CHECK_LAUNCH("dana_eval_proposal_recall (counting)");
  return DANA_OK;
}

}  // extern "C"
