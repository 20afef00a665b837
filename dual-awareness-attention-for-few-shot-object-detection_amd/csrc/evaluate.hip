// VOC-protocol detection evaluation on the device (dana_amd/evaluate.py): per-class AP at up to 16 IoU thresholds in
// one pass over the accumulated detections.
//
// Reference semantics replaced (lib/datasets/voc_eval.py, not code): the TP/FP marking of :165-199, the cumulative
// precision / recall curves of :202-207 and both voc_ap metrics of :35-66 -- all in float64, IoU with the `+ 1.` pixel
// convention and unfused operations (this file is compiled with -ffp-contract=off). It is NOT COCOeval: no crowd
// regions, area ranges or maxDets.
//
// Pipeline of dana_eval_ap (every step is its own launch; no workgroup ever waits on another one):
//   1. ground truth: radix sort by (class, image) segment -> gathered boxes / difficult flags, offsets table, npos
//   2. detections: radix sort by (class, descending score), stable in arrival order -> `order`, cls_offsets
//   3. a second stable sort of the ranks by (class, image) segment: each segment keeps its global-rank order
//   4. match_kernel: one wavefront per segment walks its detections in rank order against 64-lane ground-truth chunks
//   5. curves_ap_kernel: one workgroup per (class, threshold): forward scan of the TP/FP flags, reverse running max of
//      the precision, the AP sum in a fixed order
//
// The COCO protocol (dana_eval_coco: COCOeval for boxes, with crowd regions, area ranges and maxDets) is the second half
// of this file and reuses the sort, the segment tables and the block scans. Those, iou_voc and curves_ap_kernel live in
// eval_common.h, which diagnose.hip includes too.
#include "common.h"
#include "eval_common.h"
#include "../../include/dana_hip.h"
#include "../../include/dana_hip_debug.h"
#include <float.h>
#include <limits.h>
#include <math.h>

namespace {

// ---- keys, offsets, gathers ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
det_keys_kernel(const float* __restrict__ det, const int* __restrict__ det_img, const int* __restrict__ det_cls, long n,
                int n_img, int n_cls, u64* __restrict__ keys, int* __restrict__ vals) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)blockDim.x * gridDim.x) {
    keys[i] = det_key(det, det_img, det_cls, i, n_img, n_cls);
    vals[i] = (int)i;
  }
}

// rank r (detection order[r], class keys[r] >> 32) -> its (class, image) segment; value = the rank
__global__ void __launch_bounds__(256)
det_seg_keys_kernel(const u64* __restrict__ skeys, const int* __restrict__ order, const int* __restrict__ det_img, long n,
                    int n_img, int n_cls, u64* __restrict__ keys, int* __restrict__ vals) {
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (long)blockDim.x * gridDim.x) {
    const int c = (int)(skeys[r] >> 32);
    keys[r] = c >= n_cls ? (u64)n_cls * n_img : (u64)c * n_img + (u64)det_img[order[r]];
    vals[r] = (int)r;
  }
}

__global__ void __launch_bounds__(256)
gt_keys_kernel(const int* __restrict__ gt_img, const int* __restrict__ gt_cls, long g, int n_img, int n_cls,
               u64* __restrict__ keys, int* __restrict__ vals) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < g; i += (long)blockDim.x * gridDim.x) {
    const int c = gt_cls[i], im = gt_img[i];
    const bool ok = c >= 0 && c < n_cls && im >= 0 && im < n_img;
    keys[i] = ok ? (u64)c * n_img + (u64)im : (u64)n_cls * n_img;
    vals[i] = (int)i;
  }
}

__global__ void __launch_bounds__(256)
gt_gather_kernel(const u64* __restrict__ skeys, const int* __restrict__ svals, const float* __restrict__ gt_box,
                 const unsigned char* __restrict__ gt_difficult, long g, int n_img, long n_seg,
                 float4* __restrict__ gsbox, unsigned char* __restrict__ gsdiff, int* __restrict__ npos) {
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < g; p += (long)blockDim.x * gridDim.x) {
    const long i = svals[p];
    gsbox[p] = make_float4(gt_box[i * 4], gt_box[i * 4 + 1], gt_box[i * 4 + 2], gt_box[i * 4 + 3]);
    const unsigned char d = gt_difficult[i] ? 1 : 0;
    gsdiff[p] = d;
    const long seg = (long)skeys[p];
    if (seg < n_seg && !d) atomicAdd(&npos[seg / n_img], 1);  // integer adds: the same count in any order
  }
}

// ---- matching (voc_eval.py:165-199) -------------------------------------------------------------------------------------
// One wavefront per (class, image) segment. Lane l holds ground-truth box 64*k + l of chunk k (chunk 0 in registers);
// lane t < T owns threshold t and its taken bitmap: one 64-bit word per chunk -- chunk 0 in a register, chunks
// 1..EV_LDS_CH-1 in LDS, later chunks (more than 64 * EV_LDS_CH boxes in one segment) in the zeroed global array `ovf`,
// where segment [g0, g1) uses words (g0 >> 6) + k for k >= EV_LDS_CH: above every word of the segments before it.
constexpr int EV_LDS_CH = 32;
constexpr int EV_MAX_THR = 16;

__global__ void __launch_bounds__(256)
match_kernel(const float* __restrict__ det, const int* __restrict__ order, const int* __restrict__ srank,
             const int* __restrict__ doff, const int* __restrict__ goff, const float4* __restrict__ gsbox,
             const unsigned char* __restrict__ gsdiff, const double* __restrict__ thr, int T, long n, long n_seg,
             u64* __restrict__ ovf, long ovf_stride, unsigned char* __restrict__ tpfp) {
  __shared__ u64 lds_taken[4][EV_MAX_THR][EV_LDS_CH - 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long s = (long)blockIdx.x * 4 + w;
  if (s >= n_seg) return;  // (no block-wide barrier below: a wave leaves on its own)
  const int d0 = doff[s], d1 = doff[s + 1];
  if (d0 == d1) return;
  const int g0 = goff[s], ng = goff[s + 1] - g0;
  const int nch = (ng + 63) >> 6;
  if (lane < T)
    for (int k = 1; k < nch && k < EV_LDS_CH; ++k) lds_taken[w][lane][k - 1] = 0;
  u64 taken0 = 0;
  const double th = lane < T ? thr[lane] : 0.;
  double cx1 = 0., cy1 = 0., cx2 = 0., cy2 = 0.;  // chunk 0
  if (lane < ng) {
    const float4 b = gsbox[g0 + lane];
    cx1 = b.x; cy1 = b.y; cx2 = b.z; cy2 = b.w;
  }
  u64* my_ovf = ovf + (long)(lane < T ? lane : 0) * ovf_stride + (g0 >> 6);
  for (int p0 = d0; p0 < d1; p0 += 64) {
    const int cnt = d1 - p0 < 64 ? d1 - p0 : 64;
    int my_rank = 0;
    float mx1 = 0.f, my1 = 0.f, mx2 = 0.f, my2 = 0.f;
    if (lane < cnt) {
      my_rank = srank[p0 + lane];
      const float* b = det + (long)order[my_rank] * 5;
      mx1 = b[0]; my1 = b[1]; mx2 = b[2]; my2 = b[3];
    }
    for (int q = 0; q < cnt; ++q) {
      const int rank = __shfl(my_rank, q);
      const double bx1 = (double)__shfl(mx1, q), by1 = (double)__shfl(my1, q);
      const double bx2 = (double)__shfl(mx2, q), by2 = (double)__shfl(my2, q);
      double best = -INFINITY;  // ovmax
      int bj = 0;               // jmax
      for (int k = 0; k < nch; ++k) {
        const int j = k * 64 + lane;
        double m = -INFINITY;
        if (j < ng) {
          if (k == 0) {
            m = iou_voc(bx1, by1, bx2, by2, cx1, cy1, cx2, cy2);
          } else {
            const float4 b = gsbox[g0 + j];
            m = iou_voc(bx1, by1, bx2, by2, (double)b.x, (double)b.y, (double)b.z, (double)b.w);
          }
        }
        int mj = j;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {  // (max, lowest index): np.max / np.argmax
          const double om = __shfl_xor(m, o);
          const int oj = __shfl_xor(mj, o);
          if (om > m || (om == m && oj < mj)) {
            m = om;
            mj = oj;
          }
        }
        if (m > best) {
          best = m;
          bj = mj;
        }
      }
      if (lane < T) {
        unsigned char code = 2;  // FP
        if (ng > 0 && best > th) {
          if (gsdiff[g0 + bj]) {
            code = 0;  // difficult: neither
          } else {
            const int k = bj >> 6;
            const u64 bit = 1ull << (bj & 63);
            const u64 cur = k == 0 ? taken0 : (k < EV_LDS_CH ? lds_taken[w][lane][k - 1] : my_ovf[k]);
            if (!(cur & bit)) {
              code = 1;  // TP
              if (k == 0) taken0 = cur | bit;
              else if (k < EV_LDS_CH) lds_taken[w][lane][k - 1] = cur | bit;
              else my_ovf[k] = cur | bit;
            }
          }
        }
        tpfp[(long)lane * n + rank] = code;
      }
    }
  }
}

// ---- append -------------------------------------------------------------------------------------------------------------
// destination row dst_base + i, i in [dst_off[p], dst_off[p+1]), comes from source row src_off[p] + (i - dst_off[p])
__global__ void __launch_bounds__(256)
append_kernel(const float* __restrict__ src, const int* __restrict__ dst_off, const int* __restrict__ src_off,
              const int* __restrict__ prob_img, const int* __restrict__ prob_cls, int P, long rows,
              float* __restrict__ det, int* __restrict__ det_img, int* __restrict__ det_cls, long dst_base) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (long)blockDim.x * gridDim.x) {
    int lo = 0, hi = P - 1;  // the last p with dst_off[p] <= i
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (dst_off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    const float* s = src + ((long)src_off[lo] + (i - dst_off[lo])) * 5;
    float* d = det + (dst_base + i) * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) d[k] = s[k];
    det_img[dst_base + i] = prob_img[lo];
    det_cls[dst_base + i] = prob_cls[lo];
  }
}

// ---- workspace layout of dana_eval_ap -----------------------------------------------------------------------------------
struct EvalWs {
  size_t keys_a, keys_b, vals_a, vals_b, hist, doff, goff, gsbox, gsdiff, ovf, cum, total;
};

EvalWs eval_layout(long n, long g, int n_img, int n_cls, int n_thr) {
  EvalWs L;
  const long big = n > g ? n : g;
  const size_t n_seg = (size_t)n_img * n_cls;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += dana_align_up(bytes ? bytes : 1, 256);
    return at;
  };
  L.keys_a = take((size_t)big * 8);
  L.keys_b = take((size_t)big * 8);
  L.vals_a = take((size_t)big * 4);
  L.vals_b = take((size_t)big * 4);
  L.hist = take(rs_hist_bytes(big));
  L.doff = take((n_seg + 1) * 4);
  L.goff = take((n_seg + 1) * 4);
  L.gsbox = take((size_t)g * 16);
  L.gsdiff = take((size_t)g);
  L.ovf = take((size_t)n_thr * ((size_t)(g >> 6) + 1) * 8);
  L.cum = take((size_t)n_thr * (size_t)n * 8);
  L.total = o;
  return L;
}

bool eval_shape_ok(long n, long g, int n_img, int n_cls, int n_thr) {
  return n >= 0 && g >= 0 && n <= EV_MAX_ROWS && g <= EV_MAX_ROWS && n_img >= 1 && n_cls >= 1 && n_thr >= 1 &&
         n_thr <= EV_MAX_THR && (long)n_img * (long)n_cls < (long)INT_MAX;
}

// ==== the COCO protocol (COCOeval evaluateImg / accumulate for iouType = 'bbox', maskApi's bbIou) =======================
// Restated from the published algorithm, not from the reference tree (pycocotools is not part of it). What differs from
// the VOC pipeline above: the global rank is (class, score descending, image, arrival) -- a pre-sort by image in front of
// the stable (class, score) sort gives the image tie-break -- boxes are (x, y, w, h), a crowd object can be matched any
// number of times and divides by the detection's area, ignored objects are a second choice, a segment keeps its first
// max_dets[-1] detections, and the curves are sampled at rec_thrs per (class, area range, maxDets, threshold).
constexpr int CO_MAX_REC = 128;
constexpr int CO_MAX_AREA = 4;
constexpr int CO_MAX_MD = 4;
constexpr int CO_WAVES = 2;  // segments per workgroup of coco_match_kernel: 2 * 31 * 64 bitmap words of LDS

__global__ void __launch_bounds__(256)
coco_img_keys_kernel(const int* __restrict__ det_img, long n, int n_img, u64* __restrict__ keys, int* __restrict__ vals) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)blockDim.x * gridDim.x) {
    const int im = det_img[i];
    keys[i] = im >= 0 && im < n_img ? (u64)im : (u64)n_img;
    vals[i] = (int)i;
  }
}

// det_keys_kernel for the detection vals[p] at position p of the image-sorted list (keys are rewritten in place)
__global__ void __launch_bounds__(256)
coco_det_keys_kernel(const float* __restrict__ det, const int* __restrict__ det_img, const int* __restrict__ det_cls,
                     const int* __restrict__ vals, long n, int n_img, int n_cls, u64* __restrict__ keys) {
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long)blockDim.x * gridDim.x)
    keys[p] = det_key(det, det_img, det_cls, vals[p], n_img, n_cls);
}

// gathered flags of an object: bit 0 = crowd, bit 1 + a = ignored under area range a (ignore | iscrowd | area outside)
__global__ void __launch_bounds__(256)
coco_gt_gather_kernel(const int* __restrict__ svals, const float* __restrict__ gt_bbox, const double* __restrict__ gt_area,
                      const unsigned char* __restrict__ gt_flags, long g, const double* __restrict__ area_rng, int A,
                      float4* __restrict__ gsbox, unsigned char* __restrict__ gsflag) {
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < g; p += (long)blockDim.x * gridDim.x) {
    const long i = svals[p];
    gsbox[p] = make_float4(gt_bbox[i * 4], gt_bbox[i * 4 + 1], gt_bbox[i * 4 + 2], gt_bbox[i * 4 + 3]);
    const unsigned f = gt_flags[i];
    const bool crowd = f & 1u, ign = f & 2u;
    const double area = gt_area[i];
    unsigned o = crowd ? 1u : 0u;
    for (int a = 0; a < A; ++a)
      if (ign || crowd || area < area_rng[2 * a] || area > area_rng[2 * a + 1]) o |= 2u << a;
    gsflag[p] = (unsigned char)o;
  }
}

// npig[c][a]: one workgroup per class counts its gathered objects (positions goff[c * n_img] .. goff[(c + 1) * n_img])
__global__ void __launch_bounds__(256)
coco_npig_kernel(const unsigned char* __restrict__ gsflag, const int* __restrict__ goff, int n_img, int A,
                 int* __restrict__ npig) {
  __shared__ u64 s4[4];
  const int c = blockIdx.x;
  const long p0 = goff[(long)c * n_img], p1 = goff[(long)(c + 1) * n_img];
  for (int a = 0; a < A; ++a) {
    u64 mine = 0;
    for (long p = p0 + threadIdx.x; p < p1; p += 256) mine += (gsflag[p] & (2u << a)) ? 0 : 1;
    u64 tot;
    block_scan_add(mine, tot, s4);
    if (threadIdx.x == 0) npig[c * A + a] = (int)tot;
  }
}

// the value lane j of this wavefront holds (j is the same in every lane)
__device__ __forceinline__ double wave_bcast(double v, int j) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), j), hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
  return __hiloint2double(hi, lo);
}

// One wavefront per (class, image) segment. Lane p = a * T + t < A * T owns the pair (area range a, threshold t) and
// its taken bitmap, in the three tiers of match_kernel (chunk 0 in a register, chunks 1..EV_LDS_CH-1 in LDS, later
// chunks in the zeroed words of `ovf`). Per detection and 64-object chunk the IoUs are computed once, one object per
// lane; every pair lane then walks them in arrival order (a register broadcast per object) and keeps its two choices:
// the best available non-ignored object and the best available ignored one, `>=` so that the last of equal IoUs wins.
// codes[A][T][n] by rank: 1 TP, 2 FP, 0 ignored; rows past max_dets[-1] of their segment keep the 3 they were filled with.
__global__ void __launch_bounds__(64 * CO_WAVES)
coco_match_kernel(const float* __restrict__ det, const int* __restrict__ order, const int* __restrict__ srank,
                  const int* __restrict__ doff, const int* __restrict__ goff, const float4* __restrict__ gsbox,
                  const unsigned char* __restrict__ gsflag, const double* __restrict__ thr, int T,
                  const double* __restrict__ area_rng, int A, const int* __restrict__ max_dets, int M, long n, long n_seg,
                  u64* __restrict__ ovf, long ovf_stride, unsigned char* __restrict__ codes, int* __restrict__ segpos) {
  __shared__ u64 lds_taken[CO_WAVES][EV_LDS_CH - 1][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long s = (long)blockIdx.x * CO_WAVES + w;
  if (s >= n_seg) return;  // (no block-wide barrier below: a wave leaves on its own)
  const int d0 = doff[s], d1 = doff[s + 1];
  if (d0 == d1) return;
  for (int p = d0 + lane; p < d1; p += 64) segpos[srank[p]] = p - d0;
  const int g0 = goff[s], ng = goff[s + 1] - g0;
  const int nch = (ng + 63) >> 6;
  for (int k = 1; k < nch && k < EV_LDS_CH; ++k) lds_taken[w][k - 1][lane] = 0;
  const bool own = lane < A * T;
  const int a = own ? lane / T : 0, t = own ? lane - a * T : 0;
  const double th = fmin(thr[t], 1. - 1e-10);
  const double alo = area_rng[2 * a], ahi = area_rng[2 * a + 1];
  const unsigned igbit = 2u << a;
  const int maxd = max_dets[M - 1];
  const int dend = d1 - d0 > maxd ? d0 + (maxd > 0 ? maxd : 0) : d1;
  u64 taken0 = 0;
  double cx = 0., cy = 0., cw = 0., ch = 0.;  // chunk 0
  unsigned cf = 0;
  if (lane < ng) {
    const float4 b = gsbox[g0 + lane];
    cx = b.x; cy = b.y; cw = b.z; ch = b.w;
    cf = gsflag[g0 + lane];
  }
  u64* my_ovf = ovf + (long)(own ? lane : 0) * ovf_stride + (g0 >> 6);
  for (int p0 = d0; p0 < dend; p0 += 64) {
    const int cnt = dend - p0 < 64 ? dend - p0 : 64;
    int my_rank = 0;
    float mx1 = 0.f, my1 = 0.f, mx2 = 0.f, my2 = 0.f;
    if (lane < cnt) {
      my_rank = srank[p0 + lane];
      const float* b = det + (long)order[my_rank] * 5;
      mx1 = b[0]; my1 = b[1]; mx2 = b[2]; my2 = b[3];
    }
    for (int q = 0; q < cnt; ++q) {
      const int rank = __shfl(my_rank, q);
      const double x1 = (double)__shfl(mx1, q), y1 = (double)__shfl(my1, q);
      const double x2 = (double)__shfl(mx2, q), y2 = (double)__shfl(my2, q);
      const double dw = x2 - x1 + 1., dh = y2 - y1 + 1.;  // coco_split.py:308-312
      const double darea = dw * dh;
      double best_ni = th, best_ig = th;
      int m_ni = -1, m_ig = -1;
      for (int k = 0; k < nch; ++k) {
        const int j = k * 64 + lane;
        double gx = cx, gy = cy, gw = cw, gh = ch;
        unsigned f = cf;
        if (k > 0 && j < ng) {
          const float4 b = gsbox[g0 + j];
          gx = b.x; gy = b.y; gw = b.z; gh = b.w;
          f = gsflag[g0 + j];
        }
        double iou = 0.;
        if (j < ng) {  // bbIou
          const double iw = fmin(x1 + dw, gx + gw) - fmax(x1, gx), ih = fmin(y1 + dh, gy + gh) - fmax(y1, gy);
          if (iw > 0. && ih > 0.) {
            const double i = iw * ih;
            const double u = (f & 1u) ? darea : darea + gw * gh - i;
            iou = i / u;
          }
        }
        u64 cur = 0;
        if (own) cur = k == 0 ? taken0 : (k < EV_LDS_CH ? lds_taken[w][k - 1][lane] : my_ovf[k]);
        const int cn = ng - k * 64 < 64 ? ng - k * 64 : 64;
        for (int jj = 0; jj < cn; ++jj) {
          const double v = wave_bcast(iou, jj);
          const unsigned fj = (unsigned)__builtin_amdgcn_readlane((int)f, jj);
          const bool avail = (fj & 1u) || !((cur >> jj) & 1ull);
          if (avail) {
            if (!(fj & igbit)) {
              if (v >= best_ni) { best_ni = v; m_ni = k * 64 + jj; }
            } else if (v >= best_ig) {
              best_ig = v;
              m_ig = k * 64 + jj;
            }
          }
        }
      }
      if (own) {
        const int m = m_ni >= 0 ? m_ni : m_ig;
        unsigned char code;
        if (m_ni >= 0) code = 1;
        else if (m_ig >= 0) code = 0;
        else code = (darea < alo || darea > ahi) ? 0 : 2;
        if (m >= 0) {
          const int k = m >> 6;
          const u64 bit = 1ull << (m & 63);
          if (k == 0) taken0 |= bit;
          else if (k < EV_LDS_CH) lds_taken[w][k - 1][lane] |= bit;
          else my_ovf[k] |= bit;
        }
        codes[(long)lane * n + rank] = code;
      }
    }
  }
}

// One workgroup per (class k, area range a, maxDets m, threshold t): blockIdx = (k, a * M + m, t). The class's ranks that
// count are those with segpos < max_dets[m] and code 1 or 2. Forward: the TP (low word) / FP (high word) counts in front
// of every tile. Reverse: the in-tile scan again, precision's running max from the class's end, and the sample of
// rec_thrs where the TP count steps: a step from tp - 1 to tp at position i makes i the first position with
// rc >= rec_thr for every (tp - 1) / npig < rec_thr <= tp / npig, and the first position that counts takes every
// rec_thr below that. Each rec_thr has one writer; nothing is summed across threads.
__global__ void __launch_bounds__(256)
coco_accumulate_kernel(const unsigned char* __restrict__ codes, const int* __restrict__ segpos,
                       const float* __restrict__ det, const int* __restrict__ order, const int* __restrict__ cls_off,
                       const int* __restrict__ npig, const double* __restrict__ rec_thrs, int R,
                       const int* __restrict__ max_dets, int T, int A, int M, int K, long n, u64* __restrict__ carry_ws,
                       long carry_stride, double* __restrict__ precision, double* __restrict__ recall,
                       double* __restrict__ scores) {
  __shared__ u64 s4[4];
  __shared__ double d4[4];
  __shared__ double s_thr[CO_MAX_REC], s_prec[CO_MAX_REC], s_score[CO_MAX_REC];
  const int tid = threadIdx.x;
  const int k = blockIdx.x, a = blockIdx.y / M, m = blockIdx.y - a * M, t = blockIdx.z;
  const long r0 = cls_off[k], r1 = cls_off[k + 1];
  const int np_i = npig[k * A + a];
  const double np_d = (double)np_i;
  const int maxd = max_dets[m];
  const unsigned char* flags = codes + ((long)a * T + t) * n;
  u64* carry_of = carry_ws + (((long)a * M + m) * T + t) * carry_stride + (r0 / CV_TILE + k);
  const long out_tail = ((long)k * A + a) * M + m;  // precision / scores [T][R][K][A][M], recall [T][K][A][M]
  const long out_step = (long)K * A * M;
  if (np_i == 0) {
    if (tid < R) {
      precision[((long)t * R + tid) * out_step + out_tail] = -1.;
      scores[((long)t * R + tid) * out_step + out_tail] = -1.;
    }
    if (tid == 0) recall[(long)t * out_step + out_tail] = -1.;
    return;
  }
  if (tid < R) {
    s_thr[tid] = rec_thrs[tid];
    s_prec[tid] = 0.;
    s_score[tid] = 0.;
  }
  const long ntile = (r1 - r0 + CV_TILE - 1) / CV_TILE;
  u64 carry = 0;
  for (long ti = 0; ti < ntile; ++ti) {
    const long i0 = r0 + ti * CV_TILE + (long)tid * CV_ITEMS;
    u64 sum = 0;
#pragma unroll
    for (int j = 0; j < CV_ITEMS; ++j) {
      const long r = i0 + j;
      const unsigned f = (r < r1 && segpos[r] < maxd) ? flags[r] : 0u;
      sum += (u64)(f == 1u) + ((u64)(f == 2u) << 32);
    }
    u64 tot;
    block_scan_add(sum, tot, s4);
    if (tid == 0) carry_of[ti] = carry;
    carry += tot;
  }
  __syncthreads();  // the reverse pass reads the tile carries thread 0 wrote, and s_thr
  double env_carry = 0.;
  for (long ti = ntile - 1; ti >= 0; --ti) {
    const long i0 = r0 + ti * CV_TILE + (long)tid * CV_ITEMS;
    u64 loc[CV_ITEMS];
    unsigned fl[CV_ITEMS];
    u64 sum = 0;
#pragma unroll
    for (int j = 0; j < CV_ITEMS; ++j) {
      const long r = i0 + j;
      const unsigned f = (r < r1 && segpos[r] < maxd) ? flags[r] : 0u;
      fl[j] = (f == 1u || f == 2u) ? f : 0u;
      sum += (u64)(f == 1u) + ((u64)(f == 2u) << 32);
      loc[j] = sum;
    }
    u64 tot;
    const u64 excl = carry_of[ti] + block_scan_add(sum, tot, s4) - sum;
    double pr[CV_ITEMS], sfx[CV_ITEMS];
#pragma unroll
    for (int j = 0; j < CV_ITEMS; ++j) {
      const u64 v = excl + loc[j];
      const double tp = (double)(unsigned)v, fp = (double)(unsigned)(v >> 32);
      pr[j] = fl[j] ? tp / (fp + tp + DBL_EPSILON) : 0.;
    }
    double mx = 0.;
#pragma unroll
    for (int j = CV_ITEMS - 1; j >= 0; --j) {
      mx = fmax(mx, pr[j]);
      sfx[j] = mx;
    }
    double tile_max;
    const double incl = block_rscan_max(mx, tile_max, d4);
    double behind = __shfl_down(incl, 1);  // max over the threads behind this one: the inclusive value of the next
    if ((tid & 63) == 63) behind = 0.;
    __syncthreads();
    if ((tid & 63) == 0) d4[tid >> 6] = incl;
    __syncthreads();
    if ((tid & 63) == 63 && tid < 192) behind = d4[(tid >> 6) + 1];
    behind = fmax(behind, env_carry);
#pragma unroll
    for (int j = CV_ITEMS - 1; j >= 0; --j) {
      if (!fl[j]) continue;
      const u64 v = excl + loc[j];
      const unsigned tp = (unsigned)v, fp = (unsigned)(v >> 32);
      const bool first = tp + fp == 1u;
      if (fl[j] != 1u && !first) continue;
      const double hi = (double)tp / np_d;
      const double lo = first ? -INFINITY : (double)(tp - 1u) / np_d;
      int b = 0, e = R;  // the first rec_thr above lo
      while (b < e) {
        const int mid = (b + e) >> 1;
        if (s_thr[mid] > lo) e = mid; else b = mid + 1;
      }
      if (b < R && s_thr[b] <= hi) {
        const double env = fmax(sfx[j], behind);
        const double sc = (double)det[(long)order[i0 + j] * 5 + 4];
        for (; b < R && s_thr[b] <= hi; ++b) {
          s_prec[b] = env;
          s_score[b] = sc;
        }
      }
    }
    env_carry = fmax(env_carry, tile_max);
  }
  __syncthreads();
  if (tid < R) {
    precision[((long)t * R + tid) * out_step + out_tail] = s_prec[tid];
    scores[((long)t * R + tid) * out_step + out_tail] = s_score[tid];
  }
  if (tid == 0) recall[(long)t * out_step + out_tail] = (double)(unsigned)carry / np_d;
}

struct CocoWs {
  size_t keys_a, keys_b, vals_a, vals_b, hist, doff, goff, gsbox, gsflag, ovf, carry, total;
};

inline long coco_carry_stride(long n, int n_cls) { return n / CV_TILE + (long)n_cls + 1; }

CocoWs coco_layout(long n, long g, int n_img, int n_cls, int n_thr, int n_area, int n_md) {
  CocoWs L;
  const long big = n > g ? n : g;
  const size_t n_seg = (size_t)n_img * n_cls;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += dana_align_up(bytes ? bytes : 1, 256);
    return at;
  };
  L.keys_a = take((size_t)big * 8);
  L.keys_b = take((size_t)big * 8);
  L.vals_a = take((size_t)big * 4);
  L.vals_b = take((size_t)big * 4);
  L.hist = take(rs_hist_bytes(big));
  L.doff = take((n_seg + 1) * 4);
  L.goff = take((n_seg + 1) * 4);
  L.gsbox = take((size_t)g * 16);
  L.gsflag = take((size_t)g);
  L.ovf = take((size_t)n_area * n_thr * ((size_t)(g >> 6) + 1) * 8);
  L.carry = take((size_t)n_area * n_md * n_thr * (size_t)coco_carry_stride(n, n_cls) * 8);
  L.total = o;
  return L;
}

bool coco_params_ok(int n_thr, int n_rec, int n_area, int n_md) {
  return n_thr >= 1 && n_thr <= EV_MAX_THR && n_rec >= 1 && n_rec <= CO_MAX_REC && n_area >= 1 && n_area <= CO_MAX_AREA &&
         n_md >= 1 && n_md <= CO_MAX_MD;
}

}  // namespace

extern "C" {

size_t dana_debug_radix_sort_workspace_bytes(long n) {
  if (n < 0 || n > EV_MAX_ROWS) return 0;
  return 2 * dana_align_up((size_t)n * 8 + 8, 256) + 2 * dana_align_up((size_t)n * 4 + 4, 256) + rs_hist_bytes(n);
}

int dana_debug_radix_sort_pairs(const unsigned long long* keys_in, const int* vals_in, unsigned long long* keys_out,
                                int* vals_out, long n, int key_bits, void* workspace, size_t workspace_bytes,
                                dana_stream_t stream) {
  DANA_CHECK_ARG(n >= 0 && n <= EV_MAX_ROWS && key_bits >= 0 && key_bits <= 64,
                 "dana_debug_radix_sort_pairs: bad shape n=%ld key_bits=%d", n, key_bits);
  if (n == 0) return DANA_OK;
  DANA_CHECK_ARG(keys_in && vals_in && keys_out && vals_out && workspace, "dana_debug_radix_sort_pairs: null pointer");
  if (workspace_bytes < dana_debug_radix_sort_workspace_bytes(n)) {
    dana_set_error("dana_debug_radix_sort_pairs: workspace too small (%zu < %zu)", workspace_bytes,
                   dana_debug_radix_sort_workspace_bytes(n));
    return DANA_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const size_t kb = dana_align_up((size_t)n * 8 + 8, 256), vb = dana_align_up((size_t)n * 4 + 4, 256);
  u64* k[2] = {(u64*)ws, (u64*)(ws + kb)};
  int* v[2] = {(int*)(ws + 2 * kb), (int*)(ws + 2 * kb + vb)};
  unsigned* hist = (unsigned*)(ws + 2 * kb + 2 * vb);
  if (hipMemcpyAsync(k[0], keys_in, (size_t)n * 8, hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipMemcpyAsync(v[0], vals_in, (size_t)n * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
    dana_set_error("dana_debug_radix_sort_pairs: copy in failed");
    return DANA_ERR_HIP;
  }
  const int where = radix_sort(k[0], v[0], k[1], v[1], n, key_bits, hist, st);
  DANA_CHECK_LAUNCH("dana_debug_radix_sort_pairs");
  if (hipMemcpyAsync(keys_out, k[where], (size_t)n * 8, hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipMemcpyAsync(vals_out, v[where], (size_t)n * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
    dana_set_error("dana_debug_radix_sort_pairs: copy out failed");
    return DANA_ERR_HIP;
  }
  return DANA_OK;
}

int dana_eval_append(const float* src_dets, const int* dst_offsets, const int* src_offsets, const int* prob_img,
                     const int* prob_cls, int n_problems, long rows, float* det, int* det_img, int* det_cls,
                     long dst_base, long capacity, dana_stream_t stream) {
  DANA_CHECK_ARG(n_problems >= 0 && rows >= 0 && dst_base >= 0 && capacity >= 0 && rows <= EV_MAX_ROWS &&
                     dst_base <= EV_MAX_ROWS,
                 "dana_eval_append: bad shape n_problems=%d rows=%ld dst_base=%ld", n_problems, rows, dst_base);
  DANA_CHECK_ARG(dst_base + rows <= capacity, "dana_eval_append: %ld + %ld rows exceed the capacity %ld", dst_base, rows,
                 capacity);
  if (rows == 0) return DANA_OK;
  DANA_CHECK_ARG(n_problems > 0, "dana_eval_append: bad shape: %ld rows of no problem", rows);
  DANA_CHECK_ARG(src_dets && dst_offsets && src_offsets && prob_img && prob_cls && det && det_img && det_cls,
                 "dana_eval_append: null pointer");
  append_kernel<<<grid_for(rows), 256, 0, (hipStream_t)stream>>>(src_dets, dst_offsets, src_offsets, prob_img, prob_cls,
                                                                 n_problems, rows, det, det_img, det_cls, dst_base);
  DANA_CHECK_LAUNCH("dana_eval_append");
  return DANA_OK;
}

size_t dana_eval_ap_workspace_bytes(long n, long g, int n_img, int n_cls, int n_thr) {
  if (!eval_shape_ok(n, g, n_img, n_cls, n_thr)) return 0;
  return eval_layout(n, g, n_img, n_cls, n_thr).total;
}

int dana_eval_ap(const float* det, const int* det_img, const int* det_cls, long n, const float* gt_box,
                 const int* gt_img, const int* gt_cls, const unsigned char* gt_difficult, long g, int n_img, int n_cls,
                 const void* iou_thr_, int n_thr, int use_07_metric, int* order, int* cls_offsets, void* tpfp_, void* rec_,
                 void* prec_, void* ap_, int* npos, void* workspace, size_t workspace_bytes, dana_stream_t stream) {
  const double* iou_thr = (const double*)iou_thr_;
  unsigned char* tpfp = (unsigned char*)tpfp_;
  double *rec = (double*)rec_, *prec = (double*)prec_, *ap = (double*)ap_;
  DANA_CHECK_ARG(n_thr >= 1 && n_thr <= EV_MAX_THR, "dana_eval_ap: n_thr=%d outside 1..%d", n_thr, EV_MAX_THR);
  DANA_CHECK_ARG(n >= 0 && g >= 0 && n <= EV_MAX_ROWS && g <= EV_MAX_ROWS && n_img >= 1 && n_cls >= 1,
                 "dana_eval_ap: bad shape n=%ld g=%ld n_img=%d n_cls=%d", n, g, n_img, n_cls);
  DANA_CHECK_ARG((long)n_img * (long)n_cls < (long)INT_MAX, "dana_eval_ap: n_cls * n_img = %d * %d overflows", n_cls,
                 n_img);
  DANA_CHECK_ARG(iou_thr && cls_offsets && ap && npos && workspace, "dana_eval_ap: null pointer");
  DANA_CHECK_ARG(n == 0 || (det && det_img && det_cls && order && tpfp), "dana_eval_ap: null detection pointer");
  DANA_CHECK_ARG(g == 0 || (gt_box && gt_img && gt_cls && gt_difficult), "dana_eval_ap: null ground-truth pointer");
  DANA_CHECK_ARG((rec == nullptr) == (prec == nullptr), "dana_eval_ap: rec and prec are given together or not at all");
  const EvalWs L = eval_layout(n, g, n_img, n_cls, n_thr);
  if (workspace_bytes < L.total) {
    dana_set_error("dana_eval_ap: workspace too small (%zu < %zu)", workspace_bytes, L.total);
    return DANA_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  u64* k[2] = {(u64*)(ws + L.keys_a), (u64*)(ws + L.keys_b)};
  int* v[2] = {(int*)(ws + L.vals_a), (int*)(ws + L.vals_b)};
  unsigned* hist = (unsigned*)(ws + L.hist);
  int* doff = (int*)(ws + L.doff);
  int* goff = (int*)(ws + L.goff);
  float4* gsbox = (float4*)(ws + L.gsbox);
  unsigned char* gsdiff = (unsigned char*)(ws + L.gsdiff);
  u64* ovf = (u64*)(ws + L.ovf);
  u64* cum = (u64*)(ws + L.cum);
  const long n_seg = (long)n_img * n_cls;
  const long ovf_stride = (g >> 6) + 1;
  const int seg_bits = bits_for((u64)n_seg);

  if (hipMemsetAsync(npos, 0, (size_t)n_cls * sizeof(int), st) != hipSuccess ||
      hipMemsetAsync(ovf, 0, (size_t)n_thr * ovf_stride * 8, st) != hipSuccess ||
      (n > 0 && hipMemsetAsync(tpfp, 0, (size_t)n_thr * n, st) != hipSuccess)) {
    dana_set_error("dana_eval_ap: hipMemsetAsync failed");
    return DANA_ERR_HIP;
  }
  // 1. ground truth into (class, image) segments
  const u64* gkeys = k[0];
  if (g > 0) {
    gt_keys_kernel<<<grid_for(g), 256, 0, st>>>(gt_img, gt_cls, g, n_img, n_cls, k[0], v[0]);
    const int where = radix_sort(k[0], v[0], k[1], v[1], g, seg_bits, hist, st);
    gkeys = k[where];
    gt_gather_kernel<<<grid_for(g), 256, 0, st>>>(k[where], v[where], gt_box, gt_difficult, g, n_img, n_seg, gsbox,
                                                  gsdiff, npos);
  }
  seg_offsets_kernel<<<grid_for(g > n_seg ? g : n_seg), 256, 0, st>>>(gkeys, g, 0, n_seg, goff);
  DANA_CHECK_LAUNCH("dana_eval_ap (ground truth)");
  // 2. the global order: class ascending, score descending, arrival ascending
  const u64* skeys = k[0];
  const int* srank = v[0];
  if (n > 0) {
    det_keys_kernel<<<grid_for(n), 256, 0, st>>>(det, det_img, det_cls, n, n_img, n_cls, k[0], v[0]);
    const int w1 = radix_sort(k[0], v[0], k[1], v[1], n, 32 + bits_for((u64)n_cls), hist, st);
    skeys = k[w1];
    if (hipMemcpyAsync(order, v[w1], (size_t)n * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
      dana_set_error("dana_eval_ap: copy of the order failed");
      return DANA_ERR_HIP;
    }
  }
  seg_offsets_kernel<<<grid_for(n > n_cls ? n : n_cls), 256, 0, st>>>(skeys, n, 32, n_cls, cls_offsets);
  // 3. the ranks grouped by (class, image)
  const u64* dkeys = k[0];
  if (n > 0) {
    const int w1 = skeys == k[0] ? 0 : 1;
    det_seg_keys_kernel<<<grid_for(n), 256, 0, st>>>(skeys, order, det_img, n, n_img, n_cls, k[w1 ^ 1], v[w1 ^ 1]);
    const int w2 = radix_sort(k[w1 ^ 1], v[w1 ^ 1], k[w1], v[w1], n, seg_bits, hist, st) ^ w1 ^ 1;
    dkeys = k[w2];
    srank = v[w2];
  }
  seg_offsets_kernel<<<grid_for(n > n_seg ? n : n_seg), 256, 0, st>>>(dkeys, n, 0, n_seg, doff);
  DANA_CHECK_LAUNCH("dana_eval_ap (orderings)");
  // 4. TP / FP marking
  if (n > 0) {
    match_kernel<<<dana_ceil_div(n_seg, 4), 256, 0, st>>>(det, order, srank, doff, goff, gsbox, gsdiff, iou_thr, n_thr, n,
                                                          n_seg, ovf, ovf_stride, tpfp);
    DANA_CHECK_LAUNCH("dana_eval_ap (matching)");
  }
  // 5. curves and AP
  curves_ap_kernel<false><<<dim3((unsigned)n_cls, (unsigned)n_thr), 256, 0, st>>>(tpfp, cls_offsets, npos, n, n_thr,
                                                                           use_07_metric ? 1 : 0, cum, rec, prec, ap);
  DANA_CHECK_LAUNCH("dana_eval_ap (curves)");
  return DANA_OK;
}

size_t dana_eval_coco_workspace_bytes(long n, long g, int n_img, int n_cls, int n_thr, int n_rec, int n_area,
                                      int n_max_dets) {
  if (!eval_shape_ok(n, g, n_img, n_cls, n_thr) || !coco_params_ok(n_thr, n_rec, n_area, n_max_dets)) return 0;
  return coco_layout(n, g, n_img, n_cls, n_thr, n_area, n_max_dets).total;
}

int dana_eval_coco(const float* det, const int* det_img, const int* det_cls, long n, const float* gt_bbox,
                   const int* gt_img, const int* gt_cls, const void* gt_area_, const unsigned char* gt_flags, long g,
                   int n_img, int n_cls, const void* iou_thrs_, int n_thr, const void* rec_thrs_, int n_rec,
                   const void* area_rng_, int n_area, const int* max_dets, int n_max_dets, int* order, int* cls_offsets,
                   int* segpos, void* codes_, int* npig, void* precision_, void* recall_, void* scores_, void* workspace,
                   size_t workspace_bytes, dana_stream_t stream) {
  const double *gt_area = (const double*)gt_area_, *iou_thrs = (const double*)iou_thrs_;
  const double *rec_thrs = (const double*)rec_thrs_, *area_rng = (const double*)area_rng_;
  unsigned char* codes = (unsigned char*)codes_;
  double *precision = (double*)precision_, *recall = (double*)recall_, *scores = (double*)scores_;
  DANA_CHECK_ARG(n_thr >= 1 && n_thr <= EV_MAX_THR, "dana_eval_coco: n_thr=%d outside 1..%d", n_thr, EV_MAX_THR);
  DANA_CHECK_ARG(n_rec >= 1 && n_rec <= CO_MAX_REC, "dana_eval_coco: n_rec=%d outside 1..%d", n_rec, CO_MAX_REC);
  DANA_CHECK_ARG(n_area >= 1 && n_area <= CO_MAX_AREA, "dana_eval_coco: n_area=%d outside 1..%d", n_area, CO_MAX_AREA);
  DANA_CHECK_ARG(n_max_dets >= 1 && n_max_dets <= CO_MAX_MD, "dana_eval_coco: n_max_dets=%d outside 1..%d", n_max_dets,
                 CO_MAX_MD);
  DANA_CHECK_ARG(n >= 0 && g >= 0 && n <= EV_MAX_ROWS && g <= EV_MAX_ROWS && n_img >= 1 && n_cls >= 1,
                 "dana_eval_coco: bad shape n=%ld g=%ld n_img=%d n_cls=%d", n, g, n_img, n_cls);
  DANA_CHECK_ARG((long)n_img * (long)n_cls < (long)INT_MAX, "dana_eval_coco: n_cls * n_img = %d * %d overflows", n_cls,
                 n_img);
  DANA_CHECK_ARG(iou_thrs && rec_thrs && area_rng && max_dets && cls_offsets && npig && precision && recall && scores &&
                     workspace,
                 "dana_eval_coco: null pointer");
  DANA_CHECK_ARG(n == 0 || (det && det_img && det_cls && order && segpos && codes), "dana_eval_coco: null detection pointer");
  DANA_CHECK_ARG(g == 0 || (gt_bbox && gt_img && gt_cls && gt_area && gt_flags), "dana_eval_coco: null ground-truth pointer");
  const CocoWs L = coco_layout(n, g, n_img, n_cls, n_thr, n_area, n_max_dets);
  if (workspace_bytes < L.total) {
    dana_set_error("dana_eval_coco: workspace too small (%zu < %zu)", workspace_bytes, L.total);
    return DANA_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  u64* k[2] = {(u64*)(ws + L.keys_a), (u64*)(ws + L.keys_b)};
  int* v[2] = {(int*)(ws + L.vals_a), (int*)(ws + L.vals_b)};
  unsigned* hist = (unsigned*)(ws + L.hist);
  int* doff = (int*)(ws + L.doff);
  int* goff = (int*)(ws + L.goff);
  float4* gsbox = (float4*)(ws + L.gsbox);
  unsigned char* gsflag = (unsigned char*)(ws + L.gsflag);
  u64* ovf = (u64*)(ws + L.ovf);
  u64* carry = (u64*)(ws + L.carry);
  const long n_seg = (long)n_img * n_cls;
  const long ovf_stride = (g >> 6) + 1;
  const int seg_bits = bits_for((u64)n_seg);
  const int n_pairs = n_area * n_thr;

  if (hipMemsetAsync(ovf, 0, (size_t)n_pairs * ovf_stride * 8, st) != hipSuccess ||
      (n > 0 && (hipMemsetAsync(codes, 3, (size_t)n_pairs * n, st) != hipSuccess ||
                 hipMemsetAsync(segpos, 0xff, (size_t)n * 4, st) != hipSuccess))) {
    dana_set_error("dana_eval_coco: hipMemsetAsync failed");
    return DANA_ERR_HIP;
  }
  // 1. ground truth into (class, image) segments, arrival order inside; npig
  const u64* gkeys = k[0];
  if (g > 0) {
    gt_keys_kernel<<<grid_for(g), 256, 0, st>>>(gt_img, gt_cls, g, n_img, n_cls, k[0], v[0]);
    const int where = radix_sort(k[0], v[0], k[1], v[1], g, seg_bits, hist, st);
    gkeys = k[where];
    coco_gt_gather_kernel<<<grid_for(g), 256, 0, st>>>(v[where], gt_bbox, gt_area, gt_flags, g, area_rng, n_area, gsbox,
                                                       gsflag);
  }
  seg_offsets_kernel<<<grid_for(g > n_seg ? g : n_seg), 256, 0, st>>>(gkeys, g, 0, n_seg, goff);
  coco_npig_kernel<<<(unsigned)n_cls, 256, 0, st>>>(gsflag, goff, n_img, n_area, npig);
  DANA_CHECK_LAUNCH("dana_eval_coco (ground truth)");
  // 2. the global order: class ascending, score descending, image ascending, arrival ascending -- the stable sort by
  //    image first, then the stable sort by (class, score) on top of it
  const u64* skeys = k[0];
  const int* srank = v[0];
  if (n > 0) {
    coco_img_keys_kernel<<<grid_for(n), 256, 0, st>>>(det_img, n, n_img, k[0], v[0]);
    const int w0 = radix_sort(k[0], v[0], k[1], v[1], n, bits_for((u64)n_img), hist, st);
    coco_det_keys_kernel<<<grid_for(n), 256, 0, st>>>(det, det_img, det_cls, v[w0], n, n_img, n_cls, k[w0]);
    const int w1 = radix_sort(k[w0], v[w0], k[w0 ^ 1], v[w0 ^ 1], n, 32 + bits_for((u64)n_cls), hist, st) ^ w0;
    skeys = k[w1];
    if (hipMemcpyAsync(order, v[w1], (size_t)n * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
      dana_set_error("dana_eval_coco: copy of the order failed");
      return DANA_ERR_HIP;
    }
  }
  seg_offsets_kernel<<<grid_for(n > n_cls ? n : n_cls), 256, 0, st>>>(skeys, n, 32, n_cls, cls_offsets);
  // 3. the ranks grouped by (class, image): a segment keeps its rank order, so position = place by score
  const u64* dkeys = k[0];
  if (n > 0) {
    const int w1 = skeys == k[0] ? 0 : 1;
    det_seg_keys_kernel<<<grid_for(n), 256, 0, st>>>(skeys, order, det_img, n, n_img, n_cls, k[w1 ^ 1], v[w1 ^ 1]);
    const int w2 = radix_sort(k[w1 ^ 1], v[w1 ^ 1], k[w1], v[w1], n, seg_bits, hist, st) ^ w1 ^ 1;
    dkeys = k[w2];
    srank = v[w2];
  }
  seg_offsets_kernel<<<grid_for(n > n_seg ? n : n_seg), 256, 0, st>>>(dkeys, n, 0, n_seg, doff);
  DANA_CHECK_LAUNCH("dana_eval_coco (orderings)");
  // 4. matching
  if (n > 0) {
    coco_match_kernel<<<dana_ceil_div(n_seg, CO_WAVES), 64 * CO_WAVES, 0, st>>>(
        det, order, srank, doff, goff, gsbox, gsflag, iou_thrs, n_thr, area_rng, n_area, max_dets, n_max_dets, n, n_seg, ovf,
        ovf_stride, codes, segpos);
    DANA_CHECK_LAUNCH("dana_eval_coco (matching)");
  }
  // 5. precision / recall / scores at rec_thrs
  coco_accumulate_kernel<<<dim3((unsigned)n_cls, (unsigned)(n_area * n_max_dets), (unsigned)n_thr), 256, 0, st>>>(
      codes, segpos, det, order, cls_offsets, npig, rec_thrs, n_rec, max_dets, n_thr, n_area, n_max_dets, n_cls, n, carry,
      coco_carry_stride(n, n_cls), precision, recall, scores);
  DANA_CHECK_LAUNCH("dana_eval_coco (accumulate)");
  return DANA_OK;
}

}  // extern "C"
