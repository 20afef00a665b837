// Error diagnosis on the device (dana_amd/diagnose.py): the TIDE error types (Bolya et al., ECCV 2020) of every false
// positive and every undetected object, and the AP each type costs, on the lists the VOC evaluator accumulates.
//
// Restated from the paper, not from any code (tidecv is not part of the reference tree). Step 1, the TP / FP marking and the
// baseline AP, IS dana_eval_ap at one threshold: this file calls it, so the baseline has the evaluator's bits. Float64,
// IoU with the `+ 1.` convention, unfused (compiled with -ffp-contract=off).
//
// Pipeline of dana_diagnose_errors (every step is its own launch; no workgroup ever waits on another one):
//   1. dana_eval_ap at t_f: order, cls_offsets, tpfp, npos, ap
//   2. the counted objects (in range, not difficult) radix-sorted by image, arrival order inside: boxes, classes and the
//      caller's rows gathered, one offsets table over the images
//   3. the ranks radix-sorted by (class, image) segment
//   4. type_kernel: one wavefront per segment, one detection per lane, 64 at a time; the image's objects pass by in
//      64-object chunks (one object per lane, broadcast in turn) and every lane keeps its same-class and other-class maxima
//      apart. Claims on an object are 64-bit atomicMin on a packed (priority, row) word: no launch order shows in them.
//   5. the objects' states and their counts; the detections' counts and the confusion matrix (integer atomics)
//   6. the eight oracles: five code arrays by rank, two npos tables, and for Cls a code per detection row with a new sort
//      key, one more radix sort and a gather
//   7. curves_ap_kernel, the evaluator's own, once per oracle
#include "common.h"
#include "eval_common.h"
#include "../../include/dana_hip.h"

namespace {

constexpr u64 DG_NONE = ~0ull;
enum { DG_OUT = 0, DG_TP = 1, DG_CLS = 2, DG_LOC = 3, DG_BOTH = 4, DG_DUPE = 5, DG_BKG = 6 };
constexpr int DG_COLS = 7;     // counts[c]: TP, Cls, Loc, Both, Dupe, Bkg, Miss
constexpr int DG_ORACLES = 8;  // ap_fixed: Cls, Loc, Both, Dupe, Bkg, Miss, FP, FN

// counted objects keyed by image, everything else behind them; the states and the claim words start here
__global__ void __launch_bounds__(256)
obj_keys_kernel(const int* __restrict__ gt_img, const int* __restrict__ gt_cls, const unsigned char* __restrict__ gt_difficult,
                long g, int n_img, int n_cls, u64* __restrict__ keys, int* __restrict__ vals,
                unsigned char* __restrict__ gt_state, u64* __restrict__ loc_claim, u64* __restrict__ cls_claim) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < g; i += (long)blockDim.x * gridDim.x) {
    const int c = gt_cls[i], im = gt_img[i];
    const bool counted = c >= 0 && c < n_cls && im >= 0 && im < n_img && !gt_difficult[i];
    keys[i] = counted ? (u64)im : (u64)n_img;
    vals[i] = (int)i;
    gt_state[i] = counted ? 3 : 0;
    loc_claim[i] = DG_NONE;
    cls_claim[i] = DG_NONE;
  }
}

__global__ void __launch_bounds__(256)
obj_gather_kernel(const int* __restrict__ svals, const float* __restrict__ gt_box, const int* __restrict__ gt_cls, long g,
                  float4* __restrict__ obox, int* __restrict__ ocls, int* __restrict__ orow) {
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < g; p += (long)blockDim.x * gridDim.x) {
    const long i = svals[p];
    obox[p] = make_float4(gt_box[i * 4], gt_box[i * 4 + 1], gt_box[i * 4 + 2], gt_box[i * 4 + 3]);
    ocls[p] = gt_cls[i];
    orow[p] = (int)i;
  }
}

// rank r -> its (class, image) segment; value = the rank
__global__ void __launch_bounds__(256)
rank_seg_keys_kernel(const int* __restrict__ order, const int* __restrict__ det_img, const int* __restrict__ det_cls, long n,
                     int n_img, int n_cls, u64* __restrict__ keys, int* __restrict__ vals) {
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (long)blockDim.x * gridDim.x) {
    const long i = order[r];
    const int c = det_cls[i], im = det_img[i];
    const bool ok = c >= 0 && c < n_cls && im >= 0 && im < n_img;
    keys[r] = ok ? (u64)c * n_img + (u64)im : (u64)n_cls * n_img;
    vals[r] = (int)r;
  }
}

// One wavefront per (class, image) segment, one detection per lane. ioff[im] .. ioff[im + 1] are the image's counted
// objects in arrival order, so a strict `>` keeps the lowest index among equal maxima.
__global__ void __launch_bounds__(256)
type_kernel(const float* __restrict__ det, const int* __restrict__ order, const int* __restrict__ srank,
            const int* __restrict__ doff, const int* __restrict__ ioff, const float4* __restrict__ obox,
            const int* __restrict__ ocls, const int* __restrict__ orow, const unsigned char* __restrict__ tpfp,
            const double* __restrict__ thr, int n_img, long n_seg, unsigned char* __restrict__ det_type,
            int* __restrict__ det_ref, unsigned char* __restrict__ gt_state, u64* __restrict__ loc_claim,
            u64* __restrict__ cls_claim) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long s = (long)blockIdx.x * 4 + w;
  if (s >= n_seg) return;  // (no block-wide barrier below: a wave leaves on its own)
  const int d0 = doff[s], d1 = doff[s + 1];
  if (d0 == d1) return;
  const int c = (int)(s / n_img), im = (int)(s - (long)c * n_img);
  const int o0 = ioff[im], no = ioff[im + 1] - o0;
  const double tf = thr[0], tb = thr[1];
  for (int p0 = d0; p0 < d1; p0 += 64) {
    const bool have = p0 + lane < d1;
    int rank = 0, row = 0;
    double bx1 = 0., by1 = 0., bx2 = 0., by2 = 0.;
    unsigned sbits = 0;
    if (have) {
      rank = srank[p0 + lane];
      row = order[rank];
      const float* b = det + (long)row * 5;
      bx1 = b[0]; by1 = b[1]; bx2 = b[2]; by2 = b[3];
      float sc = b[4];
      if (sc == 0.f) sc = 0.f;  // -0 and +0 are one score (det_key)
      const unsigned u = __float_as_uint(sc);
      sbits = 0xffffffffu - ((u & 0x80000000u) ? ~u : (u | 0x80000000u));  // ascending = score descending
    }
    double ov_same = -INFINITY, ov_other = -INFINITY;
    int j_same = -1, j_other = -1;
    for (int k0 = 0; k0 < no; k0 += 64) {
      const int cn = no - k0 < 64 ? no - k0 : 64;
      float4 ob = make_float4(0.f, 0.f, 0.f, 0.f);
      int oc = -1;
      if (lane < cn) {
        ob = obox[o0 + k0 + lane];
        oc = ocls[o0 + k0 + lane];
      }
      for (int jj = 0; jj < cn; ++jj) {
        const double gx1 = (double)__shfl(ob.x, jj), gy1 = (double)__shfl(ob.y, jj);
        const double gx2 = (double)__shfl(ob.z, jj), gy2 = (double)__shfl(ob.w, jj);
        const int gc = __shfl(oc, jj);
        const double v = iou_voc(bx1, by1, bx2, by2, gx1, gy1, gx2, gy2);
        if (gc == c) {
          if (v > ov_same) { ov_same = v; j_same = k0 + jj; }
        } else if (v > ov_other) {
          ov_other = v;
          j_other = k0 + jj;
        }
      }
    }
    if (!have) continue;
    const unsigned code = tpfp[rank];
    unsigned char type = DG_OUT;
    int ref = -1;
    if (code == 1u) {
      type = DG_TP;
      if (j_same >= 0) {
        ref = orow[o0 + j_same];
        gt_state[ref] = 1;  // step 1 gives an object to one detection: one writer
      }
    } else if (code == 2u) {
      if (ov_same > tf) {
        type = DG_DUPE;
        ref = orow[o0 + j_same];
      } else if (ov_same >= tb) {
        type = DG_LOC;
        ref = orow[o0 + j_same];
        atomicMin(&loc_claim[ref], ((u64)(unsigned)rank << 32) | (u64)(unsigned)row);  // the highest-ranked one
      } else if (ov_other > tf) {
        type = DG_CLS;
        ref = orow[o0 + j_other];
        atomicMin(&cls_claim[ref], ((u64)sbits << 32) | (u64)(unsigned)row);  // the highest score, then the lowest row
      } else if (ov_other >= tb) {
        type = DG_BOTH;
        ref = orow[o0 + j_other];
      } else {
        type = DG_BKG;
      }
    }
    det_type[rank] = type;
    det_ref[rank] = ref;
  }
}

// counts[cell] += the number of lanes of this wavefront that name it. Every lane of the wavefront calls this together.
__device__ __forceinline__ void wave_count(u64* __restrict__ counts, int cell, bool valid) {
  const int lane = threadIdx.x & 63;
  u64 todo = __ballot(valid);
  while (todo) {
    const int lead = __ffsll((long long)todo) - 1;
    const int lc = __shfl(cell, lead);
    const u64 same = __ballot(valid && cell == lc);
    if (lane == lead) atomicAdd(&counts[lc], (u64)__popcll(same));
    todo &= ~same;
  }
}

// an undetected object some Loc or Cls detection refers to is covered (2), the others are missed (3)
__global__ void __launch_bounds__(256)
obj_state_kernel(const int* __restrict__ gt_cls, long g, int n_cls, const u64* __restrict__ loc_claim,
                 const u64* __restrict__ cls_claim, unsigned char* __restrict__ gt_state, u64* __restrict__ counts,
                 u64* __restrict__ confusion) {
  for (long b0 = (long)blockIdx.x * 256; b0 < g; b0 += 256l * gridDim.x) {
    const long i = b0 + threadIdx.x;
    unsigned st = 0;
    int c = 0;
    if (i < g) {
      st = gt_state[i];
      c = gt_cls[i];
      if (st == 3u && (loc_claim[i] != DG_NONE || cls_claim[i] != DG_NONE)) {
        st = 2u;
        gt_state[i] = 2;
      }
    }
    wave_count(counts, c * DG_COLS + 6, st == 3u);
    wave_count(confusion, c * (n_cls + 1) + n_cls, st >= 2u);
  }
}

__global__ void __launch_bounds__(256)
det_count_kernel(const int* __restrict__ order, const int* __restrict__ det_cls, const int* __restrict__ gt_cls,
                 const unsigned char* __restrict__ det_type, const int* __restrict__ det_ref, long n, int n_cls,
                 u64* __restrict__ counts, u64* __restrict__ confusion) {
  for (long b0 = (long)blockIdx.x * 256; b0 < n; b0 += 256l * gridDim.x) {
    const long r = b0 + threadIdx.x;
    unsigned type = DG_OUT;
    int c = 0, oc = n_cls;
    if (r < n) {
      type = det_type[r];
      if (type != DG_OUT) {
        c = det_cls[order[r]];
        if (type == DG_TP) oc = c;
        else if (type == DG_CLS) oc = gt_cls[det_ref[r]];
      }
    }
    wave_count(counts, c * DG_COLS + (int)type - 1, type != DG_OUT);
    wave_count(confusion, oc * (n_cls + 1) + c, type != DG_OUT);
  }
}

// Miss: npos loses the missed objects; FN: npos becomes the TP count
__global__ void __launch_bounds__(256)
npos_fixed_kernel(const int* __restrict__ npos, const u64* __restrict__ counts, int n_cls, int* __restrict__ npos_miss,
                  int* __restrict__ npos_fn) {
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n_cls; c += blockDim.x * gridDim.x) {
    npos_miss[c] = npos[c] - (int)counts[c * DG_COLS + 6];
    npos_fn[c] = (int)counts[c * DG_COLS];
  }
}

// codes[5][n] by rank: the marking with Loc / Both / Dupe / Bkg / FP repaired. The Cls oracle moves rows between classes, so
// it is written by detection row (arrival order): its code, and the sort key (new class, score descending).
__global__ void __launch_bounds__(256)
oracle_kernel(const float* __restrict__ det, const int* __restrict__ det_img, const int* __restrict__ det_cls,
              const int* __restrict__ order, const unsigned char* __restrict__ tpfp,
              const unsigned char* __restrict__ det_type, const int* __restrict__ det_ref, const int* __restrict__ gt_cls,
              const unsigned char* __restrict__ gt_state, const u64* __restrict__ loc_claim,
              const u64* __restrict__ cls_claim, long n, int n_img, int n_cls, unsigned char* __restrict__ codes,
              unsigned char* __restrict__ code_row, u64* __restrict__ keys, int* __restrict__ vals) {
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (long)blockDim.x * gridDim.x) {
    const long i = order[r];
    const unsigned char code = tpfp[r];
    const unsigned type = det_type[r];
    const int ref = det_ref[r];
    unsigned char loc = code;
    if (type == DG_LOC) loc = (gt_state[ref] == 2 && (long)(loc_claim[ref] >> 32) == r) ? 1 : 0;
    codes[r] = loc;
    codes[n + r] = type == DG_BOTH ? 0 : code;
    codes[2 * n + r] = type == DG_DUPE ? 0 : code;
    codes[3 * n + r] = type == DG_BKG ? 0 : code;
    codes[4 * n + r] = code == 2 ? 0 : code;
    u64 key = det_key(det, det_img, det_cls, i, n_img, n_cls);
    unsigned char cc = code;
    if (type == DG_CLS) {
      cc = 0;
      if (gt_state[ref] == 2 && (long)(unsigned)cls_claim[ref] == i) {
        cc = 1;
        key = (key & 0xffffffffull) | ((u64)gt_cls[ref] << 32);
      }
    }
    code_row[i] = cc;
    keys[i] = key;
    vals[i] = (int)i;
  }
}

__global__ void __launch_bounds__(256)
code_gather_kernel(const int* __restrict__ svals, const unsigned char* __restrict__ code_row, long n,
                   unsigned char* __restrict__ out) {
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long)blockDim.x * gridDim.x)
    out[p] = code_row[svals[p]];
}

struct DiagWs {
  size_t eval, keys_a, keys_b, vals_a, vals_b, hist, ioff, doff, cls_off, obox, ocls, orow, loc_claim, cls_claim, codes,
      code_row, cum, npos_fixed, total;
};

DiagWs diag_layout(long n, long g, int n_img, int n_cls) {
  DiagWs L;
  const long big = n > g ? n : g;
  const size_t n_seg = (size_t)n_img * n_cls;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += dana_align_up(bytes ? bytes : 1, 256);
    return at;
  };
  L.eval = take(dana_eval_ap_workspace_bytes(n, g, n_img, n_cls, 1));
  L.keys_a = take((size_t)big * 8);
  L.keys_b = take((size_t)big * 8);
  L.vals_a = take((size_t)big * 4);
  L.vals_b = take((size_t)big * 4);
  L.hist = take(rs_hist_bytes(big));
  L.ioff = take(((size_t)n_img + 1) * 4);
  L.doff = take((n_seg + 1) * 4);
  L.cls_off = take(((size_t)n_cls + 1) * 4);
  L.obox = take((size_t)g * 16);
  L.ocls = take((size_t)g * 4);
  L.orow = take((size_t)g * 4);
  L.loc_claim = take((size_t)g * 8);
  L.cls_claim = take((size_t)g * 8);
  L.codes = take((size_t)6 * (size_t)n);  // Loc, Both, Dupe, Bkg, FP by rank; Cls by its own rank
  L.code_row = take((size_t)n);
  L.cum = take((size_t)n * 8);
  L.npos_fixed = take((size_t)2 * n_cls * 4);
  L.total = o;
  return L;
}

bool diag_shape_ok(long n, long g, int n_img, int n_cls) {
  return n >= 0 && g >= 0 && n <= EV_MAX_ROWS && g <= EV_MAX_ROWS && n_img >= 1 && n_cls >= 1 &&
         (long)n_img * (long)n_cls < (long)INT_MAX && ((long)n_cls + 1) * ((long)n_cls + 1) * DG_COLS < (long)INT_MAX;
}

}  // namespace

extern "C" {

size_t dana_diagnose_errors_workspace_bytes(long n, long g, int n_img, int n_cls) {
  if (!diag_shape_ok(n, g, n_img, n_cls)) return 0;
  return diag_layout(n, g, n_img, n_cls).total;
}

int dana_diagnose_errors(const float* det, const int* det_img, const int* det_cls, long n, const float* gt_box,
                         const int* gt_img, const int* gt_cls, const unsigned char* gt_difficult, long g, int n_img,
                         int n_cls, const void* thresholds, int use_07_metric, int* order, int* cls_offsets, void* tpfp_,
                         int* npos, void* ap_, void* det_type_, int* det_ref, void* gt_state_, void* counts_,
                         void* confusion_, void* ap_fixed_, void* workspace, size_t workspace_bytes,
                         dana_stream_t stream) {
  const double* thr = (const double*)thresholds;
  unsigned char *tpfp = (unsigned char*)tpfp_, *det_type = (unsigned char*)det_type_;
  unsigned char* gt_state = (unsigned char*)gt_state_;
  u64 *counts = (u64*)counts_, *confusion = (u64*)confusion_;
  double *ap = (double*)ap_, *ap_fixed = (double*)ap_fixed_;
  DANA_CHECK_ARG(n >= 0 && g >= 0 && n <= EV_MAX_ROWS && g <= EV_MAX_ROWS && n_img >= 1 && n_cls >= 1,
                 "dana_diagnose_errors: bad shape n=%ld g=%ld n_img=%d n_cls=%d", n, g, n_img, n_cls);
  DANA_CHECK_ARG(diag_shape_ok(n, g, n_img, n_cls), "dana_diagnose_errors: n_cls * n_img = %d * %d or (n_cls + 1)^2 overflows",
                 n_cls, n_img);
  DANA_CHECK_ARG(thr && cls_offsets && npos && ap && counts && confusion && ap_fixed && workspace,
                 "dana_diagnose_errors: null pointer");
  DANA_CHECK_ARG(n == 0 || (det && det_img && det_cls && order && tpfp && det_type && det_ref),
                 "dana_diagnose_errors: null detection pointer");
  DANA_CHECK_ARG(g == 0 || (gt_box && gt_img && gt_cls && gt_difficult && gt_state),
                 "dana_diagnose_errors: null ground-truth pointer");
  const DiagWs L = diag_layout(n, g, n_img, n_cls);
  if (workspace_bytes < L.total) {
    dana_set_error("dana_diagnose_errors: workspace too small (%zu < %zu)", workspace_bytes, L.total);
    return DANA_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  u64* k[2] = {(u64*)(ws + L.keys_a), (u64*)(ws + L.keys_b)};
  int* v[2] = {(int*)(ws + L.vals_a), (int*)(ws + L.vals_b)};
  unsigned* hist = (unsigned*)(ws + L.hist);
  int* ioff = (int*)(ws + L.ioff);
  int* doff = (int*)(ws + L.doff);
  int* cls_off = (int*)(ws + L.cls_off);
  float4* obox = (float4*)(ws + L.obox);
  int* ocls = (int*)(ws + L.ocls);
  int* orow = (int*)(ws + L.orow);
  u64* loc_claim = (u64*)(ws + L.loc_claim);
  u64* cls_claim = (u64*)(ws + L.cls_claim);
  unsigned char* codes = (unsigned char*)(ws + L.codes);
  unsigned char* code_row = (unsigned char*)(ws + L.code_row);
  u64* cum = (u64*)(ws + L.cum);
  int* npos_miss = (int*)(ws + L.npos_fixed);
  int* npos_fn = npos_miss + n_cls;
  const long n_seg = (long)n_img * n_cls;

  // 1. the evaluator's marking and AP at t_f (thresholds[0])
  const int rc = dana_eval_ap(det, det_img, det_cls, n, gt_box, gt_img, gt_cls, gt_difficult, g, n_img, n_cls, thr, 1,
                              use_07_metric, order, cls_offsets, tpfp, nullptr, nullptr, ap, npos, ws + L.eval,
                              L.keys_a - L.eval, stream);
  if (rc != DANA_OK) return rc;
  if (hipMemsetAsync(counts, 0, (size_t)n_cls * DG_COLS * 8, st) != hipSuccess ||
      hipMemsetAsync(confusion, 0, (size_t)(n_cls + 1) * (n_cls + 1) * 8, st) != hipSuccess ||
      (n > 0 && (hipMemsetAsync(det_type, 0, (size_t)n, st) != hipSuccess ||
                 hipMemsetAsync(det_ref, 0xff, (size_t)n * 4, st) != hipSuccess))) {
    dana_set_error("dana_diagnose_errors: hipMemsetAsync failed");
    return DANA_ERR_HIP;
  }
  // 2. the counted objects by image
  const u64* okeys = k[0];
  if (g > 0) {
    obj_keys_kernel<<<grid_for(g), 256, 0, st>>>(gt_img, gt_cls, gt_difficult, g, n_img, n_cls, k[0], v[0], gt_state,
                                                 loc_claim, cls_claim);
    const int where = radix_sort(k[0], v[0], k[1], v[1], g, bits_for((u64)n_img), hist, st);
    okeys = k[where];
    obj_gather_kernel<<<grid_for(g), 256, 0, st>>>(v[where], gt_box, gt_cls, g, obox, ocls, orow);
  }
  seg_offsets_kernel<<<grid_for(g > n_img ? g : n_img), 256, 0, st>>>(okeys, g, 0, n_img, ioff);
  DANA_CHECK_LAUNCH("dana_diagnose_errors (ground truth)");
  if (n > 0) {
    // 3. the ranks grouped by (class, image)
    rank_seg_keys_kernel<<<grid_for(n), 256, 0, st>>>(order, det_img, det_cls, n, n_img, n_cls, k[0], v[0]);
    const int w1 = radix_sort(k[0], v[0], k[1], v[1], n, bits_for((u64)n_seg), hist, st);
    seg_offsets_kernel<<<grid_for(n > n_seg ? n : n_seg), 256, 0, st>>>(k[w1], n, 0, n_seg, doff);
    // 4. a type for every detection, the claims
    type_kernel<<<dana_ceil_div(n_seg, 4), 256, 0, st>>>(det, order, v[w1], doff, ioff, obox, ocls, orow, tpfp, thr, n_img,
                                                         n_seg, det_type, det_ref, gt_state, loc_claim, cls_claim);
    DANA_CHECK_LAUNCH("dana_diagnose_errors (typing)");
  }
  // 5. states, counts, confusion
  if (g > 0)
    obj_state_kernel<<<grid_for(g), 256, 0, st>>>(gt_cls, g, n_cls, loc_claim, cls_claim, gt_state, counts, confusion);
  if (n > 0)
    det_count_kernel<<<grid_for(n), 256, 0, st>>>(order, det_cls, gt_cls, det_type, det_ref, n, n_cls, counts, confusion);
  npos_fixed_kernel<<<grid_for(n_cls), 256, 0, st>>>(npos, counts, n_cls, npos_miss, npos_fn);
  DANA_CHECK_LAUNCH("dana_diagnose_errors (counts)");
  // 6. the oracles' markings; the Cls oracle's own order
  const u64* ckeys = k[0];
  unsigned char* codes_cls = codes + 5 * n;
  if (n > 0) {
    oracle_kernel<<<grid_for(n), 256, 0, st>>>(det, det_img, det_cls, order, tpfp, det_type, det_ref, gt_cls, gt_state,
                                               loc_claim, cls_claim, n, n_img, n_cls, codes, code_row, k[0], v[0]);
    const int w2 = radix_sort(k[0], v[0], k[1], v[1], n, 32 + bits_for((u64)n_cls), hist, st);
    ckeys = k[w2];
    code_gather_kernel<<<grid_for(n), 256, 0, st>>>(v[w2], code_row, n, codes_cls);
  }
  seg_offsets_kernel<<<grid_for(n > n_cls ? n : n_cls), 256, 0, st>>>(ckeys, n, 32, n_cls, cls_off);
  DANA_CHECK_LAUNCH("dana_diagnose_errors (oracles)");
  // 7. AP under each oracle, by the evaluator's curve rule: Cls, Loc, Both, Dupe, Bkg, Miss, FP, FN
  const unsigned char* flags[DG_ORACLES] = {codes_cls, codes, codes + n, codes + 2 * n, codes + 3 * n, tpfp, codes + 4 * n,
                                            tpfp};
  const int* offs[DG_ORACLES] = {cls_off, cls_offsets, cls_offsets, cls_offsets, cls_offsets, cls_offsets, cls_offsets,
                                 cls_offsets};
  const int* np[DG_ORACLES] = {npos, npos, npos, npos, npos, npos_miss, npos, npos_fn};
  for (int o = 0; o < DG_ORACLES; ++o)
    curves_ap_kernel<true><<<dim3((unsigned)n_cls, 1u), 256, 0, st>>>(flags[o], offs[o], np[o], n, 1, use_07_metric ? 1 : 0, cum,
                                                                nullptr, nullptr, ap_fixed + (long)o * n_cls);
  DANA_CHECK_LAUNCH("dana_diagnose_errors (curves)");
  return DANA_OK;
}

}  // extern "C"
