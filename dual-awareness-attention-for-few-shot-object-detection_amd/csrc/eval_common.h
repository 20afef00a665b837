// What the evaluation files share (evaluate.hip: the VOC and COCO protocols; diagnose.hip: the error diagnosis): the
// block-wide scans, the stable radix sort, the segment-offset table, the detection sort key, voc_eval's IoU and the
// curve / AP kernel. Everything sits in an anonymous namespace: each file that includes this header gets its own copy of
// the kernels, and both files are compiled with -ffp-contract=off.
#pragma once
#include "common.h"
#include <float.h>
#include <limits.h>
#include <math.h>

namespace {

typedef unsigned long long u64;

// ---- block-wide scans over 256 threads (4 waves) ----------------------------------------------------------------------
// inclusive prefix sum of v in thread order; total = the block's sum. Two barriers: safe to call back to back.
__device__ __forceinline__ u64 block_scan_add(u64 v, u64& total, u64* lds4) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 up = __shfl_up(v, o);
    if (lane >= o) v += up;
  }
  __syncthreads();
  if (lane == 63) lds4[w] = v;
  __syncthreads();
  u64 base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const u64 x = lds4[k];
    if (k < w) base += x;
    tot += x;
  }
  total = tot;
  return v + base;
}

// inclusive suffix max of v (max over threads >= this one)
__device__ __forceinline__ double block_rscan_max(double v, double& total, double* lds4) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double dn = __shfl_down(v, o);
    if (lane + o < 64) v = fmax(v, dn);
  }
  __syncthreads();
  if (lane == 0) lds4[w] = v;
  __syncthreads();
  double after = 0.0, tot = 0.0;  // every value scanned here is >= 0
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double x = lds4[k];
    if (k > w) after = fmax(after, x);
    tot = fmax(tot, x);
  }
  total = tot;
  return fmax(v, after);
}

// ---- stable LSD radix sort of (64-bit key, 32-bit value) pairs, 8 bits per pass ---------------------------------------
// Three launches per pass: per-tile digit histograms, one scan per digit over the tiles, the scatter. A tile is
// RS_TILE consecutive pairs; inside a tile element j*256 + thread keeps that order, so equal digits keep their order.
constexpr int RS_ITEMS = 16;
constexpr int RS_TILE = 256 * RS_ITEMS;

__global__ void __launch_bounds__(256)
rs_hist_kernel(const u64* __restrict__ keys, long n, int shift, unsigned mask, int nb, unsigned* __restrict__ hist) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const long base = (long)blockIdx.x * RS_TILE;
  for (int j = 0; j < RS_ITEMS; ++j) {
    const long e = base + j * 256 + threadIdx.x;
    if (e < n) atomicAdd(&h[(unsigned)(keys[e] >> shift) & mask], 1u);
  }
  __syncthreads();
  hist[(long)threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];  // digit-major: a digit's tiles are one row
}

// block d: hist[d][0..nb) -> its exclusive prefix over the tiles, totals[d] = the digit's count
__global__ void __launch_bounds__(256)
rs_scan_kernel(unsigned* __restrict__ hist, int nb, unsigned* __restrict__ totals) {
  __shared__ u64 s4[4];
  unsigned* row = hist + (long)blockIdx.x * nb;
  u64 carry = 0;
  for (int base = 0; base < nb; base += 256) {
    const int i = base + threadIdx.x;
    const u64 v = i < nb ? row[i] : 0;
    u64 tot;
    const u64 incl = block_scan_add(v, tot, s4);
    if (i < nb) row[i] = (unsigned)(carry + incl - v);
    carry += tot;
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = (unsigned)carry;
}

__global__ void __launch_bounds__(256)
rs_scatter_kernel(const u64* __restrict__ keys, const int* __restrict__ vals, u64* __restrict__ keys_out,
                  int* __restrict__ vals_out, long n, int shift, unsigned mask, int nb,
                  const unsigned* __restrict__ hist,
                  const unsigned* __restrict__ totals) {
  __shared__ u64 s4[4];
  __shared__ unsigned run[256];     // next output position of each digit for this tile
  __shared__ unsigned cnt[4][256];  // this round's count of each digit per wave
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  {
    const u64 t = totals[tid];
    u64 tot;
    const u64 incl = block_scan_add(t, tot, s4);
    run[tid] = (unsigned)(incl - t) + hist[(long)tid * nb + blockIdx.x];
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt[k][tid] = 0;
  }
  __syncthreads();
  const long base = (long)blockIdx.x * RS_TILE;
  for (int j = 0; j < RS_ITEMS; ++j) {
    const long e = base + j * 256 + tid;
    const bool valid = e < n;
    const u64 key = valid ? keys[e] : 0;
    const unsigned d = (unsigned)(key >> shift) & mask;
    u64 peers = __ballot(valid);  // lanes of this wave that hold the same digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const u64 bal = __ballot(valid && bit);
      peers &= bit ? bal : ~bal;
    }
    const unsigned rank = __popcll(peers & ((1ull << lane) - 1ull));
    if (valid && rank == 0) cnt[w][d] = (unsigned)__popcll(peers);
    __syncthreads();
    if (valid) {
      unsigned pos = run[d] + rank;
      for (int k = 0; k < w; ++k) pos += cnt[k][d];
      keys_out[pos] = key;
      vals_out[pos] = vals[e];
    }
    __syncthreads();
    run[tid] += cnt[0][tid] + cnt[1][tid] + cnt[2][tid] + cnt[3][tid];
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt[k][tid] = 0;
    __syncthreads();
  }
}

inline int rs_tiles(long n) { return (int)((n + RS_TILE - 1) / RS_TILE); }
inline size_t rs_hist_bytes(long n) { return dana_align_up(((size_t)rs_tiles(n) * 256 + 256) * sizeof(unsigned), 256); }

// Sorts the n pairs in (ka, va) by the low `bits` key bits only (higher bits are ignored); kb / vb are the ping-pong buffers. Returns which pair of
// buffers holds the result (0: a, 1: b), or a negative error.
int radix_sort(u64* ka, int* va, u64* kb, int* vb, long n, int bits, unsigned* hist, hipStream_t st) {
  if (n <= 1) return 0;
  const int nb = rs_tiles(n);
  unsigned* totals = hist + (size_t)nb * 256;
  int where = 0;
  for (int shift = 0; shift < bits; shift += 8) {
    const unsigned mask = bits - shift >= 8 ? 255u : (1u << (bits - shift)) - 1u;  // the last pass may be narrower
    rs_hist_kernel<<<nb, 256, 0, st>>>(ka, n, shift, mask, nb, hist);
    rs_scan_kernel<<<256, 256, 0, st>>>(hist, nb, totals);
    rs_scatter_kernel<<<nb, 256, 0, st>>>(ka, va, kb, vb, n, shift, mask, nb, hist, totals);
    u64* tk = ka; ka = kb; kb = tk;
    int* tv = va; va = vb; vb = tv;
    where ^= 1;
  }
  return where;
}

inline int bits_for(u64 max_value) {  // bits needed to hold max_value
  int b = 0;
  while (b < 64 && (max_value >> b)) ++b;
  return b;
}

unsigned grid_for(long total) {
  const long g = (total + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

// (class ascending, score descending); rows whose class or image id is out of range go to the trailing class n_cls
__device__ __forceinline__ u64 det_key(const float* __restrict__ det, const int* __restrict__ det_img,
                                       const int* __restrict__ det_cls, long i, int n_img, int n_cls) {
  const int c = det_cls[i], im = det_img[i];
  const bool ok = c >= 0 && c < n_cls && im >= 0 && im < n_img;
  float s = det[i * 5 + 4];
  if (s == 0.f) s = 0.f;  // -0 and +0 are one score
  const unsigned u = __float_as_uint(s);
  const unsigned ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // ascending in the float order
  return ((u64)(ok ? c : n_cls) << 32) | (u64)(0xffffffffu - ord);
}

// off[s] = first position whose id (keys >> shift) is >= s, for s in 0..max_id (off[max_id] closes the last real
// segment; ids equal to max_id are the out-of-range rows). n == 0: all zero.
__global__ void __launch_bounds__(256)
seg_offsets_kernel(const u64* __restrict__ keys, long n, int shift, long max_id, int* __restrict__ off) {
  const long stride = (long)blockDim.x * gridDim.x;
  const long first = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n == 0) {
    for (long s = first; s <= max_id; s += stride) off[s] = 0;
    return;
  }
  for (long r = first; r < n; r += stride) {
    const long id = (long)(keys[r] >> shift);
    const long prev = r ? (long)(keys[r - 1] >> shift) : -1;
    for (long s = prev + 1; s <= id && s <= max_id; ++s) off[s] = (int)r;
    if (r == n - 1)
      for (long s = id + 1; s <= max_id; ++s) off[s] = (int)n;
  }
}

// voc_eval.py:174-187: float64, the `+ 1.` pixel convention, the reference's operation order
__device__ __forceinline__ double iou_voc(double bx1, double by1, double bx2, double by2, double gx1, double gy1,
                                          double gx2, double gy2) {
  const double ixmin = fmax(gx1, bx1), iymin = fmax(gy1, by1);
  const double ixmax = fmin(gx2, bx2), iymax = fmin(gy2, by2);
  const double iw = fmax(ixmax - ixmin + 1., 0.), ih = fmax(iymax - iymin + 1., 0.);
  const double inters = iw * ih;
  const double uni = ((bx2 - bx1 + 1.) * (by2 - by1 + 1.) + (gx2 - gx1 + 1.) * (gy2 - gy1 + 1.) - inters);
  return inters / uni;
}

// ---- curves and AP (voc_eval.py:202-207, :35-66) ----------------------------------------------------------------------
// One workgroup per (class, threshold). Forward: inclusive counts of TP (low word) and FP (high word) from the class's
// first rank, tile by tile with a carry. Reverse: precision's running max from the class's end, and the AP terms.
constexpr int CV_ITEMS = 8;
constexpr int CV_TILE = 256 * CV_ITEMS;

// (hi, lo) += (x, y) in double-double arithmetic: the unevaluated sum hi + lo carries about 106 bits
__device__ __forceinline__ void dd_add(double& hi, double& lo, double x, double y) {
  const double s = hi + x;
  const double bb = s - hi;
  const double e = ((hi - (s - bb)) + (x - bb)) + (lo + y);
  hi = s + e;
  lo = e - (hi - s);
}

// kExactSum = false: the area metric's terms are added in the workgroup's fixed tree, in plain doubles (the evaluators).
// kExactSum = true: they are added in double-double and rounded once at the end, so the result is the correctly rounded
// sum of the terms whatever the order (the error diagnosis, whose yardstick sums the same terms exactly).
template <bool kExactSum>
__global__ void __launch_bounds__(256)
curves_ap_kernel(const unsigned char* __restrict__ tpfp, const int* __restrict__ cls_off, const int* __restrict__ npos,
                 long n, int n_thr, int use07, u64* __restrict__ cum, double* __restrict__ rec, double* __restrict__ prec,
                 double* __restrict__ ap) {
  __shared__ u64 s4[4];
  __shared__ double d4[4];
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const int c = blockIdx.x, t = blockIdx.y;
  const long r0 = cls_off[c], r1 = cls_off[c + 1];
  const int np_i = npos[c];
  const double np_d = (double)np_i;
  const unsigned char* flags = tpfp + (long)t * n;
  u64* cumt = cum + (long)t * n;
  u64 carry = 0;
  for (long base = r0; base < r1; base += CV_TILE) {
    const long i0 = base + (long)tid * CV_ITEMS;
    u64 loc[CV_ITEMS];
    u64 sum = 0;
#pragma unroll
    for (int j = 0; j < CV_ITEMS; ++j) {
      const long r = i0 + j;
      const unsigned f = r < r1 ? flags[r] : 0u;
      sum += (u64)(f == 1u) + ((u64)(f == 2u) << 32);
      loc[j] = sum;
    }
    u64 tot;
    const u64 excl = carry + block_scan_add(sum, tot, s4) - sum;
#pragma unroll
    for (int j = 0; j < CV_ITEMS; ++j) {
      const long r = i0 + j;
      if (r < r1) {
        const u64 v = excl + loc[j];
        cumt[r] = v;
        if (rec != nullptr) {
          const double tp = (double)(unsigned)v, fp = (double)(unsigned)(v >> 32);
          rec[(long)t * n + r] = tp / np_d;
          prec[(long)t * n + r] = tp / fmax(tp + fp, DBL_EPSILON);
        }
      }
    }
    carry += tot;
  }
  __syncthreads();  // the reverse pass reads counts other threads of this workgroup wrote
  double env_carry = 0.;  // mpre's trailing sentinel
  double acc = 0.;
  double acc_lo = 0.;  // kExactSum: the low word of acc
  double p11[11];
#pragma unroll
  for (int k = 0; k < 11; ++k) p11[k] = 0.;
  const long ntile = (r1 - r0 + CV_TILE - 1) / CV_TILE;
  for (long ti = ntile - 1; ti >= 0; --ti) {
    const long i0 = r0 + ti * CV_TILE + (long)tid * CV_ITEMS;
    double pr[CV_ITEMS], rc[CV_ITEMS], sfx[CV_ITEMS];
    unsigned tpc[CV_ITEMS + 1];
    tpc[0] = (i0 > r0 && i0 <= r1) ? (unsigned)cumt[i0 - 1] : 0u;  // TP count in front of this thread's first rank
#pragma unroll
    for (int j = 0; j < CV_ITEMS; ++j) {
      const long r = i0 + j;
      pr[j] = 0.;
      rc[j] = 0.;
      tpc[j + 1] = tpc[j];
      if (r < r1) {
        const u64 v = cumt[r];
        const double tp = (double)(unsigned)v, fp = (double)(unsigned)(v >> 32);
        tpc[j + 1] = (unsigned)v;
        rc[j] = tp / np_d;
        pr[j] = tp / fmax(tp + fp, DBL_EPSILON);
      }
    }
    double m = 0.;
#pragma unroll
    for (int j = CV_ITEMS - 1; j >= 0; --j) {
      m = fmax(m, pr[j]);
      sfx[j] = m;
    }
    double tile_max;
    const double incl = block_rscan_max(m, tile_max, d4);
    // max over the threads behind this one: the inclusive value of the next thread
    double behind = __shfl_down(incl, 1);
    if ((tid & 63) == 63) behind = 0.;
    __syncthreads();
    if ((tid & 63) == 0) d4[tid >> 6] = incl;
    __syncthreads();
    if ((tid & 63) == 63 && tid < 192) behind = d4[(tid >> 6) + 1];
    behind = fmax(behind, env_carry);
    if (use07) {
#pragma unroll
      for (int j = 0; j < CV_ITEMS; ++j)
        if (i0 + j < r1) {
#pragma unroll
          for (int k = 0; k < 11; ++k)
            if (rc[j] >= (double)k * 0.1) p11[k] = fmax(p11[k], pr[j]);
        }
    } else {
#pragma unroll
      for (int j = CV_ITEMS - 1; j >= 0; --j)
        if (i0 + j < r1 && tpc[j + 1] != tpc[j]) {  // recall changes here
          const double env = fmax(sfx[j], behind);
          const double rprev = tpc[j] ? (double)tpc[j] / np_d : 0.;
          if constexpr (kExactSum) dd_add(acc, acc_lo, (rc[j] - rprev) * env, 0.);
          else acc += (rc[j] - rprev) * env;
        }
    }
    env_carry = fmax(env_carry, tile_max);
  }
  double result;
  if (use07) {
    result = 0.;
    for (int k = 0; k < 11; ++k) {
      __syncthreads();
      red[tid] = p11[k];
      __syncthreads();
      for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] = fmax(red[tid], red[tid + o]);
        __syncthreads();
      }
      result = result + red[0] / 11.;
    }
  } else if constexpr (kExactSum) {
    __shared__ double red_lo[256];
    __syncthreads();
    red[tid] = acc;
    red_lo[tid] = acc_lo;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) {
        double hi = red[tid], lo = red_lo[tid];
        dd_add(hi, lo, red[tid + o], red_lo[tid + o]);
        red[tid] = hi;
        red_lo[tid] = lo;
      }
      __syncthreads();
    }
    result = red[0];  // hi is the rounded hi + lo
  } else {
    __syncthreads();
    red[tid] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {  // fixed tree: the same bits on every run
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    result = red[0];
  }
  if (tid == 0) ap[(long)c * n_thr + t] = np_i > 0 ? result : (double)NAN;
}

constexpr long EV_MAX_ROWS = 1l << 30;

}  // namespace
