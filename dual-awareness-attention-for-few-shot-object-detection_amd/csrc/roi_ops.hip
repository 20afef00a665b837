// RoIAlign / RoIPool for gfx950 -- HBM-bound gather kernels behind the C ABI.
//
// Replaces the reference's native ops (semantics, not code):
//   RoIAlignForward          lib/model/csrc/cuda/ROIAlign_cuda.cu:64-122
//   RoIAlignBackwardFeature  lib/model/csrc/cuda/ROIAlign_cuda.cu:177-254
//   RoIPoolFForward/Backward lib/model/csrc/cuda/ROIPool_cuda.cu:16-108
//
// Two feature-map layouts:
//   NCHW  -- the layout the reference's `_C.roi_align_forward` contract hands over.
//   NHWC  -- the layout of this build's trunk: one wave per (roi, bin, slice of 256
//            channels), 64 lanes x float4, so every bilinear tap is a fully coalesced
//            16 B/lane read; a channel slice stays on one or two XCDs (its L2 holds the
//            slice of the image the rois come from). Channel counts whose slices do not
//            divide the 8 XCDs: one workgroup per (roi, bin) sweeping all channels.
//
// This file is compiled with -ffp-contract=off so the per-sample arithmetic
// (w1*v1 + w2*v2 + w3*v3 + w4*v4, running sum, final divide) rounds exactly like the
// reference's C++ and like oracle/dana_oracle.c: parity is bit-exact.
#include "common.h"
#include "../../include/dana_hip.h"
#include "../../include/dana_hip_debug.h"
#include <float.h>
#include <stdlib.h>
#include <atomic>

namespace {

// the form of the most recent dana_roi_align_backward (dana_debug_last_roi_align_backward_form; host state only)
std::atomic<int> g_last_roi_align_bwd(0);

struct AxisSample {  // one bilinear sample position along one axis
  int lo, hi;
  float l, h;  // l = frac toward hi, h = 1 - l
  bool empty;
};

// ROIAlign_cuda.cu:22-47 (bilinear_interpolate), split per axis. `size` = H or W.
__device__ __forceinline__ AxisSample axis_sample(float v, int size) {
  AxisSample s;
  s.empty = (v < -1.0f || v > (float)size);
  if (v <= 0.f) v = 0.f;
  int lo = (int)v;
  int hi;
  if (lo >= size - 1) {
    hi = lo = size - 1;
    v = (float)lo;
  } else {
    hi = lo + 1;
  }
  s.lo = lo;
  s.hi = hi;
  s.l = v - (float)lo;
  s.h = 1.f - s.l;
  return s;
}

struct RoiGeom {
  int batch;
  float start_w, start_h, bin_w, bin_h;
  int grid_h, grid_w;
  float count;
};

// ROIAlign_cuda.cu:78-103
__device__ __forceinline__ RoiGeom roi_geom(const float* roi, float scale, int ph, int pw, int sampling_ratio) {
  RoiGeom g;
  g.batch = (int)roi[0];
  g.start_w = roi[1] * scale;
  g.start_h = roi[2] * scale;
  float end_w = roi[3] * scale;
  float end_h = roi[4] * scale;
  float rw = fmaxf(end_w - g.start_w, 1.f);
  float rh = fmaxf(end_h - g.start_h, 1.f);
  g.bin_h = rh / (float)ph;
  g.bin_w = rw / (float)pw;
  g.grid_h = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rh / (float)ph);
  g.grid_w = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rw / (float)pw);
  g.count = (float)(g.grid_h * g.grid_w);
  return g;
}

// ---------------------------------------------------------------------------------
// NCHW forward: one lane per output element, grid-stride.
__global__ void __launch_bounds__(256)
roi_align_fwd_nchw(const float* __restrict__ in, const float* __restrict__ rois, float* __restrict__ out,
                   long total, int C, int H, int W, int PH, int PW, float scale, int sr) {
  for (long index = (long)blockIdx.x * blockDim.x + threadIdx.x; index < total;
       index += (long)blockDim.x * gridDim.x) {
    int pw = (int)(index % PW);
    int ph = (int)((index / PW) % PH);
    int c = (int)((index / PW / PH) % C);
    int n = (int)(index / PW / PH / C);
    RoiGeom g = roi_geom(rois + (long)n * 5, scale, PH, PW, sr);
    const float* plane = in + ((long)g.batch * C + c) * H * W;
    float acc = 0.f;
    for (int iy = 0; iy < g.grid_h; ++iy) {
      float y = g.start_h + ph * g.bin_h + ((float)iy + .5f) * g.bin_h / (float)g.grid_h;
      AxisSample sy = axis_sample(y, H);
      for (int ix = 0; ix < g.grid_w; ++ix) {
        float x = g.start_w + pw * g.bin_w + ((float)ix + .5f) * g.bin_w / (float)g.grid_w;
        AxisSample sx = axis_sample(x, W);
        float val = 0.f;
        if (!(sy.empty || sx.empty)) {
          float v1 = plane[sy.lo * W + sx.lo], v2 = plane[sy.lo * W + sx.hi];
          float v3 = plane[sy.hi * W + sx.lo], v4 = plane[sy.hi * W + sx.hi];
          float w1 = sy.h * sx.h, w2 = sy.h * sx.l, w3 = sy.l * sx.h, w4 = sy.l * sx.l;
          val = w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4;
        }
        acc += val;
      }
    }
    out[index] = acc / g.count;
  }
}

// ---------------------------------------------------------------------------------
// NHWC forward: workgroup = (roi, bin); lane = 4 consecutive channels (float4), stride 256*4.
// (Round 5 built the verdict's alternative -- one workgroup per roi and bin ROW, sample geometry once per workgroup in LDS,
// every feature column fetched once per sample row through a two-column register window, bit-exact -- and measured it SLOWER:
// 120.8 vs ~85 us at the bench's 512 rois with two outputs. A bin row's samples form ONE dependent chain per wave (table
// read -> window decision -> column fetch -> FMAs, up to 9 x 63 samples for the large proposals of this workload), where
// 25 088 one-bin workgroups give the chip 7x as many short independent chains and the L1 absorbs the taps samples share.
// Removed again; the separable non-exact kernel of rounds 3-4 is gone as well.)
// in pixel (b,y,x) lives at in + ((b*H+y)*W+x)*in_pix_stride; out[n][bin][C] (+ optional second
// output out2 = out + add2[bin][C], used to emit the positional-encoded copy in the same pass).
__global__ void __launch_bounds__(256)
roi_align_fwd_nhwc(const float* __restrict__ in, const float* __restrict__ rois, float* __restrict__ out,
                   float* __restrict__ out2, const float* __restrict__ add2,
                   int C, int H, int W, int PH, int PW, float scale, int sr, long in_pix_stride,
                   long out_pix_stride, long out2_pix_stride, int group) {
  // XCD-aware order (block b runs on XCD b % 8): each XCD gets a contiguous run of (roi, bin) pairs, so the 49 bins of
  // a roi -- whose bilinear taps overlap -- and the rois of one image share ONE L2 instead of being dealt over all eight
  const int nwg = gridDim.x * gridDim.y, lin = blockIdx.y * gridDim.x + blockIdx.x;
  const int q8 = nwg / 8, r8 = nwg % 8, xcd = lin % 8;
  const int v = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + lin / 8;
  const int bins = PH * PW;
  const int n = v / bins;
  const int bin = v % bins;
  const int ph = bin / PW, pw = bin % PW;
  RoiGeom g = roi_geom(rois + (long)n * 5, scale, PH, PW, sr);
  // (group > 1: roi column 0 is a class-sweep problem index, its image is problem / group)
  const float* img = in + (long)(g.batch / group) * H * W * in_pix_stride;
  for (int c = threadIdx.x * 4; c < C; c += blockDim.x * 4) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int iy = 0; iy < g.grid_h; ++iy) {
      float y = g.start_h + ph * g.bin_h + ((float)iy + .5f) * g.bin_h / (float)g.grid_h;
      AxisSample sy = axis_sample(y, H);
      for (int ix = 0; ix < g.grid_w; ++ix) {
        float x = g.start_w + pw * g.bin_w + ((float)ix + .5f) * g.bin_w / (float)g.grid_w;
        AxisSample sx = axis_sample(x, W);
        if (sy.empty || sx.empty) continue;  // contributes exactly +0
        const float4 v1 = *(const float4*)(img + ((long)sy.lo * W + sx.lo) * in_pix_stride + c);
        const float4 v2 = *(const float4*)(img + ((long)sy.lo * W + sx.hi) * in_pix_stride + c);
        const float4 v3 = *(const float4*)(img + ((long)sy.hi * W + sx.lo) * in_pix_stride + c);
        const float4 v4 = *(const float4*)(img + ((long)sy.hi * W + sx.hi) * in_pix_stride + c);
        float w1 = sy.h * sx.h, w2 = sy.h * sx.l, w3 = sy.l * sx.h, w4 = sy.l * sx.l;
        acc.x += w1 * v1.x + w2 * v2.x + w3 * v3.x + w4 * v4.x;
        acc.y += w1 * v1.y + w2 * v2.y + w3 * v3.y + w4 * v4.y;
        acc.z += w1 * v1.z + w2 * v2.z + w3 * v3.z + w4 * v4.z;
        acc.w += w1 * v1.w + w2 * v2.w + w3 * v3.w + w4 * v4.w;
      }
    }
    float4 r = make_float4(acc.x / g.count, acc.y / g.count, acc.z / g.count, acc.w / g.count);
    *(float4*)(out + ((long)n * PH * PW + bin) * out_pix_stride + c) = r;
    if (out2) {
      const float4 a = *(const float4*)(add2 + (long)bin * C + c);
      *(float4*)(out2 + ((long)n * PH * PW + bin) * out2_pix_stride + c) =
          make_float4(r.x + a.x, r.y + a.y, r.z + a.z, r.w + a.w);
    }
  }
}

// ---------------------------------------------------------------------------------
// NHWC forward, channel slices pinned to XCDs (end of round 5; the default whenever ceil(C / 256) divides the 8 XCDs).
// Counters of the workgroup-per-bin kernel above on the bench's own proposals (profiles/r5_roi_align_counters.md): every
// XCD works on whole rois, i.e. on all 1024 channels of an image's map -- 9.8 MB touched per image against a 4 MB L2 per
// XCD -- and the launch fetches 1.5x its algorithmic bytes; and its contiguous (roi, bin) run per XCD makes the launch as
// slow as its unluckiest XCD: the same 512 rois sorted by falling size (what a proposal list sorted by score tends to
// look like) take 188 us instead of 80. Here an XCD owns a SLICE of 256 channels (64 lanes x float4 = one full wave load
// per tap) of EVERY roi: with C = 1024 two XCDs share a slice, the rois of one image -- which arrive together -- keep
// 38 x 63 x 1 KB = 2.4 MB of that image in the XCD's L2, and every XCD sees the same mix of small and large rois. One
// wave per (roi, bin, slice); per-channel arithmetic and order are the kernel's above (bit-identical). Measured: memory
// reads per launch halved (TCC_EA0_RDREQ 1.46 M -> 0.83 M), 77-80 us on the bench's rois (as before), 76 us on the
// sorted list (188). What the launch costs is no longer its reads: with every roi shrunk to one sample per bin it still
// takes 55 us -- 205 MB of output rows (the pooled map and its positional-encoded copy) from 100 352 short waves.
__global__ void __launch_bounds__(256)
roi_align_fwd_nhwc_sliced(const float* __restrict__ in, const float* __restrict__ rois, float* __restrict__ out,
                          float* __restrict__ out2, const float* __restrict__ add2,
                          int C, int H, int W, int PH, int PW, float scale, int sr, long in_pix_stride,
                          long out_pix_stride, long out2_pix_stride, int total_bins, int xps, int group) {
  // workgroup b runs on XCD b % 8: XCDs slice * xps .. slice * xps + xps - 1 take that slice's (roi, bin) quadruples in turn
  const int lin = blockIdx.x, xcd = lin & 7, idx = lin >> 3;
  const int slice = xcd / xps, part = xcd - slice * xps;
  const int lane = threadIdx.x & 63;
  const int gb = __builtin_amdgcn_readfirstlane((idx * xps + part) * 4 + (int)(threadIdx.x >> 6));
  if (gb >= total_bins) return;
  const int bins = PH * PW;
  const int n = gb / bins;
  const int bin = gb - n * bins;
  const int ph = bin / PW, pw = bin - ph * PW;
  const RoiGeom g = roi_geom(rois + (long)n * 5, scale, PH, PW, sr);
  const int c = slice * 256 + lane * 4;
  const bool act = c < C;  // (the last slice of a C that is not a multiple of 256: idle lanes read channel 0)
  const float* img = in + (long)(g.batch / group) * H * W * in_pix_stride + (act ? c : 0);
  // (the second output's addend does not depend on the samples: in flight beside the first taps, not behind the last)
  float4 pe = make_float4(0.f, 0.f, 0.f, 0.f);
  if (out2) pe = *(const float4*)(add2 + (long)bin * C + (act ? c : 0));
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int iy = 0; iy < g.grid_h; ++iy) {
    const float y = g.start_h + ph * g.bin_h + ((float)iy + .5f) * g.bin_h / (float)g.grid_h;
    const AxisSample sy = axis_sample(y, H);
    for (int ix = 0; ix < g.grid_w; ++ix) {
      const float x = g.start_w + pw * g.bin_w + ((float)ix + .5f) * g.bin_w / (float)g.grid_w;
      const AxisSample sx = axis_sample(x, W);
      if (sy.empty || sx.empty) continue;  // contributes exactly +0
      const float4 v1 = *(const float4*)(img + ((long)sy.lo * W + sx.lo) * in_pix_stride);
      const float4 v2 = *(const float4*)(img + ((long)sy.lo * W + sx.hi) * in_pix_stride);
      const float4 v3 = *(const float4*)(img + ((long)sy.hi * W + sx.lo) * in_pix_stride);
      const float4 v4 = *(const float4*)(img + ((long)sy.hi * W + sx.hi) * in_pix_stride);
      const float w1 = sy.h * sx.h, w2 = sy.h * sx.l, w3 = sy.l * sx.h, w4 = sy.l * sx.l;
      acc.x += w1 * v1.x + w2 * v2.x + w3 * v3.x + w4 * v4.x;
      acc.y += w1 * v1.y + w2 * v2.y + w3 * v3.y + w4 * v4.y;
      acc.z += w1 * v1.z + w2 * v2.z + w3 * v3.z + w4 * v4.z;
      acc.w += w1 * v1.w + w2 * v2.w + w3 * v3.w + w4 * v4.w;
    }
  }
  if (!act) return;
  const float4 r = make_float4(acc.x / g.count, acc.y / g.count, acc.z / g.count, acc.w / g.count);
  *(float4*)(out + ((long)n * bins + bin) * out_pix_stride + c) = r;
  if (out2)
    *(float4*)(out2 + ((long)n * bins + bin) * out2_pix_stride + c) = make_float4(r.x + pe.x, r.y + pe.y, r.z + pe.z, r.w + pe.w);
}

// total weight the sample lattice of one bin puts on feature row / column `cell` (the gather backward below)

__device__ __forceinline__ float axis_weight(int cell, int n_samples, float start, float bin, int idx, int size) {
  float w = 0.f;
  for (int i = 0; i < n_samples; ++i) {
    const float v = start + idx * bin + ((float)i + .5f) * bin / (float)n_samples;
    const AxisSample s = axis_sample(v, size);
    if (s.empty) continue;
    if (s.lo == cell) w += s.h;
    if (s.hi == cell) w += s.l;
  }
  return w;
}

// ---------------------------------------------------------------------------------
// Backward (NCHW and NHWC): scatter grad*w/count to the four taps with fp32 atomics
// (ROIAlign_cuda.cu:233-250; summation order is not deterministic there either).
template <bool NHWC>
__global__ void __launch_bounds__(256)
roi_align_bwd(const float* __restrict__ gout, const float* __restrict__ rois, float* __restrict__ gin,
              long total, int C, int H, int W, int PH, int PW, float scale, int sr) {
  for (long index = (long)blockIdx.x * blockDim.x + threadIdx.x; index < total;
       index += (long)blockDim.x * gridDim.x) {
    int pw, ph, c, n;
    if (NHWC) {  // gout [n][ph][pw][c]
      c = (int)(index % C);
      pw = (int)((index / C) % PW);
      ph = (int)((index / C / PW) % PH);
      n = (int)(index / C / PW / PH);
    } else {  // gout [n][c][ph][pw]
      pw = (int)(index % PW);
      ph = (int)((index / PW) % PH);
      c = (int)((index / PW / PH) % C);
      n = (int)(index / PW / PH / C);
    }
    RoiGeom g = roi_geom(rois + (long)n * 5, scale, PH, PW, sr);
    const float go = gout[index];
    for (int iy = 0; iy < g.grid_h; ++iy) {
      float y = g.start_h + ph * g.bin_h + ((float)iy + .5f) * g.bin_h / (float)g.grid_h;
      AxisSample sy = axis_sample(y, H);
      for (int ix = 0; ix < g.grid_w; ++ix) {
        float x = g.start_w + pw * g.bin_w + ((float)ix + .5f) * g.bin_w / (float)g.grid_w;
        AxisSample sx = axis_sample(x, W);
        if (sy.empty || sx.empty) continue;
        float w1 = sy.h * sx.h, w2 = sy.h * sx.l, w3 = sy.l * sx.h, w4 = sy.l * sx.l;
        float g1 = go * w1 / g.count, g2 = go * w2 / g.count, g3 = go * w3 / g.count, g4 = go * w4 / g.count;
        if (NHWC) {
          float* base = gin + (long)g.batch * H * W * C + c;
          atomicAdd(base + ((long)sy.lo * W + sx.lo) * C, g1);
          atomicAdd(base + ((long)sy.lo * W + sx.hi) * C, g2);
          atomicAdd(base + ((long)sy.hi * W + sx.lo) * C, g3);
          atomicAdd(base + ((long)sy.hi * W + sx.hi) * C, g4);
        } else {
          float* base = gin + ((long)g.batch * C + c) * H * W;
          atomicAdd(base + sy.lo * W + sx.lo, g1);
          atomicAdd(base + sy.lo * W + sx.hi, g2);
          atomicAdd(base + sy.hi * W + sx.lo, g3);
          atomicAdd(base + sy.hi * W + sx.hi, g4);
        }
      }
    }
  }
}

// NHWC backward, one workgroup per (roi, bin) like the forward: the bilinear weight of a sample is separable, so the
// weights of all grid_h x grid_w samples of the bin collapse to a row vector times a column vector over the few
// feature pixels the bin touches -- one atomic per touched pixel and channel instead of four per sample, and the
// geometry is computed once per workgroup instead of once per element. Used for maps of at most RB_MAX x RB_MAX pixels.
constexpr int RB_MAX = 128;  // lo / hi are clamped to the map, so a bin never spans more than the map side
__global__ void __launch_bounds__(256)
roi_align_bwd_nhwc_bins(const float* __restrict__ gout, const float* __restrict__ rois, float* __restrict__ gin, int C,
                        int H, int W, int PH, int PW, float scale, int sr) {
  __shared__ float wy[RB_MAX], wx[RB_MAX];
  __shared__ int base[2], span[2];
  const int n = blockIdx.x, bin = blockIdx.y;
  const int ph = bin / PW, pw = bin % PW;
  const RoiGeom g = roi_geom(rois + (long)n * 5, scale, PH, PW, sr);
  for (int i = threadIdx.x; i < 2 * RB_MAX; i += blockDim.x) (i < RB_MAX ? wy : wx)[i % RB_MAX] = 0.f;
  __syncthreads();
  if (threadIdx.x == 0 || threadIdx.x == 64) {  // one lane per axis (different waves)
    const bool ax = threadIdx.x == 64;  // false: rows, true: columns
    const int grid = ax ? g.grid_w : g.grid_h, size = ax ? W : H;
    const float start = ax ? g.start_w + pw * g.bin_w : g.start_h + ph * g.bin_h, bsz = ax ? g.bin_w : g.bin_h;
    float* wv = ax ? wx : wy;
    int b0 = -1, last = -1;
    for (int i = 0; i < grid; ++i) {
      const AxisSample sa = axis_sample(start + ((float)i + .5f) * bsz / (float)grid, size);
      if (sa.empty) continue;
      if (b0 < 0) b0 = sa.lo;  // sample positions increase with i, so do lo / hi
      if (sa.hi - b0 < RB_MAX) {
        wv[sa.lo - b0] += sa.h;
        wv[sa.hi - b0] += sa.l;
      }
      last = sa.hi;
    }
    base[ax] = b0;
    span[ax] = b0 < 0 ? 0 : last - b0 + 1;
  }
  __syncthreads();
  const int ry = span[0], rx = span[1];
  if (ry == 0 || rx == 0) return;  // every sample of the bin falls outside the map
  const int y0 = base[0], x0 = base[1];
  const float inv = 1.f / g.count;
  const float* go = gout + ((long)n * PH * PW + bin) * C;
  float* img = gin + (long)g.batch * H * W * C;
  // lanes own consecutive channels: one atomic instruction covers 256 contiguous bytes of the feature gradient
  for (int r = 0; r < ry; ++r) {
    const float wr = wy[r] * inv;
    if (wr == 0.f) continue;
    for (int q = 0; q < rx; ++q) {
      const float wgt = wr * wx[q];
      if (wgt == 0.f) continue;
      float* p = img + ((long)(y0 + r) * W + x0 + q) * C;
      for (int c = threadIdx.x; c < C; c += blockDim.x) atomicAdd(p + c, go[c] * wgt);
    }
  }
}

// NHWC backward as a GATHER (round 3): one workgroup per 2 x 2 tile of feature cells, each wave owns 256 channels
// (float4 per lane). The wave tests 64 rois at a time against the tile (lane = roi, one ballot), and for every roi that
// can touch it computes -- one lane per entry -- the row / column weights its bins' sample lattices put on the tile's two
// rows and two columns (the separable weights of the kernels above: at most 8 bins per axis), parks them in LDS, and
// adds w_y w_x / count times the bin's gradient row to the four cells' accumulators: every gradient row is read once
// per tile it touches, the feature gradient is WRITTEN ONCE, no atomics, no memset, and the sum runs in a fixed
// (roi, bin) order -- bit-reproducible, which the scatter of ROIAlign_cuda.cu:233-250 is not.
constexpr int GB_MAXP = 8;  // pooled height / width the gather kernel supports (else: the atomic kernel)
__global__ void __launch_bounds__(256)
roi_align_bwd_gather_nhwc(const float* __restrict__ gout, const float* __restrict__ rois, float* __restrict__ gin, int R,
                          int C, int H, int W, int PH, int PW, float scale, int sr, int tiles_y, int tiles_x) {
  __shared__ float wsm[4][4 * GB_MAXP];  // per wave: wy(row 0), wy(row 1), wx(col 0), wx(col 1) for up to 8 bins each
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = tiles_y * tiles_x;
  const int b = blockIdx.x / per, t = blockIdx.x - b * per;
  const int y0 = (t / tiles_x) * 2, x0 = (t % tiles_x) * 2;
  const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);  // (a tile at the map's edge repeats its last row / column)
  const bool has_y1 = y0 + 1 < H, has_x1 = x0 + 1 < W;
  float* wv = wsm[wave];
  const int P2 = PH * PW;
  for (int c0 = wave * 256; c0 < C; c0 += 1024) {
    const int c = c0 + lane * 4;
    const bool c_ok = c < C;
    float4 a00 = make_float4(0.f, 0.f, 0.f, 0.f), a01 = a00, a10 = a00, a11 = a00;
    for (int rb = 0; rb < R; rb += 64) {
      const int r = rb + lane;
      bool hit = false;
      if (r < R) {
        const float* roi = rois + (long)r * 5;
        if ((int)roi[0] == b) {
          // conservative cell box of the roi: samples lie in [start, start + max(size, 1)], each touches floor and floor + 1
          const float sw = roi[1] * scale, sh = roi[2] * scale;
          const float ew = sw + fmaxf(roi[3] * scale - sw, 1.f), eh = sh + fmaxf(roi[4] * scale - sh, 1.f);
          hit = (float)(y0 - 1) <= eh && (float)(y1 + 1) >= sh && (float)(x0 - 1) <= ew && (float)(x1 + 1) >= sw;
        }
      }
      unsigned long long mask = __ballot(hit);
      while (mask) {
        const int bit = __builtin_ctzll(mask);
        mask &= mask - 1;
        const int rr = rb + bit;
        const RoiGeom g = roi_geom(rois + (long)rr * 5, scale, PH, PW, sr);
        // bins whose lattice can reach the tile's rows / columns (a sample at v touches cells floor(v), floor(v) + 1;
        // v < 0 clamps to 0, v > size - 1 to size - 1)
        int ph_lo = (int)floorf(((float)(y0 - 1) - g.start_h) / g.bin_h), ph_hi = (int)floorf(((float)(y1 + 1) - g.start_h) / g.bin_h);
        int pw_lo = (int)floorf(((float)(x0 - 1) - g.start_w) / g.bin_w), pw_hi = (int)floorf(((float)(x1 + 1) - g.start_w) / g.bin_w);
        if (y0 == 0) ph_lo = 0;
        if (y1 == H - 1) ph_hi = PH - 1;
        if (x0 == 0) pw_lo = 0;
        if (x1 == W - 1) pw_hi = PW - 1;
        ph_lo = max(ph_lo, 0); ph_hi = min(ph_hi, PH - 1);
        pw_lo = max(pw_lo, 0); pw_hi = min(pw_hi, PW - 1);
        if (ph_lo > ph_hi || pw_lo > pw_hi) continue;
        const int nph = ph_hi - ph_lo + 1, npw = pw_hi - pw_lo + 1;
        {  // lanes 0..31: one weight each
          const int which = lane >> 3, k = lane & 7;  // 0: wy row y0, 1: wy row y1, 2: wx col x0, 3: wx col x1
          float w = 0.f;
          if (lane < 32) {
            if (which < 2) {
              if (k < nph && (which == 0 || has_y1)) w = axis_weight(which ? y1 : y0, g.grid_h, g.start_h, g.bin_h, ph_lo + k, H);
            } else {
              if (k < npw && (which == 2 || has_x1)) w = axis_weight(which == 3 ? x1 : x0, g.grid_w, g.start_w, g.bin_w, pw_lo + k, W);
            }
            wv[lane] = w;
          }
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the wave's own LDS writes are done (one wave: no barrier)
        __builtin_amdgcn_wave_barrier();
        const float inv = 1.f / g.count;
        for (int i = 0; i < nph; ++i) {
          const float wy0 = wv[i] * inv, wy1 = wv[GB_MAXP + i] * inv;
          if (wy0 == 0.f && wy1 == 0.f) continue;
          for (int j = 0; j < npw; ++j) {
            const float wx0 = wv[2 * GB_MAXP + j], wx1 = wv[3 * GB_MAXP + j];
            if (wx0 == 0.f && wx1 == 0.f) continue;
            if (c_ok) {
              const float4 gv = *(const float4*)(gout + ((long)rr * P2 + (ph_lo + i) * PW + pw_lo + j) * C + c);
              const float w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1;
              a00.x += w00 * gv.x; a00.y += w00 * gv.y; a00.z += w00 * gv.z; a00.w += w00 * gv.w;
              a01.x += w01 * gv.x; a01.y += w01 * gv.y; a01.z += w01 * gv.z; a01.w += w01 * gv.w;
              a10.x += w10 * gv.x; a10.y += w10 * gv.y; a10.z += w10 * gv.z; a10.w += w10 * gv.w;
              a11.x += w11 * gv.x; a11.y += w11 * gv.y; a11.z += w11 * gv.z; a11.w += w11 * gv.w;
            }
          }
        }
        __builtin_amdgcn_wave_barrier();  // (the next roi's weights overwrite wv)
      }
    }
    if (c_ok) {
      float* img = gin + (long)b * H * W * C + c;
      *(float4*)(img + ((long)y0 * W + x0) * C) = a00;
      if (has_x1) *(float4*)(img + ((long)y0 * W + x1) * C) = a01;
      if (has_y1) *(float4*)(img + ((long)y1 * W + x0) * C) = a10;
      if (has_y1 && has_x1) *(float4*)(img + ((long)y1 * W + x1) * C) = a11;
    }
  }
}

// ---------------------------------------------------------------------------------
// RoIPool (NCHW): ROIPool_cuda.cu:16-77 forward (max + int32 argmax), :79-108 backward.
__global__ void __launch_bounds__(256)
roi_pool_fwd_nchw(const float* __restrict__ in, const float* __restrict__ rois, float* __restrict__ out,
                  int* __restrict__ argmax, long total, int C, int H, int W, int PH, int PW, float scale) {
  for (long index = (long)blockIdx.x * blockDim.x + threadIdx.x; index < total;
       index += (long)blockDim.x * gridDim.x) {
    int pw = (int)(index % PW);
    int ph = (int)((index / PW) % PH);
    int c = (int)((index / PW / PH) % C);
    int n = (int)(index / PW / PH / C);
    const float* roi = rois + (long)n * 5;
    int b = (int)roi[0];
    int rsw = (int)roundf(roi[1] * scale), rsh = (int)roundf(roi[2] * scale);
    int rew = (int)roundf(roi[3] * scale), reh = (int)roundf(roi[4] * scale);
    int rw = max(rew - rsw + 1, 1), rh = max(reh - rsh + 1, 1);
    float bh = (float)rh / (float)PH, bw = (float)rw / (float)PW;
    int hs = (int)floorf((float)ph * bh), ws = (int)floorf((float)pw * bw);
    int he = (int)ceilf((float)(ph + 1) * bh), we = (int)ceilf((float)(pw + 1) * bw);
    hs = min(max(hs + rsh, 0), H);
    he = min(max(he + rsh, 0), H);
    ws = min(max(ws + rsw, 0), W);
    we = min(max(we + rsw, 0), W);
    bool empty = (he <= hs) || (we <= ws);
    float m = empty ? 0.f : -FLT_MAX;
    int mi = -1;
    const float* plane = in + ((long)b * C + c) * H * W;
    for (int h = hs; h < he; ++h)
      for (int w = ws; w < we; ++w) {
        float v = plane[h * W + w];
        if (v > m) {
          m = v;
          mi = h * W + w;
        }
      }
    out[index] = m;
    argmax[index] = mi;
  }
}

__global__ void __launch_bounds__(256)
roi_pool_bwd_nchw(const float* __restrict__ gout, const int* __restrict__ argmax, const float* __restrict__ rois,
                  float* __restrict__ gin, long total, int C, int H, int W, int PH, int PW) {
  for (long index = (long)blockIdx.x * blockDim.x + threadIdx.x; index < total;
       index += (long)blockDim.x * gridDim.x) {
    int c = (int)((index / PW / PH) % C);
    int n = (int)(index / PW / PH / C);
    int b = (int)rois[(long)n * 5];
    int a = argmax[index];
    if (a != -1) atomicAdd(gin + ((long)b * C + c) * H * W + a, gout[index]);
  }
}

int stream_grid(long total, int block) {
  long g = (total + block - 1) / block;
  return (int)(g < 8192 ? (g < 1 ? 1 : g) : 8192);  // 256 CUs x 32 resident blocks, grid-stride the rest
}

}  // namespace

extern "C" {

static int roi_align_forward_impl(const float* input, const float* rois, float* output, int batch, int channels,
                                  int height, int width, int num_rois, float spatial_scale, int pooled_h,
                                  int pooled_w, int sampling_ratio, int layout, long in_pix_stride,
                                  long out_pix_stride, float* output2, const float* add2, long out2_pix_stride, int group,
                                  dana_stream_t stream) {
  DANA_CHECK_ARG(batch >= 0 && channels > 0 && height > 0 && width > 0 && num_rois >= 0 && pooled_h > 0 &&
                     pooled_w > 0,
                 "dana_roi_align_forward: bad shape B=%d C=%d H=%d W=%d R=%d P=%dx%d", batch, channels, height,
                 width, num_rois, pooled_h, pooled_w);
  if (num_rois == 0) return DANA_OK;  // ROIAlign_cuda.cu:278-281: empty -> no launch
  DANA_CHECK_ARG(input && rois && output, "dana_roi_align_forward: null pointer");
  hipStream_t s = (hipStream_t)stream;
  DANA_CHECK_ARG(group > 0 && (group == 1 || layout == DANA_LAYOUT_NHWC), "dana_roi_align_forward: group %d (NHWC only)",
                 group);
  if (layout == DANA_LAYOUT_NCHW) {
    DANA_CHECK_ARG(!output2, "dana_roi_align_forward: second output is NHWC-only");
    long total = (long)num_rois * channels * pooled_h * pooled_w;
    roi_align_fwd_nchw<<<stream_grid(total, 256), 256, 0, s>>>(input, rois, output, total, channels, height, width,
                                                              pooled_h, pooled_w, spatial_scale, sampling_ratio);
  } else if (layout == DANA_LAYOUT_NHWC) {
    if (in_pix_stride <= 0) in_pix_stride = channels;
    if (out_pix_stride <= 0) out_pix_stride = channels;
    if (out2_pix_stride <= 0) out2_pix_stride = channels;
    DANA_CHECK_ARG(channels % 4 == 0 && in_pix_stride % 4 == 0 && out_pix_stride % 4 == 0 &&
                       out2_pix_stride % 4 == 0,
                   "dana_roi_align_forward: NHWC needs C and pixel strides %% 4 == 0");
    DANA_CHECK_ARG(!output2 || add2, "dana_roi_align_forward: output2 needs add2");
    const int nsl = (channels + 255) / 256;  // channel slices of 256
    const long total_bins = (long)num_rois * pooled_h * pooled_w;
    if (nsl <= 8 && 8 % nsl == 0 && total_bins < (1l << 28)) {
      const int xps = 8 / nsl;  // XCDs per slice
      const long quads = (total_bins + 3) / 4;
      roi_align_fwd_nhwc_sliced<<<(unsigned)(8 * ((quads + xps - 1) / xps)), 256, 0, s>>>(
          input, rois, output, output2, add2, channels, height, width, pooled_h, pooled_w, spatial_scale, sampling_ratio,
          in_pix_stride, out_pix_stride, out2_pix_stride, (int)total_bins, xps, group);
    } else {  // (a slice count that does not divide the 8 XCDs: every workgroup sweeps all channels of its bin)
      dim3 grid(num_rois, pooled_h * pooled_w);
      roi_align_fwd_nhwc<<<grid, 256, 0, s>>>(input, rois, output, output2, add2, channels, height, width, pooled_h,
                                              pooled_w, spatial_scale, sampling_ratio, in_pix_stride,
                                              out_pix_stride, out2_pix_stride, group);
    }
  } else {
    DANA_CHECK_ARG(false, "dana_roi_align_forward: unknown layout %d", layout);
  }
  DANA_CHECK_LAUNCH("dana_roi_align_forward");
  return DANA_OK;
}

int dana_roi_align_forward(const float* input, const float* rois, float* output, int batch, int channels,
                           int height, int width, int num_rois, float spatial_scale, int pooled_h,
                           int pooled_w, int sampling_ratio, int layout, long in_pix_stride,
                           long out_pix_stride, float* output2, const float* add2, long out2_pix_stride,
                           dana_stream_t stream) {
  return roi_align_forward_impl(input, rois, output, batch, channels, height, width, num_rois, spatial_scale, pooled_h,
                                pooled_w, sampling_ratio, layout, in_pix_stride, out_pix_stride, output2, add2,
                                out2_pix_stride, 1, stream);
}

int dana_roi_align_forward_nhwc_grouped(const float* input, const float* rois, float* output, int batch, int channels,
                                        int height, int width, int num_rois, float spatial_scale, int pooled,
                                        int sampling_ratio, long in_pix_stride, long out_pix_stride, float* output2,
                                        const float* add2, long out2_pix_stride, int group, dana_stream_t stream) {
  return roi_align_forward_impl(input, rois, output, batch, channels, height, width, num_rois, spatial_scale, pooled,
                                pooled, sampling_ratio, DANA_LAYOUT_NHWC, in_pix_stride, out_pix_stride, output2, add2,
                                out2_pix_stride, group, stream);
}

int dana_roi_align_backward(const float* grad_out, const float* rois, float* grad_in, int batch, int channels,
                            int height, int width, int num_rois, float spatial_scale, int pooled_h,
                            int pooled_w, int sampling_ratio, int layout, dana_stream_t stream) {
  DANA_CHECK_ARG(batch >= 0 && channels > 0 && height > 0 && width > 0 && num_rois >= 0,
                 "dana_roi_align_backward: bad shape");
  hipStream_t s = (hipStream_t)stream;
  if (layout == DANA_LAYOUT_NHWC && num_rois > 0 && batch > 0 && channels % 4 == 0 && pooled_h <= GB_MAXP &&
      pooled_w <= GB_MAXP && ((uintptr_t)grad_out & 15) == 0 && ((uintptr_t)grad_in & 15) == 0) {
    // gather form: writes every cell once (no memset), deterministic
    DANA_CHECK_ARG(grad_out && rois && grad_in, "dana_roi_align_backward: null pointer");
    const int ty = (height + 1) / 2, tx = (width + 1) / 2;
    roi_align_bwd_gather_nhwc<<<batch * ty * tx, 256, 0, s>>>(grad_out, rois, grad_in, num_rois, channels, height, width,
                                                              pooled_h, pooled_w, spatial_scale, sampling_ratio, ty, tx);
    DANA_CHECK_LAUNCH("dana_roi_align_backward(gather)");
    g_last_roi_align_bwd.store(DANA_ROI_ALIGN_BWD_GATHER, std::memory_order_relaxed);
    return DANA_OK;
  }
  size_t bytes = (size_t)batch * channels * height * width * sizeof(float);
  if (bytes) {
    DANA_CHECK_ARG(grad_in, "dana_roi_align_backward: null grad_in");
    if (hipMemsetAsync(grad_in, 0, bytes, s) != hipSuccess) {  // ROIAlign_cuda.cu:316 zero-init
      dana_set_error("dana_roi_align_backward: memset failed");
      return DANA_ERR_HIP;
    }
  }
  if (num_rois == 0) {
    g_last_roi_align_bwd.store(DANA_ROI_ALIGN_BWD_MEMSET, std::memory_order_relaxed);
    return DANA_OK;
  }
  DANA_CHECK_ARG(grad_out && rois, "dana_roi_align_backward: null pointer");
  long total = (long)num_rois * channels * pooled_h * pooled_w;
  int form = DANA_ROI_ALIGN_BWD_SCATTER_NHWC;
  if (layout == DANA_LAYOUT_NCHW) {
    form = DANA_ROI_ALIGN_BWD_SCATTER_NCHW;
    roi_align_bwd<false><<<stream_grid(total, 256), 256, 0, s>>>(grad_out, rois, grad_in, total, channels, height,
                                                                 width, pooled_h, pooled_w, spatial_scale,
                                                                 sampling_ratio);
  } else if (channels % 4 == 0 && height <= RB_MAX && width <= RB_MAX && pooled_h * pooled_w <= 65535 &&
           ((uintptr_t)grad_out & 15) == 0) {
    dim3 grid(num_rois, pooled_h * pooled_w);
    form = DANA_ROI_ALIGN_BWD_BINS;
    roi_align_bwd_nhwc_bins<<<grid, 256, 0, s>>>(grad_out, rois, grad_in, channels, height, width, pooled_h, pooled_w,
                                                 spatial_scale, sampling_ratio);
  } else
    roi_align_bwd<true><<<stream_grid(total, 256), 256, 0, s>>>(grad_out, rois, grad_in, total, channels, height,
                                                                width, pooled_h, pooled_w, spatial_scale,
                                                                sampling_ratio);
  DANA_CHECK_LAUNCH("dana_roi_align_backward");
  g_last_roi_align_bwd.store(form, std::memory_order_relaxed);
  return DANA_OK;
}

int dana_debug_last_roi_align_backward_form(void) { return g_last_roi_align_bwd.load(std::memory_order_relaxed); }

int dana_roi_pool_forward(const float* input, const float* rois, float* output, int* argmax, int batch,
                          int channels, int height, int width, int num_rois, float spatial_scale, int pooled_h,
                          int pooled_w, dana_stream_t stream) {
  DANA_CHECK_ARG(batch >= 0 && channels > 0 && height > 0 && width > 0 && num_rois >= 0,
                 "dana_roi_pool_forward: bad shape");
  if (num_rois == 0) return DANA_OK;
  DANA_CHECK_ARG(input && rois && output && argmax, "dana_roi_pool_forward: null pointer");
  long total = (long)num_rois * channels * pooled_h * pooled_w;
  roi_pool_fwd_nchw<<<stream_grid(total, 256), 256, 0, (hipStream_t)stream>>>(
      input, rois, output, argmax, total, channels, height, width, pooled_h, pooled_w, spatial_scale);
  DANA_CHECK_LAUNCH("dana_roi_pool_forward");
  return DANA_OK;
}

int dana_roi_pool_backward(const float* grad_out, const int* argmax, const float* rois, float* grad_in,
                           int batch, int channels, int height, int width, int num_rois, int pooled_h,
                           int pooled_w, dana_stream_t stream) {
  DANA_CHECK_ARG(batch >= 0 && channels > 0 && height > 0 && width > 0 && num_rois >= 0,
                 "dana_roi_pool_backward: bad shape");
  hipStream_t s = (hipStream_t)stream;
  size_t bytes = (size_t)batch * channels * height * width * sizeof(float);
  if (bytes) {
    DANA_CHECK_ARG(grad_in, "dana_roi_pool_backward: null grad_in");
    if (hipMemsetAsync(grad_in, 0, bytes, s) != hipSuccess) {
      dana_set_error("dana_roi_pool_backward: memset failed");
      return DANA_ERR_HIP;
    }
  }
  if (num_rois == 0) return DANA_OK;
  DANA_CHECK_ARG(grad_out && argmax && rois, "dana_roi_pool_backward: null pointer");
  long total = (long)num_rois * channels * pooled_h * pooled_w;
  roi_pool_bwd_nchw<<<stream_grid(total, 256), 256, 0, s>>>(grad_out, argmax, rois, grad_in, total, channels,
                                                            height, width, pooled_h, pooled_w);
  DANA_CHECK_LAUNCH("dana_roi_pool_backward");
  return DANA_OK;
}

}  // extern "C"
