// Class sweep (dana.SupportCache.sweep): each of B query images against each of C cached support sets, laid out as
// B*C problems p = b*C + c. The query side (trunk, RPN-level Q projection, the base_feat half of the RPN conv) runs once
// per image; what is per class runs as one launch batched over the problems. This file holds the pieces that map a
// problem back to its image (p / C) and the class-interleaved attention softmax.
//
// Reference semantics replaced (lib/model/framework/dana.py, not code): the per-class forward of dana.py:87-220 run for
// every class of an image, as inference.py:70-140 does to fill all_boxes[j][i].
#include "common.h"
#include "../../include/dana_hip.h"
#include "attn_segments.h"
#include <float.h>

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// Input row r = (b*hw + i)*C + c of scores[B][hw][C][ld_in] (one GEMM per image over N = C*K1: the C classes' keys
// side by side) -> output row ((b*C + c)*hw + i) of out[B*C][hw][ld_out], with the unary term of problem b*C + c:
//   out[seg*L + l] = (softmax_l(in[seg*L .. +L)) + ugamma * unary[p][seg][l]) * out_scale,  cols nseg*L .. kpad-1 zeroed.
// The per-row arithmetic and its order are attn_softmax_unary_kernel's (attention.hip): C = 1 gives the same bits.
__global__ void __launch_bounds__(256)
attn_softmax_unary_sweep_kernel(const float* __restrict__ scores, float* __restrict__ out,
                                const float* __restrict__ unary, long rows, long hw, int C, long unary_stride, int nseg,
                                int L, long ld_in, long ld_out, int kpad, float ugamma, float out_scale) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long bi = row / C;
  const int c = (int)(row - bi * C);
  const long b = bi / hw, i = bi - b * hw;
  const long p = b * C + c;
  const float* in = scores + row * ld_in;
  float* r = out + (p * hw + i) * ld_out;
  const float* u = unary + p * unary_stride;
  constexpr int RV = 8;
  if (L <= 64 * RV) {
    for (int sgm = 0; sgm < nseg; ++sgm) {
      const float* xi = in + sgm * L;
      float* x = r + sgm * L;
      float v[RV];
      float m = -FLT_MAX;
#pragma unroll
      for (int k = 0; k < RV; ++k) {
        const int l = lane + 64 * k;
        v[k] = l < L ? xi[l] : -FLT_MAX;
        m = fmaxf(m, v[k]);
      }
      m = wave_max(m);
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < RV; ++k)
        if (lane + 64 * k < L) {
          v[k] = expf(v[k] - m);
          s += v[k];
        }
      s = wave_sum(s);
#pragma unroll
      for (int k = 0; k < RV; ++k) {
        const int l = lane + 64 * k;
        if (l < L) x[l] = (v[k] / s + ugamma * u[sgm * L + l]) * out_scale;
      }
    }
    for (int l = nseg * L + lane; l < kpad; l += 64) r[l] = 0.f;
    return;
  }
  for (int sgm = 0; sgm < nseg; ++sgm) {
    const float* xi = in + sgm * L;
    float* x = r + sgm * L;
    float m = -FLT_MAX;
    for (int l = lane; l < L; l += 64) m = fmaxf(m, xi[l]);
    m = wave_max(m);
    float s = 0.f;
    for (int l = lane; l < L; l += 64) {
      const float e = expf(xi[l] - m);
      x[l] = e;
      s += e;
    }
    s = wave_sum(s);
    for (int l = lane; l < L; l += 64) x[l] = (x[l] / s + ugamma * u[sgm * L + l]) * out_scale;
  }
  for (int l = nseg * L + lane; l < kpad; l += 64) r[l] = 0.f;
}

// attn_softmax_unary_sweep_kernel with a per-segment scale seg_scale[p][seg] in place of out_scale (attn_segments.h)
__global__ void __launch_bounds__(256)
attn_softmax_unary_sweep_w_kernel(const float* __restrict__ scores, float* __restrict__ out,
                                  const float* __restrict__ unary, const float* __restrict__ seg_scale, long rows, long hw,
                                  int C, long unary_stride, long scale_stride, int nseg, int L, long ld_in, long ld_out,
                                  int kpad, float ugamma) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long bi = row / C;
  const int c = (int)(row - bi * C);
  const long b = bi / hw, i = bi - b * hw;
  const long p = b * C + c;
  attn_softmax_unary_row_w(scores + row * ld_in, out + (p * hw + i) * ld_out, unary + p * unary_stride,
                           seg_scale + p * scale_stride, nseg, L, kpad, ugamma, lane);
}

// dst row (p*rows + i) <- src row ((p / group)*rows + i), `cols` floats each; one thread per float
__global__ void __launch_bounds__(256)
repeat_rows_grouped_kernel(const float* __restrict__ src, float* __restrict__ dst, long rows, int cols, long ld_src,
                           long ld_dst, int group, long total) {
  for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (long)blockDim.x * gridDim.x) {
    const long r = k / cols;
    const int j = (int)(k - r * cols);
    const long p = r / rows, i = r - p * rows;
    dst[r * ld_dst + j] = src[((p / group) * rows + i) * ld_src + j];
  }
}

// y row (p*rows + i) *= x row ((p / group)*rows + i), float4 lanes (the product of mul_rows_kernel, backward.hip)
__global__ void __launch_bounds__(256)
mul_rows_grouped_kernel(float4* __restrict__ y, const float4* __restrict__ x, long rows, int C4, long ldy4, long ldx4,
                        int group, long total) {
  for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (long)blockDim.x * gridDim.x) {
    const long r = k / C4;
    const int c = (int)(k - r * C4);
    const long p = r / rows, i = r - p * rows;
    const float4 a = x[((p / group) * rows + i) * ldx4 + c];
    float4 v = y[r * ldy4 + c];
    v.x *= a.x;
    v.y *= a.y;
    v.z *= a.z;
    v.w *= a.w;
    y[r * ldy4 + c] = v;
  }
}

// Meta R-CNN's class head over a sweep (meta.py:129-142 per class): one wave per RoI row b*R + r of fc7 [B*R][K], held
// in registers (16-byte loads, K <= 64 * 4 * MH_V); for each of the C classes of its image, problem p = b*C + c:
//   z = (fc7[b*R + r] * vec[p]) . W^T + bias  (the product rounded to fp32 first, as scale_rows_by_group writes it),
//   cls_prob[p*R + r] = softmax_2(z), and the row's rois (column 0 = p) / bbox_pred copied to problem p's block.
constexpr int MH_V = 8;

__global__ void __launch_bounds__(256)
meta_class_head_kernel(const float4* __restrict__ fc7, const float4* __restrict__ vec, const float4* __restrict__ w,
                       const float* __restrict__ bias, const float* __restrict__ rois, const float* __restrict__ bbox,
                       float* __restrict__ cls_prob, float* __restrict__ rois_out, float* __restrict__ bbox_out, int C,
                       int R, int K4, long rows) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long b = row / R, r = row - b * R;
  float4 f[MH_V];
#pragma unroll
  for (int t = 0; t < MH_V; ++t) {
    const int j = lane + 64 * t;
    f[t] = j < K4 ? fc7[row * K4 + j] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const float b0 = bias[0], b1 = bias[1];
  for (int c = 0; c < C; ++c) {
    const long p = b * C + c;
    const float4* v = vec + p * K4;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int t = 0; t < MH_V; ++t) {
      const int j = lane + 64 * t;
      if (j < K4) {
        const float4 a = v[j], w0 = w[j], w1 = w[K4 + j];
        const float x0 = f[t].x * a.x, x1 = f[t].y * a.y, x2 = f[t].z * a.z, x3 = f[t].w * a.w;
        s0 += x0 * w0.x;
        s0 += x1 * w0.y;
        s0 += x2 * w0.z;
        s0 += x3 * w0.w;
        s1 += x0 * w1.x;
        s1 += x1 * w1.y;
        s1 += x2 * w1.z;
        s1 += x3 * w1.w;
      }
    }
    s0 = wave_sum(s0) + b0;
    s1 = wave_sum(s1) + b1;
    const long o = p * R + r;
    if (lane == 0) {
      const float m = fmaxf(s0, s1);
      const float e0 = expf(s0 - m), e1 = expf(s1 - m);
      const float s = e0 + e1;
      cls_prob[o * 2] = e0 / s;
      cls_prob[o * 2 + 1] = e1 / s;
    } else if (lane < 5) {
      rois_out[o * 5 + lane] = rois[row * 5 + lane];
    } else if (lane == 5) {
      rois_out[o * 5] = (float)p;
    } else if (lane < 10) {
      bbox_out[o * 4 + (lane - 6)] = bbox[row * 4 + (lane - 6)];
    }
  }
}

unsigned grid_for(long total) {
  const long g = (total + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));  // 256 CUs x 32 resident blocks, grid-stride the rest
}

}  // namespace

extern "C" {

int dana_attn_softmax_unary_sweep(const float* scores, float* out, const float* unary, int B, int C, long hw,
                                  long unary_stride, int nseg, int length, long ld_in, long ld_out, int kpad,
                                  float unary_gamma, float out_scale, dana_stream_t stream) {
  DANA_CHECK_ARG(B >= 0 && C > 0 && hw > 0 && nseg > 0 && length > 0 && ld_in >= (long)nseg * length &&
                     ld_out >= (long)nseg * length && kpad <= ld_out,
                 "dana_attn_softmax_unary_sweep: bad shape B=%d C=%d hw=%ld nseg=%d L=%d", B, C, hw, nseg, length);
  if (B == 0) return DANA_OK;
  DANA_CHECK_ARG(scores && out && unary, "dana_attn_softmax_unary_sweep: null pointer");
  DANA_CHECK_ARG(scores != out, "dana_attn_softmax_unary_sweep: out of place only (rows move)");
  const long rows = (long)B * C * hw;
  attn_softmax_unary_sweep_kernel<<<dana_ceil_div(rows, 4), 256, 0, (hipStream_t)stream>>>(
      scores, out, unary, rows, hw, C, unary_stride > 0 ? unary_stride : (long)nseg * length, nseg, length, ld_in, ld_out,
      kpad, unary_gamma, out_scale);
  DANA_CHECK_LAUNCH("dana_attn_softmax_unary_sweep");
  return DANA_OK;
}

int dana_attn_softmax_unary_sweep_w(const float* scores, float* out, const float* unary, int B, int C, long hw,
                                    long unary_stride, int nseg, int length, long ld_in, long ld_out, int kpad,
                                    float unary_gamma, const float* seg_scale, long scale_stride, dana_stream_t stream) {
  DANA_CHECK_ARG(B >= 0 && C > 0 && hw > 0 && nseg > 0 && length > 0 && ld_in >= (long)nseg * length &&
                     ld_out >= (long)nseg * length && kpad <= ld_out,
                 "dana_attn_softmax_unary_sweep_w: bad shape B=%d C=%d hw=%ld nseg=%d L=%d", B, C, hw, nseg, length);
  if (B == 0) return DANA_OK;
  DANA_CHECK_ARG(scores && out && unary && seg_scale, "dana_attn_softmax_unary_sweep_w: null pointer");
  DANA_CHECK_ARG(scores != out, "dana_attn_softmax_unary_sweep_w: out of place only (rows move)");
  const long rows = (long)B * C * hw;
  attn_softmax_unary_sweep_w_kernel<<<dana_ceil_div(rows, 4), 256, 0, (hipStream_t)stream>>>(
      scores, out, unary, seg_scale, rows, hw, C, unary_stride > 0 ? unary_stride : (long)nseg * length,
      scale_stride > 0 ? scale_stride : (long)nseg, nseg, length, ld_in, ld_out, kpad, unary_gamma);
  DANA_CHECK_LAUNCH("dana_attn_softmax_unary_sweep_w");
  return DANA_OK;
}

int dana_repeat_rows_grouped(const float* src, float* dst, long rows, int cols, long ld_src, long ld_dst, int group,
                             long n_blocks, dana_stream_t stream) {
  DANA_CHECK_ARG(rows > 0 && cols > 0 && group > 0 && n_blocks >= 0, "dana_repeat_rows_grouped: bad shape");
  if (n_blocks == 0) return DANA_OK;
  DANA_CHECK_ARG(src && dst, "dana_repeat_rows_grouped: null pointer");
  if (ld_src <= 0) ld_src = cols;
  if (ld_dst <= 0) ld_dst = cols;
  DANA_CHECK_ARG(ld_src >= cols && ld_dst >= cols, "dana_repeat_rows_grouped: row strides below cols");
  const long total = n_blocks * rows * cols;
  repeat_rows_grouped_kernel<<<grid_for(total), 256, 0, (hipStream_t)stream>>>(src, dst, rows, cols, ld_src, ld_dst,
                                                                               group, total);
  DANA_CHECK_LAUNCH("dana_repeat_rows_grouped");
  return DANA_OK;
}

int dana_mul_rows_grouped(float* y, const float* x, long rows, int channels, long ld_y, long ld_x, int group,
                          long n_blocks, dana_stream_t stream) {
  DANA_CHECK_ARG(rows > 0 && channels > 0 && channels % 4 == 0 && group > 0 && n_blocks >= 0,
                 "dana_mul_rows_grouped: bad shape");
  if (n_blocks == 0) return DANA_OK;
  DANA_CHECK_ARG(y && x, "dana_mul_rows_grouped: null pointer");
  if (ld_y <= 0) ld_y = channels;
  if (ld_x <= 0) ld_x = channels;
  DANA_CHECK_ARG(ld_y % 4 == 0 && ld_x % 4 == 0 && (((uintptr_t)y | (uintptr_t)x) & 15) == 0,
                 "dana_mul_rows_grouped: strides %% 4 != 0 or unaligned rows");
  const long total = n_blocks * rows * (channels / 4);
  mul_rows_grouped_kernel<<<grid_for(total), 256, 0, (hipStream_t)stream>>>((float4*)y, (const float4*)x, rows,
                                                                            channels / 4, ld_y / 4, ld_x / 4, group, total);
  DANA_CHECK_LAUNCH("dana_mul_rows_grouped");
  return DANA_OK;
}

int dana_meta_class_head(const float* fc7, const float* vec, const float* weight, const float* bias, const float* rois,
                         const float* bbox_pred, float* cls_prob, float* rois_out, float* bbox_out, int B, int C, int R,
                         int K, dana_stream_t stream) {
  DANA_CHECK_ARG(B >= 0 && C > 0 && R > 0 && K > 0 && K % 4 == 0 && K <= 256 * MH_V,
                 "dana_meta_class_head: bad shape B=%d C=%d R=%d K=%d (K %% 4 == 0, K <= %d)", B, C, R, K, 256 * MH_V);
  if (B == 0) return DANA_OK;
  DANA_CHECK_ARG(fc7 && vec && weight && bias && rois && bbox_pred && cls_prob && rois_out && bbox_out,
                 "dana_meta_class_head: null pointer");
  DANA_CHECK_ARG((((uintptr_t)fc7 | (uintptr_t)vec | (uintptr_t)weight) & 15) == 0,
                 "dana_meta_class_head: fc7 / vec / weight not 16-byte aligned");
  const long rows = (long)B * R;
  meta_class_head_kernel<<<dana_ceil_div(rows, 4), 256, 0, (hipStream_t)stream>>>(
      (const float4*)fc7, (const float4*)vec, (const float4*)weight, bias, rois, bbox_pred, cls_prob, rois_out, bbox_out,
      C, R, K / 4, rows);
  DANA_CHECK_LAUNCH("dana_meta_class_head");
  return DANA_OK;
}

}  // extern "C"
