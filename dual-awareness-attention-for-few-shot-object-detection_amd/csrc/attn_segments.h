// The attention softmax row with a per-segment output scale (shot views of unequal length: a problem's segment s is
// scaled by seg_scale[s] = 1 / len(view), 0 on a padding slot). Shared by dana_attn_softmax_unary_w (attention.hip, in
// place: in == out) and dana_attn_softmax_unary_sweep_w (class_sweep.hip, out of place).
#pragma once
#include <float.h>

__device__ __forceinline__ float attn_w_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float attn_w_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// One wave per row: out[seg*L + l] = (softmax_l(in[seg*L .. +L)) + ugamma * u[seg*L + l]) * sc[seg]; a segment whose
// scale is 0 is not read and comes back as +0.0f (sc is the same in every lane: the branch is wave-uniform); columns
// nseg*L .. kpad-1 are zeroed. The per-row arithmetic and its order are attn_softmax_unary_kernel's (attention.hip): with
// every scale equal to its out_scale the row has the same bits.
__device__ __forceinline__ void attn_softmax_unary_row_w(const float* in, float* out, const float* __restrict__ u,
                                                         const float* __restrict__ sc, int nseg, int L, int kpad,
                                                         float ugamma, int lane) {
  constexpr int RV = 8;  // a segment of up to 512 scores stays in registers, as in attn_softmax_unary_kernel
  for (int sgm = 0; sgm < nseg; ++sgm) {
    const float* xi = in + sgm * L;
    float* x = out + sgm * L;
    const float out_scale = sc[sgm];
    if (out_scale == 0.f) {
      for (int l = lane; l < L; l += 64) x[l] = 0.f;
      continue;
    }
    if (L <= 64 * RV) {
      float v[RV];
      float m = -FLT_MAX;
#pragma unroll
      for (int i = 0; i < RV; ++i) {
        const int l = lane + 64 * i;
        v[i] = l < L ? xi[l] : -FLT_MAX;
        m = fmaxf(m, v[i]);
      }
      m = attn_w_wave_max(m);
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < RV; ++i)
        if (lane + 64 * i < L) {
          v[i] = expf(v[i] - m);
          s += v[i];
        }
      s = attn_w_wave_sum(s);
#pragma unroll
      for (int i = 0; i < RV; ++i) {
        const int l = lane + 64 * i;
        if (l < L) x[l] = (v[i] / s + ugamma * u[sgm * L + l]) * out_scale;
      }
    } else {
      float m = -FLT_MAX;
      for (int l = lane; l < L; l += 64) m = fmaxf(m, xi[l]);
      m = attn_w_wave_max(m);
      float s = 0.f;
      for (int l = lane; l < L; l += 64) {
        const float e = expf(xi[l] - m);
        x[l] = e;
        s += e;
      }
      s = attn_w_wave_sum(s);
      for (int l = lane; l < L; l += 64) x[l] = (x[l] / s + ugamma * u[sgm * L + l]) * out_scale;
    }
  }
  for (int l = nseg * L + lane; l < kpad; l += 64) out[l] = 0.f;
}
