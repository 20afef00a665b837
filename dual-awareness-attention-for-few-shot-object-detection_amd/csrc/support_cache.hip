// Cached support sets (dana.SupportCache): the query-independent support tensors of C support sets are encoded once;
// a cached forward of B query images gathers set index[b] of every cached tensor into slot b of its B-batched buffers,
// all tensors and images in ONE launch. The index lives in device memory, so a replay (launch program, hipGraph) reads
// the selection of the moment without being recorded again.
#include "common.h"
#include "../../include/dana_hip.h"

// grid (gx, B): workgroup row b copies block index[b] of every tensor, grid-striding over the block's bytes with 16-byte
// loads / stores where source, destination and block size allow it (4-byte words otherwise: an fp32 block whose size is
// not a multiple of 16 -- un2 is shot * 49 floats -- leaves the odd slots of the destination 4-byte aligned only).
__global__ void __launch_bounds__(256)
gather_blocks_kernel(const char* const* __restrict__ src, char* const* __restrict__ dst,
                     const long long* __restrict__ block_bytes, int n_tensors, const int* __restrict__ index, int n_sets) {
  const int b = blockIdx.y;
  const int sel = index[b];
  if (sel < 0 || sel >= n_sets) return;  // (validated on the host; never read outside a source tensor)
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (int t = 0; t < n_tensors; ++t) {
    const long long nb = block_bytes[t];
    const char* s = src[t] + (long long)sel * nb;
    char* d = dst[t] + (long long)b * nb;
    const uintptr_t al = (uintptr_t)s | (uintptr_t)d | (uintptr_t)nb;
    if ((al & 15) == 0) {
      const long long n16 = nb >> 4;
      const int4* s4 = (const int4*)s;
      int4* d4 = (int4*)d;
      for (long long i = tid; i < n16; i += stride) d4[i] = s4[i];
    } else if ((al & 3) == 0) {
      const long long n4 = nb >> 2;
      const int* s1 = (const int*)s;
      int* d1 = (int*)d;
      for (long long i = tid; i < n4; i += stride) d1[i] = s1[i];
    } else {
      for (long long i = tid; i < nb; i += stride) d[i] = s[i];
    }
  }
}

// Shot views (SupportCache.select / sweep with shots=): dana_gather_blocks with a shot axis. A set's tensor is
// [rows][shot][block]; problem p's destination [rows][m][block] takes shot block view[p][j] of set index[p] in slot j, and
// zeros where view[p][j] is padding (-1): a padding slot is written, never copied, so no unused slot of a set reaches a
// forward. The destination is walked as a flat array of U-sized units (u = (r*m + j)*n + k: consecutive lanes write
// consecutive addresses whatever rows is), U by the three alignment tiers of gather_blocks_kernel.
constexpr int GSB_MAX_SHOT = 64;

template <class U>
__device__ __forceinline__ void gather_shot_units(const char* s, char* d, long long rows, long long nb, int shot, int m,
                                                  const int* sv, long long tid, long long stride) {
  const long long n = nb / (long long)sizeof(U), mn = (long long)m * n, total = rows * mn;
  const U* su = (const U*)s;
  U* du = (U*)d;
  U zero;
  memset(&zero, 0, sizeof(U));
  if (total <= 0x7fffffffLL) {  // (32-bit divisions: every cached tensor of the model)
    const unsigned n32 = (unsigned)n, mn32 = (unsigned)mn;
    for (long long u = tid; u < total; u += stride) {
      const unsigned r = (unsigned)u / mn32, rem = (unsigned)u - r * mn32;
      const unsigned j = rem / n32, k = rem - j * n32;
      const int v = sv[j];
      du[u] = v >= 0 ? su[((long long)r * shot + v) * n + k] : zero;
    }
  } else {
    for (long long u = tid; u < total; u += stride) {
      const long long r = u / mn, rem = u - r * mn;
      const long long j = rem / n, k = rem - j * n;
      const int v = sv[j];
      du[u] = v >= 0 ? su[(r * shot + v) * n + k] : zero;
    }
  }
}

// grid (gx, P): workgroup row p. w[p][j] = 1 / (number of real slots of view p), 0 on padding (block x == 0 writes it).
__global__ void __launch_bounds__(256)
gather_shot_blocks_kernel(const char* const* __restrict__ src, char* const* __restrict__ dst,
                          const long long* __restrict__ rows, const long long* __restrict__ block_bytes, int n_tensors,
                          const int* __restrict__ index, const int* __restrict__ view, float* __restrict__ w, int n_sets,
                          int shot, int m) {
  __shared__ int sv[GSB_MAX_SHOT];
  const int p = blockIdx.y;
  const int sel = index[p];
  if (sel < 0 || sel >= n_sets) return;  // (validated on the host; never read outside a source tensor)
  if ((int)threadIdx.x < m) {
    const int v = view[(long long)p * shot + threadIdx.x];
    sv[threadIdx.x] = (v >= 0 && v < shot) ? v : -1;  // (an out-of-range shot is padding: nothing is read for it)
  }
  __syncthreads();
  if (blockIdx.x == 0 && (int)threadIdx.x < m) {
    int n_real = 0;
    for (int j = 0; j < m; ++j) n_real += sv[j] >= 0;
    w[(long long)p * m + threadIdx.x] = sv[threadIdx.x] >= 0 ? 1.0f / (float)n_real : 0.f;
  }
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (int t = 0; t < n_tensors; ++t) {
    const long long nr = rows[t], nb = block_bytes[t];
    const char* s = src[t] + (long long)sel * nr * shot * nb;
    char* d = dst[t] + (long long)p * nr * m * nb;
    const uintptr_t al = (uintptr_t)s | (uintptr_t)d | (uintptr_t)nb;
    if ((al & 15) == 0)
      gather_shot_units<int4>(s, d, nr, nb, shot, m, sv, tid, stride);
    else if ((al & 3) == 0)
      gather_shot_units<int>(s, d, nr, nb, shot, m, sv, tid, stride);
    else
      gather_shot_units<char>(s, d, nr, nb, shot, m, sv, tid, stride);
  }
}

extern "C" {

int dana_gather_blocks(const void* src_ptrs, const void* dst_ptrs, const long long* block_bytes, int n_tensors,
                       const int* index, int n_sets, int B, dana_stream_t stream) {
  DANA_CHECK_ARG(n_tensors >= 0 && n_sets >= 0 && B >= 0 && B <= 65535, "dana_gather_blocks: bad shape n_tensors=%d "
                 "n_sets=%d B=%d", n_tensors, n_sets, B);
  if (n_tensors == 0 || B == 0) return DANA_OK;
  DANA_CHECK_ARG(src_ptrs && dst_ptrs && block_bytes && index && n_sets > 0, "dana_gather_blocks: null pointer");
  // ~2 048 workgroups in all (8 per CU): a few MB per image leave every lane a handful of 16-byte copies
  int gx = (2048 + B - 1) / B;
  if (gx < 1) gx = 1;
  gather_blocks_kernel<<<dim3(gx, B), 256, 0, (hipStream_t)stream>>>((const char* const*)src_ptrs, (char* const*)dst_ptrs,
                                                                    block_bytes, n_tensors, index, n_sets);
  DANA_CHECK_LAUNCH("dana_gather_blocks");
  return DANA_OK;
}

int dana_gather_shot_blocks(const void* src_ptrs, const void* dst_ptrs, const long long* rows, const long long* block_bytes,
                            int n_tensors, const int* index, const int* view, float* w, int n_sets, int shot, int m, int P,
                            dana_stream_t stream) {
  DANA_CHECK_ARG(n_tensors >= 0 && n_sets >= 0 && P >= 0 && P <= 65535 && shot >= 1 && shot <= GSB_MAX_SHOT && m >= 1 &&
                     m <= shot,
                 "dana_gather_shot_blocks: bad shape n_tensors=%d n_sets=%d P=%d shot=%d m=%d (1 <= m <= shot <= %d)",
                 n_tensors, n_sets, P, shot, m, GSB_MAX_SHOT);
  if (P == 0) return DANA_OK;
  DANA_CHECK_ARG(index && view && w && n_sets > 0 && (n_tensors == 0 || (src_ptrs && dst_ptrs && rows && block_bytes)),
                 "dana_gather_shot_blocks: null pointer");
  int gx = (2048 + P - 1) / P;  // ~2 048 workgroups in all, as dana_gather_blocks
  if (gx < 1) gx = 1;
  gather_shot_blocks_kernel<<<dim3(gx, P), 256, 0, (hipStream_t)stream>>>(
      (const char* const*)src_ptrs, (char* const*)dst_ptrs, rows, block_bytes, n_tensors, index, view, w, n_sets, shot, m);
  DANA_CHECK_LAUNCH("dana_gather_shot_blocks");
  return DANA_OK;
}

}  // extern "C"
