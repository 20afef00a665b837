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

}  // extern "C"
