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

// Support bank (dana.SupportBank): the weight-independent support tensors of a pool of N images -- map_pe [N][L][C], the
// trunk map + PE, and pool_pe [N][P][C], its average pool + PE -- are encoded once; a training iteration over a frozen trunk
// names its B*way*shot supports by bank row. Slot s = (b, r), r = s % (way*shot), with n = index[s]:
//   every slot    pool_pe[n] -> block s of sp_pe [B*way*shot][P][C]
//   r < shot      map_pe[n]  -> block (b, r) of s_pe [B][shot*L][C]   (the positives come first: dana.py:103-104)
// grid (gx, slots): workgroup row s walks the slot's 16-byte units, the P*C/4 of the pooled block first, then (positives)
// the L*C/4 of the map block; a workgroup takes BANK_UNROLL * 256 consecutive units, each lane BANK_UNROLL of them 256
// apart (all loads issued before the first store). Workgroups past a negative slot's pooled units leave at once.
constexpr int BANK_UNROLL = 4;

__global__ void __launch_bounds__(256)
bank_gather_episode_kernel(const float4* __restrict__ map_pe, const float4* __restrict__ pool_pe,
                           const int* __restrict__ index, int n_bank, int ws, int shot, long long map_units,
                           long long pool_units, float4* __restrict__ s_pe, float4* __restrict__ sp_pe) {
  const int s = blockIdx.y;
  const int r = s % ws, b = s / ws;
  const bool positive = r < shot;
  const long long total = pool_units + (positive ? map_units : 0);
  const long long u0 = (long long)blockIdx.x * (BANK_UNROLL * 256) + threadIdx.x;
  if (u0 - threadIdx.x >= total) return;
  const int n = index[s];
  if (n < 0 || n >= n_bank) return;  // (validated on the host; never read outside the bank)
  const float4* src_pool = pool_pe + (long long)n * pool_units;
  const float4* src_map = map_pe + (long long)n * map_units;
  float4* dst_pool = sp_pe + (long long)s * pool_units;
  float4* dst_map = s_pe + ((long long)b * shot + r) * map_units;  // (read for positives only)
  // (a unit past the slot's end reads the slot's last unit again, total >= 1 here, and stores nothing: the loads carry no
  //  branch, so all BANK_UNROLL of them are in flight before the first store waits)
  float4 v[BANK_UNROLL];
#pragma unroll
  for (int k = 0; k < BANK_UNROLL; ++k) {
    const long long u = min(u0 + (long long)k * 256, total - 1);
    const float4* src = u < pool_units ? src_pool + u : src_map + (u - pool_units);
    v[k] = *src;
  }
  asm volatile("" ::: "memory");  // (keeps the compiler from sinking each load into its store's branch)
#pragma unroll
  for (int k = 0; k < BANK_UNROLL; ++k) {
    const long long u = u0 + (long long)k * 256;
    if (u < total) {
      float4* dst = u < pool_units ? dst_pool + u : dst_map + (u - pool_units);
      *dst = v[k];
    }
  }
}

// Query bank (dana.QueryBank): the trunk maps [N][rows][C] of a pool of query images are encoded once over a frozen trunk; a
// forward names its B images by bank row and ONE launch copies them into the first C columns of corr [B*rows][ld_out] -- where
// the query trunk writes its result -- and leaves columns C .. ld_out-1 (the attended half) alone.
// grid (gx, B): workgroup row b walks the rows*C/4 16-byte units of image index[b]; a workgroup takes BANK_UNROLL * 256
// consecutive units, each lane BANK_UNROLL of them 256 apart, every load in front of the first store (a unit past the image's
// end reads the image's last unit again and stores nothing). Unit u = (r, c4) lands at row b*rows + r, 16-byte column c4.
__global__ void __launch_bounds__(256)
qbank_gather_kernel(const float4* __restrict__ maps, const int* __restrict__ index, int n_bank, unsigned units,
                    unsigned c4s, int rows, float4* __restrict__ out, int ld4) {
  const int b = blockIdx.y;
  // (units < 2^31 - 1024, checked by the entry point: unit numbers and their row / column split stay in 32 bits)
  const unsigned u0 = blockIdx.x * (BANK_UNROLL * 256) + threadIdx.x;
  if (u0 - threadIdx.x >= units) return;
  const int n = index[b];
  if (n < 0 || n >= n_bank) return;  // (validated on the host; never read outside the bank)
  const float4* src = maps + (long long)n * units;
  float4* dst = out + (long long)b * rows * ld4;
  float4 v[BANK_UNROLL];
#pragma unroll
  for (int k = 0; k < BANK_UNROLL; ++k) v[k] = src[min(u0 + (unsigned)k * 256, units - 1)];
#pragma unroll
  for (int k = 0; k < BANK_UNROLL; ++k) {
    const unsigned u = u0 + (unsigned)k * 256;
    if (u < units) {
      const unsigned r = u / c4s;
      dst[(long long)r * ld4 + (u - r * c4s)] = v[k];
    }
  }
}

extern "C" {

int dana_qbank_gather(const float* maps, const int* index, int n_bank, int B, int rows, int channels, float* out, int ld_out,
                      dana_stream_t stream) {
  DANA_CHECK_ARG(n_bank >= 0 && B >= 0 && B <= 65535 && rows >= 0 && channels >= 4 && channels % 4 == 0 &&
                     ld_out >= channels && ld_out % 4 == 0,
                 "dana_qbank_gather: bad shape n_bank=%d B=%d rows=%d channels=%d ld_out=%d (channels and ld_out multiples "
                 "of 4, ld_out >= channels, B <= 65535)", n_bank, B, rows, channels, ld_out);
  const long long units = (long long)rows * (channels / 4);
  if (B == 0 || units == 0) return DANA_OK;
  DANA_CHECK_ARG(maps && index && out && n_bank > 0, "dana_qbank_gather: null pointer");
  DANA_CHECK_ARG((((uintptr_t)maps | (uintptr_t)out) & 15) == 0, "dana_qbank_gather: maps and out must be 16-byte aligned");
  const long long per_wg = (long long)BANK_UNROLL * 256;
  DANA_CHECK_ARG(units < 0x7fffffffLL - per_wg, "dana_qbank_gather: %lld 16-byte units per image (fewer than 2^31 - %lld)",
                 units, per_wg);
  const long long gx = (units + per_wg - 1) / per_wg;
  qbank_gather_kernel<<<dim3((unsigned)gx, (unsigned)B), 256, 0, (hipStream_t)stream>>>(
      (const float4*)maps, index, n_bank, (unsigned)units, (unsigned)(channels / 4), rows, (float4*)out, ld_out / 4);
  DANA_CHECK_LAUNCH("dana_qbank_gather");
  return DANA_OK;
}

int dana_bank_gather_episode(const float* map_pe, const float* pool_pe, const int* index, int n_bank, int B, int way,
                             int shot, int map_rows, int pool_rows, int channels, float* s_pe, float* sp_pe,
                             dana_stream_t stream) {
  DANA_CHECK_ARG(n_bank >= 0 && B >= 0 && way >= 1 && shot >= 1 && map_rows >= 0 && pool_rows >= 0 && channels >= 4 &&
                     channels % 4 == 0,
                 "dana_bank_gather_episode: bad shape n_bank=%d B=%d way=%d shot=%d map_rows=%d pool_rows=%d channels=%d "
                 "(channels a multiple of 4)", n_bank, B, way, shot, map_rows, pool_rows, channels);
  const long long slots = (long long)B * way * shot;
  DANA_CHECK_ARG(slots <= 65535, "dana_bank_gather_episode: B*way*shot = %lld support slots (at most 65535)", slots);
  const long long map_units = (long long)map_rows * (channels / 4), pool_units = (long long)pool_rows * (channels / 4);
  if (slots == 0 || map_units + pool_units == 0) return DANA_OK;
  DANA_CHECK_ARG(map_pe && pool_pe && index && s_pe && sp_pe && n_bank > 0, "dana_bank_gather_episode: null pointer");
  DANA_CHECK_ARG((((uintptr_t)map_pe | (uintptr_t)pool_pe | (uintptr_t)s_pe | (uintptr_t)sp_pe) & 15) == 0,
                 "dana_bank_gather_episode: the four tensors must be 16-byte aligned");
  const long long per_wg = (long long)BANK_UNROLL * 256;
  const long long gx = (map_units + pool_units + per_wg - 1) / per_wg;
  DANA_CHECK_ARG(gx <= 0x7fffffffLL, "dana_bank_gather_episode: %lld workgroups per slot", gx);
  bank_gather_episode_kernel<<<dim3((unsigned)gx, (unsigned)slots), 256, 0, (hipStream_t)stream>>>(
      (const float4*)map_pe, (const float4*)pool_pe, index, n_bank, way * shot, shot, map_units, pool_units, (float4*)s_pe,
      (float4*)sp_pe);
  DANA_CHECK_LAUNCH("dana_bank_gather_episode");
  return DANA_OK;
}

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
