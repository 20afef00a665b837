/* libdana_hip.so -- debug / tuning / profiling switches. NOT part of the drop-in ABI (include/dana_hip.h): nothing the
 * reference binds goes through these, no product code path depends on a non-default value, and they may change between
 * rounds. They exist for the A/B tools under tools/ and for the bit-identity tests that compare two forms of one kernel.
 * All are process-wide configuration calls (issue them between forwards, not while other threads are inside one). */
#ifndef DANA_HIP_DEBUG_H
#define DANA_HIP_DEBUG_H
#include "dana_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Force the tile shape of the split kernel (dana_set_mfma_mode(1)) for every launch that can take it: 0 = the dispatcher's
 * own choice (default), 2 = 128x64, 3 = 64x64, 4 = 128x128, 5 = 64x128 (tools/tile_sweep.py). No effect on the f32-MFMA
 * kernel; dana_set_mfma_mode() resets it. */
int dana_debug_force_tile(int tile);
/* Epilogue form of the split kernel. 0 (default): scale / shift / residual / ReLU / ReLU-adjoint mask run on the
 * accumulator registers and the results leave as dword buffer stores (a 32x32 accumulator row = 32 consecutive channels =
 * one 128-byte segment per row and half-wave): no LDS C tile, 49 instead of 67.6 KB of LDS per 128x128 tile. 1: the
 * round-1..4 form through an LDS C tile (float4 rows). Same arithmetic in the same order -> the same bits
 * (tests/test_gpu_contractions.py uses mode 1 as the reference of test_register_epilogue_*). */
int dana_set_epilogue_mode(int mode);
int dana_get_epilogue_mode(void);
/* Kernel choice of the contractions on pre-split weights, in-process (the environment's DANA_DMA_KERNEL / DANA_PP_STAGES
 * only give these two process-wide atomics their initial value, once). Every launch reads them when it is issued.
 *  dma kernel: 0 = never the DMA kernel on fp32 activation rows (the split kernel of round 4), 1 = the measured rule
 *    (default), 2 = the DMA kernel wherever it can run (64-wide tiles for N <= 64).
 *  pp stages (planes x planes launches, DANA_A_SPLIT3): 2 / 3 / 4 / 6 staging stages, 13 / 14 = 3 / 4 stages with two
 *    fragment sets; launches with N <= 64 have two forms only (2 -> two stages, every other value -> three).
 * v = -1 returns to the environment's value, or without one to the dispatcher's own rule (the getters then return -1).
 * Any other value is refused. */
int dana_debug_set_dma_kernel(int v);
int dana_debug_get_dma_kernel(void);
int dana_debug_set_pp_stages(int v);
int dana_debug_get_pp_stages(void);
/* Which kernel instantiation the most recent conv / GEMM launch of this process took (stored when the launch is issued;
 * 0 = none yet; the skinny N <= 8 GEMM and the Winograd transforms are not contractions of this family and leave it):
 *   bits  0..3  family (DANA_IGEMM_FAMILY_*: f32-MFMA kernel, igemm_split_kernel, igemm_split_kernel_128, igemm_dma_kernel)
 *   bits  4..5  BM / 64        bits  6..7  BN / 64
 *   bit   8     STEM           bit   9     BPRE (weights as split planes; always 1 for the dma family)
 *   bit  10     FUSE           bit  11     ELDS (epilogue through an LDS C tile)
 *   bits 12..15 NST (dma family: staging stages; 0 elsewhere)
 *   bit  16     APRE (dma family: activation rows as split planes)      bit 17  DF (dma family: two fragment sets) */
#define DANA_IGEMM_FAMILY_F32 1
#define DANA_IGEMM_FAMILY_SPLIT 2
#define DANA_IGEMM_FAMILY_SPLIT_128 3
#define DANA_IGEMM_FAMILY_DMA 4
int dana_debug_last_igemm_form(void);
/* Tile and pixel split of the weight-gradient launches (csrc/wgrad.hip: dana_conv2d_wgrad_nhwc, dana_gemm_tn_batched and the
 * Winograd-domain weight gradient), which a cost model picks otherwise. tile: 0 = the cost model (default), 64 = the 64x64
 * tile (always wgrad_f32_kernel), 128 = the 128x128 tile (the bf16x6 split kernels, or wgrad_f32_128_kernel under
 * dana_set_mfma_mode(0), as without the switch). slices: 0 = the cost model, 1..64 = that many pixel slices S, clamped on
 * the host to ceil(M / 32), to the largest count that leaves no slice empty and to planes * S <= 65535 -- a forced value
 * never gives a launch the cost model could not give for some shape. Any other argument is refused and changes nothing.
 * The workspace-size functions follow the forced choice: size the workspace and launch under the same setting. */
int dana_debug_force_wgrad(int tile, int slices);
/* The most recent weight-gradient launch of this process (stored when the launch is issued; 0 = none yet):
 *   bits  0..3  compute kernel (DANA_WGRAD_KERNEL_*: wgrad_f32_kernel, wgrad_f32_128_kernel, wgrad_split_128_kernel,
 *               wgrad_split_128p_kernel)
 *   bits  4..10 S, the pixel slices (with S == 1 the Winograd-domain launch writes its result itself; every other launch
 *               goes through wgrad_reduce_kernel)
 *   bits 12..27 planes of a batched launch, capped at 65535 */
#define DANA_WGRAD_KERNEL_F32_64 1
#define DANA_WGRAD_KERNEL_F32_128 2
#define DANA_WGRAD_KERNEL_SPLIT_128 3
#define DANA_WGRAD_KERNEL_SPLIT_128P 4
int dana_debug_last_wgrad_form(void);
/* Which form the most recent dana_roi_align_backward of this process took (csrc/roi_ops.hip; 0 = none yet): 1 = the NHWC
 * gather (pooled size <= 8, channels % 4 == 0), 2 = the NHWC per-bin kernel (maps of at most 128 x 128), 3 = the NHWC atomic
 * scatter, 4 = the NCHW atomic scatter, 5 = the zero fill alone (no rois). */
#define DANA_ROI_ALIGN_BWD_GATHER 1
#define DANA_ROI_ALIGN_BWD_BINS 2
#define DANA_ROI_ALIGN_BWD_SCATTER_NHWC 3
#define DANA_ROI_ALIGN_BWD_SCATTER_NCHW 4
#define DANA_ROI_ALIGN_BWD_MEMSET 5
int dana_debug_last_roi_align_backward_form(void);
/* While `buffer` is non-null every split-kernel block writes eight 64-bit words {shader-clock at start, at the first
 * K-step, after the K loop, at the end, HW_ID, 100 MHz wall clock at the end, wall clock at the start, 0} at
 * buffer[(z * grid + block) * 8]. The pointer is read when a launch is ISSUED, so two launches issued with two buffers can
 * run concurrently (tools/overlap_probe.py). The caller sizes the buffer for the launches it traces; null switches it
 * off. (tools/igemm_trace.py, gemm_power.py) */
int dana_set_igemm_trace(unsigned long long* buffer);
/* dana_topk_desc / dana_sort_desc dispatch: 0 = the measured rule (default), 1 = the sample sort for every row, 2 = the
 * single-workgroup kernel wherever it can run (n <= 40 960, min(topn, n) <= 12 288). */
int dana_set_sort_mode(int mode);

/* A HIP stream restricted to a set of compute units (hipExtStreamCreateWithCUMask), for the overlap experiments of
 * profiles/r6_overlap.md. mask_words 32-bit words, bit i of the mask = CU (i / n_xcd) of XCD (i % n_xcd) on a multi-XCD part
 * in SPX mode (the KFD deals the bits round-robin over the XCDs), 256 bits on an MI355X. EVERY XCD must keep at least one
 * CU: the command processor deals a launch's workgroups over all XCDs whatever the mask says, and an XCD without CUs
 * never retires its share (the call refuses such masks). *stream_out receives the hipStream_t. */
int dana_debug_stream_create_cumask(const unsigned int* mask, int mask_words, int n_xcd, dana_stream_t* stream_out);
int dana_debug_stream_destroy(dana_stream_t stream);

/* The evaluator's sort on its own (csrc/evaluate.hip): a stable LSD radix sort of n (64-bit key, 32-bit value) pairs,
 * ascending in the low key_bits bits of the key (passes above them are skipped), eight bits per pass, three launches per
 * pass. in / out may not overlap. (tests/test_gpu_evaluate.py) */
size_t dana_debug_radix_sort_workspace_bytes(long n);
int dana_debug_radix_sort_pairs(const unsigned long long* keys_in, const int* vals_in, unsigned long long* keys_out,
                                int* vals_out, long n, int key_bits, void* workspace, size_t workspace_bytes,
                                dana_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
