/* libdana_hip.so -- C ABI of the MI355X (gfx950) DAnA forward hot path.
 *
 * Every entry point takes raw DEVICE pointers, explicit sizes/strides, scalars and a HIP stream
 * (passed as void*); returns 0 on success or a negative DANA_ERR_* code, with the message
 * available from dana_last_error() (thread-local). No entry point allocates device memory or
 * synchronises with the host: scratch comes from the caller (`*_workspace_bytes`), launches go
 * to the caller's stream, so the functions are re-entrant across threads/devices (the reference
 * is driven from one Python thread per device under nn.DataParallel, train.py:104-105).
 *
 * Each declaration cites the reference interface it replaces (paths relative to the reference
 * repository root). INTEGRATION.md shows the binding a reference maintainer would add.
 */
#ifndef DANA_HIP_H
#define DANA_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dana_stream_t; /* hipStream_t */

#define DANA_LAYOUT_NCHW 0
#define DANA_LAYOUT_NHWC 1

/* epilogue flags of dana_conv2d_nhwc / dana_gemm_nt */
#define DANA_EPI_RELU 1
#define DANA_CONV_STEM7 2 /* 7x7/2 stem over NHWC4 input, weight packed [cout][7][8][4] */
/* the weight / `b` / `u` argument points at dana_split_weight's output instead of fp32 rows: three bf16 planes per
 * 16-wide K-step, [kp / 16][3][n][16], of the SAME values (exact split, kp = k rounded up to 16; dana_gemm_nt: ldb = kp,
 * batch_b = bf16 elements between the slices' first K-steps). Split kernel only (dana_set_mfma_mode != 0);
 * results are bit-identical to the fp32-weight call, the K loop just does not repeat the split per tile and step. */
#define DANA_W_SPLIT3 256
/* dana_gemm_nt only: `a` holds the activation rows as split planes as well, [lda / 16][3][m][16] with lda = k rounded up to
 * 16 and batch_a in bf16 elements (the layout of dana_split_weight with n = m): planes x planes form of igemm_dma_kernel -- both
 * operands by LDS-DMA, no split and no staging registers in the K loop. Needs DANA_W_SPLIT3. Bit-identical to the fp32-rows
 * call on the values the planes were split from. (Measured in round 5, profiles/r5_activation_planes.md: the GEMM itself is
 * 6-19 % faster, a PRODUCER that writes planes pays 1.5x the bytes -- not used on the model's path.) */
#define DANA_A_SPLIT3 512

const char* dana_last_error(void);
int dana_abi_version(void);

/* How the fp32 contractions (every conv / GEMM below) use the matrix cores. 1 (default; DANA_MFMA_SPLIT overrides the
 * initial value): each fp32 operand is split EXACTLY into three bf16 numbers and the six products of weight >= 2^-16
 * run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (error vs an fp64 contraction equal to the f32 kernel's,
 * tests/test_gpu_contractions.py); 0: v_mfma_f32_32x32x2_f32. (Forced tile shapes, the LDS epilogue form, the sort dispatch and the per-block trace are
 * debug switches: include/dana_hip_debug.h.)
 * Replaces nothing in the reference: cuDNN picks its own algorithm / math mode there (lib/model/framework/resnet.py). */
int dana_set_mfma_mode(int mode);
int dana_get_mfma_mode(void);

/* ---- native operators: lib/model/csrc/vision.cpp:7-13 (module `model._C`) ------------------- */

/* ROIAlign_forward: lib/model/csrc/ROIAlign.h:11-25 -> cuda/ROIAlign_cuda.cu:257-305.
 * rois[num_rois][5] = (batch_idx, x1, y1, x2, y2) in image pixels. layout NCHW: input
 * [B][C][H][W] -> output [R][C][PH][PW] (the reference contract). layout NHWC: pixel (b,y,x) at
 * input + ((b*H+y)*W+x)*in_pix_stride (stride 0 => C) -> output [R][PH*PW][out_pix_stride];
 * optional output2 = output + add2[PH*PW][C] written in the same pass (fused positional
 * encoding, dana.py:258-259).
 * Arithmetic: the reference's per-sample loop in the reference's order -- bit-identical to cpu/ROIAlign_cpu.cpp in both
 * layouts. */
int dana_roi_align_forward(const float* input, const float* rois, float* output, int batch, int channels,
                           int height, int width, int num_rois, float spatial_scale, int pooled_h,
                           int pooled_w, int sampling_ratio, int layout, long in_pix_stride,
                           long out_pix_stride, float* output2, const float* add2, long out2_pix_stride,
                           dana_stream_t stream);

/* ROIAlign_backward: lib/model/csrc/ROIAlign.h:27-45 -> cuda/ROIAlign_cuda.cu:308-346.
 * grad_in [B][C][H][W] (NCHW) or [B][H][W][C] (NHWC) is completely (over)written: NCHW zero-fills it and scatters with
 * fp32 atomics like the reference (unordered sum); NHWC (channels % 4 == 0, pooled sides <= 8) gathers per feature cell
 * in a fixed (roi, bin) order -- no atomics, bit-reproducible. */
int dana_roi_align_backward(const float* grad_out, const float* rois, float* grad_in, int batch, int channels,
                            int height, int width, int num_rois, float spatial_scale, int pooled_h,
                            int pooled_w, int sampling_ratio, int layout, dana_stream_t stream);

/* ROIPool_forward / ROIPool_backward: lib/model/csrc/ROIPool.h:11-46 -> cuda/ROIPool_cuda.cu:111-202. NCHW. */
int dana_roi_pool_forward(const float* input, const float* rois, float* output, int* argmax, int batch,
                          int channels, int height, int width, int num_rois, float spatial_scale, int pooled_h,
                          int pooled_w, dana_stream_t stream);
int dana_roi_pool_backward(const float* grad_out, const int* argmax, const float* rois, float* grad_in,
                           int batch, int channels, int height, int width, int num_rois, int pooled_h,
                           int pooled_w, dana_stream_t stream);

/* nms: lib/model/csrc/nms.h:10-28 -> cuda/nms.cu:70-131 (nms_cuda) / cpu/nms_cpu.cpp:5-75.
 * boxes[problems][n][4] must already be in descending-score order (the reference sorts inside
 * nms_cuda, nms.cu:73-75; here the sort is dana_sort_desc). keep[p][0..num_keep[p]) receives
 * the kept POSITIONS, ascending; at most max_keep (<=0: all). inclusive=0: suppress IoU > thr
 * (nms.cu:60); inclusive=1: IoU >= thr (nms_cpu.cpp:60).
 * With max_keep < n the mask is filled and scanned in column bands (the first covers ~2.5 x max_keep boxes; the later
 * ones leave at once when max_keep is reached): the result is the same greedy NMS truncated at max_keep, only the
 * work differs. A band of <= 128 column blocks (every band of the proposal layer's problems) is scanned by a barrier-free
 * dataflow of one workgroup's waves -- resolver, word loaders, row workers over LDS flags --, a wider one by the
 * resolver + workers kernel with one barrier per 64-box block. */
size_t dana_nms_workspace_bytes(int n, int problems);
int dana_nms(const float* boxes, int n, int problems, float thr, int inclusive, int max_keep, int* keep,
             int keep_stride, int* num_keep, void* workspace, size_t workspace_bytes, dana_stream_t stream);

/* ---- RPN proposal path: lib/model/rpn/proposal_layer.py:49-190 ------------------------------- */

/* Anchor grid + bbox_transform_inv (bbox_transform.py:77-103) + clip_boxes (:125-133) + fg score.
 * cls element (b, ch, k=h*W+w) at cls + b*cls_sb + ch*cls_sc + k*cls_sp (2A channels: bg a, fg A+a);
 * cls_is_prob=0 applies the pair softmax of rpn.py:67-69. bbox likewise with 4A channels.
 * proposals[B][H*W*A][4], scores[B][H*W*A], index = k*A + a (proposal_layer.py:98-103). */
int dana_rpn_decode(const float* cls, long cls_sb, long cls_sc, long cls_sp, int cls_is_prob, const float* bbox,
                    long bbox_sb, long bbox_sc, long bbox_sp, const float* im_info, const float* base_anchors,
                    int B, int A, int H, int W, int feat_stride, float* proposals, float* scores,
                    dana_stream_t stream);

/* torch.sort(scores, 1, True) (proposal_layer.py:135): stable, per row. sorted_scores may be NULL. (= dana_topk_desc with
 * topn = n) */
size_t dana_sort_desc_workspace_bytes(int B, int n);
int dana_sort_desc(const float* scores, int B, int n, int* order, float* sorted_scores, void* workspace,
                   size_t workspace_bytes, dana_stream_t stream);
/* proposal_layer.py:135-150 as one operation: order[b][0..min(topn, n)) = the indices of row b's `topn` largest scores in
 * descending score order, equal scores in ascending index order -- the first topn entries of torch.sort(scores, 1, True)
 * (row stride of order / sorted_scores: order_stride >= min(topn, n); sorted_scores may be NULL). Two hand-written sorts, no
 * library: rows of <= 4 096 scores take ONE workgroup per row (radix select in registers + stable LDS radix sort, one
 * launch: 19 us at n = 300); longer rows a sample sort over the whole chip (splitters from 2 048 sampled keys, classify,
 * scatter, per-bucket rank: four launches, `workspace` of dana_topk_desc_workspace_bytes; 4 x 21 546 -> 12 000 in 45 us
 * where the single-workgroup kernel takes 122 us and rocPRIM's device-wide radix sort, used through round 4, took 88 us). */
size_t dana_topk_desc_workspace_bytes(int B, int n, int topn);
int dana_topk_desc(const float* scores, int B, int n, int topn, int* order, int order_stride, float* sorted_scores,
                   void* workspace, size_t workspace_bytes, dana_stream_t stream);

/* proposals_single[order_single[:topn]] (proposal_layer.py:148-151) */
int dana_gather_boxes(const float* src, const int* order, int B, int n, int order_stride, int topn, float* dst,
                      dana_stream_t stream);

/* output[i,:,0]=i; output[i,:num,1:]=kept boxes; zero padding (proposal_layer.py:136,183-188) */
int dana_rois_assemble(const float* sorted_boxes, const int* keep, const int* num_keep, int B, int topn,
                       int keep_stride, int post_n, float* rois, dana_stream_t stream);

/* _ProposalLayer.forward as one call: decode -> sort -> top-N -> NMS -> rois[B][post_nms_topn][5]. */
size_t dana_proposal_layer_workspace_bytes(int B, int A, int H, int W, int pre_nms_topn, int post_nms_topn);
int dana_proposal_layer(const float* cls, long cls_sb, long cls_sc, long cls_sp, int cls_is_prob, const float* bbox,
                        long bbox_sb, long bbox_sc, long bbox_sp, const float* im_info, const float* base_anchors,
                        int B, int A, int H, int W, int feat_stride, int pre_nms_topn, int post_nms_topn,
                        float nms_thresh, int nms_inclusive, float* rois, void* workspace, size_t workspace_bytes,
                        dana_stream_t stream);

/* Inference post-processing for one image (inference.py:106-140, utils.py:312-317): deltas*stds+means ->
 * bbox_transform_inv on the rois -> clip_boxes -> / im_scale; rows with cls_prob[:,1] <= score_thresh sort last
 * (score -inf); descending sort; NMS(nms_thresh). dets[R][5] holds every row in sorted order, keep_pos the kept
 * positions; meta[0] = rows above the threshold, meta[1] = rows kept: the detections are
 * dets[keep_pos[i]] for the i with keep_pos[i] < meta[0]. stds4 / means4 are HOST float[4]. */
size_t dana_detect_postprocess_workspace_bytes(int R);
int dana_detect_postprocess(const float* rois, const float* cls_prob, const float* bbox_pred, const float* im_info,
                            int R, const float* stds4, const float* means4, int normalize, float score_thresh,
                            float nms_thresh, int nms_inclusive, float* dets, int* keep_pos, int* meta,
                            void* workspace, size_t workspace_bytes, dana_stream_t stream);
/* dana_detect_postprocess for B images of R rois each in one call: rois[B][R][5], cls_prob[B*R][2], bbox_pred[B*R][4],
 * im_info[B][3]; the same decode, sort and NMS per image (B sort rows, B NMS problems). Output packed in image order:
 * dets[sum K_b][5] (capacity B*R rows), image b's K_b = counts[b] detections at rows offsets[b].. (offsets[B] = sum K_b),
 * each image's rows equal to what dana_detect_postprocess gives for it. */
size_t dana_detect_postprocess_batched_workspace_bytes(int B, int R);
int dana_detect_postprocess_batched(const float* rois, const float* cls_prob, const float* bbox_pred,
                                    const float* im_info, int B, int R, const float* stds4, const float* means4,
                                    int normalize, float score_thresh, float nms_thresh, int nms_inclusive, float* dets,
                                    int* counts, int* offsets, void* workspace, size_t workspace_bytes,
                                    dana_stream_t stream);

/* Merging detection lists (utils.py:182-204, generate_pseudo_label: torch.cat of the per-shot lists, torch.sort by score,
 * nms(..., cfg.TEST.NMS) over the union; and the max_per_image cut over an image's class lists, inference.py:70).
 * dets_in is a packed buffer of rows (x1, y1, x2, y2, score); input problem p = l*groups + g has counts_in[p] rows starting
 * at row offsets_in[p] (the layout dana_detect_postprocess_batched writes; both arrays are read on the DEVICE). For every
 * output list l < n_lists independently: (1) concatenate its `groups` input lists in group order; (2) sort by score,
 * descending and STABLE -- equal scores keep concatenation order, lower group first, then lower row (torch.sort leaves ties
 * undefined; this is the evaluators' arrival-order rule); (3) if do_nms, greedy NMS at nms_thresh under dana_nms' contract
 * (legacy +1 widths, `>` or, with nms_inclusive, `>=`); (4) keep the first max_dets survivors (max_dets <= 0: all);
 * (5) write them packed in list order: dets_out[sum K_l][5] (capacity n_lists*capacity rows), counts_out[n_lists],
 * offsets_out[n_lists + 1], and per output row its source, group_out = g and row_out = the row inside list (l, g). Every
 * output row is a bit-for-bit copy of an input row. `capacity` is the row count of the padded frame a list is sorted in,
 * >= max over l of sum_g counts_in[l*groups + g] and <= 520 064 (what dana_nms takes per problem); the entry point cannot
 * check the lower bound without a host read, so a smaller value truncates a list's concatenation at `capacity` rows -- it
 * never writes outside the frame. n_lists <= 65 535. n_lists == 0 or capacity == 0 zero the output layout and return. */
size_t dana_detect_merge_workspace_bytes(int n_lists, int groups, int capacity);
int dana_detect_merge(const float* dets_in, const int* counts_in, const int* offsets_in, int n_lists, int groups,
                      int capacity, int do_nms, float nms_thresh, int nms_inclusive, int max_dets, float* dets_out,
                      int* group_out, int* row_out, int* counts_out, int* offsets_out, void* workspace,
                      size_t workspace_bytes, dana_stream_t stream);

/* dana_detect_merge with Soft-NMS in place of the hard NMS and / or box voting after it. Neither is in the reference tree;
 * both are restated from their papers -- Bodla et al., "Soft-NMS: Improving Object Detection With One Line of Code", ICCV
 * 2017, and Gidaris & Komodakis, "Object detection via a multi-region & semantic segmentation-aware CNN model", ICCV 2015
 * (box voting, scores kept: the "ID" scoring) -- and postprocess.merge_soft_numpy is the same definition in numpy. Inputs,
 * concatenation, output layout and `capacity` as above; j below is a row's index in its list's concatenation, n its length.
 * iou(a, b) = inter / ((area(a) + area(b)) - inter) in fp32 with the +1 widths, one IEEE operation per written operation.
 * method 0 (hard): steps (2)-(4) of dana_detect_merge, bit for bit (do_nms is read by this method only).
 * method 1 (linear) / 2 (gaussian): every row starts live with working score t_j = its score. While a row is live and fewer
 *   than max_dets rows are out (max_dets <= 0: no limit): pick the live row i with the largest t (ties: the lowest j; a NaN
 *   ranks behind every number), emit (box_i, t_i), retire i; for every live j with o = iou(box_i, box_j): linear
 *   t_j = t_j * (1 - o) if o > nms_thresh (>= with nms_inclusive); gaussian t_j = (float)((double)t_j * exp(-(double)(o * o) /
 *   (double)sigma)), nms_thresh unused; then every live j with t_j < min_score is retired without being emitted. Emitted
 *   scores never increase, so the lists are in descending score order. One workgroup per list holds the list in LDS:
 *   capacity <= 3072 (21 bytes per row in 64 KiB), checked here -- a larger frame is DANA_ERR_ARG, never a launch.
 * vote_thresh >= 0 (negative: off; above 1: DANA_ERR_ARG): for every emitted row k, over ALL n rows j of the concatenation in
 *   ascending j (suppressed rows and k itself included) with iou(box_k, box_j) >= vote_thresh: X_c += (double)s_j *
 *   (double)box_j[c] for the four coordinates and W += (double)s_j, from 0.0, sequentially, with the ORIGINAL scores s_j. If
 *   W > 0 the row's coordinates become (float)(X_c / W). vote_score 0 (id) leaves the score, 1 (avg) makes it
 *   (float)(W / votes). votes_out[row] = the number of voters (written only when voting is on; may be null otherwise).
 * group_out / row_out are the source of the emitted box as above. The workspace is dana_detect_merge's. */
size_t dana_detect_merge_soft_workspace_bytes(int n_lists, int groups, int capacity);
int dana_detect_merge_soft(const float* dets_in, const int* counts_in, const int* offsets_in, int n_lists, int groups,
                           int capacity, int do_nms, float nms_thresh, int nms_inclusive, int max_dets, int method,
                           float sigma, float min_score, float vote_thresh, int vote_score, float* dets_out, int* group_out,
                           int* row_out, int* votes_out, int* counts_out, int* offsets_out, void* workspace,
                           size_t workspace_bytes, dana_stream_t stream);

/* View ensembles (test-time augmentation: an image seen mirrored and at several scales, each view detected on its own, the
 * lists mapped back and merged). Not in the reference tree; the area window follows Detectron's BBOX_AUG.AREA_TH_LO /
 * AREA_TH_HI, and postprocess.fold_views_numpy is the same definition in numpy. This call maps the lists of a class sweep
 * over n_images * views view images into the frame of their original image and lays them out for dana_detect_merge /
 * dana_detect_merge_soft with groups = views; neither of those changes. dets_in is the packed layout above, read on the
 * DEVICE: problem p = (i * views + v) * lists_per_view + c (image i, view v, class slot c) has counts_in[p] rows from row
 * offsets_in[p], already in original-image pixels (post-processing divided by the view's im_info[2]).
 * view_table[(i * views + v) * view_stride + 0..4] = (fw, fh, flip, area_lo, area_hi), view_stride >= 5: the original
 * frame's width and height as floats, flip 0 or 1, the area window (area_hi may be +inf, area_lo -inf).
 * Per row, in fp32, one IEEE operation per written operation, with wm1 = fw - 1 and hm1 = fh - 1:
 *   (1) if flip: (x1, x2) <- (wm1 - x2, wm1 - x1) -- the involution of imdb.append_flipped_images, written wm1 - x: ONE
 *       rounding after wm1, not (fw - x) - 1;
 *   (2) the row is kept only if it touches the frame: x1 <= wm1 && y1 <= hm1 && x2 >= 0 && y2 >= 0 (a NaN coordinate fails
 *       its comparison and drops the row);
 *   (3) clip: x <- min(max(x, 0), wm1), y <- min(max(y, 0), hm1), with max(x, 0) = (x < 0 ? 0 : x) and
 *       min(x, m) = (x > m ? m : x);
 *   (4) area = (x2 - x1 + 1) * (y2 - y1 + 1); kept only if area_lo <= area && area < area_hi;
 *   (5) the score is copied unchanged.
 * The kept rows of problem p are written in their input order (stable: still descending by score) to
 * dets_out[offsets_in[p] + k], k < kept, and the layout is transposed to list-major: with q = (i * lists_per_view + c) *
 * views + v, counts_out[q] = kept and offsets_out[q] = offsets_in[p], so the `views` lists of one (image, class) are
 * consecutive problems. src_row_out[offsets_in[p] + k] = the row's index inside input list p (may be null). dets_out has the
 * rows of dets_in and must not alias it (DANA_ERR_ARG); its rows beyond a list's kept count, and the rows no list owns, are
 * left UNWRITTEN. No row moves between lists; no atomics and no ordering between workgroups: two runs give the same bytes.
 * n_images * views * lists_per_view == 0 returns without a launch. */
int dana_detect_fold_views(const float* dets_in, const int* counts_in, const int* offsets_in, int n_images, int views,
                           int lists_per_view, const float* view_table, int view_stride, float* dets_out, int* counts_out,
                           int* offsets_out, int* src_row_out, dana_stream_t stream);

/* Tiled inference: a frame cut into overlapping tiles, each tile detected at the network's normal input size beside an
 * optional full-frame view, the lists mapped back and merged. Not in the reference tree; postprocess.fold_tiles_numpy is the
 * same definition in numpy and pipeline.plan_tiles makes the table. The call is dana_detect_fold_views for views that are
 * WINDOWS of the frame: same arguments, same layout of dets_in / dets_out / counts / offsets / src_row_out, same guarantees
 * (rows written in input order to the list's own rows, the rest UNWRITTEN, counts_out / offsets_out at the transposed index
 * q = (i * lists_per_view + c) * views + v, no atomics, two runs give the same bytes, dets_out must not alias dets_in, a zero
 * shape returns without a launch), and dana_detect_fold_views itself is unchanged. dets_in holds a tile's boxes in
 * original-image pixels measured from the TILE's origin (post-processing divided by the view's im_info[2]).
 * view_table[(i * views + v) * view_stride + 0..12], view_stride >= 13:
 *    0..4   fw, fh, flip, area_lo, area_hi   as above: the ORIGINAL frame, 0 or 1, the area window;
 *    5, 6   x_off, y_off                     the tile's origin in the frame -- for flip = 1 in the MIRRORED frame, where the
 *                                            tile's window lies;
 *    7, 8   tw, th                           the tile's width and height;
 *    9..12  lim_x1, lim_y1, lim_x2, lim_y2   the seam limits in tile coordinates: margin and (size - 1 - margin) on a side
 *                                            that lies inside the frame, -inf / +inf on a side that is a side of the frame.
 * Per row, in fp32, one IEEE operation per written operation, with twm1 = tw - 1 and thm1 = th - 1; min and max are the
 * selects of step (3) above and a NaN coordinate fails its comparison:
 *   (a) the row is kept only if it touches the tile: x1 <= twm1 && y1 <= thm1 && x2 >= 0 && y2 >= 0;
 *   (b) the seam rule, on the UNCLIPPED coordinates: kept only if x1 >= lim_x1 && y1 >= lim_y1 && x2 <= lim_x2 &&
 *       y2 <= lim_y2. A box that runs off a frame-side edge of the tile stays and is clipped; a box within the margin of an
 *       interior side -- most likely an object the tile's side cut, whose whole box the neighbouring tile has -- or one
 *       running past it into the holder's padding goes;
 *   (c) clip to the tile: x <- min(max(x, 0), twm1), y <- min(max(y, 0), thm1);
 *   (d) translate: x <- x + x_off, y <- y + y_off;
 *   (e) steps (1) - (5) of dana_detect_fold_views on the result: un-mirror, frame test, clip to the frame, area window,
 *       score copied. The row is kept if (a), (b), (2) and (4) all hold.
 * A whole-frame view is the row (.., 0, 0, fw, fh, -inf, -inf, +inf, +inf): it folds as dana_detect_fold_views does, except
 * that a -0 coordinate comes back +0 from step (d). */
int dana_detect_fold_tiles(const float* dets_in, const int* counts_in, const int* offsets_in, int n_images, int views,
                           int lists_per_view, const float* view_table, int view_stride, float* dets_out, int* counts_out,
                           int* offsets_out, int* src_row_out, dana_stream_t stream);

/* Detection lists -> the ground-truth tensors of a train-mode forward (fs_loader.py:325; pseudo-labels are trained on,
 * utils.py:130-179): one list per image in the packed layout above (counts[B], offsets[B], device). Image b's first
 * max_boxes rows with score > score_thresh, in list order, become gt_boxes[b][i] = (x1, y1, x2, y2) * im_info[b][2] (back
 * from original-image to network-input coordinates, the inverse of inference.py:125; one fp32 multiply each), labels[b];
 * the remaining rows of gt_boxes[B][max_boxes][5] are zero; num_boxes[b] (int64) = rows written. im_info rows are
 * im_info_stride (>= 3) floats apart. */
int dana_dets_to_gt_boxes(const float* dets, const int* counts, const int* offsets, const float* im_info,
                          int im_info_stride, const float* labels, int B, float score_thresh, int max_boxes,
                          float* gt_boxes, long long* num_boxes, dana_stream_t stream);

/* Cached support sets (dana.SupportCache): for every tensor t < n_tensors and image b < B, copy block index[b] (block_bytes[t]
 * bytes) of tensor t's sources into block b of its destination, all in ONE launch. src_ptrs / dst_ptrs are DEVICE arrays of
 * n_tensors device pointers (const void* const* / void* const*), block_bytes a device array; index[B] is read on the device,
 * so a recorded replay gathers the selection of the moment. Indices outside [0, n_sets) copy nothing. */
int dana_gather_blocks(const void* src_ptrs, const void* dst_ptrs, const long long* block_bytes, int n_tensors,
                       const int* index, int n_sets, int B, dana_stream_t stream);
/* Shot views of cached sets (SupportCache.select / sweep with shots=): dana_gather_blocks with a shot axis. Tensor t of a set
 * is [rows[t]][shot][block_bytes[t]]; problem p < P's destination is [rows[t]][m][block_bytes[t]]. Slot j < m takes shot block
 * view[p*shot + j] of set index[p]; a slot whose view entry is -1 (padding; any entry outside [0, shot) counts as padding) is
 * written as zeros and nothing is read for it. w[p*m + j] = 1.0f / (real slots of problem p), 0 on padding. src_ptrs,
 * dst_ptrs, rows, block_bytes are DEVICE arrays of n_tensors entries; index [P], view [P][shot] and w [P][m] are device
 * memory too (a recorded replay gathers the selection of the moment). One launch; a set index outside [0, n_sets) writes
 * nothing. 1 <= m <= shot <= 64. */
int dana_gather_shot_blocks(const void* src_ptrs, const void* dst_ptrs, const long long* rows, const long long* block_bytes,
                            int n_tensors, const int* index, const int* view, float* w, int n_sets, int shot, int m, int P,
                            dana_stream_t stream);
/* Support bank (dana.SupportBank): the episode of a training iteration over a frozen trunk, gathered from the bank's two
 * weight-independent tensors map_pe [n_bank][map_rows][channels] (trunk map + PE) and pool_pe [n_bank][pool_rows][channels]
 * (average pool + PE). For every support slot s < B*way*shot with n = index[s]: pool_pe[n] -> block s of sp_pe
 * [B*way*shot][pool_rows][channels]; and, when the slot is a positive (s % (way*shot) < shot), map_pe[n] -> block
 * (b, j) = (s / (way*shot), s % (way*shot)) of s_pe [B][shot*map_rows][channels]. index [B*way*shot] is read on the device,
 * so a recorded replay gathers the episode of the moment; an index outside [0, n_bank) writes nothing. One launch of 16-byte
 * copies: channels % 4 == 0 and 16-byte aligned tensors; B*way*shot <= 65 535. */
int dana_bank_gather_episode(const float* map_pe, const float* pool_pe, const int* index, int n_bank, int B, int way,
                             int shot, int map_rows, int pool_rows, int channels, float* s_pe, float* sp_pe,
                             dana_stream_t stream);
/* Query bank (dana.QueryBank): the trunk maps of a pool of query images, maps [n_bank][rows][channels], encoded once over a
 * frozen trunk. For b < B, r < rows, c < channels: out[(b*rows + r)*ld_out + c] = maps[index[b]][r][c]; columns
 * channels .. ld_out-1 of out are not touched (out is corr [B*rows][ld_out], whose second half holds the attended rows).
 * index [B] is read on the device, so a recorded replay gathers the batch of the moment; an index outside [0, n_bank) leaves
 * its image's rows alone. One launch of 16-byte copies: channels % 4 == 0, ld_out % 4 == 0, ld_out >= channels, maps and out
 * 16-byte aligned; B <= 65 535; rows * channels / 4 < 2^31 - 1024 (32-bit unit numbers in the kernel). */
int dana_qbank_gather(const float* maps, const int* index, int n_bank, int B, int rows, int channels, float* out, int ld_out,
                      dana_stream_t stream);

/* ---- class sweep (dana.SupportCache.sweep): B query images x C cached support sets as B*C problems p = b*C + c, the
 * per-class forward of dana.py:87-220 for every class of an image (inference.py:70-140 fills all_boxes[j][i] with it).
 * A problem reads its image's query-side tensors through p / C ("group" = C below). */
/* dana.py:143-146 over the class-interleaved scores of one GEMM per image (N = C*K1: the C classes' keys side by side):
 * input row (b*hw + i)*C + c of scores [B][hw][C][ld_in] -> output row (b*C + c)*hw + i of out [B*C][hw][ld_out], per
 * `length`-wide segment (one per shot) (softmax + unary_gamma * unary[p]) * out_scale, unary + p*unary_stride ->
 * [nseg][length]; cols nseg*length..kpad-1 zeroed. The per-row arithmetic of dana_attn_softmax_unary (C = 1: same bits). */
int dana_attn_softmax_unary_sweep(const float* scores, float* out, const float* unary, int B, int C, long hw,
                                  long unary_stride, int nseg, int length, long ld_in, long ld_out, int kpad,
                                  float unary_gamma, float out_scale, dana_stream_t stream);
/* ... with a per-segment scale in place of out_scale: segment s of a row of problem p is scaled by
 * seg_scale[p*scale_stride + s] (scale_stride <= 0: nseg). A segment whose scale is 0 is not read and written as +0.0f.
 * Equal scales give the bits of dana_attn_softmax_unary_sweep. */
int dana_attn_softmax_unary_sweep_w(const float* scores, float* out, const float* unary, int B, int C, long hw,
                                    long unary_stride, int nseg, int length, long ld_in, long ld_out, int kpad,
                                    float unary_gamma, const float* seg_scale, long scale_stride, dana_stream_t stream);
/* dst row p*rows + i <- src row (p / group)*rows + i (`cols` floats), p < n_blocks: a problem's copy of its image's rows
 * (im_info of proposal_layer.py:49-190 / inference.py:106-140 per problem) */
int dana_repeat_rows_grouped(const float* src, float* dst, long rows, int cols, long ld_src, long ld_dst, int group,
                             long n_blocks, dana_stream_t stream);
/* y row p*rows + i *= x row (p / group)*rows + i, p < n_blocks (dana.py:155-156 product attention: base_feat of image
 * p / group times problem p's attended rows); channels % 4 == 0, 16-byte aligned rows */
int dana_mul_rows_grouped(float* y, const float* x, long rows, int channels, long ld_y, long ld_x, int group,
                          long n_blocks, dana_stream_t stream);
/* Meta R-CNN's class head over a class sweep (framework/meta.py:129-142 for each of C classes): for RoI row b*R + r of
 * fc7 [B*R][K] and problem p = b*C + c, cls_prob[p*R + r] = softmax_2((fc7 row * vec[p]) . weight^T + bias) with the
 * product rounded to fp32 (weight [2][K], vec [B*C][K]); rois [B][R][5] / bbox_pred [B*R][4] rows copied to problem p's
 * block of rois_out [B*C][R][5] (column 0 = p) / bbox_out [B*C*R][4]. K % 4 == 0, K <= 2048 */
int dana_meta_class_head(const float* fc7, const float* vec, const float* weight, const float* bias, const float* rois,
                         const float* bbox_pred, float* cls_prob, float* rois_out, float* bbox_out, int B, int C, int R,
                         int K, dana_stream_t stream);
/* RoIAlign (dana.py:181-186, ROIAlign_cuda.cu) in NHWC with rois' column 0 a problem index: roi n reads image
 * (int)rois[n][0] / group. Arguments and outputs as dana_roi_align_forward(layout NHWC); group 1: the same bits. */
int dana_roi_align_forward_nhwc_grouped(const float* input, const float* rois, float* output, int batch, int channels,
                                        int height, int width, int num_rois, float spatial_scale, int pooled,
                                        int sampling_ratio, long in_pix_stride, long out_pix_stride, float* output2,
                                        const float* add2, long out2_pix_stride, int group, dana_stream_t stream);

/* ---- dense contractions on the fp32 matrix cores (v_mfma_f32_32x32x2_f32) --------------------- */

/* nn.Conv2d + frozen BatchNorm2d/bias + residual + ReLU (resnet.py:66-102 Bottleneck, :109-112 stem;
 * rpn.py:28,63 RPN_Conv). input NHWC [batch][in_h][in_w][in_pix_stride>=cin]; weight [cout][kh][kw][cin]
 * (see dana_pack_conv_weight); out[m][n] = relu?( acc*scale[n] + shift[n] + residual[m][n] ) written
 * with row stride out_pix_stride. scale/shift/residual may be NULL. cin % 32 == 0 unless STEM7. */
int dana_conv2d_nhwc(const float* input, const float* weight, float* output, const float* scale,
                     const float* shift, const float* residual, int batch, int in_h, int in_w, int cin,
                     int cout, int kh, int kw, int stride, int pad, long in_pix_stride, long out_pix_stride,
                     long res_pix_stride, int flags, dana_stream_t stream);

/* dana_conv2d_nhwc with the ReLU adjoint fused into the epilogue: out = mask_act > 0 ? conv(...) + residual : 0.
 * Used for data gradients (backward of resnet.py:83-100): mask_act is the activation whose ReLU sits in front of the
 * differentiated conv's input, [batch*oh*ow][mask_pix_stride]. */
int dana_conv2d_nhwc_masked(const float* input, const float* weight, float* output, const float* scale,
                            const float* shift, const float* residual, const float* mask_act, int batch, int in_h,
                            int in_w, int cin, int cout, int kh, int kw, int stride, int pad, long in_pix_stride,
                            long out_pix_stride, long res_pix_stride, long mask_pix_stride, int flags,
                            dana_stream_t stream);
/* The tail of a Bottleneck in ONE launch (resnet.py:92-100): out = relu?( bn3(conv3(relu(bn2(conv2(x))))) + residual ),
 * conv2 3x3 / stride 1 / pad 1 with cmid = 64 output channels, conv3 1x1 cmid -> cout. Both weights are dana_split_weight
 * planes (of the packed [cmid][3][3][cin] rows and of the [cout][cmid] rows); scale2 / shift2 and scale3 / shift3 are the
 * folded frozen BatchNorms. conv2's output tile stays in LDS as conv3's A operand -- the [M][64] map is never written --
 * and the result is bit-identical to dana_conv2d_nhwc (3x3, DANA_EPI_RELU) followed by dana_conv2d_nhwc (1x1, residual).
 * flags: DANA_EPI_RELU = the final ReLU. Split kernel only (dana_set_mfma_mode != 0). */
int dana_bottleneck_tail_nhwc(const float* input, const float* w2_split, const float* scale2, const float* shift2,
                              const float* w3_split, const float* scale3, const float* shift3, const float* residual,
                              float* output, int batch, int h, int w, int cin, int cmid, int cout, long in_pix_stride,
                              long out_pix_stride, long res_pix_stride, int flags, dana_stream_t stream);
/* ... computing only the pixels a stride-`stride` 1x1 consumer reads (stride 1 or 2; resnet.py:71,136 put a layer's stride
 * on the next block's 1x1 conv1 / downsample): conv2 runs 3x3 / stride `stride` / pad 1 over the h x w input, OH = (h-1)/stride+1,
 * conv3 + bn3 (+ ReLU) on those rows only; output is the dense [batch*OH*OW][out_pix_stride] map, the residual row of output
 * pixel (oh, ow) is pixel (stride*oh, stride*ow) of the [batch][h][w][res_pix_stride] map. Every written value has the bits
 * dana_bottleneck_tail_nhwc writes at that pixel. stride = 1 is dana_bottleneck_tail_nhwc. */
int dana_bottleneck_tail_strided_nhwc(const float* input, const float* w2_split, const float* scale2, const float* shift2,
                                      const float* w3_split, const float* scale3, const float* shift3,
                                      const float* residual, float* output, int batch, int h, int w, int cin, int cmid,
                                      int cout, long in_pix_stride, long out_pix_stride, long res_pix_stride, int stride,
                                      int flags, dana_stream_t stream);
/* dana_conv2d_nhwc whose residual is SAMPLED: output pixel (oh, ow) adds pixel (res_sample*oh, res_sample*ow) of the
 * [batch][res_h][res_w][res_pix_stride] map; (res_h-1)/res_sample+1 x (res_w-1)/res_sample+1 must be the conv's output map
 * (the expand conv of a block whose consumer has stride 2: the rows are the even pixels, the residual is x at those pixels).
 * Runs on the split kernel's register epilogue at a 64 x 64 or 128 x 128 tile (dana_set_mfma_mode(1), cout > 64); any
 * other path returns DANA_ERR_ARG. res_sample 1 or 2; same bits as dana_conv2d_nhwc over a gathered residual. */
int dana_conv2d_nhwc_sampled_res(const float* input, const float* weight, float* output, const float* scale,
                                 const float* shift, const float* residual, int batch, int in_h, int in_w, int cin,
                                 int cout, int kh, int kw, int stride, int pad, long in_pix_stride, long out_pix_stride,
                                 long res_pix_stride, int res_h, int res_w, int res_sample, int flags, dana_stream_t stream);

/* The same conv over TWO image groups in one launch: input rows = batch0 images of h0 x w0 followed by
 * batch1 images of h1 x w1 (same channels / pixel stride); outputs go to out0 / out1 with their own row
 * strides. RCNN_base is applied to the query batch and to the support batch (dana.py:98,100): sharing
 * each layer's launch doubles the tile count and halves the tail on the 256 CUs. */
int dana_conv2d_nhwc_dual(const float* input, const float* weight, float* out0, float* out1, const float* scale,
                          const float* shift, const float* res0, const float* res1, int batch0, int h0, int w0,
                          int batch1, int h1, int w1, int cin, int cout, int kh, int kw, int stride, int pad,
                          long in_pix_stride, long out0_stride, long out1_stride, long res0_stride,
                          long res1_stride, int flags, dana_stream_t stream);

/* Winograd F(2x2,3x3) path for the stride-1 pad-1 3x3 convs with many channels (layer3/layer4 conv2,
 * RPN_Conv): u = dana_winograd_filter_transform(packed weight [cout][3][3][cin]) -> [16][cout][cin], then
 * out = relu?(conv3x3(input) * scale + shift) with 2.25x fewer multiplies (the 16 GEMMs run on the igemm kernels, see dana_set_mfma_mode). */
int dana_winograd_filter_transform(const float* w_packed, float* u, int cout, int cin, dana_stream_t stream);
size_t dana_conv3x3_winograd_workspace_bytes(int batch, int h, int w, int cin, int cout);
int dana_conv3x3_winograd_nhwc(const float* input, const float* u, float* output, const float* scale,
                               const float* shift, int batch, int h, int w, int cin, int cout, long in_pix_stride,
                               long out_pix_stride, int flags, void* workspace, size_t workspace_bytes,
                               dana_stream_t stream);
/* same, with the ReLU adjoint fused into the output transform (out = mask_act > 0 ? conv : 0): the data gradient of
 * a 3x3 conv is a 3x3 conv on flipped weights, masked by the activation in front of the differentiated conv */
int dana_conv3x3_winograd_nhwc_masked(const float* input, const float* u, float* output, const float* scale,
                                      const float* shift, const float* mask_act, int batch, int h, int w, int cin,
                                      int cout, long in_pix_stride, long out_pix_stride, long mask_pix_stride,
                                      int flags, void* workspace, size_t workspace_bytes, dana_stream_t stream);

/* F(4x4,3x3) variant: u = dana_winograd4_filter_transform(...) -> [36][cout][cin]; 4x fewer multiplies than the
 * direct conv and smaller transformed tensors than F(2x2,3x3), at ~1e-5 relative error (transform constants up to 8) */
int dana_winograd4_filter_transform(const float* w_packed, float* u, int cout, int cin, dana_stream_t stream);
size_t dana_conv3x3_winograd4_workspace_bytes(int batch, int h, int w, int cin, int cout);
int dana_conv3x3_winograd4_nhwc_masked(const float* input, const float* u, float* output, const float* scale,
                                       const float* shift, const float* mask_act, int batch, int h, int w, int cin,
                                       int cout, long in_pix_stride, long out_pix_stride, long mask_pix_stride,
                                       int flags, void* workspace, size_t workspace_bytes, dana_stream_t stream);
/* The F(4x4,3x3) forward whose output transform finishes and writes only rows / columns 0 and 2 of each 4 x 4 tile
 * (sub = 2), i.e. the even pixels, into the dense [batch][(h-1)/2+1][(w-1)/2+1][out_pix_stride] map a stride-2 1x1 consumer
 * reads. Input transform and plane GEMM are the full-size ones (same workspace); every written value has the bits of the
 * full output at that pixel. sub = 1: the full map (dana_conv3x3_winograd4_nhwc_masked without a mask). */
int dana_conv3x3_winograd4_nhwc_sub(const float* input, const float* u, float* output, const float* scale,
                                    const float* shift, int batch, int h, int w, int cin, int cout, long in_pix_stride,
                                    long out_pix_stride, int sub, int flags, void* workspace, size_t workspace_bytes,
                                    dana_stream_t stream);
/* The RPN 3x3 conv of a class sweep (rpn.py:63 RPN_Conv on cat([base_feat, attended]) of dana.py:157), split by input
 * channels: W[:, :1024] * base_feat once per image (no shift, no ReLU) gives `residual`, then this launch runs
 * W[:, 1024:] * attended per problem with out = relu?(conv*scale + shift + residual[image / res_group]): output image n
 * reads residual image n / res_group (row stride res_pix_stride). tile 2: F(2x2,3x3) filters (dana_winograd_filter_transform),
 * 4: F(4x4,3x3) (dana_winograd4_filter_transform, DANA_W_SPLIT3 split planes allowed); workspace as for that tile. */
int dana_conv3x3_winograd_nhwc_grouped_res(const float* input, const float* u, float* output, const float* scale,
                                           const float* shift, const float* residual, int batch, int h, int w, int cin,
                                           int cout, long in_pix_stride, long out_pix_stride, long res_pix_stride,
                                           int res_group, int tile, int flags, void* workspace, size_t workspace_bytes,
                                           dana_stream_t stream);
/* F(4x4,3x3) over TWO image groups (input: group 0's [n0][h0][w0] pixels, then group 1's [n1][h1][w1]): two input
 * transforms, ONE batched plane GEMM over all tiles, two output transforms (resnet.py:92-94 on the query and the support
 * batch of dana.py:98,100 with the same filters) */
size_t dana_conv3x3_winograd4_dual_workspace_bytes(int n0, int h0, int w0, int n1, int h1, int w1, int cin, int cout);
int dana_conv3x3_winograd4_nhwc_dual(const float* input, const float* u, float* out0, float* out1, const float* scale,
                                     const float* shift, int n0, int h0, int w0, int n1, int h1, int w1, int cin,
                                     int cout, long in_pix_stride, long out0_pix_stride, long out1_pix_stride, int flags,
                                     void* workspace, size_t workspace_bytes, dana_stream_t stream);
/* ... with the ReLU adjoint of the masked data-gradient form (dana_conv3x3_winograd4_nhwc_masked) per group: out = mask > 0 ?
 * conv : 0. The merged backward of an identity bottleneck (resnet.py:84-100 differentiated over the [query | support]
 * buffers) runs its 3x3 data gradient for both batches as ONE batched plane GEMM with it. mask0 / mask1 may be NULL. */
int dana_conv3x3_winograd4_nhwc_dual_masked(const float* input, const float* u, float* out0, float* out1,
                                            const float* scale, const float* shift, const float* mask0,
                                            const float* mask1, int n0, int h0, int w0, int n1, int h1, int w1, int cin,
                                            int cout, long in_pix_stride, long out0_pix_stride, long out1_pix_stride,
                                            long mask0_pix_stride, long mask1_pix_stride, int flags, void* workspace,
                                            size_t workspace_bytes, dana_stream_t stream);

/* weight gradient of a stride-1 pad-1 3x3 conv in the F(4x4,3x3) domain: dU[36] = sum over tiles of
 * (A dY A^T)^T (B^T x B), dW = G^T dU G -- 4x fewer multiplies than dana_conv2d_wgrad_nhwc; same packed
 * [cout][3][3][cin] result, same row_scale / accumulate semantics. cin % 64 == 0, cout % 4 == 0. */
size_t dana_conv3x3_wgrad_winograd4_workspace_bytes(int batch, int h, int w, int cin, int cout);
int dana_conv3x3_wgrad_winograd4(const float* grad_out, const float* input, float* grad_weight, int batch, int h, int w,
                                 int cin, int cout, long in_pix_stride, long grad_pix_stride, const float* row_scale,
                                 int accumulate, void* workspace, size_t workspace_bytes, dana_stream_t stream);
/* ... with the input's transform handed in: v = the V planes [36][tiles][cin] that the forward's
 * dana_conv3x3_winograd4_nhwc(_masked) call over the same input left in the FIRST 36*tiles*cin floats of its workspace
 * (the caller keeps that buffer until the backward) -- the weight gradient skips its own input transform. Same workspace
 * size as dana_conv3x3_wgrad_winograd4. */
int dana_conv3x3_wgrad_winograd4_v(const float* grad_out, const float* v, float* grad_weight, int batch, int h, int w,
                                   int cin, int cout, long grad_pix_stride, const float* row_scale, int accumulate,
                                   void* workspace, size_t workspace_bytes, dana_stream_t stream);

/* nn.Linear / torch.bmm (dana.py:124,140,142,147,266-290): c[z][m][n] = epi(alpha * sum_k a[z][m][k]*b[z][n][k]).
 * Both operands K-contiguous ("NT"); nn.Linear weights [out][in] are used as stored. k % 4 == 0. */
int dana_gemm_nt(const float* a, const float* b, float* c, const float* scale, const float* shift,
                 const float* residual, int m, int n, int k, long lda, long ldb, long ldc, long ldr, int batch,
                 long batch_a, long batch_b, long batch_c, float alpha, int flags, dana_stream_t stream);

/* ---- HBM-bound layout / pooling / packing kernels ---------------------------------------------- */

/* boundary conversions between the reference's NCHW tensors and this build's NHWC activations */
int dana_nchw_to_nhwc(const float* in, float* out, int batch, int channels, int height, int width, int cpad,
                      long out_pix_stride, dana_stream_t stream);
int dana_nhwc_to_nchw(const float* in, float* out, int batch, int channels, int height, int width,
                      long in_pix_stride, dana_stream_t stream);
/* nn.MaxPool2d(3, 2, padding=0, ceil_mode=True): resnet.py:113 */
int dana_maxpool3x3s2_ceil_nhwc(const float* in, float* out, int batch, int height, int width, int channels,
                                dana_stream_t stream);
/* nn.AvgPool2d(14, stride=1) on the 20x20 support maps: dana.py:42,105-108 */
int dana_avgpool_nhwc(const float* in, float* out, int batch, int height, int width, int channels, int k, int stride,
                      dana_stream_t stream);
/* RCNN_top(pool5).mean(3).mean(2): dana.py:387-389; in[groups][positions][stride] -> out[groups][channels] */
int dana_spatial_mean_nhwc(const float* in, float* out, int groups, int positions, int channels, long in_pix_stride,
                           dana_stream_t stream);
/* sibling model `fgn` (framework/fgn.py:36-39,156-161): its head's nn.BatchNorm2d layers are NOT frozen. Batch
 * statistics over rows (= N*H*W) per channel, two passes (mean, then biased variance about it); workspace:
 * dana_colsum_workspace_bytes(rows, channels). dana_bn_fold turns (gamma, beta, mean, var) into scale / shift for
 * dana_scale_shift_relu: x = relu?(x * scale + shift), in place. */
int dana_batch_stats(const float* x, float* mean, float* var_biased, long rows, int channels, long ld, void* workspace,
                     size_t workspace_bytes, dana_stream_t stream);
int dana_scale_shift_relu(float* x, const float* scale, const float* shift, long rows, int channels, int relu,
                          dana_stream_t stream);
/* adjoint of a TRAIN-mode nn.BatchNorm2d over NHWC rows (batch statistics mean / var_biased of x, as dana_batch_stats
 * returns them): grad_x = gamma / sqrt(var + eps) * (g - mean(g) - xhat * mean(g * xhat)), grad_gamma (+)= sum g * xhat,
 * grad_beta (+)= sum g (fgn.py:147-153: the head's bn1 / bn2 are ordinary, trainable BatchNorm layers) */
int dana_bn_train_backward(const float* grad_out, const float* x, const float* mean, const float* var_biased,
                           const float* gamma, float eps, long rows, int channels, float* grad_x, float* grad_gamma,
                           float* grad_beta, int accumulate, dana_stream_t stream);
/* sibling model `fsod` (framework/fsod.py:109-116, 207-214): depth-wise "valid" cross-correlation
 * F.conv2d(feat, kernel.view(C, 1, kh, kw), groups=C): out[n][oh][ow][c] = sum feat[n][oh+i][ow+j][c] *
 * kernels[n / maps_per_kernel][i][j][c]; feat [n_maps][height][width][feat_pix_stride], out [n_maps][oh][ow][channels] */
int dana_depthwise_corr_nhwc(const float* feat, const float* kernels, float* out, long n_maps, int height, int width,
                             int channels, int kh, int kw, long maps_per_kernel, long feat_pix_stride,
                             dana_stream_t stream);
/* class sweep of the fsod attention RPN (framework/fsod.py:109-116 per problem): out map n = the depth-wise
 * correlation of feat map n / group with kernels[n], n < n_maps; feat [ceil(n_maps / group)][height][width][feat_pix_stride].
 * Per-element arithmetic and order of dana_depthwise_corr_nhwc (a replicated feat map gives the same bits) */
int dana_depthwise_corr_nhwc_grouped(const float* feat, const float* kernels, float* out, long n_maps, int height,
                                     int width, int channels, int kh, int kw, int group, long feat_pix_stride,
                                     dana_stream_t stream);
/* adjoints of dana_depthwise_corr_nhwc: grad_feat [n_maps][height][width][channels] (dense; null to skip) and
 * grad_kernels [ceil(n_maps / maps_per_kernel)][kh][kw][channels] (null to skip; accumulated when accumulate_kernels) */
int dana_depthwise_corr_backward_nhwc(const float* grad_out, const float* feat, const float* kernels, float* grad_feat,
                                      float* grad_kernels, long n_maps, int height, int width, int channels, int kh,
                                      int kw, long maps_per_kernel, long feat_pix_stride, int accumulate_kernels,
                                      dana_stream_t stream);
/* sibling model `meta` (framework/meta.py): nn.MaxPool2d(2) of the PRN (:203,246), nn.Sigmoid (:202,250), and the
 * channel-wise product of the RoI features with their image's class-attentive vector (:136-140) */
int dana_maxpool2x2s2_nhwc(const float* in, float* out, int batch, int height, int width, int channels,
                           dana_stream_t stream);
/* adjoint of dana_maxpool2x2s2_nhwc: grad_in[b][y][x][c] = grad_out of the window whose (first) maximum the element is */
int dana_maxpool2x2s2_backward_nhwc(const float* in, const float* grad_out, float* grad_in, int batch, int height,
                                    int width, int channels, dana_stream_t stream);
int dana_sigmoid(float* x, long n, dana_stream_t stream);
int dana_scale_rows_by_group(const float* x, const float* group_vec, float* out, long rows, long rows_per_group,
                             int channels, dana_stream_t stream);
/* class sweep of the fgn attention RPN (framework/fgn.py:71-73 per problem): out row p*rows + i = x row
 * (p / group)*rows + i (row stride ld_x; 0 = channels) times vec[p], channel-wise, p < n_blocks; out dense. The product of
 * dana_scale_rows_by_group on replicated rows (same bits); channels % 4 == 0, 16-byte aligned pointers */
int dana_scale_rows_grouped(const float* x, const float* vec, float* out, long rows, int channels, long ld_x, int group,
                            long n_blocks, dana_stream_t stream);
/* PositionalEncoding.forward: dana.py:322-324; out[r] = in[r] + pe[r % length] */
int dana_add_pe(const float* in, const float* pe, float* out, long rows, int length, int channels,
                long in_stride, long out_stride, dana_stream_t stream);
/* ... for `groups` row groups whose inputs sit in_group_stride floats apart (the positive supports of every image of the
 * batch, way * shot maps apart: dana.py:103,126-130) in one launch; out[g][r] = in[g][r] + pe[r % length] */
int dana_add_pe_groups(const float* in, const float* pe, float* out, long groups, long rows_per_group, int length, int channels,
                       long in_group_stride, long out_group_stride, dana_stream_t stream);
/* x - x.mean(1, keepdim=True): dana.py:125,141,267,272; x[groups][length][ld], in place */
size_t dana_colmean_sub_workspace_bytes(int groups, int length, int dim);
int dana_colmean_sub(float* x, int groups, int length, int dim, long ld, void* workspace, size_t workspace_bytes,
                     dana_stream_t stream);
/* .transpose(1, 2).contiguous() of [groups][rows][cols] -> [groups][cols][ldo] */
int dana_transpose_batched(const float* in, float* out, int groups, int rows, int cols, long ldi, long ldo,
                           long in_batch, long out_batch, dana_stream_t stream);
/* nn.Conv2d weight OIHW -> [O][KH][KW][I] (stem7: [O][7][8][4], zero padded) for dana_conv2d_nhwc */
int dana_pack_conv_weight(const float* w_oihw, float* out, int cout, int cin, int kh, int kw, int stem7,
                          dana_stream_t stream);
/* eval-mode nn.BatchNorm2d (dana.py:362-385) -> scale = gamma/sqrt(var+eps), shift = beta - mean*scale */
int dana_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps, float* scale,
                 float* shift, int n, dana_stream_t stream);

/* ---- BA block + CISA reductions: dana.py:133-147, 266-279 -------------------------------------- */

/* nn.Linear(dim, 1): out[r] = x[r].w + bias[0] (rpn_unary_layer, rcnn_unary_layer, rpn_channel_k_layer) */
int dana_rowdot(const float* x, const float* w, const float* bias, float* out, long rows, int dim, long ld,
                dana_stream_t stream);
/* F.softmax(x, last dim), in place, x[groups][length] */
int dana_softmax_rows(float* x, long groups, int length, long ld, dana_stream_t stream);
/* out-of-place: out[g][:length] = softmax(x[g][:length]) (cls_prob next to the untouched cls_score, dana.py:290-292) */
int dana_softmax_rows_to(const float* x, float* out, long groups, int length, long ld_in, long ld_out, dana_stream_t stream);
/* rois_label of the training forward (dana.py:191-194): out[0..n) = (int64) labels[i], out[n..2n) = 0 */
int dana_labels_posneg_i64(const float* labels, long long* out, long n, dana_stream_t stream);
/* S += gamma * leaky_relu(w^T S): dana.py:136-137; s[groups][length][ld], w[groups][length] */
int dana_ba_apply(float* s, const float* w, int groups, int length, int dim, long ld, float gamma, float slope,
                  dana_stream_t stream);
/* A = (softmax_keys(scores) + unary_gamma * unary^T) * out_scale per `length`-wide segment (one per shot):
 * dana.py:143-146 / :274-278; unary + (row / rows_per_batch)*unary_batch_stride -> [nseg][length]; cols nseg*length..kpad-1 zeroed */
int dana_attn_softmax_unary(float* scores, const float* unary, long rows, long rows_per_batch, long unary_batch_stride,
                            int nseg, int length, long ld, int kpad, float unary_gamma, float out_scale,
                            dana_stream_t stream);
/* ... with a per-segment scale in place of out_scale (shot views of unequal length): segment s of a row of batch
 * b = row / rows_per_batch is scaled by seg_scale[b*scale_batch_stride + s] (scale_batch_stride <= 0: nseg). A segment
 * whose scale is 0 is not read and written as +0.0f. Equal scales give the bits of dana_attn_softmax_unary. */
int dana_attn_softmax_unary_w(float* scores, const float* unary, long rows, long rows_per_batch, long unary_batch_stride,
                              int nseg, int length, long ld, int kpad, float unary_gamma, const float* seg_scale,
                              long scale_batch_stride, dana_stream_t stream);

/* ---- training targets for the sampled RoIs: lib/model/rpn/proposal_target_layer_cascade.py:33-213 ---- */

/* candidates = rois[B][n_rois][5] (cols 1..4) followed by gt_boxes[B][n_gt][5] (cols 0..3) (:43-47).
 * max_overlaps / gt_assignment [B][n_rois+n_gt] (bbox_overlaps_batch + torch.max, :122-124),
 * fg_list / bg_list: ascending candidate indices with max_overlap >= fg_thresh / in [bg_lo, bg_hi)
 * (:128-133), counts[B][2] = their lengths -- the only values the host RNG needs. */
int dana_proposal_target_prepare(const float* rois, const float* gt_boxes, int B, int n_rois, int n_gt,
                                 float fg_thresh, float bg_thresh_hi, float bg_thresh_lo, float* max_overlaps,
                                 int* gt_assignment, int* fg_list, int* bg_list, int* counts, dana_stream_t stream);
/* picks[B][rois_per_image]: position in fg_list for slot r < fg_taken[b], in bg_list otherwise (the
 * host draws them with np.random exactly as :143-175). means4/stds4/inside_w4 are HOST float[4].
 * -> rois_out[B][R][5], labels_out[B][R], bbox_targets / inside / outside weights [B][R][4] (:83-91,:183-204). */
int dana_proposal_target_gather(const float* rois, const float* gt_boxes, int B, int n_rois, int n_gt,
                                const int* gt_assignment, const int* fg_list, const int* bg_list, const int* picks,
                                const int* fg_taken, int rois_per_image, const float* means4, const float* stds4,
                                const float* inside_w4, int normalize, float* rois_out, float* labels_out,
                                float* bbox_targets, float* inside_weights, float* outside_weights,
                                dana_stream_t stream);

/* ---- anchor targets + RPN losses: lib/model/rpn/anchor_target_layer.py:48-193, rpn.py:97-115 ---------- */

/* All H*W*A anchors per image in (h, w, a) order. labels[B][n] before subsampling (-1 / 0 / 1; anchors
 * outside image 0's bounds stay -1), max_overlaps (-2 = outside), argmax over gt, ascending fg (label 1) /
 * bg (label 0) lists and counts[B][2] for the host's np.random.permutation draws (:137-156). */
int dana_anchor_target_prepare(const float* gt_boxes, const float* im_info, const float* base_anchors, int B,
                               int A, int H, int W, int feat_stride, int n_gt, float negative_overlap,
                               float positive_overlap, float* labels, float* max_overlaps, int* argmax,
                               int* fg_list, int* bg_list, int* counts, dana_stream_t stream);
/* labels[image][list[pos]] = -1 for n subsampled-away entries; which[e] = image*2 + (0 fg | 1 bg). */
int dana_anchor_target_disable(float* labels, const int* fg_list, const int* bg_list, const int* which,
                               const int* pos, int n, int anchors_per_image, dana_stream_t stream);
/* the same with the number of entries read from DEVICE memory (n_dev[0] <= capacity) and the entries interleaved as
 * (which, pos) pairs: the launch parameters never change, so a captured hipGraph can replay it with each step's draws */
int dana_anchor_target_disable_dev(float* labels, const int* fg_list, const int* bg_list, const int* n_dev,
                                   const int* which_pos_pairs, int capacity, int anchors_per_image,
                                   dana_stream_t stream);
/* _AnchorTargetLayer's four outputs in the reference layouts: labels_out[B][A*H*W] (a-major),
 * bbox_targets / inside / outside weights [B][4A][H*W] (:171-191). */
int dana_anchor_target_outputs(const float* labels, const float* max_overlaps, const int* argmax,
                               const float* gt_boxes, const float* base_anchors, int B, int A, int H, int W,
                               int feat_stride, int n_gt, float inside_weight, float outside_weight, const float* outside_weight_dev,
                               float* labels_out, float* bbox_targets, float* inside_weights,
                               float* outside_weights, dana_stream_t stream);
/* RCNN losses of the training forward (dana.py:199-217), fused: rows 0..n-1 = positive-support head scores
 * [n][2] with the proposal-target labels [n] (0 / 1), rows n..2n-1 = negative-support head scores (labels 0).
 * losses3[0] = cross-entropy over fg + hard-negative-mined bg rows (1:2:1: bg ranked by fg probability, descending, per
 * half; dana.py:204-215), losses3[1] = _smooth_l1_loss(bbox_pred, targets, in, out) (net_utils.py:71-85, sigma,
 * mean over rois), losses3[2] = number of rows kept. Optional gradient seeds (may be NULL): d losses3[0] / d scores
 * and d losses3[1] / d bbox_pred. No host sync (the reference's nonzero / sort / index chain has three). */
/* the plain losses of the sibling detectors (faster_rcnn.py:93-98): losses2[0] = F.cross_entropy(scores [n][n_classes],
 * labels int64 [n]) (mean), losses2[1] = _smooth_l1_loss(sigma) (net_utils.py:71-85); optional gradient seeds
 * d losses2[0] / d scores [n][n_classes] and d losses2[1] / d bbox_pred [n][4]. One launch, no host sync.
 * A label outside 0..n_classes-1 is never used as an index: losses2[0] and that row's score gradient become NaN
 * (F.cross_entropy would raise); there is no ignore_index. */
int dana_plain_rcnn_loss(const float* scores, const long long* labels, const float* bbox_pred, const float* bbox_targets,
                         const float* inside_weights, const float* outside_weights, int n, int n_classes, float sigma,
                         float* losses2, float* grad_scores, float* grad_bbox, dana_stream_t stream);
size_t dana_rcnn_loss_workspace_bytes(int n);
int dana_rcnn_loss(const float* score_pos, const float* score_neg, const float* labels, const float* bbox_pred,
                   const float* bbox_targets, const float* inside_weights, const float* outside_weights, int n,
                   float sigma, float* losses3, float* grad_score_pos, float* grad_score_neg, float* grad_bbox,
                   void* workspace, size_t workspace_bytes, dana_stream_t stream);
/* losses3[0] = F.cross_entropy over labels >= 0 (rpn.py:97-105), losses3[1] = _smooth_l1_loss(sigma, dims 1,2,3)
 * (rpn.py:114), losses3[2] = number of labels >= 0; outside_weight_dev (optional, device) overrides outside_weight; fused over heads[B*H*W][row stride] = (2A cls | 4A bbox) without materialising the targets. */
size_t dana_rpn_loss_workspace_bytes(void);
int dana_rpn_loss(const float* heads, long head_row_stride, const float* labels, const int* argmax,
                  const float* gt_boxes, const float* base_anchors, int B, int A, int H, int W, int feat_stride,
                  int n_gt, float sigma, float inside_weight, float outside_weight, const float* outside_weight_dev, float* losses3, void* workspace,
                  size_t workspace_bytes, dana_stream_t stream);

/* ---- backward building blocks of the conv / Linear layers (training step, SURVEY.md 8d variant S) --------
 * what autograd + cuDNN compute for nn.Conv2d in the reference's loss.backward() (train.py:141-143) */

/* grad_weight[cout][kh][kw][cin] (+)= row_scale[cout] * sum_m grad_out[m][cout] * im2col(input)[m][...]; deterministic
 * split-M reduction through the workspace. row_scale (optional) = the frozen-BN scale of each output channel, so the
 * launch can accumulate straight into a parameter gradient kept in this layout. cin % 64 == 0, cout % 4 == 0. */
size_t dana_conv2d_wgrad_workspace_bytes(int batch, int in_h, int in_w, int cin, int cout, int kh, int kw, int stride,
                                         int pad);
int dana_conv2d_wgrad_nhwc(const float* grad_out, const float* input, float* grad_weight, int batch, int in_h,
                           int in_w, int cin, int cout, int kh, int kw, int stride, int pad, long in_pix_stride,
                           long grad_pix_stride, const float* row_scale, int accumulate, void* workspace, size_t workspace_bytes,
                           dana_stream_t stream);
/* A batch of "TN" GEMMs, out[z][n][k] (+)= sum_m y[z][m][n] * x[z][m][k] for n < n_valid -- the adjoints of torch.bmm
 * w.r.t. its right operand (dana.py:140-150, 270-283: d value / d key of the dual-awareness attention), one plane z per
 * image in ONE launch. y rows have ldy >= n floats (columns n_valid..n-1 may be zero padding), x rows ldx >= k; planes
 * are batch_y / batch_x / batch_out floats apart. k % 64 == 0, n % 4 == 0; deterministic split-M reduction. */
size_t dana_gemm_tn_batched_workspace_bytes(int planes, int m, int n, int k);
int dana_gemm_tn_batched(const float* y, const float* x, float* out, int planes, int m, int n, int k, long ldy, long ldx,
                         long batch_y, long batch_x, long batch_out, int n_valid, int accumulate, void* workspace,
                         size_t workspace_bytes, dana_stream_t stream);
/* weights for the data gradient of a stride-1 conv: out[cin][kh][kw][cout] = w[cout][KH-1-kh][KW-1-kw][cin]*scale[cout];
 * grad_input = dana_conv2d_nhwc(grad_out, out, cin <-> cout swapped, same kernel size / pad) */
int dana_conv2d_dgrad_weight(const float* w_packed, const float* scale, float* out, int cout, int cin, int kh, int kw,
                             dana_stream_t stream);
/* data gradient of a strided 1x1 conv: scatter the compact result to the strided positions, zero elsewhere;
 * mask_act (optional, [batch][ih][iw][channels]): zero the gradient where that activation is <= 0 (ReLU adjoint) */
int dana_upsample_scatter_nhwc(const float* compact, float* out, const float* mask_act, int batch, int oh, int ow,
                               int ih, int iw, int channels, int stride, dana_stream_t stream);

/* the rows a strided 1x1 conv reads (resnet.py:71), compacted: compact[b][oh][ow][:] = x[b][oh*stride][ow*stride][:];
 * its weight gradient is then dana_conv2d_wgrad_nhwc with stride 1 over [batch][oh][ow] */
int dana_downsample_gather_nhwc(const float* x, float* compact, int batch, int ih, int iw, int channels, int stride,
                                long in_pix_stride, dana_stream_t stream);

/* element-wise / reduction glue of the backward pass */
int dana_relu_mask(float* grad, const float* act, long rows, int channels, long ld_grad, long ld_act,
                   dana_stream_t stream);                       /* grad *= (saved output > 0) */
int dana_axpy_rows(float* y, const float* x, long rows, int channels, long ld_y, long ld_x, float alpha,
                   int accumulate, dana_stream_t stream);        /* y (+)= alpha * x, strided rows */
/* y *= x over strided rows: the correlation of attention_type 'product' (dana.py:155-156: base_feat * dense_support_feature;
 * :285-286: query_mat * dense_support_feature), in place in the attended buffer */
int dana_mul_rows(float* y, const float* x, long rows, int channels, long ld_y, long ld_x, dana_stream_t stream);
int dana_rowscale(float* dw, const float* scale, int rows, long cols, dana_stream_t stream); /* frozen-BN scale on dW rows */
int dana_unpack_conv_weight_grad(const float* packed, float* w_oihw, int cout, int cin, int kh, int kw, int accumulate,
                                 dana_stream_t stream);          /* packed [O][KH][KW][I] -> OIHW (.grad layout) */
size_t dana_colsum_workspace_bytes(long rows, int channels);
int dana_colsum(const float* x, float* out, long rows, int channels, long ld, float alpha, int accumulate,
                void* workspace, size_t workspace_bytes, dana_stream_t stream);   /* bias gradients, deterministic */
int dana_avgpool_backward_nhwc(const float* grad_out, float* grad_in, int batch, int height, int width, int channels,
                               int k, int stride, dana_stream_t stream);
/* dana_colsum over `batch` matrices in one launch pair: matrix z at x + z * x_batch, its sums at out + z * out_batch
 * (the unary-term adjoint of the attention, one matrix per image: dana.py:132-137); workspace = batch x the single one */
int dana_colsum_batched(const float* x, float* out, int batch, long rows, int channels, long ld, long x_batch, long out_batch,
                        float alpha, int accumulate, void* workspace, size_t workspace_bytes, dana_stream_t stream);
int dana_softmax_rows_backward(float* grad, const float* prob, long rows, int length, long ld_grad, long ld_prob,
                               dana_stream_t stream);            /* grad <- p * (grad - <p, grad>) */
int dana_gemm_small(const float* a, long a_stride_m, long a_stride_k, const float* b, long b_stride_k, long b_stride_n,
                    float* c, long c_stride_m, long c_stride_n, int m, int n, int k, float alpha, int accumulate,
                    dana_stream_t stream);                       /* skinny heads (N or K of 2 / 4) */

/* torch.optim.SGD with momentum over a flat fp32 segment (train.py:76-87: lr, 2x lr and no decay for biases):
 * g' = grad_scale * g + weight_decay * p; buf = first_step ? g' : momentum * buf + g'; p -= lr * buf */
int dana_sgd_momentum(float* params, const float* grads, float* momentum_buf, long n, float lr, float momentum,
                      float weight_decay, float grad_scale, int first_step, dana_stream_t stream);
/* torch.optim.Adam over a flat fp32 segment (train.py:84-85; defaults betas (0.9, 0.999), eps 1e-8): step = 1, 2, ... */
int dana_adam(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1,
              float beta2, float eps, float weight_decay, float grad_scale, int step, dana_stream_t stream);
/* ---- optimizer scalars in device memory (train.py:76-87,118-120; net_utils.py:37-48) ---------------------------------
 * dana_sgd_momentum / dana_adam take lr, grad_scale and Adam's step as launch parameters, which a recorded launch list
 * (launch programs, hipGraph) freezes. The *_ctl forms below read them from a control block of two small fp32 arrays in
 * device memory, so that a learning-rate schedule (train.py:118-120), Adam's step count (train.py:84-85) and the
 * gradient-norm clipping of net_utils.clip_gradient (net_utils.py:37-48; imported by train.py:18) are DATA of a replay:
 *
 *   hyper[DANA_OPTIM_HYPER_FLOATS], written by the HOST (one stream-ordered upload per iteration, packed by
 *   dana_optim_pack_hyper):  [0..3] effective learning rate of parameter group 0..3 (lr * the group's multiplier,
 *   train.py:79-84), [4] grad_scale (1 / world size of the gradient mean), [5] clip_norm (0 = no clipping),
 *   [6] bc1 = 1 - beta1^step, [7] bc2 = 1 - beta2^step (Adam's bias corrections; 1 for SGD)
 *   state[DANA_OPTIM_STATE_FLOATS], written by the DEVICE (dana_optim_prepare; the upload never touches it):
 *   [0] sqnorm = sum of g^2 over all groups, [1] total_norm = grad_scale * sqrt(sqnorm): the norm clip_gradient measures
 *   on the mean gradients, before clipping, [2] coef = clip_norm / max(total_norm, clip_norm) (1 when clip_norm == 0),
 *   [3] gs_eff = grad_scale * coef: what the *_ctl updates multiply the raw gradient sums by
 *
 * Without clipping nobody runs dana_optim_prepare: the caller initialises state once to (0, 0, 1, grad_scale). */
#define DANA_OPTIM_MAX_GROUPS 4
#define DANA_OPTIM_HYPER_FLOATS 8
#define DANA_OPTIM_STATE_FLOATS 4
/* Host only (no GPU, no stream): fills hyper_host[DANA_OPTIM_HYPER_FLOATS] (pinned or pageable host memory) in the layout
 * above. lrs[groups] are the effective rates, 1 <= groups <= DANA_OPTIM_MAX_GROUPS (the other slots become 0);
 * clip_norm >= 0; step >= 1 counts like dana_adam's and the bias corrections are formed exactly as dana_adam forms them
 * (1.0 - pow((double)beta, step), rounded to float); beta1 = beta2 = 0 (SGD) gives bc1 = bc2 = 1. */
int dana_optim_pack_hyper(float* hyper_host, const float* lrs, int groups, float grad_scale, float clip_norm, float beta1,
                          float beta2, int step);
/* Sum of g^2 over one flat fp32 segment (n % 4 == 0, 16-byte aligned; n == 0 writes nothing and contributes 0) as one
 * DOUBLE partial per workgroup in partials[dana_grad_sqnorm_workspace_bytes(n) / 8] (8-byte aligned). Deterministic: the
 * grid is a function of n alone (ceil(n / 1024) workgroups of 256 threads, at most 2048), every thread sums a fixed
 * grid-strided set of float4s in four fp32 chains (18 FMAs each at the 37 M gradients of a DAnA trainer, 256 at 2^29
 * elements), and the chains, the 64 lanes of a wave (cross-lane shuffles) and the four waves (LDS) are combined in double
 * in a fixed order; one plain store per workgroup, no atomics -- two calls, on any stream, give the same bits. */
size_t dana_grad_sqnorm_workspace_bytes(long n);
int dana_grad_sqnorm(const float* grads, long n, void* partials, size_t partials_bytes, dana_stream_t stream);
/* One workgroup: sums partials[count] (the partials of all groups, laid out one group behind the other; count >= 0) in
 * double -- thread t takes elements t, t + 256, ... in index order, then the fixed lane / wave tree -- so that the sum
 * depends on the concatenated sequence only, not on where one group ends; then writes state[0..3] as defined above from
 * hyper[4] (grad_scale) and hyper[5] (clip_norm) with plain stores of one lane. coef is exactly 1.0f, and gs_eff the bits
 * of grad_scale, when clip_norm == 0 or total_norm <= clip_norm. */
int dana_optim_prepare(const void* partials, long count, const float* hyper, float* state, dana_stream_t stream);
/* dana_sgd_momentum / dana_adam with the same arithmetic in the same order (the same bits when coef == 1), where
 * lr = hyper[group], grad_scale = state[3] (gs_eff) and Adam's bc1 / bc2 = hyper[6] / hyper[7]; what never changes during
 * a run (momentum, weight decay, betas, eps, first_step) stays a launch parameter. 0 <= group < DANA_OPTIM_MAX_GROUPS. */
int dana_sgd_momentum_ctl(float* params, const float* grads, float* momentum_buf, long n, const float* hyper,
                          const float* state, int group, float momentum, float weight_decay, int first_step,
                          dana_stream_t stream);
int dana_adam_ctl(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long n, const float* hyper,
                  const float* state, int group, float beta1, float beta2, float eps, float weight_decay,
                  dana_stream_t stream);
/* adjoint of dana_rowdot: grad_w[dim] (+)= sum_r grad_out[r] x[r]; grad_x[r] += grad_out[r] w (grad_x may be NULL);
 * workspace: dana_colsum_workspace_bytes(rows, dim) */
int dana_rowdot_backward(const float* x, const float* grad_out, const float* w, float* grad_x, float* grad_w, long rows,
                         int dim, long ld_x, long ld_grad_x, int accumulate_w, void* workspace, size_t workspace_bytes,
                         dana_stream_t stream);
/* out[g][p][:] (+)= alpha * in[g][:] : adjoint of dana_spatial_mean_nhwc (alpha = 1/positions) */
int dana_broadcast_rows(const float* in, float* out, long groups, int positions, int channels, float alpha,
                        int accumulate, dana_stream_t stream);
/* adjoint of dana_ba_apply (dana.py:133-137), in place on grad_s [groups*length][dim]: s = the block's INPUT,
 * gvec[groups][dim] = weights^T s, gsum[groups][dim] = column sums of grad_s per group; grad_weights[groups*length] out */
/* ... its two per-group reductions in one launch: gvec[g][:] = weights[g]^T s[g], gsum[g][:] = column sums of grad_s[g] */
int dana_ba_backward_prep(const float* s, const float* weights, const float* grad_s, float* gvec, float* gsum, long groups,
                          int length, int dim, dana_stream_t stream);
int dana_ba_backward(float* grad_s, const float* s, const float* weights, const float* gvec, const float* gsum,
                     float* grad_weights, long groups, int length, int dim, float gamma, float slope,
                     dana_stream_t stream);
/* adjoint of dana_attn_softmax_unary, in place on grad_a: -> alpha * dL/d(raw scores) (alpha = the 1/sqrt(d) of QK^T) */
int dana_attn_softmax_unary_backward(float* grad_a, const float* a, const float* unary, long rows, long rows_per_batch,
                                     long unary_batch_stride, int nseg, int length, long ld, int kpad,
                                     float unary_gamma, float out_scale, float alpha, dana_stream_t stream);
/* adjoint of dana_rpn_loss w.r.t. the head buffer: grad_heads[B*H*W][row stride] (zero-filled here);
 * losses3 = dana_rpn_loss's DEVICE output (its [2] is the cross-entropy's divisor); grad_cls / grad_box = upstream scalars,
 * or grad_scales_dev (2 floats in device memory) when given */
int dana_rpn_loss_backward(const float* heads, long head_row_stride, const float* labels, const int* argmax,
                           const float* gt_boxes, const float* base_anchors, int B, int A, int H, int W,
                           int feat_stride, int n_gt, float sigma, float inside_weight, float outside_weight, const float* outside_weight_dev,
                           const float* losses3, float grad_cls, float grad_box, const float* grad_scales_dev,
                           float* grad_heads, dana_stream_t stream);
/* x[0..n) *= scalar_dev[0]: applies an upstream loss gradient that lives in device memory (no host sync) */
int dana_scale_by_device_scalar(float* x, long n, const float* scalar_dev, dana_stream_t stream);

/* ---- episode input pipeline: the loaders' per-image cv2 / numpy work ------------------------ */

/* minibatch.py:70-84 + blob.py:35-52 (prep_im_for_blob): RGB uint8 [h][w][3] -> BGR, optional horizontal flip,
 * fp32 minus cfg.PIXEL_MEANS (3 HOST floats, BGR order), cv2.resize(fx = fy = im_scale, INTER_LINEAR)
 * -> out [out_h][out_w][3] fp32 (the caller computes out_h/out_w = round(h * im_scale) like cv2 does) */
int dana_prep_image(const unsigned char* rgb_hwc, int height, int width, long row_stride_bytes, int flipped,
                    const float* pixel_means_bgr, double im_scale, float* out_hwc, int out_h, int out_w,
                    dana_stream_t stream);
/* fs_loader.py:118-139: crop [y_min..y_max] x [x_min..x_max] (inclusive) out of a prepared fp32 HWC image,
 * cv2.resize(dsize = (resized_w, resized_h), INTER_LINEAR), transpose to CHW, zero-pad to [3][target][target] */
int dana_crop_resize_pad(const float* im_hwc, int height, int width, int x_min, int y_min, int x_max, int y_max,
                         int resized_w, int resized_h, int target, float* out_chw, dana_stream_t stream);
/* fs_loader.py:186-280,318: crop window (start, size) of a prepared fp32 HWC image, zero-padded to [out_h][out_w] and
 * permuted to CHW: one plane set of the batch holder */
int dana_crop_pad_chw(const float* im_hwc, int height, int width, int y_start, int x_start, int crop_h, int crop_w,
                      float* out_chw, int out_h, int out_w, dana_stream_t stream);

/* A batch of episodes from a resident image pool (csrc/episode.hip; dana_amd/pipeline.py builds the pool and the plan).
 * pool: packed uint8 RGB frames in one DEVICE byte buffer; offsets[n_rows] = byte offset of each row's frame,
 * meta[n_rows][5] = (h, w, flipped, first box, box count). plan: DEVICE int32 words: 16-word query records at q_off,
 * 16-word support records at s_off, the queries' box orders behind them (word layout: the enums of episode.hip,
 * written by pipeline.plan_episode). pixel_means_bgr: 3 HOST floats. A record that names no image of the pool writes
 * zeros; nothing outside the pool is read. Results have the bits of the per-image entry points above. */

/* minibatch.py:70-96 + blob.py:35-52 + fs_loader.py:186-280,318 for all `batch` queries: im_data [batch][3][height][width]
 * = dana_prep_image's value at prepared pixel (y_s + y, x_s + x) inside each record's copy window, 0 elsewhere (no fp32
 * intermediate image); im_info [batch][3] = (height, width, im_scale) (fs_loader.py:266-283,319) */
int dana_episode_queries(const unsigned char* pool, long pool_bytes, const long long* offsets, const int* meta,
                         int n_rows, const int* plan, int plan_words, int q_off, int batch,
                         const float* pixel_means_bgr, float* im_data, int height, int width, float* im_info,
                         dana_stream_t stream);
/* fs_loader.py:113-139,149-174 for all n_supports supports: whole image to im_scale, box crop resized to rw x rh, CHW,
 * zero-padded -> out_chw [n_supports][3][target][target] (dana_prep_image then dana_crop_resize_pad, composed per pixel) */
int dana_episode_supports(const unsigned char* pool, long pool_bytes, const long long* offsets, const int* meta,
                          int n_rows, const int* plan, int plan_words, int s_off, int n_supports,
                          const float* pixel_means_bgr, int target, float* out_chw, dana_stream_t stream);
/* minibatch.py:52-54 + fs_loader.py:183-315 for all `batch` queries: boxes [n_boxes_total][5] (x1, y1, x2, y2, class,
 * unscaled) gathered in the plan's order, scaled (product in double, rounded to float), shifted by the crop start, clamped,
 * degenerate boxes dropped, compacted, cut at max_num_box, zero-filled -> gt_boxes [batch][max_num_box][5] (the positive
 * class only, label 1) with num_boxes [batch], and all_cls_gt_boxes / all_cls_num_boxes of the same shapes */
int dana_episode_boxes(const float* boxes, long n_boxes_total, const int* meta, int n_rows, const int* plan,
                       int plan_words, int q_off, int batch, int max_num_box, float* gt_boxes, long long* num_boxes,
                       float* all_cls_gt_boxes, long long* all_cls_num_boxes, dana_stream_t stream);

/* Training-time augmentation of such a batch. NOT IN THE REFERENCE: its loader has the flipped twin and the aspect-ratio
 * crop (fs_loader.py:186-255) and nothing else, so these three extend those lines and have no counterpart to be checked
 * against; with records that ask for nothing they give the bits of the three entry points above.
 * The plan carries a third section of 16-word augmentation records (pipeline.plan_episode writes it when a query or a
 * support asks for augmentation): float M[3][4] in words 0..11, float min_visible in word 12, flags in word 13 (1: the
 * record has a colour map, 2: it has a visibility threshold). a_off is the word offset of the FIRST record the call reads
 * -- the queries' records come first in the section, the supports' follow them -- and must be even and inside plan_words.
 * Colour: every source tap (r, g, b) of a record with flag 1 counts as
 *   d_j = clamp(((M[j][0]*r + M[j][1]*g) + M[j][2]*b) + M[j][3], 0, 255), j in R, G, B   (float32, in this order, unfused)
 * before the mean is subtracted and before any interpolation: the image that was distorted and then prepared, except
 * that the distorted image is never rounded to uint8. */

/* dana_episode_queries (blob.py:35-52 + fs_loader.py:186-280) with the colour map of record b at its four source taps */
int dana_episode_queries_aug(const unsigned char* pool, long pool_bytes, const long long* offsets, const int* meta,
                             int n_rows, const int* plan, int plan_words, int q_off, int a_off, int batch,
                             const float* pixel_means_bgr, float* im_data, int height, int width, float* im_info,
                             dana_stream_t stream);
/* dana_episode_supports (fs_loader.py:113-139) with the colour map of record n at the (up to) sixteen source taps of its
 * two composed resamples */
int dana_episode_supports_aug(const unsigned char* pool, long pool_bytes, const long long* offsets, const int* meta,
                              int n_rows, const int* plan, int plan_words, int s_off, int a_off, int n_supports,
                              const float* pixel_means_bgr, int target, float* out_chw, dana_stream_t stream);
/* dana_episode_boxes (fs_loader.py:183-315) with one more reason to drop a box, in front of both compactions beside the
 * degenerate-box filter of :294,306: for a record with flag 2, u = the shifted row before the clamp, v = after it,
 * full = (u2 - u0) * (u3 - u1), seen = (v2 - v0) * (v3 - v1) in float32, and the box stays only if
 * seen >= min_visible * full */
int dana_episode_boxes_aug(const float* boxes, long n_boxes_total, const int* meta, int n_rows, const int* plan,
                           int plan_words, int q_off, int a_off, int batch, int max_num_box, float* gt_boxes,
                           long long* num_boxes, float* all_cls_gt_boxes, long long* all_cls_num_boxes,
                           dana_stream_t stream);

/* Composed queries: mosaic, copy-paste, random erasing. NOT IN THE REFERENCE (its loader, fs_loader.py:81-325, reads one
 * image per query), so the rule is this project's own; a query of one part at (0, 0) gives the bits of the entry points
 * above. A composed query is an ordered list of 1..16 parts painted into one holder image, later parts over earlier ones.
 * The plan carries one more section at c_off (an even word, written by pipeline.plan_episode when a query asks for it):
 *   `batch` headers of 8 words: part count, positive class, float min_visible, flags (2: a visibility threshold)
 *   `batch` tables of max_parts part records of 32 words each (query b's table starts at record b * max_parts):
 *     words 0..11 as a query record (row, order length, double im_scale, double 1 / im_scale, y_s, x_s, h, w, clamp_x,
 *     clamp_y), 12..13 the destination (dy, dx), 14 the word offset of the part's box order, 15 flags (1: a colour map),
 *     16..27 float M[3][4]. A part whose row is outside the pool (an erase part has row -1) paints zeros, has no boxes and
 *     occludes like any other.
 * max_parts is the largest part count of the batch and must lie in 1..16; a header's own count is limited to it. Both
 * entry points refuse a section that does not fit plan_words, an odd c_off and a max_parts outside 1..16. */

/* dana_episode_queries_aug (blob.py:35-52 + fs_loader.py:186-280) per part: holder pixel (y, x) belongs to the LAST part
 * whose rectangle [dy, dy + h) x [dx, dx + w) contains it and holds that part's value at prepared pixel (y_s + y - dy,
 * x_s + x - dx), the same expressions with that part's colour map; 0 under no part. im_info [batch][3] = (height, width,
 * im_scale of part 0) */
int dana_episode_queries_composed(const unsigned char* pool, long pool_bytes, const long long* offsets, const int* meta,
                                  int n_rows, const int* plan, int plan_words, int c_off, int max_parts, int batch,
                                  const float* pixel_means_bgr, float* im_data, int height, int width, float* im_info,
                                  dana_stream_t stream);
/* dana_episode_boxes_aug (minibatch.py:52-54 + fs_loader.py:183-315) over the parts in order: u, v of a box as there, the
 * output row t = v + (dx, dy, dx, dy); hidden = the sum over the later parts r, in order, of ox * oy with ox = max(min(t2,
 * dx_r + w_r - 1) - max(t0, dx_r), 0) and oy alike (float32; an area two later parts share counts twice). A box stays if
 * v is not degenerate and, under a threshold, (seen - hidden) >= min_visible * full. Both lists are compacted in walk
 * order across the parts and cut at max_num_box. */
int dana_episode_boxes_composed(const float* boxes, long n_boxes_total, const int* meta, int n_rows, const int* plan,
                                int plan_words, int c_off, int max_parts, int batch, int max_num_box, float* gt_boxes,
                                long long* num_boxes, float* all_cls_gt_boxes, long long* all_cls_num_boxes,
                                dana_stream_t stream);

/* ---- counter-based device RNG for the training target layers (opt-in) ---------------------------
 * Philox-4x32-10 keyed by (seed, offset, image): the draws of anchor_target_layer.py:137-156 and
 * proposal_target_layer_cascade.py:143-175 without reading the fg / bg counts back to the host. */

/* counts[B][2] (fg, bg) from dana_proposal_target_prepare -> picks[B][rois_per_image] (positions in the fg list for
 * the first fg_taken[b] slots, in the bg list for the rest) for dana_proposal_target_gather */
int dana_proposal_target_sample(const int* counts, int B, int n_candidates, int rois_per_image, int fg_rois_per_image,
                                unsigned long long seed, unsigned long long offset, int* picks, int* fg_taken,
                                dana_stream_t stream);
/* labels[B][anchors_per_image] from dana_anchor_target_prepare: keep a uniform random num_fg-subset of the positives and
 * (rpn_batchsize - kept) of the negatives, label the rest -1; inv_num_examples[0] = 1 / (examples of the LAST image)
 * for the outside_weight_dev argument of dana_rpn_loss / dana_rpn_loss_backward / dana_anchor_target_outputs */
int dana_anchor_target_subsample(float* labels, const int* fg_list, const int* bg_list, const int* counts, int B,
                                 int anchors_per_image, int rpn_batchsize, int num_fg, unsigned long long seed,
                                 unsigned long long offset, float* inv_num_examples, dana_stream_t stream);
/* fp32 weight rows [batch][n][k] (row stride ldw, batch stride batch_w floats) -> bf16 planes [batch][kp / 16][3][n][16]
 * (out: dana_split_weight_bytes bytes) for the DANA_W_SPLIT3 flag of the contraction entry points. A weight of the
 * reference (conv: packed [cout][kh*kw*cin]; nn.Linear: [out][in]) is split once per weight version. */
size_t dana_split_weight_bytes(int n, int k, int batch);
int dana_split_weight(const float* w, long ldw, int n, int k, int batch, long batch_w, void* out, dana_stream_t stream);

/* One contraction over TWO concatenated channel segments: out[m][n] = epi(sum_{k<k0} a0[m][k] w[n][k] +
 * sum_{k<k1} a1[pix1(m)][k] w[n][k0+k]) where a0 is an NHWC map on the OUTPUT grid [batch][oh][ow] (pixel stride
 * a0_pix_stride) and a1 an NHWC map [batch][h1][w1] sampled at (oh*stride1, ow*stride1). This is a Caffe-ResNet
 * bottleneck's 1x1 expand conv and its (strided) 1x1 downsample conv (resnet.py:84-100: out = relu(bn3(conv3(t)) +
 * bn_d(downsample(x)))) with both frozen-BN scales folded into the weight rows [cout][k0 + k1] (dana_pack_cat2_weight)
 * and the two shifts added: the downsample's output never goes through HBM. Split kernel only (dana_set_mfma_mode != 0). */
int dana_conv1x1_cat2_nhwc(const float* a0, long a0_pix_stride, int k0, const float* a1, long a1_pix_stride, int k1,
                           int batch, int h1, int w1, int stride1, const float* weight, float* output,
                           const float* scale, const float* shift, const float* residual, long out_pix_stride,
                           long res_pix_stride, int cout, int flags, dana_stream_t stream);
/* the same over TWO image groups in one launch (query batch + support batch of one trunk layer): a0 holds group 0's
 * output-grid rows, then group 1's; a1 group 0's [n0][h0][w0] pixels, then group 1's [n1][h1][w1]; results go to out0 /
 * out1 with their own row strides (dana.py:98,100: RCNN_base runs on both batches with the same weights) */
int dana_conv1x1_cat2_nhwc_dual(const float* a0, long a0_pix_stride, int k0, const float* a1, long a1_pix_stride, int k1,
                                int n0, int h0, int w0, int n1, int h1, int w1, int stride1, const float* weight,
                                float* out0, float* out1, const float* scale, const float* shift, long out0_pix_stride,
                                long out1_pix_stride, int cout, int flags, dana_stream_t stream);
/* Second half of a split-K contraction: out[m][n] = epi(alpha * sum_s partials[s][m][n]) with the same epilogue as
 * dana_gemm_nt (scale, shift, residual, DANA_EPI_RELU), summed in slice order (deterministic). The slices themselves
 * are one batched dana_gemm_nt launch whose batch strides walk K (batch_a = batch_b = K / slices). n % 4 == 0. */
int dana_splitk_reduce(const float* partials, int slices, int m, int n, float* out, long ldc, const float* scale,
                       const float* shift, const float* residual, long ldr, float alpha, int flags,
                       dana_stream_t stream);
/* w_cat[n][0:k0] = s0[n] * w0[n][:], w_cat[n][k0:] = s1[n] * w1[n][:], shift[n] = b0[n] + b1[n] (w0 / w1 packed [cout][k]) */
int dana_pack_cat2_weight(const float* w0, const float* s0, const float* b0, int k0, const float* w1, const float* s1,
                          const float* b1, int k1, int cout, float* w_cat, float* shift, dana_stream_t stream);
/* hipGraph-friendly forms of the two samplers: the per-call Philox offset is `offset + counter_dev[0]`, with the call
 * counter living in device memory and advanced by dana_counter_add inside the same captured graph, so that every replay
 * draws fresh samples */
int dana_proposal_target_sample_ctr(const int* counts, int B, int n_candidates, int rois_per_image,
                                    int fg_rois_per_image, unsigned long long seed, unsigned long long offset,
                                    const unsigned long long* counter_dev, int* picks, int* fg_taken,
                                    dana_stream_t stream);
int dana_anchor_target_subsample_ctr(float* labels, const int* fg_list, const int* bg_list, const int* counts, int B,
                                     int anchors_per_image, int rpn_batchsize, int num_fg, unsigned long long seed,
                                     unsigned long long offset, const unsigned long long* counter_dev,
                                     float* inv_num_examples, dana_stream_t stream);
int dana_counter_add(unsigned long long* counter_dev, unsigned long long inc, dana_stream_t stream);

/* ---- launch programs -------------------------------------------------------------------------------------------------
 * The reference's training iteration (train.py:125-143) is ~1 500 launches on this library; issued one by one from the host
 * language they cost more host time than the GPU needs for them at eight ranks per host. A program is a recorded list of
 * calls of THIS header's `int dana_*(...)` entry points (the stream is one of their arguments), hipEventRecord and
 * hipStreamWaitEvent operations, re-issued in order from one C loop: the recorded step's launches with its arguments on
 * its streams behind its event edges (dana_amd/program.py records them from the eager step). Host-only; no device memory,
 * no synchronisation. A program is replayed by one thread at a time.
 *   signature: one character per argument of the entry point -- i (int), l (long / size_t / unsigned long long), p (pointer /
 *   dana_stream_t), f (float), d (double); words[k]: argument k as a 64-bit word (integers sign-extended, a float's bits in
 *   the low half, a double's bits). dana_program_run re-issues entries [begin, end) and returns the first non-zero status. */
int dana_program_create(void** program_out);
int dana_program_destroy(void* program);
int dana_program_add_call(void* program, void* entry_point, const char* signature, const unsigned long long* words, int nargs);
int dana_program_add_event_record(void* program, void* event, dana_stream_t stream);
int dana_program_add_event_wait(void* program, void* event, dana_stream_t stream);
int dana_program_size(void* program);
/* device memory zero fill / device-to-device copy on a stream (hipMemsetAsync / hipMemcpyAsync): what torch's zeros / zero_
 * and copy_ / clone do inside a recorded backward, as entry points a launch program can re-issue from its C loop */
int dana_fill_zero(void* dst, size_t bytes, dana_stream_t stream);
int dana_copy_d2d(void* dst, const void* src, size_t bytes, dana_stream_t stream);
int dana_program_run(void* program, int begin, int end);

/* ---- detection evaluation: lib/datasets/voc_eval.py (the last line of inference.py, :181) ---------------------------------
 * The VOC protocol on the device, in float64: NOT COCOeval (no crowd regions, area ranges or maxDets). Evaluating at the
 * thresholds 0.50:0.05:0.95 is voc_eval called with ten `ovthresh` values, done here in one pass. The COCO protocol is
 * dana_eval_coco, at the end of this section. */

/* Grows the evaluator's detection buffers (what pascal_voc.py:268-291 writes to per-class text files and voc_eval.py:143-151
 * parses again): the packed rows of n_problems detection sets -> det[capacity][5] / det_img / det_cls from row dst_base on.
 * Destination row dst_base + i with dst_offsets[p] <= i < dst_offsets[p+1] is source row src_offsets[p] + (i - dst_offsets[p])
 * and gets the ids prob_img[p], prob_cls[p] (all four tables in device memory; `rows` = dst_offsets[n_problems] is the
 * caller's host copy of the count). */
int dana_eval_append(const float* src_dets, const int* dst_offsets, const int* src_offsets, const int* prob_img,
                     const int* prob_cls, int n_problems, long rows, float* det, int* det_img, int* det_cls,
                     long dst_base, long capacity, dana_stream_t stream);
/* 0 for a shape dana_eval_ap refuses */
size_t dana_eval_ap_workspace_bytes(long n, long g, int n_img, int n_cls, int n_thr);
/* voc_eval.py:157-210 for every class and n_thr (1..16) IoU thresholds at once. det[n][5] = (x1, y1, x2, y2, score) with
 * image / class ids det_img / det_cls; ground truth gt_box[g][4], gt_img, gt_cls, gt_difficult (bytes, non-zero =
 * difficult). Rows whose ids are outside [0, n_img) x [0, n_cls) take no part.
 *   order[n]: detection index by rank -- class ascending, score descending, equal scores in arrival order (:159-162; the
 *     reference's argsort leaves the order of ties undefined); cls_offsets[n_cls + 1]: class c holds ranks
 *     cls_offsets[c] .. cls_offsets[c+1];
 *   tpfp[n_thr][n] by rank: 1 = TP, 2 = FP, 0 = matched a difficult box (:165-199; IoU with the `+ 1.` convention, the
 *     lowest index among equal maxima, the taken state per class, image and threshold);
 *   rec / prec [n_thr][n] by rank (:202-207), both null when not wanted; npos[n_cls]: non-difficult boxes per class;
 *   ap[n_cls][n_thr]: voc_ap (:35-66), the 11-point metric when use_07_metric != 0. A class with npos == 0 has AP = NaN
 *     under both metrics (the reference: 0 under the 11-point one, NaN under the other).
 * iou_thr, rec, prec and ap are arrays of C `double` and tpfp one of bytes, passed as void* (this header keeps to the
 * pointer types it already had). Sums run in a fixed order: two calls give the same bits. No synchronisation, no
 * device-to-host copy. */
int dana_eval_ap(const float* det, const int* det_img, const int* det_cls, long n, const float* gt_box,
                 const int* gt_img, const int* gt_cls, const unsigned char* gt_difficult, long g, int n_img, int n_cls,
                 const void* iou_thr, int n_thr, int use_07_metric, int* order, int* cls_offsets, void* tpfp, void* rec,
                 void* prec, void* ap, int* npos, void* workspace, size_t workspace_bytes, dana_stream_t stream);

/* The COCO protocol: what lib/datasets/coco_split.py:287-298 asks of pycocotools -- COCOeval.evaluate() and accumulate()
 * for iouType = 'bbox' with maskApi's bbIou -- restated from the published algorithm (pycocotools is not part of the
 * reference tree). Float64, unfused. 0 for a shape dana_eval_coco refuses. */
size_t dana_eval_coco_workspace_bytes(long n, long g, int n_img, int n_cls, int n_thr, int n_rec, int n_area,
                                      int n_max_dets);
/* det[n][5] = (x1, y1, x2, y2, score) with det_img / det_cls; a detection is the COCO box (x1, y1, x2 - x1 + 1,
 * y2 - y1 + 1) of coco_split.py:308-312. Ground truth: gt_bbox[g][4] = (x, y, w, h), gt_img, gt_cls, gt_area[g] (C
 * `double`: the annotation's area), gt_flags[g] (bytes: bit 0 = iscrowd, bit 1 = ignore). Rows whose ids are outside
 * [0, n_img) x [0, n_cls) take no part. Parameters, all in device memory and used as given: iou_thrs[n_thr] (1..16),
 * rec_thrs[n_rec] (1..128, ascending), area_rng[n_area][2] (1..4) as C `double`, max_dets[n_max_dets] (1..4, ascending).
 *   order[n]: detection index by rank -- class ascending, score descending, image ascending, arrival (COCOeval's stable
 *     mergesort over the per-image lists); cls_offsets[n_cls + 1] as in dana_eval_ap; segpos[n] by rank: the place of the
 *     detection among those of its (class, image) by score, -1 for rows that take no part;
 *   codes[n_area][n_thr][n] bytes by rank (evaluateImg): 1 = matched a non-ignored object, 0 = ignored (matched an
 *     ignored object, or unmatched with its own area outside the range), 2 = unmatched, 3 = at or past max_dets[last] in
 *     its (class, image) or taking no part. An object is ignored under a range when ignore | iscrowd | area outside; a
 *     detection takes the available object of the largest IoU >= min(t, 1 - 1e-10) (the last of equals) among the
 *     non-ignored ones, else among the ignored ones; a crowd stays available and its IoU divides by the detection's area;
 *   npig[n_cls][n_area]: non-ignored objects; precision / scores [n_thr][n_rec][n_cls][n_area][n_max_dets] and recall
 *     [n_thr][n_cls][n_area][n_max_dets] (accumulate): -1 where npig == 0.
 * Doubles and bytes are passed as void* / const void*. Fixed positions, no sums across threads: two calls give the same
 * bits. No synchronisation, no device-to-host copy. */
int dana_eval_coco(const float* det, const int* det_img, const int* det_cls, long n, const float* gt_bbox,
                   const int* gt_img, const int* gt_cls, const void* gt_area, const unsigned char* gt_flags, long g,
                   int n_img, int n_cls, const void* iou_thrs, int n_thr, const void* rec_thrs, int n_rec,
                   const void* area_rng, int n_area, const int* max_dets, int n_max_dets, int* order, int* cls_offsets,
                   int* segpos, void* codes, int* npig, void* precision, void* recall, void* scores, void* workspace,
                   size_t workspace_bytes, dana_stream_t stream);

/* ---- proposal recall: lib/datasets/imdb.py:137-225 (`evaluate_recall`, which the reference carries commented out) ---------
 * Proposals and ground truth matched one to one, greedily; the matched IoUs held against n_thr thresholds; counted per
 * proposal budget (`limits`) and object-size range (`area_rng`). Float64, unfused.
 *
 * Units (built by the host, dana_amd/evaluate.py): a problem is one proposal list -- box_count rows (x1, y1, x2, y2) of
 * `boxes` from row box_off on, best first -- made for image i under class c. Its TARGET unit (role 0) holds the ground truth
 * of image i with class c, its OTHER unit (role 1) the ground truth of image i with any other class. gt_order[g] is the
 * ground truth sorted stably by (image, class), so a unit's objects are at most two position ranges of gt_order. A pair is
 * one (unit, object); pairs are numbered unit by unit in position order from the unit's pair_off.
 *   unit_tab[n_units][9] = (box_off, box_count, gt0_begin, gt0_end, gt1_begin, gt1_end, pair_off, cls, role), device memory.
 *
 * Matching, for every unit, limit l and area range a: the candidates are the unit's first m rows (m = box_count when
 * limits[l] <= 0, else min(limits[l], box_count); at most 65 536 are considered), the objects its boxes with
 * area_rng[a][0] <= area <= area_rng[a][1] (both ends inclusive, :173-174), area = gt_area[g] when given, else
 * (x2 - x1 + 1) * (y2 - y1 + 1). Until no object is left: among the remaining (candidate, object) entries the largest IoU
 * (the `+ 1.` convention) -- among equal IoUs the lowest object position, then the lowest candidate row, as :196-204's two
 * argmax calls give -- is recorded, ov[pair] = IoU and match[pair] = candidate row, and both leave. An IoU of 0 is still
 * a match. When the candidates run out the remaining objects get ov = 0, match = -1 (the reference's assert fires there).
 * An object outside the area range gets ov = -1, match = -1 and takes no part. The kernel stays inside its buffers
 * whatever the coordinates are; results are defined for finite coordinates.
 *   ov [n_limits][n_area][n_pairs] (C `double`), match [n_limits][n_area][n_pairs].
 *
 * Counts (:220-221 before the division): npos[role][a][k] = pairs of class k with ov != -1; hits[role][t][l][a][k] = those
 * with ov >= iou_thr[t]. k is the unit's cls: for role 1 the class the proposals were made for.
 *   hits [2][n_thr][n_limits][n_area][n_cls], npos [2][n_area][n_cls], both C `long long`, zeroed by the call.
 *
 * n_thr 1..16, n_limits 1..8, n_area 1..8 (the reference names eight ranges); iou_thr, limits and area_rng[n_area][2] in
 * device memory; boxes and gt_box 16-byte aligned (read as float4). The objects of a unit are bounded by the workspace
 * only. Doubles and long longs are passed as void*. n_units == 0 or n_pairs == 0 zeroes the counts and returns. Integer
 * counts, fixed positions: two calls give the same bytes. No synchronisation, no device-to-host copy.
 * dana_eval_proposal_recall_workspace_bytes is 0 for a shape the call refuses. */
size_t dana_eval_proposal_recall_workspace_bytes(long n_boxes, long n_units, long n_pairs, int n_thr, int n_limits,
                                                 int n_area);
int dana_eval_proposal_recall(const float* boxes, const int* unit_tab, long n_units, const float* gt_box,
                              const void* gt_area /* double[g] or null */, const int* gt_order, long g, long n_pairs,
                              int n_cls, const void* iou_thr, int n_thr, const int* limits, int n_limits,
                              const void* area_rng, int n_area, void* ov, int* match, void* hits, void* npos,
                              void* workspace, size_t workspace_bytes, dana_stream_t stream);

/* ---- error diagnosis: TIDE (Bolya et al., "TIDE: A General Toolbox for Identifying Object Detection Errors", ECCV 2020) ------
 * Why the AP is not higher: every false positive and every undetected object of dana_eval_ap's marking gets one of six
 * error types, and each type gets the AP that repairing it alone would give. Restated from the paper (the reference tree
 * has nothing of the kind); the choices the paper leaves open are the ones written here. Inputs as for dana_eval_ap.
 * thresholds: two C `double` in device memory, (t_f, t_b), the foreground and background IoU thresholds with
 * 0 <= t_b < t_f (the caller's to keep: the values are not read on the host). IoU is voc_eval's: float64, `+ 1.`, unfused.
 *
 * Step 1 is dana_eval_ap at the one threshold t_f -- the call is made inside -- so order[n], cls_offsets[n_cls + 1],
 * tpfp[n] (1 = TP, 2 = FP, 0 = matched a difficult box), npos[n_cls] and ap[n_cls] are the evaluator's, bit for bit.
 *
 * Step 2, a type for every FP. Only the COUNTED objects of the detection's image are looked at: ids in range and not
 * difficult (a difficult object is never a ref). For a detection of class c, (ov_same, j_same) are the largest IoU and the
 * lowest object index among equal maxima over the counted objects of class c, (ov_other, j_other) the same over the counted
 * objects of every other class; a side without objects has IoU -inf and no index. The first rule that holds decides:
 *   Dupe: ov_same > t_f (strictly, as voc_eval has it: step 1 gave the object to a higher-ranked detection), ref = j_same
 *   Loc:  t_b <= ov_same <= t_f, ref = j_same (Loc is asked before Cls)
 *   Cls:  ov_other > t_f, ref = j_other
 *   Both: t_b <= ov_other <= t_f, ref = j_other
 *   Bkg:  otherwise, ref = -1
 *   det_type[n] bytes by rank: 0 = no part (tpfp 0, or ids out of range), 1 = TP (ref = its object), 2 = Cls, 3 = Loc,
 *     4 = Both, 5 = Dupe, 6 = Bkg; det_ref[n] by rank: the caller's ground-truth row, or -1;
 *   gt_state[g] bytes by the caller's row: 0 = not counted, 1 = detected in step 1, 2 = undetected but a Loc or Cls
 *     detection refers to it (covered), 3 = Miss;
 *   counts[n_cls][7] (C `long long`): TP, Cls, Loc, Both, Dupe, Bkg per detection class, Miss per object class;
 *   confusion[n_cls + 1][n_cls + 1] (C `long long`), [object class][detection class]: a TP at [c][c], a Cls at [class of
 *     its ref][c], Loc / Both / Dupe / Bkg at [n_cls][c], an object in state 2 or 3 at [c][n_cls].
 *
 * Step 3, ap_fixed[8][n_cls] (C `double`): the AP with one error type repaired, in the order Cls, Loc, Both, Dupe, Bkg,
 * Miss, FP, FN; each oracle alone on step 1's marking, then the evaluator's curve rule (the same metric; NaN where the
 * oracle's npos is 0). Under the area metric the terms are those of dana_eval_ap, added in double-double and rounded
 * once: a repaired AP is the correctly rounded sum of its terms and does not depend on the order they are added in
 * (`ap` keeps the evaluator's bits, so an oracle that changes nothing can differ from it in the last bit).
 *   Both, Dupe, Bkg: the detections of that type are removed. FP: every tpfp 2 is removed.
 *   Loc: a Loc detection becomes a TP when its ref is undetected (state 2) and it is the highest-ranked Loc detection with
 *     that ref; every other Loc detection is removed.
 *   Cls: a Cls detection becomes a TP of its ref's class, with its own score, when its ref is undetected and it wins the
 *     ref: the highest score among all Cls detections with that ref whatever their class, equal scores to the lower
 *     detection row; every other Cls detection is removed. The rows are ranked again by (class, score descending,
 *     arrival); npos is unchanged.
 *   Miss: npos[c] loses the class's state-3 objects. FN: npos[c] becomes the class's TP count.
 * Every finite ap_fixed[o][c] >= ap[c].
 *
 * Bytes, doubles and long longs are passed as void*. The claims on an object are 64-bit integer atomic minima, the counts
 * integer atomic adds, the float64 sums run in a fixed order: two calls give the same bits. No synchronisation, no
 * device-to-host copy. (n_cls + 1)^2 * 7 < 2^31. dana_diagnose_errors_workspace_bytes is 0 for a shape the call refuses. */
size_t dana_diagnose_errors_workspace_bytes(long n, long g, int n_img, int n_cls);
int dana_diagnose_errors(const float* det, const int* det_img, const int* det_cls, long n, const float* gt_box,
                         const int* gt_img, const int* gt_cls, const unsigned char* gt_difficult, long g, int n_img,
                         int n_cls, const void* thresholds, int use_07_metric, int* order, int* cls_offsets, void* tpfp,
                         int* npos, void* ap, void* det_type, int* det_ref, void* gt_state, void* counts,
                         void* confusion, void* ap_fixed, void* workspace, size_t workspace_bytes,
                         dana_stream_t stream);

/* ---- attention maps: README.md "Attention Visualization" (images/attention_visualization.jpg) ------------------------------
 * The reference shows where a query region looks in a support image; the weights are the tensors its forward builds and
 * drops: support_adaptive_attention_weight at the RPN level (lib/model/framework/dana.py:142-146) and at the RoI level
 * (:273-277), support_spatial_weight of the BA block (:134-135). */

/* The mean of the attention rows a box covers. attn [n_problems][rows_b][ld] (the first k columns of a row are used),
 * out [n_problems][n][k].
 * mode 0 (RPN level, dana.py:142-146: one row per query feature cell): rows_b = gh * gw; boxes [n_problems / group][n][4]
 *   = (x1, y1, x2, y2) in network-input pixels, problem p reads the boxes of image p / group (a class sweep's C problems per
 *   image). Box j averages the rows of the cells y_lo..y_hi x x_lo..x_hi, x_lo = clamp(floor(x1 / cell), 0, gw - 1),
 *   x_hi = clamp(floor(x2 / cell), x_lo, gw - 1), the same for y with gh (cell: the feature stride, 16): the rectangle is
 *   computed in the kernel, is never empty and never leaves the grid.
 * mode 1 (RoI level, dana.py:273-277: gh * gw = 49 rows per RoI): rows_b = n * gh * gw, box j averages its own rows
 *   j * gh * gw .. (j + 1) * gh * gw - 1; boxes is not read (may be null).
 * The rows are summed in row-major order into a float64 accumulator: two calls give the same bits. float4 loads when
 * ld % 4 == 0 and attn is 16-byte aligned. */
int dana_attn_box_mean(const float* attn, const float* boxes, float* out, int n_problems, int rows_b, long ld, int k, int n,
                       int gh, int gw, int group, int mode, float cell, dana_stream_t stream);

/* maps [n_maps][gh][gw] -> out [n_maps][size][size]: cv2.resize(INTER_LINEAR) (the convention of dana_prep_image: sample
 * position (d + 0.5) * g / size - 0.5, clamped at the borders), the sample position kept in double. */
int dana_heatmap_upsample(const float* maps, float* out, long n_maps, int gh, int gw, int size, dana_stream_t stream);

/* The README figure in one launch: maps [n_maps][gh][gw] upsampled as above, normalised per map by the map's own minimum
 * and maximum (a workgroup reduction inside the launch; a constant map goes to 0), looked up in table[256][3] (RGB bytes)
 * at round(255 t) and blended over images [n_maps][3][size][size] -- prepared as the model is fed: BGR planes minus
 * cfg.PIXEL_MEANS (lib/model/utils/config.py:258, blob.py:35-52) -- restored with mean_b / mean_g / mean_r and clamped to
 * 0..255: out [n_maps][size][size][3] RGB bytes (passed as void*) = round((1 - alpha) * image + alpha * colour). */
int dana_heatmap_render(const float* maps, const float* images, const unsigned char* table, void* out, long n_maps,
                        int gh, int gw, int size, float alpha, float mean_b, float mean_g, float mean_r,
                        dana_stream_t stream);

/* ---- the prediction figure: README images/prediction.jpg, fsod_logger.py:22-34,56-102, net_utils.py:50-60 -----------------
 * Images, boxes and sheets as RGB bytes on the device (csrc/render.hip states the pixel rule; dana_amd/render.py restates
 * it in numpy). Byte buffers are passed as void*.
 *
 * images [n_images][3][height][width] prepared as the model is fed (BGR planes minus the means) -> out
 * [n_images][height][width][3] RGB: clamp(image + mean, 0, 255) rounded as dana_heatmap_render does at alpha = 0; NaN -> 0. */
int dana_render_to_rgb(const float* images, void* out, long n_images, int height, int width, float mean_b, float mean_g,
                       float mean_r, dana_stream_t stream);

/* Outlines (and labels) of every box of every image into canvas [n_images][height][width][3], in place, in one launch.
 * boxes: n_rows rows of row_ld >= 5 floats (x1, y1, x2, y2, v). Two forms:
 *   counts != NULL: counts / offsets of n_images * lists_per_image lists (the layout dana_detect_postprocess_batched and
 *     dana_detect_merge write); list p belongs to image p / lists_per_image and has class slot p % lists_per_image;
 *   counts == NULL: image b owns rows b * per_image .. + min(num_boxes[b], per_image) (lists_per_image = 1); rows with
 *     v == 0 are not drawn.
 * Coordinates are multiplied by scale_dev[b] (or `scale` when scale_dev is NULL) in fp32; rows with a non-finite product,
 * a NaN v, v < min_score (use_min_score != 0) or x2 < x1 / y2 < y1 after truncation are skipped, and so is a row outside
 * the buffer. Colour: colors[n_colors][3] at color_index[row] modulo n_colors; a row at or beyond n_color_index (NULL: every
 * row) takes its class slot, which is 0 in the ground-truth form. height <= 65535 * 16. labels != 0 prints
 * "<slot> <v to hundredths>" (ground-truth form: "<v as integer>") with font[12][7] ("0123456789. ", 5 bits per row).
 * top_last = 0: the first row of an image's order is painted on top; 1: the last. Pixels nothing covers are not written. */
int dana_render_draw_boxes(void* canvas, int n_images, int height, int width, const float* boxes, int row_ld, long n_rows,
                           const int* counts, const int* offsets, int lists_per_image, const int* num_boxes,
                           int per_image, const float* scale_dev, float scale, int thickness, int use_min_score,
                           float min_score, const unsigned char* colors, int n_colors, const int* color_index,
                           long n_color_index, const unsigned char* font, int labels, int top_last,
                           dana_stream_t stream);

/* query [n_images][height][width][3] and supports [n_images][n_shots][shot_h][shot_w][3] -> out
 * [n_images][height][width + cols * (pad + side)][3], rows_per_col = max(1, (height + pad) / (side + pad)), cols =
 * ceil(n_shots / rows_per_col): the query at the left, shot s resized to side x side (cv2.resize(INTER_LINEAR), the
 * convention of dana_prep_image) at x = width + pad + (s / rows_per_col) * (side + pad), y = (s % rows_per_col) *
 * (side + pad), pad_value everywhere else. side <= height. */
int dana_render_sheet(const void* query, const void* supports, void* out, int n_images, int height, int width, int n_shots,
                      int shot_h, int shot_w, int side, int pad, int pad_value, dana_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DANA_HIP_H */
