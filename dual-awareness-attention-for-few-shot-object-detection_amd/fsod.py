"""Sibling model `fsod` of the reference's factory (utils.py:111-112): the attention-RPN + multi-relation detector of
lib/model/framework/fsod.py:19-327 on the same HIP operators.

* attention RPN (fsod.py:96-119): the query feature map is cross-correlated depth-wise with the 7x7 pooled mean of the
  positive supports (`dana_depthwise_corr_nhwc`), and the RPN runs on that (h-6) x (w-6) map;
* multi-relation head (fsod.py:181-249): global relation (mean-pooled [roi | support] -> 2 FC -> 2-way), local
  correlation (1x1 conv on both, depth-wise 7x7 correlation -> 2-way), patch relation (1x1 conv on [roi | support],
  3x3/1 average pool, 3x3 conv, 1x1 conv, average pool -> 2-way); the three scores are summed and divided by 10.
  The [roi | support] concatenations never exist: the 1x1 layers are split into their roi and support halves, the
  support half is computed once per image and added as a residual.
Same parameter tree as the reference class. Trainable: `FSOD._backward` (the three relation heads, the depth-wise
correlation adjoints of the attention RPN and of the local-correlation head, the support trunk)."""
import torch
import torch.nn as nn

from . import backward as BW
from . import ops
from .cached_inputs import ClassSweep
from .dana import DAnARCNN
from .frcnn import FasterRCNN


class FSOD(FasterRCNN):
    def __init__(self, classes, num_layers=50, pretrained=False, num_way=2, num_shot=5):
        self.n_way, self.n_shot = num_way, num_shot
        FasterRCNN.__init__(self, classes, num_layers, pretrained)

    def _init_modules(self):
        FasterRCNN._init_modules(self)
        del self.RCNN_cls_score  # fsod.py:267: the relation heads replace it
        d = 1024
        self.global_fc_1, self.global_fc_2, self.global_cls_score = nn.Linear(2 * d, d), nn.Linear(d, d), nn.Linear(d, 2)
        self.corr_conv = nn.Conv2d(d, d, 1, padding=0, bias=False)
        self.corr_cls_score = nn.Linear(d, 2)
        self.patch_conv_1 = nn.Conv2d(2 * d, d // 4, 1, padding=0, bias=False)
        self.patch_conv_2 = nn.Conv2d(d // 4, d // 4, 3, padding=0, bias=False)
        self.patch_conv_3 = nn.Conv2d(d // 4, d, 1, padding=0, bias=False)
        self.patch_cls_score = nn.Linear(d, 2)
        for m in (self.global_fc_1, self.global_fc_2, self.global_cls_score, self.corr_conv, self.corr_cls_score,
                  self.patch_conv_1, self.patch_conv_2, self.patch_conv_3, self.patch_cls_score):
            nn.init.normal_(m.weight, std=0.01)  # fsod.py:49-75
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        # keep the reference's registration order of the state_dict (fsod.py:29-75 then :262-268)
        order = ["RCNN_rpn", "global_fc_1", "global_fc_2", "global_cls_score", "corr_conv", "corr_cls_score",
                 "patch_conv_1", "patch_conv_2", "patch_conv_3", "patch_cls_score", "RCNN_base", "RCNN_top",
                 "RCNN_bbox_pred"]
        mods = self._modules
        for k in order:
            mods[k] = mods.pop(k)

    def _init_weights(self):
        DAnARCNN._init_weights(self)

    # ---- cached support sets (encode_supports): per set, the pooled positive map and the support halves of the heads ----
    def _cache_layout(self, shot, sup_map):
        """pos: AvgPool2d(14, 1) of the shots' mean map (fsod.py:103-104); g_sup / corr_sup / p_sup: the support halves of
        the global, local-correlation and patch relation heads (fsod.py:185-234)"""
        return dict(pos=(49, 1024), g_sup=(1024,), corr_sup=(49, 1024), p_sup=(49, 256))

    def _sup_global(self, support, n):
        """global relation's support half (fsod.py:185-199): mean_49(support) . W1[:, 1024:]^T -> (m_sup, g_sup [n][1024])"""
        d = 1024
        w1, _ = self._w(self.global_fc_1)
        m_sup = ops.spatial_mean(support, n, 49, d)
        return m_sup, ops.gemm_nt(m_sup, w1.view(-1)[d:], n, d, d, ldb=2 * d)

    def _sup_corr(self, support, n):
        """local correlation's support half (fsod.py:201-216): corr_conv(support) -> [n*49][1024]"""
        d = 1024
        return ops.gemm_nt(support, self.corr_conv.weight.detach().view(d, d).contiguous(), n * 49, d, d)

    def _sup_patch(self, support, n):
        """patch relation's support half (fsod.py:218-234): support . W_p1[:, 1024:]^T -> [n][49*256]"""
        d = 1024
        wp1 = self.patch_conv_1.weight.detach().view(d // 4, 2 * d).contiguous()
        return ops.gemm_nt(support, wp1.view(-1)[d:], n * 49, d // 4, d, ldb=2 * d)

    def _support_set(self, sup_ims, plan, dev):
        """one support set's cache tensors, with the launches of the uncached eval forward at B = 1"""
        shot = sup_ims.size(0)
        sup, sh_, sw_ = self._rcnn_base(sup_ims, plan)
        L = sh_ * sw_
        pos = ops.avgpool(ops.spatial_mean(sup, 1, shot, L * 1024), 1, sh_, sw_, 1024, 14, 1)
        return dict(pos=pos, g_sup=self._sup_global(pos, 1)[1], corr_sup=self._sup_corr(pos, 1),
                    p_sup=self._sup_patch(pos, 1))

    def forward(self, im_data, im_info, gt_boxes, num_boxes, support_ims, all_cls_gt_boxes=None):
        training = self.training
        shot = self.n_shot
        way = self.n_way if training else 1
        B = im_data.size(0)
        dev = im_data.device
        plan = self._get_plan()
        # cached: the support sets' tensors gathered per problem (a class sweep: B*Cs problems p = b*Cs + c)
        cached, Cs = self._cached_supports(support_ims, B, dev)
        sweep = isinstance(support_ims, ClassSweep)
        NP = B * Cs
        if cached is None:
            sup_ims = self._support_batch(support_ims, B, way, shot)
            Ns = sup_ims.size(0)
        bridge, ctx = self._saving_ctx(("q_saved", "l4_saved", "s_saved", "heads"), align_only_for="fsod")
        self._ctx = None
        if cached is None:
            sup, sh_, sw_ = self._rcnn_base(sup_ims, plan, save=ctx["s_saved"] if ctx is not None else None,
                                            save_from=ctx["t"] if ctx is not None else 3)  # [Ns*400][1024]
            if (sh_, sw_) != (20, 20):
                raise RuntimeError("support images must be 320x320 (fsod.py:44: AvgPool2d(14) of a 20x20 map -> 7x7)")
            L = sh_ * sw_

        def pooled_support(offset):  # mean over the shots [offset, offset+shot), then AvgPool2d(14, 1): [B][49][1024]
            m = torch.empty((B, L * 1024), dtype=torch.float32, device=dev)
            for b in range(B):
                m[b:b + 1] = ops.spatial_mean(sup.view(-1)[(b * way * shot + offset) * L * 1024:], 1, shot, L * 1024)
            return ops.avgpool(m, B, sh_, sw_, 1024, 14, 1)

        pos = pooled_support(0) if cached is None else cached["pos"]

        def attention_rpn_input(base, B_, fh, fw, plan_):
            if ctx is not None:
                ctx["base"] = base
            if sweep:  # problem p: image p / Cs's map against set p's kernel
                return ops.depthwise_corr_grouped(base, pos, NP, fh, fw, 1024, 7, 7, Cs)
            return ops.depthwise_corr(base, pos, B_, fh, fw, 1024, 7, 7)

        st = self._stages(im_data, im_info, gt_boxes, rpn_input=attention_rpn_input, ctx=ctx, group=Cs)
        R, n_roi, pooled, fc7 = st["R"], st["n_roi"], st["pooled"], st["fc7"]
        wb, bb = self._w(self.RCNN_bbox_pred)
        bbox_pred = ops.gemm_nt(fc7, wb, n_roi, 4, 2048, shift=bb)
        P2, d = 49, 1024
        # roi halves of the relation heads: computed once, shared by the positive and the negative support
        w1, b1 = self._w(self.global_fc_1)
        w2, b2 = self._w(self.global_fc_2)
        wg, bg = self._w(self.global_cls_score)
        wcc = self.corr_conv.weight.detach().view(d, d).contiguous()
        wcs, bcs = self._w(self.corr_cls_score)
        wp1 = self.patch_conv_1.weight.detach().view(d // 4, 2 * d).contiguous()
        wp2 = ops.pack_conv_weight(self.patch_conv_2.weight)
        wp3 = self.patch_conv_3.weight.detach().view(d, d // 4).contiguous()
        wps, bps = self._w(self.patch_cls_score)
        g_roi = ops.spatial_mean(pooled, n_roi, P2, d)                       # avgpool_fc of the roi half [n][1024]
        corr_roi = ops.gemm_nt(pooled, wcc, n_roi * P2, d, d)                # corr_conv(rois) [n*49][1024]

        def head(support, offset=0):  # support [NP][49][1024]; cached: the support halves come from the cache
            # global relation (fsod.py:185-199): fc1([mean(roi) | mean(support)]) = roi half + support half
            m_sup, g_sup = self._sup_global(support, NP) if cached is None else (None, cached["g_sup"])
            h1 = ops.gemm_nt(g_roi, w1, n_roi, d, d, ldb=2 * d, shift=b1, residual=ops.broadcast_rows(g_sup, NP, R, d),
                             ldr=d, relu=True)
            h2 = ops.gemm_nt(h1, w2, n_roi, d, d, shift=b2, relu=True)
            s_g = ops.gemm_nt(h2, wg, n_roi, 2, d, shift=bg)
            # local correlation (fsod.py:201-216)
            corr_sup = self._sup_corr(support, NP) if cached is None else cached["corr_sup"]
            oc, _, _ = ops.depthwise_corr(corr_roi, corr_sup, n_roi, 7, 7, d, 7, 7, maps_per_kernel=R)
            s_c = ops.gemm_nt(oc, wcs, n_roi, 2, d, shift=bcs)
            # patch relation (fsod.py:218-234)
            p_sup = self._sup_patch(support, NP) if cached is None else cached["p_sup"]  # [NP][49*256]
            x0 = ops.gemm_nt(pooled, wp1, n_roi * P2, d // 4, d, ldb=2 * d,
                             residual=ops.broadcast_rows(p_sup, NP, R, P2 * (d // 4)), ldr=d // 4, relu=True)
            x1 = ops.avgpool(x0, n_roi, 7, 7, d // 4, 3, 1)                                    # 7x7 -> 5x5
            x2, _, _ = ops.conv2d_nhwc(x1, n_roi, 5, 5, d // 4, wp2, d // 4, 3, 3, 1, 0, relu=True)  # -> 3x3
            x3 = ops.gemm_nt(x2, wp3, n_roi * 9, d, d // 4, relu=True)
            x4 = ops.avgpool(x3, n_roi, 3, 3, d, 3, 1)                                         # -> 1x1
            s_p = ops.gemm_nt(x4, wps, n_roi, 2, d, shift=bps)
            score = (s_g + s_c + s_p) / 10.0  # fsod.py:237 (soft_gamma)
            if ctx is not None:
                ctx["heads"].append(dict(offset=offset, support=support, m_sup=m_sup, h1=h1, h2=h2, corr_sup=corr_sup, oc=oc,
                                         x0=x0, x1=x1, x2=x2, x3=x3, x4=x4))
            return ops.softmax_rows_(score.clone(), n_roi, 2), score.contiguous()

        cls_prob, cls_score = head(pos)
        RCNN_loss_cls = RCNN_loss_bbox = 0
        rois_label = st["rois_label"]
        if training:
            neg_prob, neg_score = head(pooled_support(shot), shot)
            cls_prob = torch.cat([cls_prob, neg_prob], 0)
            rois_label = torch.cat([rois_label, torch.zeros_like(rois_label)], 0)
            rl, seeds = ops.rcnn_losses(cls_score, neg_score, st["labels_f"], bbox_pred, st["rois_target"].contiguous(),
                                        st["rois_inside_ws"].contiguous(), st["rois_outside_ws"].contiguous(),
                                        with_grad=ctx is not None)
            RCNN_loss_cls, RCNN_loss_bbox = rl[0], rl[1]
        rpn_loss_cls, rpn_loss_bbox = st["rpn_loss_cls"], st["rpn_loss_bbox"]
        if ctx is not None:
            ctx.update(loss_seeds=seeds, Ns=Ns, shot=shot, way=way, L=L, pos=pos, pooled=pooled, g_roi=g_roi,
                       corr_roi=corr_roi, wp2=wp2)
            self._ctx = ctx
            if bridge:  # loss.backward() (train.py:141-143) runs self._backward on the HIP kernels
                rpn_loss_cls, rpn_loss_bbox, RCNN_loss_cls, RCNN_loss_bbox = self._loss_bridge(
                    dev, (rpn_loss_cls, rpn_loss_bbox, RCNN_loss_cls, RCNN_loss_bbox))
        return (st["rois"], cls_prob, bbox_pred, rpn_loss_cls, rpn_loss_bbox, RCNN_loss_cls, RCNN_loss_bbox, rois_label)

    # ---- training backward ---------------------------------------------------------------------------------------------
    _head_params = (BW.lin("global_fc_1") + BW.lin("global_fc_2") + BW.lin("global_cls_score") + ["corr_conv.weight"]
                    + BW.lin("corr_cls_score") + ["patch_conv_1.weight", "patch_conv_2.weight", "patch_conv_3.weight"]
                    + BW.lin("patch_cls_score"))  # fsod.py:29-75: the three relation heads replace RCNN_cls_score

    def _relation_heads_backward(self, ctx, grads, a3):
        """Adjoint of both `head` calls of the forward (fsod.py:181-249): score = (global + local-correlation + patch) / 10
        for the positive and the negative support (a3 = g3 / 10); every [roi | support] concatenation is a split layer (roi
        half + support half). -> (d pooled [n_roi*49][1024] through the roi halves, {offset: d support [B*49][1024]}).
        Over a frozen trunk (ctx["t"] == 3) both results have no reader: their buffers are not made and every launch that
        only writes into them (the Linears' data gradients -- linear_backward(need_dx=False) --, the global relation's
        support half, the roi halves' broadcast) is not issued; the weight gradients stay -> (None, {})"""
        d_pos, d_neg, _ = ctx["loss_seeds"]
        B, R = ctx["B"], ctx["R"]
        n_roi, P2, d, dq_ = B * R, 49, 1024, 256
        pooled, g_roi, corr_roi = ctx["pooled"], ctx["g_roi"], ctx["corr_roi"]
        dev, trunk = pooled.device, ctx["t"] < 3
        w1 = self.global_fc_1.weight.detach()
        w2 = self.global_fc_2.weight.detach()
        wcc = self.corr_conv.weight.detach().view(d, d).contiguous()
        wp1 = self.patch_conv_1.weight.detach().view(dq_, 2 * d).contiguous()
        wp3 = self.patch_conv_3.weight.detach().view(d, dq_).contiguous()
        c_p2 = dict(cin=dq_, cout=dq_, k=3, stride=1, pad=0, w=ctx["wp2"], scale=None, u=None)
        d_pooled_head = torch.zeros((n_roi * P2, d), dtype=torch.float32, device=dev) if trunk else None
        d_g_roi = torch.zeros((n_roi, d), dtype=torch.float32, device=dev) if trunk else None
        d_corr_roi = torch.zeros((n_roi * P2, d), dtype=torch.float32, device=dev)
        d_w1 = torch.zeros((d, 2 * d), dtype=torch.float32, device=dev)
        d_wp1 = torch.zeros((dq_, 2 * d), dtype=torch.float32, device=dev)
        d_wcc = torch.zeros((d, d), dtype=torch.float32, device=dev)
        d_supports = {}
        for hc in ctx["heads"]:
            ds = (d_pos if hc["offset"] == 0 else d_neg)
            support = hc["support"]
            d_support = torch.zeros((B * P2, d), dtype=torch.float32, device=dev) if trunk else None
            # .. global relation: Linear(2) <- relu fc2 <- relu fc1([mean(roi) | mean(support)])
            BW.seed_linear_grads(self.global_cls_score, ds, hc["h2"], a3)
            d_h2 = BW.seed_linear_dx(self.global_cls_score, ds, a3)
            ops.relu_mask_(d_h2, hc["h2"], n_roi, d)
            dw2, db2, d_h1 = ops.linear_backward(d_h2, hc["h1"], w2, n_roi, d, d)
            BW.acc(self.global_fc_2.weight, dw2)
            BW.acc(self.global_fc_2.bias, db2)
            ops.relu_mask_(d_h1, hc["h1"], n_roi, d)
            dw1r, db1, _ = ops.linear_backward(d_h1, g_roi, w1, n_roi, d, d, ldw=2 * d, need_dx=trunk, dx_out=d_g_roi, dx_ld=d)
            ops.axpy_rows_(d_w1, dw1r, d, d, ld_y=2 * d)
            BW.acc(self.global_fc_1.bias, db1)
            d_gs = ops.spatial_mean(d_h1, B, R, d)  # the support half was broadcast over the image's R rois
            d_gs.mul_(float(R))
            dw1s = ops.gemm_small(d_gs, (1, d), hc["m_sup"], (d, 1), d, d, B)            # [d][d] = d_gs^T . mean(support)
            ops.axpy_rows_(d_w1.view(-1)[d:], dw1s, d, d, ld_y=2 * d)
            if trunk:
                d_m_sup = ops.gemm_small(d_gs, (d, 1), w1.view(-1)[d:], (2 * d, 1), B, d, d)  # [B][d] = d_gs . w1[:, d:]
                ops.broadcast_rows(d_m_sup, B, P2, d, alpha=1.0 / P2, out=d_support)
            # .. local correlation: Linear(2) <- sum over the 49 positions of corr_conv(roi) * corr_conv(support)
            BW.seed_linear_grads(self.corr_cls_score, ds, hc["oc"], a3)
            d_oc = BW.seed_linear_dx(self.corr_cls_score, ds, a3)  # [n][1024] = a 1x1 output map
            g_feat, g_kern = ops.depthwise_corr_backward(d_oc, corr_roi, hc["corr_sup"], n_roi, 7, 7, d, 7, 7,
                                                         maps_per_kernel=R)
            ops.axpy_rows_(d_corr_roi, g_feat, n_roi * P2, d)
            dwc_s, _, _ = ops.linear_backward(g_kern.view(B * P2, d), support.view(B * P2, d), wcc, B * P2, d, d,
                                              need_dx=trunk, dx_out=d_support, dx_ld=d)
            ops.axpy_rows_(d_wcc, dwc_s, d, d)
            # .. patch relation: Linear(2) <- avgpool3 <- relu 1x1 <- relu 3x3 <- avgpool 3/1 <- relu 1x1([roi | support])
            BW.seed_linear_grads(self.patch_cls_score, ds, hc["x4"], a3)
            d_x4 = BW.seed_linear_dx(self.patch_cls_score, ds, a3)
            d_x3 = ops.avgpool_backward(d_x4, n_roi, 3, 3, d, 3, 1).view(n_roi * 9, d)
            ops.relu_mask_(d_x3, hc["x3"], n_roi * 9, d)
            dwp3, _, d_x2 = ops.linear_backward(d_x3, hc["x2"], wp3, n_roi * 9, d, dq_)
            BW.acc(self.patch_conv_3.weight, dwp3.view(d, dq_, 1, 1))
            ops.relu_mask_(d_x2, hc["x2"], n_roi * 9, dq_)
            grads.add_conv("patch_conv_2", d_x2, hc["x1"].view(n_roi * 25, dq_), n_roi, 5, 5, c_p2)
            d_x1 = BW.conv_dgrad(d_x2, n_roi, 5, 5, c_p2)
            d_x0 = ops.avgpool_backward(d_x1, n_roi, 7, 7, dq_, 3, 1).view(n_roi * P2, dq_)
            ops.relu_mask_(d_x0, hc["x0"], n_roi * P2, dq_)
            dwp1r, _, _ = ops.linear_backward(d_x0, pooled.view(n_roi * P2, d), wp1, n_roi * P2, dq_, d, ldw=2 * d,
                                              need_dx=trunk, dx_out=d_pooled_head, dx_ld=d)
            ops.axpy_rows_(d_wp1, dwp1r, dq_, d, ld_y=2 * d)
            d_p_sup = ops.spatial_mean(d_x0, B, R, P2 * dq_)  # the support half was broadcast over the image's rois
            d_p_sup.mul_(float(R))
            dwp1s, _, _ = ops.linear_backward(d_p_sup.view(B * P2, dq_), support.view(B * P2, d), wp1.view(-1)[d:],
                                              B * P2, dq_, d, ldw=2 * d, need_dx=trunk, dx_out=d_support, dx_ld=d)
            ops.axpy_rows_(d_wp1.view(-1)[d:], dwp1s, dq_, d, ld_y=2 * d)
            d_supports[hc["offset"]] = d_support
        # the roi halves shared by both heads: mean over the 49 positions, corr_conv(rois)
        if trunk:
            ops.broadcast_rows(d_g_roi, n_roi, P2, d, alpha=1.0 / P2, out=d_pooled_head)
        dwc_r, _, _ = ops.linear_backward(d_corr_roi, pooled.view(n_roi * P2, d), wcc, n_roi * P2, d, d,
                                          need_dx=trunk, dx_out=d_pooled_head, dx_ld=d)
        ops.axpy_rows_(d_wcc, dwc_r, d, d)
        BW.acc(self.global_fc_1.weight, d_w1)
        BW.acc(self.patch_conv_1.weight, d_wp1.view(dq_, 2 * d, 1, 1))
        BW.acc(self.corr_conv.weight, d_wcc.view(d, d, 1, 1))
        return (d_pooled_head, d_supports) if trunk else (None, {})

    def _backward(self, ctx, g, grads):
        """frcnn's adjoint with the multi-relation head in place of RCNN_cls_score and the attention RPN's correlation in
        front of the RPN; the supports are differentiated through the trunk (where it trains: ctx["t"] < 3)"""
        g1, g2, g3, g4, g_dev = g
        B, n_roi, fh, fw, d_bbox = ctx["B"], ctx["B"] * ctx["R"], ctx["fh"], ctx["fw"], ctx["loss_seeds"][2]
        trunk = ctx["t"] < 3
        d_fc7 = BW.seed_linear_dx(self.RCNN_bbox_pred, d_bbox, g4)
        gs = None
        if trunk:
            gs = torch.zeros((ctx["Ns"] * ctx["L"], 1024), dtype=torch.float32, device=d_fc7.device)  # d(support trunk output)
        d_pooled_head, d_supports = self._relation_heads_backward(ctx, grads, g3 / 10.0)  # fsod.py:237: (sum of 3) / 10
        BW.seed_linear_grads(self.RCNN_bbox_pred, d_bbox, ctx["fc7"], g4)
        d_pooled = BW.layer4_backward(d_fc7, n_roi, ctx["l4_saved"], grads, need_dx=trunk)
        grads.finish_all(self, "RCNN_top")
        grads.finish_all(self, "patch_conv_2")
        if trunk:
            ops.axpy_rows_(d_pooled, d_pooled_head, n_roi * 49, 1024)  # the pooled features also feed the heads' roi halves
        BW.ready(self, self._grad_stages(ctx["plan"], ctx["t"])[0][1])
        d_bf = BW.roi_features_backward(ctx, d_pooled) if trunk else None
        d_rfeat = BW.sibling_rpn_backward(self, ctx, g1, g2, g_dev, grads)
        if not trunk:  # frozen trunk: base_feat, the correlation kernel and the support maps have no trainable producer
            grads.finish_all(self, "RCNN_rpn")
            BW.ready(self, BW.RPN_PARAMS)
            BW.trunk_backward(self, ctx, grads, None)
            return
        # attention RPN (fsod.py:109-116): the RPN ran on the depth-wise correlation of base_feat with the pooled positive
        # support -> d base = full correlation of d rfeat with that kernel + RoIAlign path; d kernel -> positive supports
        gq, d_pos_kernel = ops.depthwise_corr_backward(d_rfeat, ctx["base"], ctx["pos"], B, fh, fw, 1024, 7, 7)
        ops.axpy_rows_(gq, d_bf, B * fh * fw, 1024)
        ops.axpy_rows_(d_supports[0], d_pos_kernel.view(B * 49, 1024), B * 49, 1024)
        for off_, d_sup_ in d_supports.items():  # AvgPool2d(14, 1) of the shots' mean map (fsod.py:98-101)
            BW.shot_mean_backward(gs, ops.avgpool_backward(d_sup_, B, 20, 20, 1024, 14, 1), ctx, off_)
        grads.finish_all(self, "RCNN_rpn")
        BW.ready(self, BW.RPN_PARAMS)
        BW.trunk_backward(self, ctx, grads, gq, gs)
