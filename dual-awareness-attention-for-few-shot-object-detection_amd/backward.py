"""Backward pass of the DAnA forward path on the HIP kernels (groundwork for the training step, SURVEY.md 8d
variant S). What `loss.backward()` does through autograd + cuDNN/cuBLAS in the reference (train.py:141-143) is
assembled here from the C-ABI building blocks: data gradients on the forward implicit-GEMM kernel with
transformed weights, weight gradients on the split-M TN MFMA kernel, and the element-wise adjoints of
backward.hip. Frozen BatchNorm (dana.py:362-385) only scales gradients; BN parameters and conv1/bn1 get none, and
neither do the trunk stages that cfg.RESNET.FIXED_BLOCKS froze when the model was built (dana.py:350-360): the saving
forward derives t, the first trainable trunk stage, from the parameters' requires_grad (`first_trainable_stage`) and
stores it in its context; every piece below reads it there and neither saves, differentiates nor derives weights for
the stages in front of it (t = 3, the frozen-trunk fine-tuning stage: nothing below layer4, the RPN and the heads).

`model_backward` is the whole-model adjoint: it consumes the context a `save_for_backward` forward left in
`model._ctx` and accumulates `.grad` on every trainable parameter, checked against autograd of the oracle
(tests/test_gpu_backward.py)."""
import math

import torch

from . import ops
from .config import cfg


class WeightGrads:
    """Accumulates packed weight gradients per conv (query and support passes share the weights).
    With `stream`, the weight-gradient launches go to that side stream: they only consume (g, x) and nothing on the
    data-gradient chain waits for them, so their tiles fill the CUs the chain's launches leave idle in their tails."""

    def __init__(self, stream=None, model=None):
        self.packed = {}
        self.convs = {}
        self.stream = stream
        self.model = model
        self.direct = {}  # key -> packed VIEW of param.grad (trainer layout): weight gradients land there directly
        # ONE weight-gradient stream for every caller stream (the box branch issues its weight gradients from the layer4
        # stream, the RPN chain from its own, the rest of the backward from the caller's). Round 4 gave every caller stream
        # a side stream of its own; measured in round 5 (profiles/r5_role_streams.md): more streams than hardware queues
        # make unrelated chains share a queue, and a second weight-gradient stream costs the iteration 1.3-1.7 ms.
        self.side = {}    # caller stream handle -> [side stream, operands kept alive while its launches are in flight]
        self.compact = {}  # gathered input rows of strided 1x1 convs (shared by a block's conv1 and downsample conv)

    def _side_for_current(self):
        cur = ops.cur_stream()
        ent = self.side.get(cur.cuda_stream)
        if ent is None:
            ent = self.side[cur.cuda_stream] = [self.stream, []]
        return ent

    def _direct_view(self, key):
        """the parameter's gradient as a packed [cout][kh*kw*cin] view, if the trainer stores it that way"""
        if key in self.direct:
            return self.direct[key]
        v = None
        if self.model is not None:
            g = self.model.get_parameter(key + ".weight").grad
            if g is not None:
                v = ops.packed_view(g)
                if v is not None and v.data_ptr() != g.data_ptr():
                    v = None
        self.direct[key] = v
        return v

    def add_conv(self, key, g, x, n, h, w, c, in_stride=0, grad_stride=0, v=None):
        """v: the forward launch's kept Winograd workspace (V planes of x), if that conv ran in the F(4x4,3x3) domain"""
        self.convs[key] = c
        self.side_run(lambda: self._launch(key, g, x, n, h, w, c, in_stride, grad_stride, v), g, x, v)

    def side_run(self, fn, *keep):
        """fn() on the weight-gradient stream of the caller's stream, behind everything queued so far; `keep` stays
        alive until join(). For work that consumes the chain's gradients and feeds nothing back into it (a Linear's
        dW / db and their accumulation): off the data-gradient chain, joined with the conv weight gradients."""
        if self.stream is None:
            fn()
            return
        st, kept = self._side_for_current()
        st.wait_event(ops.record_event())
        kept.append(keep)
        with ops.on_stream(st):
            fn()

    def linear(self, g, x, m, n, k, then, ldx=0, ldg=0):
        """dW / db of a Linear (ops.linear_wgrad) on the side stream; then(dw, db) accumulates them there"""
        # eager issue: on the caller's chain (with the RPN chain, the box branch and the heads running from the backward's
        # start the side stream costs 0.3 ms, round 4); under stream capture the side stream (the box branch shares the
        # caller's stream there)
        if not torch.cuda.is_current_stream_capturing():
            then(*ops.linear_wgrad(g, x, m, n, k, ldx=ldx, ldg=ldg))
            return
        self.side_run(lambda: then(*ops.linear_wgrad(g, x, m, n, k, ldx=ldx, ldg=ldg)), g, x)

    def _launch(self, key, g, x, n, h, w, c, in_stride, grad_stride, v=None):
        view = self._direct_view(key)
        if c["k"] == 1 and c["stride"] > 1 and c["pad"] == 0:
            # a strided 1x1 conv (first block of layer2-4: conv1 and the downsample conv read the same pixels): gather those
            # pixels once into plain rows -- both weight gradients then run on the software-pipelined plain-row kernel
            ck = (x.data_ptr(), n, h, w, c["cin"], c["stride"], in_stride, ops.cur_stream().cuda_stream)
            ent = self.compact.get(ck)
            if ent is None:
                ent = self.compact[ck] = (ops.downsample_gather(x, n, h, w, c["cin"], c["stride"], in_stride), x)
            (x, h, w), in_stride = ent[0], 0
            c = dict(c, stride=1)
        # into the trainer's view (scaled by the frozen BN and accumulated straight into param.grad: nothing to finish),
        # else into the key's packed buffer, allocated by its first launch
        out = view if view is not None else self.packed.get(key)
        row_scale = c.get("scale") if view is not None else None
        u = c.get("u")
        if u is not None and u.size(0) == 36 and c["cin"] % 64 == 0:
            # the conv ran in the F(4x4,3x3) domain forward: so does its weight gradient (4x fewer multiplies)
            res = ops.conv3x3_wgrad_winograd(g, x, n, h, w, c["cin"], c["cout"], in_stride=in_stride,
                                             grad_stride=grad_stride, out=out, row_scale=row_scale, v=v)
        else:
            res = ops.conv2d_wgrad(g, x, n, h, w, c["cin"], c["cout"], c["k"], c["k"], c["stride"], c["pad"],
                                   in_stride=in_stride, grad_stride=grad_stride, out=out, row_scale=row_scale)
        if out is None:
            self.packed[key] = res

    def join(self):
        """the caller's stream waits for every weight-gradient launch issued so far"""
        if self.stream is not None:
            cur = ops.cur_stream()
            for t in _FRESH.grads:
                t.record_stream(cur)
            # the packed gradients were allocated in the weight-gradient stream's pool and are finished on the CALLER's
            # stream (finish_conv): without this a buffer popped there goes back to that pool while the caller's kernel still
            # reads it -- harmless as long as every caller had a weight-gradient stream to itself, a wrong RPN_Conv gradient
            # with the one shared stream of round 5 (the trunk's next weight gradient took the block)
            for t in self.packed.values():
                t.record_stream(cur)
            for st, keep in self.side.values():
                if keep:
                    done = torch.cuda.Event()
                    done.record(st)
                    cur.wait_event(done)
                    del keep[:]
        del _FRESH.grads[:]
        self.compact.clear()

    def finish_conv(self, key, c, param):
        """apply the frozen-BN scale to the rows and add into param.grad (OIHW)"""
        buf = self.packed.pop(key)
        if c.get("scale") is not None:
            ops.rowscale_(buf, c["scale"], c["cout"], c["k"] * c["k"] * c["cin"])
        fresh = param.grad is None
        if fresh:
            param.grad = torch.empty_like(param)
        ops.unpack_conv_weight_grad(buf, param.grad, c["cout"], c["cin"], c["k"], c["k"], accumulate=not fresh)

    def finish_all(self, model, prefix=""):
        self.join()
        for key in list(self.packed):
            if key.startswith(prefix):
                self.finish_conv(key, self.convs[key], model.get_parameter(key + ".weight"))


def _dgrad_weights(c):
    """flipped / transposed / BN-scaled weights of the data-gradient conv (+ their Winograd transform when the
    forward conv took the Winograd path), cached in the plan entry: computed once per weight update"""
    if c.get("wd") is None:
        c["wd"] = ops.conv2d_dgrad_weight(c["w"], c["cout"], c["cin"], c["k"], c["k"], c.get("scale"))
        c["ud"] = None
        if c.get("u") is not None and c["cout"] % 64 == 0:
            c["ud"] = ops.winograd_filter_transform(c["wd"], c["cin"], c["cout"], 2 if c["u"].size(0) == 16 else 4)
    return c["wd"], c["ud"]


def conv_dgrad(g, n, h, w, c, residual=None, mask=None, compact_out=False, out=None):
    """dL/d(conv input) [n*h*w][cin] from g = dL/d(conv+BN output); + residual, then the ReLU adjoint of `mask`"""
    wd, ud = _dgrad_weights(c)
    return ops.conv2d_dgrad(g, c["w"], n, h, w, c["cin"], c["cout"], c["k"], c["k"], c["stride"], c["pad"], wd=wd, ud=ud,
                            residual=residual, mask=mask, compact_out=compact_out, out=out)


def bottleneck_backward(g, saved, n, h, w, bp, grads, key, need_dx=True, mask_dx=True, g_masked=False):
    """Adjoint of DAnARCNN._bottleneck. saved = dict(x, o1, o2, o3, h1, w1) from the forward; g = dL/d(o3), with the
    final ReLU's adjoint (resnet.py:100) already applied when g_masked. Returns dL/dx [n*h*w][cin] (None if not
    needed); with mask_dx the ReLU adjoint of the layer that produced x is already applied to it (x is then the
    previous bottleneck's output, so the caller passes g_masked=True there). Every ReLU adjoint and the residual
    sum ride in the epilogue of a data-gradient conv."""
    h1, w1 = saved["h1"], saved["w1"]
    m_out = n * h1 * w1
    cout = bp["c3"]["cout"]
    if not g_masked:
        ops.relu_mask_(g, saved["o3"], m_out, cout, ld_act=saved.get("o3_ld", 0))
    x = saved["x"]
    grads.add_conv(key + ".conv3", g, saved["o2"], n, h1, w1, bp["c3"])
    g2 = conv_dgrad(g, n, h1, w1, bp["c3"], mask=saved["o2"])
    grads.add_conv(key + ".conv2", g2, saved["o1"], n, h1, w1, bp["c2"], v=saved.get("v2"))
    g1 = conv_dgrad(g2, n, h1, w1, bp["c2"], mask=saved["o1"])
    grads.add_conv(key + ".conv1", g1, x, n, h, w, bp["c1"])
    if bp["ds"] is not None:
        grads.add_conv(key + ".downsample.0", g, x, n, h, w, bp["ds"])
    if not need_dx:
        return None
    mk = x if mask_dx else None
    if bp["ds"] is None:  # identity shortcut (resnet.py:96-99): dx = dgrad(conv1) + g
        return conv_dgrad(g1, n, h, w, bp["c1"], residual=g, mask=mk)
    if bp["c1"]["stride"] == 1:
        dxr = conv_dgrad(g, n, h, w, bp["ds"])
        return conv_dgrad(g1, n, h, w, bp["c1"], residual=dxr, mask=mk)
    # both 1x1 convs are strided (resnet.py:71, downsample): sum the compact gradients, scatter once
    cr = conv_dgrad(g, n, h, w, bp["ds"], compact_out=True)
    return conv_dgrad(g1, n, h, w, bp["c1"], residual=cr, mask=mk)


def bottleneck_backward_merged(g, sq, ss, sm, bp, grads, key):
    """bottleneck_backward for an identity-shortcut block (no downsample, stride 1) over the [query | support] buffers of
    DAnARCNN._trunk_gen's two-segment walk: g = dL/d(o3) of BOTH batches in one [Mq + Ms][cout] tensor, ReLU adjoint applied. The three
    1x1 convs are row-wise contractions -- their weight gradients and data gradients run ONCE over all rows (half the
    launches, twice the reduction length per weight-gradient slice); the 3x3 conv in the middle keeps one call per batch
    (its Winograd tiles follow the image geometry), writing into the two row ranges of one buffer. -> dL/dx, merged, with
    the ReLU adjoint of the layer that produced x applied."""
    mq, mt = sm["mq_out"], sm["m_out"]
    c1, c2, c3 = bp["c1"], bp["c2"], bp["c3"]
    grads.add_conv(key + ".conv3", g, sm["o2"], 1, mt, 1, c3)
    g2 = conv_dgrad(g, 1, mt, 1, c3, mask=sm["o2"])
    g1 = torch.empty((mt, c2["cin"]), dtype=torch.float32, device=g.device)
    ud = _dgrad_weights(c2)[1]
    dual = ud is not None and ud.size(0) == 36
    for part, s_ in ((slice(0, mq), sq), (slice(mq, mt), ss)):
        grads.add_conv(key + ".conv2", g2[part], sm["o1"][part], s_["n"], s_["h1"], s_["w1"], c2, v=s_.get("v2"))
        if not dual:
            conv_dgrad(g2[part], s_["n"], s_["h1"], s_["w1"], c2, mask=sm["o1"][part], out=g1[part])
    if dual:
        # both batches' 3x3 data gradients as ONE batched plane GEMM (two input / output transforms around it): the
        # 600-tile launches of one batch leave a third of the chip's slots empty
        ops.conv3x3_winograd_dual_dgrad(g2, sq["n"], sq["h1"], sq["w1"], ss["n"], ss["h1"], ss["w1"], c2["cout"], ud,
                                        c2["cin"], mask=sm["o1"], out=g1)
    grads.add_conv(key + ".conv1", g1, sm["x"], 1, mt, 1, c1)
    return conv_dgrad(g1, 1, mt, 1, c1, residual=g, mask=sm["x"])


def _block_convs(prefix, bp):
    names = [prefix + ".conv3.weight", prefix + ".conv2.weight", prefix + ".conv1.weight"]
    if bp["ds"] is not None:
        names.append(prefix + ".downsample.0.weight")
    return names


def lin(name):
    return [name + ".weight", name + ".bias"]


RPN_PARAMS = lin("RCNN_rpn.RPN_cls_score") + lin("RCNN_rpn.RPN_bbox_pred") + lin("RCNN_rpn.RPN_Conv")


def _stage_convs(model, li):
    """[(name, parameter)] of the conv weights of trunk stage li (0: layer1 .. 2: layer3), in module order"""
    prefix = "RCNN_base.%d." % (4 + li)
    return [(prefix + n, p) for n, p in model.RCNN_base[4 + li].named_parameters()
            if ".conv" in n or n.endswith("downsample.0.weight")]


def first_trainable_stage(model):
    """t, the first trunk stage the backward differentiates: 0 (layer1) .. 2 (layer3), 3: the whole trunk is frozen. The
    parameters' requires_grad decide -- what `_init_modules` set from cfg.RESNET.FIXED_BLOCKS (dana.py:354-360). The
    trainable stages must form a suffix layer_t .. layer3 (a gradient cannot skip a stage's weights on its way down and
    nothing is saved in front of t) and a stage's conv weights must agree with each other: ValueError naming the first
    parameter that breaks either rule. Stem and BatchNorms are frozen always and not looked at."""
    flags, first = [], []
    for li in range(3):
        convs = _stage_convs(model, li)
        for n, p in convs:
            if p.requires_grad != convs[0][1].requires_grad:
                raise ValueError("%s has requires_grad=%s while %s has %s: the conv weights of one trunk stage train or "
                                 "freeze together" % (n, p.requires_grad, convs[0][0], convs[0][1].requires_grad))
        flags.append(convs[0][1].requires_grad)
        first.append(convs[0][0])
    for li in (1, 2):
        if flags[li - 1] and not flags[li]:
            raise ValueError("%s is frozen behind the trainable %s: the trainable trunk stages must be a suffix "
                             "(layer_t .. layer3), as cfg.RESNET.FIXED_BLOCKS sets them" % (first[li], first[li - 1]))
    return 3 - sum(flags)


def top_params(plan):
    """RCNN_top's (layer4's) conv weights, in the order layer4_backward finishes them"""
    return [n for bi in (2, 1, 0) for n in _block_convs("RCNN_top.0.%d" % bi, plan["layer4"][bi])]


def base_stages(plan, t):
    """one stage per trainable trunk block, last block first: RCNN_base.6 (layer3) down to RCNN_base.(4 + t); the stages
    in front of t (first_trainable_stage; 1: layer1 is frozen, the reference's default) have none. t has no default:
    a list that silently disagrees with the parameters' flags is what this argument exists to prevent"""
    st = []
    for li in range(2, t - 1, -1):
        layer = plan["layers"][li]
        for bi in reversed(range(len(layer))):
            key = "RCNN_base.%d.%d" % (4 + li, bi)
            st.append((key, _block_convs(key, layer[bi])))
    return st


def grad_stages(model, plan=None, t=None):
    """[(stage, [parameter names])] in the order model_backward FINISHES the gradients (the model's class knows it:
    `_grad_stages`): the trainer lays its flat gradient buffer out in this order so that all-reduce buckets can leave
    while the rest of the backward runs.
    plan: the forward's plan (the backward passes the one its context saved: asking the model for a plan INSIDE the
    backward -- autograd runs it with gradients disabled, i.e. not `_live()` -- re-derived and pre-split every trainable
    weight once per iteration for nothing: ~100 small launches at the head of the backward).
    t: the first trainable trunk stage (the backward passes its context's); None: from the parameters' requires_grad."""
    return model._grad_stages(plan if plan is not None else model._get_plan(), t)


def dana_grad_stages(model, plan, t=None):
    """t None: read off the model's parameters (first_trainable_stage)"""
    t = first_trainable_stage(model) if t is None else t
    st = [("box branch", lin("RCNN_bbox_pred") + top_params(plan))]
    st.append(("roi heads", lin("output_score_layer.linear2") + lin("output_score_layer.linear1")
               + lin("rcnn_adapt_q_layer") + lin("rcnn_transform_layer") + lin("rcnn_adapt_k_layer")
               + lin("rcnn_unary_layer")))
    rpn_att = lin("rpn_adapt_q_layer") + lin("rpn_adapt_k_layer") + lin("rpn_unary_layer")
    if model.semantic_enhance:
        rpn_att += lin("rpn_channel_k_layer")
    st.append(("rpn", RPN_PARAMS + rpn_att))
    return st + base_stages(plan, t)


def sibling_grad_stages(plan, head_params, t):
    """the sibling detectors (frcnn.py, fsod.py, fgn.py): one RoI stage (RCNN_bbox_pred, the class's `_head_params`,
    layer4), the RPN, the trunk"""
    return ([("roi head", lin("RCNN_bbox_pred") + head_params + top_params(plan)), ("rpn", RPN_PARAMS)]
            + base_stages(plan, t))


def ready(model, names):
    cb = getattr(model, "_grad_ready_cb", None)
    if cb is not None:
        cb(names)


class _Fresh(__import__("threading").local):
    """gradients acc() allocated since the last WeightGrads.join() (possibly in a side stream's pool); per THREAD: under
    nn.DataParallel every replica's backward runs in its own thread (train.py:104-105)"""

    def __init__(self):
        self.grads = []


_FRESH = _Fresh()


def acc(param, g):
    g = g.view_as(param)
    if param.grad is None:
        # (the reference's optimizer.zero_grad() sets grads to None, so the bridge path comes here every iteration.)
        # When this runs on the weight-gradient side stream, the clone's block belongs to THAT stream's pool, while the
        # optimizer / clipping / all-reduce read it on the caller's stream: join() marks it as used there
        param.grad = g.clone()
        _FRESH.grads.append(param.grad)
    else:
        param.grad.add_(g)


def _attention_backward(d_dense, ld_dd, a, unary, q, k_, s_mat, Bn, rows_b, nseg, L, Kp, dq, ugamma, k_batch, s_batch,
                        u_batch, d_k_out, d_s_out, d_u_out, vw=1024):
    """Adjoint of one dual-awareness attention  dense = ((softmax_seg(q k^T / sqrt(dq)) + ugamma u) / nseg) s
    (dana.py:118-154 / 258-283) for Bn images of rows_b query rows each.
      d_dense [Bn*rows_b][vw] (row stride ld_dd; vw = width of the value rows s_mat: 1024, or 64 where the values are the
      re-associated table S . Wt_a^T of the RoI heads); a = the saved attention [Bn][rows_b][Kp]; q [Bn*rows_b][dq];
      k_ / s_mat / unary: key, value and unary rows of image b start at b * k_batch / s_batch / u_batch (floats).
    Accumulates into d_k_out (rows of image b at b*k_batch), d_s_out (b*s_batch; None: nobody reads the values' gradient,
    its launch is not issued), d_u_out (b*u_batch); returns d_q."""
    dev = a.device
    K = nseg * L
    dA = torch.zeros((Bn, rows_b, Kp), dtype=torch.float32, device=dev)
    ops.gemm_nt(d_dense, s_mat, rows_b, K, vw, lda=ld_dd, out=dA, ldc=Kp, batch=Bn, batch_a=rows_b * ld_dd,
                batch_b=s_batch, batch_c=rows_b * Kp)
    # d s[b] += a[b]^T . d_dense[b], every image in one launch (a's zero-padded columns K..Kp-1 are computed, not stored)
    if d_s_out is not None:
        ops.gemm_tn_batched(a, d_dense, Bn, rows_b, Kp, vw, d_s_out, ldy=Kp, ldx=ld_dd, batch_y=rows_b * Kp,
                            batch_x=rows_b * ld_dd, batch_out=s_batch, n_valid=K)
    ops.colsum_batched(dA, Bn, rows_b, K, d_u_out, ld=Kp, x_batch=rows_b * Kp, out_batch=u_batch, alpha=ugamma / nseg)
    ops.attn_softmax_unary_backward_(dA, a, unary, Bn * rows_b, rows_b, nseg, L, Kp, Kp, ugamma, 1.0 / nseg,
                                     1.0 / math.sqrt(dq), unary_batch_stride=u_batch)
    kt = ops.transpose_batched(k_, Bn, K, dq, ldi=dq, ldo=Kp, in_batch=k_batch)  # [Bn][dq][Kp], zero padded
    d_q = ops.gemm_nt(dA, kt, rows_b, dq, Kp, lda=Kp, ldb=Kp, batch=Bn, batch_a=rows_b * Kp, batch_b=dq * Kp)
    # d k[b] += dS0[b]^T . q[b]
    ops.gemm_tn_batched(dA, q, Bn, rows_b, Kp, dq, d_k_out, ldy=Kp, ldx=dq, batch_y=rows_b * Kp, batch_x=rows_b * dq,
                        batch_out=k_batch, n_valid=K)
    return d_q.view(Bn * rows_b, dq)


def _rpn_conv_plan(model, ctx):
    """the RPN 3x3 conv as a plan entry, one per saved forward (its data-gradient weights are derived into it once)"""
    c = ctx.get("_c_rpn")
    if c is None:
        plan = ctx["plan"]
        c = ctx["_c_rpn"] = dict(cin=model.RCNN_rpn.din, cout=512, k=3, stride=1, pad=1, w=plan["rpn_conv_w"], scale=None,
                                 u=plan["rpn_conv_u"])
    return c


def _derive_dgrad_weights(blocks, no_dx=None):
    """the data-gradient weights of the given block plans' convs, in the order the backward needs them (each is derived
    once per weight update: _dgrad_weights). no_dx: a block plan whose input gradient nobody reads (layer4's first block
    over a frozen trunk): its conv1 / downsample conv need none"""
    for bp in blocks:
        for name in ("c3", "c2") if bp is no_dx else ("c3", "c2", "c1", "ds"):
            if bp.get(name) is not None:
                _dgrad_weights(bp[name])


def prefetch_dgrad_weights(model, ctx, dev):
    """The backward's weight-only launches (flipped / transposed / BN-scaled data-gradient weights and their Winograd
    transforms: ~70 per iteration, 0.3-0.4 ms of kernels) issued from the SAVING FORWARD behind the RPN head, on the role
    stream `model.prefetch_dgrad` names (layer4: idle until RoIAlign): they run under the proposal layer and the host round
    trip instead of in front of the backward's first contractions (a kernel trace of the replayed iteration showed 0.65 ms
    without a contraction there). The weights do not change between a forward and its backward. Records
    ctx['dgw_prefetched']. Measured -0.2 ms per iteration on `layer4`, +0.5 ms on `wgrad` / `targets` (dana.py)."""
    role = getattr(model, "prefetch_dgrad", None)
    if getattr(model, "_single_stream", False) or not role or torch.cuda.is_current_stream_capturing():
        return
    plan = ctx["plan"]
    prep = model._stream(role, dev)
    ev0 = ops.record_event()
    prep.wait_event(ev0)  # (behind the optimizer's update of the weights on the caller's stream)
    with ops.on_stream(prep):
        _dgrad_weights(_rpn_conv_plan(model, ctx))
        t = ctx["t"]
        _derive_dgrad_weights(reversed(plan["layer4"]), no_dx=plan["layer4"][0] if t == 3 else None)
        for layer in reversed(plan["layers"][t:]):  # (the stages in front of t are frozen: no data gradient reaches them)
            _derive_dgrad_weights(reversed(layer))
        ctx["dgw_prefetched"] = ops.record_event()


def _rpn_chain(model, ctx, g1, g2, g_dev, grads_r, rpnw_ready=None):
    """Adjoint of the RPN branch: RPN losses -> heads -> 3x3 conv -> RPN-level attention (rpn.py:58-115, dana.py:118-154),
    on the CURRENT stream. It reads the forward's saved tensors only; -> (d_corr [B*hw][2048]: the gradient into
    [base_feat | attended], d_s_pe [B][shot*L][1024]: into the positive supports' PE-added maps). Weight gradients of the
    branch are accumulated into .grad (through grads_r) before it returns.
    Over a frozen trunk (ctx["t"] == 3) nothing reads the two results: the launches that only complete them (the Q
    projection's data gradient; without the BA block every launch into d_s_pe) are not issued, d_s_pe lives up to the BA
    block's adjoint (rpn_channel_k_layer's gradient needs it there) and the chain returns (None, None)."""
    plan = ctx["plan"]
    B, shot = ctx["B"], ctx["shot"]
    fh, fw = ctx["fh"], ctx["fw"]
    hw = fh * fw
    L = ctx["s_pe"].size(1) // shot
    d = model.rpn_reduce_dim
    corr = ctx["corr"]
    dev = corr.device
    ug = model.unary_gamma
    trunk = ctx["t"] < 3
    c_rpn = _rpn_conv_plan(model, ctx)
    # -- RPN: losses -> heads -> 3x3 conv (rpn.py:58-115) --
    rpn = model.RCNN_rpn
    nh = ctx["nh"]
    d_heads = ops.rpn_loss_backward(ctx["rpn_heads"], nh, ctx["at"], ctx["rpn_l"], g1, g2, sigma=3.0,
                                    inside_weight=cfg.TRAIN.RPN_BBOX_INSIDE_WEIGHTS[0], grad_dev=g_dev)
    ns = rpn.nc_score_out
    grads_r.linear(d_heads, ctx["rpn_x"], B * hw, nh, 512,
                 lambda dw, db: (acc(rpn.RPN_cls_score.weight, dw[:ns]), acc(rpn.RPN_cls_score.bias, db[:ns]),
                                 acc(rpn.RPN_bbox_pred.weight, dw[ns:]), acc(rpn.RPN_bbox_pred.bias, db[ns:])))
    _, _, d_x = ops.linear_backward(d_heads, ctx["rpn_x"], plan["rpn_head_w"], B * hw, nh, 512, need_dw=False)
    ops.relu_mask_(d_x, ctx["rpn_x"], B * hw, 512)
    if rpnw_ready is not None:
        ops.cur_stream().wait_event(rpnw_ready)
    grads_r.add_conv("RCNN_rpn.RPN_Conv", d_x, corr, B, fh, fw, c_rpn, v=ctx.get("rpn_v"))
    acc(rpn.RPN_Conv.bias, ops.colsum(d_x, B * hw, 512))
    d_corr = conv_dgrad(d_x, B, fh, fw, c_rpn)  # [B*hw][2048]

    # -- RPN-level attention (dana.py:118-154): corr = [base_feat | dense] --
    K1 = shot * L
    s_pe, kp, qp, unary = ctx["s_pe"], ctx["kp"], ctx["qp"], ctx["unary"]
    d_s_pe = torch.zeros((B, K1, 1024), dtype=torch.float32, device=dev) if trunk or model.semantic_enhance else None
    d_kp = torch.zeros((B * K1, d), dtype=torch.float32, device=dev)
    d_un = torch.zeros((B * shot, L), dtype=torch.float32, device=dev)
    d_qp = _attention_backward(d_corr.view(-1)[1024:], 2048, ctx["scores"], unary, qp, kp, s_pe, B, hw, shot, L, K1, d,
                               ug, K1 * d, K1 * 1024, K1, d_kp, d_s_pe, d_un)
    ops.colmean_sub_(d_qp, B, hw, d)
    ops.colmean_sub_(d_kp, B * shot, L, d)
    wq = model.rpn_adapt_q_layer.weight.detach()
    grads_r.linear(d_qp, corr, B * hw, d, 1024,
                 lambda dw, db: (acc(model.rpn_adapt_q_layer.weight, dw), acc(model.rpn_adapt_q_layer.bias, db)), ldx=2048)
    if trunk:
        ops.linear_backward(d_qp, corr, wq, B * hw, d, 1024, ldx=2048, dx_out=d_corr, dx_ld=2048, need_dw=False)
    wk = model.rpn_adapt_k_layer.weight.detach()
    grads_r.linear(d_kp, s_pe, B * K1, d, 1024,
                 lambda dw, db: (acc(model.rpn_adapt_k_layer.weight, dw), acc(model.rpn_adapt_k_layer.bias, db)))
    if d_s_pe is not None:
        ops.linear_backward(d_kp, s_pe, wk, B * K1, d, 1024, dx_out=d_s_pe, dx_ld=1024, need_dw=False)
    ops.softmax_rows_backward_(d_un, unary, B * shot, L)
    wu = model.rpn_unary_layer.weight.detach()
    acc(model.rpn_unary_layer.weight, ops.rowdot_backward(s_pe, d_un, wu, B * K1, 1024, grad_x=d_s_pe))
    acc(model.rpn_unary_layer.bias, ops.colsum(d_un, B * K1, 1))
    if model.semantic_enhance:  # BA block (dana.py:133-137)
        s_pre, ba_w = ctx["s_pre"], ctx["ba_w"]
        G = B * shot
        gvec, gsum = ops.ba_backward_prep(s_pre, ba_w, d_s_pe, G, L, 1024)  # (one launch; a loop of 4 per group until round 6)
        d_w = ops.ba_backward_(d_s_pe, s_pre, ba_w, gvec, gsum, G, L, 1024, gamma=model.channel_gamma, slope=0.01)
        ops.softmax_rows_backward_(d_w, ba_w, G, L)
        wc = model.rpn_channel_k_layer.weight.detach()
        acc(model.rpn_channel_k_layer.weight,
            ops.rowdot_backward(s_pre, d_w, wc, G * L, 1024, grad_x=d_s_pe if trunk else None))
        acc(model.rpn_channel_k_layer.bias, ops.colsum(d_w, G * L, 1))
    grads_r.finish_all(model, "RCNN_rpn")
    return (d_corr, d_s_pe) if trunk else (None, None)


def model_backward(model, grad_losses=(1.0, 1.0, 1.0, 1.0), ctx=None):
    """model_backward_gen run to completion (the eager path and single-graph captures)"""
    for _ in model_backward_gen(model, grad_losses, ctx=ctx):
        pass


def model_backward_gen(model, grad_losses=(1.0, 1.0, 1.0, 1.0), ctx=None):
    """(generator; for DAnA it pauses ONCE, where the gradients of everything except the trunk are final and every side
    stream is joined into the caller's stream: graphs.GraphedTrainer ends one hipGraph there and starts the next, so that
    the RCCL all-reduce of the finished buckets overlaps the trunk's backward. The sibling detectors do not pause.)

    d(sum_i grad_losses[i] * loss_i)/d(parameters) for the four training losses (rpn_loss_cls, rpn_loss_bbox,
    RCNN_loss_cls, RCNN_loss_bbox) of the last `save_for_backward` forward: what train.py:141-143's
    `loss.backward()` computes, accumulated into `.grad` of the trainable parameters (BN, conv1 and the first
    cfg.RESNET.FIXED_BLOCKS trunk stages are frozen: dana.py:350-385; their `.grad` stays None). The adjoint is the
    class's `_backward_gen`: dana_backward_gen below, each sibling's beside its forward (frcnn.py, fsod.py, fgn.py), all
    composed of the shared pieces that follow."""
    yield from model._backward_gen(grad_losses, ctx)


# ---- pieces every model's backward is composed of ------------------------------------------------------------------------
def scale_seeds(seeds, g_dev):
    """the fused loss kernel's gradient seeds (class seeds..., bbox seed) times the device-resident (g3, g4)"""
    if g_dev is not None:
        for seed in seeds[:-1]:
            ops.scale_by_device_scalar_(seed, g_dev[2:])
        ops.scale_by_device_scalar_(seeds[-1], g_dev[3:])


def begin(model, grad_losses, ctx):
    """-> (ctx, (g1, g2, g3, g4, g_dev), WeightGrads on the model's "wgrad" stream). ctx: the saved-for-backward context to
    differentiate, the one handed in (the loss bridge captured it at forward time) or the model's latest; it is consumed
    exactly once: trunk_backward, the last stage, releases its tensors. grad_losses: four host numbers, the alpha of the
    first launches that consume them (g_dev None), or a tensor, which stays on the device (no host sync in the backward):
    g_dev, read by rpn_loss_backward and scale_seeds, with ones for the host scalars."""
    if ctx is None:
        ctx = model._ctx
    if ctx is None or ctx.get("consumed"):
        raise RuntimeError("no saved training forward to differentiate (run a train-mode forward with grad enabled "
                           "or model.save_for_backward = True first; each forward can be differentiated once)")
    if isinstance(grad_losses, torch.Tensor):
        g = (1.0, 1.0, 1.0, 1.0, grad_losses.detach().to(torch.float32).contiguous())
    else:
        g = tuple(float(x) for x in grad_losses) + (None,)
    stream = None if getattr(model, "_single_stream", False) else model._stream("wgrad", ctx["fc7"].device)
    return ctx, g, WeightGrads(stream, model)


def seed_linear_grads(layer, seed, x, alpha):
    """weight and bias gradient of a Linear whose output gradient is a loss seed [n][C] (RCNN_bbox_pred's d_bbox, a score
    layer's d_score) times the upstream scalar alpha; x [n][in_features]: the layer's input"""
    (n, C), k = seed.shape, layer.in_features
    acc(layer.weight, ops.gemm_small(seed, (1, C), x, (k, 1), C, k, n, alpha=alpha))
    acc(layer.bias, ops.colsum(seed, n, C, alpha=alpha))


def seed_linear_dx(layer, seed, alpha):
    """-> the gradient [n][in_features] into that layer's input (RCNN_bbox_pred: d_fc7)"""
    (n, C), k = seed.shape, layer.in_features
    return ops.gemm_small(seed, (C, 1), layer.weight.detach(), (k, 1), n, k, C, alpha=alpha)


def layer4_backward(d_top, n, saved, grads, need_dx=True):
    """Adjoint of `_head_to_tail` over the blocks a forward saved: d_top [n][2048] into the mean over layer4's output
    positions -> dL/d(layer4's input): the RoIAlign output (meta: the max-pooled support map), no ReLU output: not masked.
    need_dx False (a frozen trunk: the input's gradient has no reader): the first block's data gradients are not run -> None"""
    npos = saved[-1]["h1"] * saved[-1]["w1"]
    g = ops.broadcast_rows(d_top, n, npos, 2048, alpha=1.0 / npos)
    for i, sv in enumerate(reversed(saved)):
        g = bottleneck_backward(g, sv, sv["n"], sv["h"], sv["w"], sv["bp"], grads, sv["key"], mask_dx=i < len(saved) - 1,
                                g_masked=i > 0, need_dx=need_dx or i < len(saved) - 1)
    return g


def roi_features_backward(ctx, d_pooled):
    """d_pooled [n_roi*49][1024] -> d base_feat [B*fh*fw][1024] through RoIAlign or (a saved argmax) RoIPool"""
    B, n_roi, fh, fw = ctx["B"], ctx["B"] * ctx["R"], ctx["fh"], ctx["fw"]
    if ctx.get("roi_argmax") is not None:
        # cfg.POOLING_MODE == 'pool' (dana.py:183-184): every bin's gradient goes to its argmax element (ROIPool_cuda.cu:79-108)
        g_nchw = ops.roi_pool_backward(ops.nhwc_to_nchw(d_pooled, n_roi, 1024, 7, 7), None, ctx["rois"].view(-1, 5),
                                       ctx["roi_argmax"], 1.0 / 16.0, 7, 7, B, 1024, fh, fw)
        return ops.nchw_to_nhwc(g_nchw).view(B * fh * fw, 1024)
    return ops.roi_align_backward(d_pooled.view(n_roi, 7, 7, 1024), ctx["rois"].view(-1, 5), 1.0 / 16.0, 7, 7, B, 1024,
                                  fh, fw, 0, layout=ops.NHWC).view(B * fh * fw, 1024)


# ---- DAnA (dana.py): the stages of dana_backward_gen, named after the forward stages they differentiate ---------------
def _dgrad_weights_ready(model, ctx, dev):
    """The data-gradient weights (flipped / transposed / BN-scaled copies, Winograd-domain filters: ~45 small launches
    that depend on the weights only) are derived at the head of the weight-gradient stream instead of one by one in front
    of the data-gradient launches that need them (the chain every other launch of the trunk's backward waits for). (Round
    4 gave them a stream of their own; which hardware queue that stream landed on decided 1-2 ms of the iteration:
    profiles/r5_role_streams.md.) -> the events (RPN conv's, layer4's, all) are ready; None: derived in place."""
    early = ctx.get("dgw_prefetched")
    if early is not None:
        # round 6: the saving forward already issued them on the weight-gradient stream, under its own trunk
        # (prefetch_dgrad_weights): the backward's three chains start at once instead of behind ~70 weight-only launches
        return early, early, early
    if getattr(model, "_single_stream", False):
        return None, None, None
    prep = model._stream("wgrad", dev)  # (at the head of the weight-gradient stream: nothing is queued there yet)
    prep.wait_event(ops.record_event())
    with ops.on_stream(prep):
        # (in the order the backward needs them: the RPN chain and the box branch start at once, then the trunk)
        _dgrad_weights(_rpn_conv_plan(model, ctx))
        rpnw_ready = ops.record_event()
        _derive_dgrad_weights((sv["bp"] for sv in reversed(ctx["l4_saved"])),
                              no_dx=ctx["l4_saved"][0]["bp"] if ctx["t"] == 3 else None)
        l4w_ready = ops.record_event()
        _derive_dgrad_weights(sv["bp"] for sv in reversed(ctx["q_saved"]))
        return rpnw_ready, l4w_ready, ops.record_event()


def _box_branch_backward(model, ctx, grads, d_bbox, g4):
    """RCNN_bbox_pred <- mean <- layer4 (dana.py:246,387-389) -> d pooled [n_roi*49][1024] (None over a frozen trunk)"""
    seed_linear_grads(model.RCNN_bbox_pred, d_bbox, ctx["fc7"], g4)
    d_fc7 = seed_linear_dx(model.RCNN_bbox_pred, d_bbox, g4)
    return layer4_backward(d_fc7, ctx["B"] * ctx["R"], ctx["l4_saved"], grads, need_dx=ctx["t"] < 3)


def _roi_heads_backward(model, ctx, grads, d_scores, g3):
    """RoI-level attention heads (dana.py:248-292), positive then negative supports. -> what both heads accumulate into:
    (d_q2, d_trq) of the query side's Q projection and transform input, (d_k2, d_un2, d_sp_pe) of the support side's keys,
    unary term and PE-added maps (None over a frozen trunk, ctx["t"] == 3: the support trunk is its only reader), d_wt: the
    attended half of rcnn_transform_layer's weight gradient."""
    B, shot, way, R, Ns = ctx["B"], ctx["shot"], ctx["way"], ctx["R"], ctx["Ns"]
    P2, n_roi, dq, rd, ug = 49, B * R, model.rcnn_reduce_dim, model.rcnn_dim, model.unary_gamma
    q2, sp_pe, k2, un2, K2p = ctx["q2"], ctx["sp_pe"], ctx["k2"], ctx["un2"], ctx["K2p"]
    dev = q2.device
    wt = model.rcnn_transform_layer.weight.detach()
    lin1, lin2 = model.output_score_layer.linear1, model.output_score_layer.linear2
    w1 = lin1.weight.detach()
    nhid = w1.size(0)
    d_q2 = torch.zeros((n_roi * P2, dq), dtype=torch.float32, device=dev)
    d_trq = torch.zeros((n_roi * P2, rd), dtype=torch.float32, device=dev)
    d_sp_pe = torch.zeros((Ns * P2, 1024), dtype=torch.float32, device=dev) if ctx["t"] < 3 else None
    d_k2 = torch.zeros((Ns * P2, dq), dtype=torch.float32, device=dev)
    d_un2 = torch.zeros((Ns, P2), dtype=torch.float32, device=dev)
    d_wt = torch.zeros_like(wt)
    d_sw = None
    for hc in ctx["heads"]:
        off = hc["offset"]
        ds = d_scores[0 if off == 0 else 1]  # rows of cls_score_all: positive-support scores first (dana.py:194)
        seed_linear_grads(lin2, ds, hc["hid"], g3)
        d_hid = seed_linear_dx(lin2, ds, g3)
        ops.relu_mask_(d_hid, hc["hid"], n_roi, nhid)
        grads.linear(d_hid, hc["tr"], n_roi, nhid, P2 * rd, lambda dw, db: (acc(lin1.weight, dw), acc(lin1.bias, db)))
        _, _, d_tr = ops.linear_backward(d_hid, hc["tr"], w1, n_roi, nhid, P2 * rd, need_dw=False)
        ops.axpy_rows_(d_trq, d_tr, n_roi * P2, rd)
        if hc["dense"] is None:
            # the forward ran  tr = A . (S . Wt_a^T) + q half  (DAnARCNN.fold_roi_attn): the attention's VALUE rows are the
            # [147][64] table sw of each image, so its adjoint works on 64-wide rows -- the [n*49][1024] gradient of the
            # attended tensor, its two GEMMs against Wt_a and the two K = 1024 attention adjoints per head do not exist
            if d_sw is None:
                d_sw = torch.zeros((Ns * P2, rd), dtype=torch.float32, device=dev)
            d_att, vw, val, d_val = d_tr, rd, ctx["sw"], d_sw
        else:
            grads.linear(d_tr, hc["dense"], n_roi * P2, rd, 1024,
                         lambda dw, db: ops.axpy_rows_(d_wt.view(-1)[1024:], dw, rd, 1024, ld_y=2048))
            _, _, d_att = ops.linear_backward(d_tr, hc["dense"], wt.view(-1)[1024:], n_roi * P2, rd, 1024, ldw=2048,
                                              need_dw=False)
            vw, val, d_val = 1024, sp_pe, d_sp_pe
        d_qh = _attention_backward(d_att, vw, hc["sc2"], un2.view(-1)[off * P2:], q2, k2.view(-1)[off * P2 * dq:],
                                   val.view(-1)[off * P2 * vw:], B, R * P2, shot, P2, K2p, dq, ug, way * shot * P2 * dq,
                                   way * shot * P2 * vw, way * shot * P2, d_k2.view(-1)[off * P2 * dq:],
                                   d_val.view(-1)[off * P2 * vw:] if d_val is not None else None,
                                   d_un2.view(-1)[off * P2:], vw=vw)
        ops.axpy_rows_(d_q2, d_qh, n_roi * P2, dq)
    if d_sw is not None:
        # sw = sp_pe . Wt_a^T (once per support, both heads): d Wt_a = d_sw^T . sp_pe, d sp_pe += d_sw . Wt_a
        grads.linear(d_sw, sp_pe, Ns * P2, rd, 1024,
                     lambda dw, db: ops.axpy_rows_(d_wt.view(-1)[1024:], dw, rd, 1024, ld_y=2048))
        if d_sp_pe is not None:
            ops.linear_backward(d_sw, sp_pe, wt.view(-1)[1024:], Ns * P2, rd, 1024, ldw=2048, dx_out=d_sp_pe, dx_ld=1024,
                                need_dw=False)
    return d_q2, d_trq, d_k2, d_un2, d_sp_pe, d_wt


def _roi_query_backward(model, ctx, grads, d_q2, d_trq, d_wt):
    """RoI-level query side: Q projection + the q half of rcnn_transform_layer; PE is additive. -> d q_pe [n_roi*49][1024],
    the heads' gradient into the pooled features (over a frozen trunk: the weight gradients only, -> None)"""
    rows, dq, rd, q_pe = ctx["B"] * ctx["R"] * 49, model.rcnn_reduce_dim, model.rcnn_dim, ctx["q_pe"]
    ops.colmean_sub_(d_q2, rows // 49, 49, dq)
    wq2 = model.rcnn_adapt_q_layer.weight.detach()
    grads.linear(d_q2, q_pe, rows, dq, 1024,
                 lambda dw, db: (acc(model.rcnn_adapt_q_layer.weight, dw), acc(model.rcnn_adapt_q_layer.bias, db)))
    d_q_pe = None
    if ctx["t"] < 3:
        _, _, d_q_pe = ops.linear_backward(d_q2, q_pe, wq2, rows, dq, 1024, need_dw=False)

    def _transform_grads(dw, db):  # (both halves of rcnn_transform_layer's weight gradient are in d_wt now)
        ops.axpy_rows_(d_wt, dw, rd, 1024, ld_y=2048)
        acc(model.rcnn_transform_layer.weight, d_wt)
        acc(model.rcnn_transform_layer.bias, db)

    grads.linear(d_trq, q_pe, rows, rd, 1024, _transform_grads)
    if d_q_pe is not None:
        ops.linear_backward(d_trq, q_pe, model.rcnn_transform_layer.weight.detach(), rows, rd, 1024, ldw=2048,
                            dx_out=d_q_pe, dx_ld=1024, need_dw=False)
    return d_q_pe


def _roi_support_backward(model, ctx, grads, d_k2, d_un2, d_sp_pe):
    """RoI-level support side: K projection, unary term, PE, 14x14 average pool (dana.py:105-108,271-277)
    -> d_sup [Ns][L][1024], the gradient into the support trunk's output (d_sp_pe None, a frozen trunk: the weight
    gradients only, -> None)"""
    Ns, P2, dq, sp_pe, un2 = ctx["Ns"], 49, model.rcnn_reduce_dim, ctx["sp_pe"], ctx["un2"]
    ops.colmean_sub_(d_k2, Ns, P2, dq)
    wk2 = model.rcnn_adapt_k_layer.weight.detach()
    grads.linear(d_k2, sp_pe, Ns * P2, dq, 1024,
                 lambda dw, db: (acc(model.rcnn_adapt_k_layer.weight, dw), acc(model.rcnn_adapt_k_layer.bias, db)))
    if d_sp_pe is not None:
        ops.linear_backward(d_k2, sp_pe, wk2, Ns * P2, dq, 1024, dx_out=d_sp_pe, dx_ld=1024, need_dw=False)
    ops.softmax_rows_backward_(d_un2, un2, Ns, P2)
    wu2 = model.rcnn_unary_layer.weight.detach()
    acc(model.rcnn_unary_layer.weight, ops.rowdot_backward(sp_pe, d_un2, wu2, Ns * P2, 1024, grad_x=d_sp_pe))
    acc(model.rcnn_unary_layer.bias, ops.colsum(d_un2, Ns * P2, 1))
    if d_sp_pe is None:
        return None
    (sh_, sw_), pool = ctx["sup_map"], ctx["sup_pool"]
    return ops.avgpool_backward(d_sp_pe, Ns, sh_, sw_, 1024, pool[0], pool[1])


def trunk_backward(model, ctx, grads, gq, gs=None):
    """The last stage of every model's backward: the trunk stages the forward saved, layer3 down to layer_t (ctx["t"]; conv1,
    every BN and the stages in front of t are frozen; t = 3: nothing was saved, gq and gs are None and only the context is
    released) from gq = d base_feat and, if the model differentiates its supports, gs = d(support trunk output). The first
    saved block computes no input gradient: nothing in front of it trains. Block by block for both
    batches (shared weights), so that each block's weight gradient is final (and may be all-reduced) while the earlier
    blocks are differentiated; merged where the forward saved the [query | support] buffers. Releases the context."""
    qs, ss = ctx["q_saved"], ctx.get("s_saved") or []
    ms = ctx.get("m_saved") or []
    merged_ok = len(ms) == len(qs) and getattr(model, "merge_backward", True)
    nblk = len(qs)
    gm = None  # dL/d(block output) of both batches in one buffer (while the blocks run merged)
    for i in range(nblk - 1, -1, -1):
        sq, s_ = qs[i], ss[i] if gs is not None else None
        bp = sq["bp"]
        if merged_ok and bp["ds"] is None and bp["c1"]["stride"] == 1 and i > 0:
            sm = ms[i]
            if gm is None:  # enter the merged form: the two gradients into the two row ranges of one buffer
                cout = bp["c3"]["cout"]
                if i == nblk - 1:  # (the last block's outputs live in corr / sup: mask per batch, then join)
                    ops.relu_mask_(gq, sq["o3"], sm["mq_out"], cout, ld_act=sq.get("o3_ld", 0))
                    ops.relu_mask_(gs, s_["o3"], sm["m_out"] - sm["mq_out"], cout, ld_act=s_.get("o3_ld", 0))
                gm = torch.empty((sm["m_out"], cout), dtype=torch.float32, device=gq.device)
                ops.axpy_rows_(gm, gq, sm["mq_out"], cout, accumulate=False)
                ops.axpy_rows_(gm[sm["mq_out"]:], gs, sm["m_out"] - sm["mq_out"], cout, accumulate=False)
            gm = bottleneck_backward_merged(gm, sq, s_, sm, bp, grads, sq["key"])
            gq, gs = gm[:sm["mq_in"]], gm[sm["mq_in"]:]
        else:
            gm = None
            gq = bottleneck_backward(gq, sq, sq["n"], sq["h"], sq["w"], sq["bp"], grads, sq["key"], need_dx=i > 0,
                                     g_masked=i < nblk - 1)
            if gs is not None:
                gs = bottleneck_backward(gs, s_, s_["n"], s_["h"], s_["w"], s_["bp"], grads, s_["key"], need_dx=i > 0,
                                         g_masked=i < nblk - 1)
        grads.finish_all(model, sq["key"] + ".")
        ready(model, _block_convs(sq["key"], sq["bp"]))
    assert not grads.packed
    ctx.clear()
    ctx["consumed"] = True
    if model._ctx is ctx:
        model._ctx = None


def dana_backward_gen(model, grad_losses, ctx=None):
    """DAnARCNN's adjoint (model_backward_gen): from the start the RPN chain on the forward's support stream, the box branch
    on its layer4 stream and the RoI heads on the caller's, joined where they meet; one pause; then the trunk."""
    ctx, (g1, g2, g3, g4, g_dev), grads = begin(model, grad_losses, ctx)
    dev, main = ctx["corr"].device, ops.cur_stream()
    trunk = ctx["t"] < 3  # a frozen trunk: no launch whose results only the trunk's backward would read
    single = getattr(model, "_single_stream", False)
    capturing = torch.cuda.is_current_stream_capturing()
    rpnw_ready, l4w_ready, dgw_ready = _dgrad_weights_ready(model, ctx, dev)

    # -- RPN chain (_rpn_chain). It depends on the forward's saved tensors only and meets the RoI stage's gradients in
    #    base_feat / the support maps, so it runs on a stream of its own FROM THE START of the backward, beside the box
    #    branch and the RoI heads (round 4: it used to follow them on the caller's stream, 1.4 ms of launches with nothing
    #    beside them). Under stream capture its weight gradients stay inline on the chain's stream (a side stream forked
    #    from an already forked stream crashes hipStreamEndCapture on ROCm 7.2). Issuing the chain even earlier -- from the
    #    eager forward, right behind the RPN head, under the proposal layer and the host round trip -- was built and
    #    measured: +-0 (18.10 / 18.03 vs 18.07 ms): the eager iteration is host-bound there, the chain's ~100 launches
    #    delay the host's count read by what they save on the GPU. Letting every side stream enter the capture through
    #    an event of the capturing stream itself (a flat fork structure) does not avoid that crash either (measured). --
    if not single:  # (issued FIRST: its two 300 us launches buy the host the time to issue the other chains; round 4: 1.2 ms)
        rpn_stream = model._stream("support", dev)  # (the forward's support stream: idle in the backward)
        rpn_stream.wait_event(ops.record_event())
        with ops.on_stream(rpn_stream):
            grads_r = WeightGrads(None if capturing else model._stream("wgrad", dev), model)
            rpn_out = _rpn_chain(model, ctx, g1, g2, g_dev, grads_r, rpnw_ready)
            for t_ in rpn_out:
                if t_ is not None:
                    t_.record_stream(main)
            rpn_done = ops.record_event()

    # -- seeds: d RCNN losses / d (scores, bbox_pred) were written by the fused loss kernel (dana_rcnn_loss);
    #    the upstream scalars g3 / g4 ride as alpha on the first launches that consume them --
    d_score_pos, d_score_neg, d_bbox = ctx["loss_seeds"]
    scale_seeds(ctx["loss_seeds"], g_dev)

    # -- box branch. Independent of the attention heads until the two gradients of the pooled features meet, so it runs
    #    on the forward's layer4 stream: the heads' backward (many small launches) fills the CUs its big launches leave
    #    idle in their tails. (Under stream capture it stays on the caller's stream: a weight-gradient side stream forked
    #    from an already forked stream crashes hipStreamEndCapture on ROCm 7.2 -- tools/graph_debug.py modes 8 / 12 / 13) --
    l4_stream = main if (single or capturing) else model._stream("layer4", dev)
    seeds_ready = ops.record_event()
    stages = grad_stages(model, ctx["plan"], ctx["t"])
    with ops.on_stream(l4_stream):
        l4_stream.wait_event(seeds_ready)
        if l4w_ready is not None:
            l4_stream.wait_event(l4w_ready)
        d_pooled = _box_branch_backward(model, ctx, grads, d_bbox, g4)  # [n_roi*49][1024]
        if d_pooled is not None:
            d_pooled.record_stream(main)
        grads.finish_all(model, "RCNN_top")
        ready(model, stages[0][1])
        box_done = ops.record_event()

    # -- RoI stage on the caller's stream: heads, query side (it meets the box branch in the pooled features), support side --
    d_q2, d_trq, d_k2, d_un2, d_sp_pe, d_wt = _roi_heads_backward(model, ctx, grads, (d_score_pos, d_score_neg), g3)
    d_q_pe = _roi_query_backward(model, ctx, grads, d_q2, d_trq, d_wt)
    main.wait_event(box_done)
    d_bf = None
    if trunk:
        ops.axpy_rows_(d_pooled, d_q_pe, d_q_pe.size(0), 1024)
        d_bf = roi_features_backward(ctx, d_pooled)
    d_sup = _roi_support_backward(model, ctx, grads, d_k2, d_un2, d_sp_pe)  # [Ns][L][1024]
    grads.join()  # (the heads' Linear weight / bias gradients were accumulated on the weight-gradient stream)
    ready(model, stages[1][1])

    if not single:
        main.wait_event(rpn_done)
        for n_ in stages[2][1]:  # (gradients first allocated on the chain's streams are read on the caller's from here on)
            g_ = model.get_parameter(n_).grad
            if g_ is not None:
                g_.record_stream(main)
    else:
        rpn_out = _rpn_chain(model, ctx, g1, g2, g_dev, grads, rpnw_ready)
    d_corr, d_s_pe = rpn_out
    if trunk:
        K1 = d_s_pe.size(1)  # shot * L rows per image
        for b in range(ctx["B"]):  # the positive supports' PE-added maps (dana.py:103,130)
            ops.axpy_rows_(d_sup.view(-1)[b * ctx["way"] * K1 * 1024:], d_s_pe[b], K1, 1024)
    grads.finish_all(model, "RCNN_rpn")
    ready(model, stages[2][1])
    if dgw_ready is not None:
        ops.cur_stream().wait_event(dgw_ready)
    yield "heads, RPN and attention done; trunk next"

    # -- trunk: the RoIAlign and the RPN paths meet in base_feat (the first half of corr's columns) --
    if not trunk:
        trunk_backward(model, ctx, grads, None)
        return
    ops.axpy_rows_(d_corr, d_bf, d_bf.size(0), 1024, ld_y=2048)
    g = torch.empty_like(d_bf)
    ops.axpy_rows_(g, d_corr, d_bf.size(0), 1024, ld_x=2048, accumulate=False)
    trunk_backward(model, ctx, grads, g, d_sup.view(-1, 1024))


# ---- the sibling detectors (frcnn.py, fsod.py, fgn.py): shared pieces of their backwards ----------------------------------
def sibling_rpn_backward(model, ctx, g1, g2, g_dev, grads, residual=None):
    """Adjoint of the siblings' RPN (rpn.py:58-115): RPN losses -> heads -> ReLU -> 3x3 conv, with the weight and bias
    gradients of the heads and of RPN_Conv. -> the gradient into the RPN's input [B*rfh*rfw][1024] (+ residual), in that
    input's own geometry (fsod: the correlation map is smaller than base_feat); the model differentiates it from there.
    Over a frozen trunk (ctx["t"] == 3) the conv's data gradient has no reader: not run, -> None."""
    plan, B, rpn, nh = ctx["plan"], ctx["B"], model.RCNN_rpn, ctx["nh"]
    d_heads = ops.rpn_loss_backward(ctx["rpn_heads"], nh, ctx["at"], ctx["rpn_l"], g1, g2, sigma=3.0,
                                    inside_weight=cfg.TRAIN.RPN_BBOX_INSIDE_WEIGHTS[0], grad_dev=g_dev)
    rfh, rfw = ctx.get("rfh", ctx["fh"]), ctx.get("rfw", ctx["fw"])
    rhw = rfh * rfw
    dwh, dbh, d_x = ops.linear_backward(d_heads, ctx["rpn_x"], plan["rpn_head_w"], B * rhw, nh, 512)
    ns = rpn.nc_score_out
    acc(rpn.RPN_cls_score.weight, dwh[:ns])
    acc(rpn.RPN_cls_score.bias, dbh[:ns])
    acc(rpn.RPN_bbox_pred.weight, dwh[ns:])
    acc(rpn.RPN_bbox_pred.bias, dbh[ns:])
    ops.relu_mask_(d_x, ctx["rpn_x"], B * rhw, 512)
    c_rpn = _rpn_conv_plan(model, ctx)
    grads.add_conv("RCNN_rpn.RPN_Conv", d_x, ctx["rpn_feat"], B, rfh, rfw, c_rpn)
    acc(rpn.RPN_Conv.bias, ops.colsum(d_x, B * rhw, 512))
    if ctx["t"] == 3:
        return None
    return conv_dgrad(d_x, B, rfh, rfw, c_rpn, residual=residual)


def shot_mean_backward(gs, d_map, ctx, offset):
    """Adjoint of the mean over the shots [offset, offset + shot) of every episode's support maps (fsod.py:98-101,
    fgn.py:57-60): d_map [B][L][1024] / shot into those shots' rows of gs [Ns*L][1024] = d(support trunk output)"""
    shot, way, L = ctx["shot"], ctx["way"], ctx["L"]
    for b in range(ctx["B"]):
        for s in range(shot):
            ops.axpy_rows_(gs.view(-1)[(b * way * shot + offset + s) * L * 1024:], d_map[b], L, 1024, alpha=1.0 / shot)
