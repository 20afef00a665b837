"""Query bank (DAnARCNN.encode_query_bank -> QueryBank -> bank.batch(index)): the gather kernel, the bank rows against what the
forward's query trunk writes into corr, the launch lists, Trainer and the launch-program replay with both banks, the eval-mode
forwards and the refusals. Shape of test_gpu_support_bank.py: B 2, way 2, query 128x160 (map 8x10), supports 320x320, `test`
weight profile, model built under cfg.RESNET.FIXED_BLOCKS = 3 with the BA block; shot 1 and 2."""
from collections import Counter

import numpy as np
import pytest
import torch

from test_gpu_support_cache import _close as _close_eval  # (the same bar on an eval forward's one-head cls_prob rows)
from test_gpu_support_bank import B, H, W, WAY, _build, _close, _inputs, _params, _pool_and_draws, _recorded, _support_ims

pytestmark = pytest.mark.gpu

HW = 8 * 10  # rows of one 128x160 image's trunk map


@pytest.fixture
def split_default():
    """the launch counts and the refusal after a mode change are stated for a process whose default kernel is the bf16x6
    split kernel: pin it, whatever DANA_MFMA_SPLIT says"""
    from dana_amd import ops
    prev = ops.set_mfma_mode(1)
    yield
    ops.set_mfma_mode(prev)


# ---- 1. the gather alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 3, 3, 8, 16), (3, 4, 7, 12, 12), (2, 5, 80, 1024, 2048), (1, 2, 2394, 1024, 2048)],
                         ids=lambda v: "B%d-N%d-rows%d-C%d-ld%d" % v)
def test_gather_equals_numpy_indexing_bit_for_bit(dev, shape):
    """dana_qbank_gather against numpy indexing into a sentinel-prefilled destination: a whole image smaller than one
    workgroup's 1024-unit chunk; a dense destination with C a multiple of 4 but not of 8; the test model's shape; one
    production image (2394 * 256 units: no multiple of 256 * 4). Indices repeat and are not monotone. Columns C .. ld_out-1
    and the rows behind the last image keep the sentinel."""
    from dana_amd import ops
    Bq, N, rows, C, ld = shape
    rng = np.random.RandomState(3 + rows + C)
    maps = rng.standard_normal((N, rows, C)).astype(np.float32)
    idx = {1: [N - 1], 2: [N - 1, 1], 3: [2, 0, 2]}[Bq]
    tail = 3
    out0 = np.full((Bq * rows + tail, ld), -7.5, dtype=np.float32)
    out = ops.qbank_gather(torch.from_numpy(maps).to(dev), torch.tensor(idx, dtype=torch.int32, device=dev), Bq,
                           out=torch.from_numpy(out0).to(dev), ld_out=ld)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = out0.copy()
    want[:Bq * rows, :C] = maps[np.asarray(idx)].reshape(Bq * rows, C)
    assert np.array_equal(got[:Bq * rows, :C], want[:Bq * rows, :C])
    assert np.all(got[:Bq * rows, C:] == -7.5)
    assert np.all(got[Bq * rows:] == -7.5)
    assert np.array_equal(got, want)
    if Bq == 3:  # a fresh dense destination, other order
        fresh = ops.qbank_gather(torch.from_numpy(maps).to(dev), torch.tensor([3, 1, 1], dtype=torch.int32, device=dev), Bq)
        assert fresh.shape == (Bq * rows, C) and np.array_equal(fresh.cpu().numpy(), maps[[3, 1, 1]].reshape(-1, C))


# ---- 2. bank rows are what the forward computes ---------------------------------------------------------------------------
def _forward(m, inputs, seed=33):
    np.random.seed(seed)
    with torch.no_grad():
        out = m(*inputs)
    torch.cuda.synchronize()
    return tuple(t.clone() if torch.is_tensor(t) else t for t in out)


def _losses_agree(out, ref):
    for a, b in zip(out[3:7], ref[3:7]):
        print("loss %.6f against %.6f from images" % (float(a), float(b)))
        assert abs(float(a) - float(b)) <= 1e-4 * max(1.0, abs(float(b)))


@pytest.mark.parametrize("shot", [1, 2])
def test_bank_rows_are_what_the_forward_computes(dev, shot):
    """The B query images encoded as ONE chunk in batch order run `_rcnn_base` over the same batch as the from-images forward's
    query walk, which saves nothing at FIXED_BLOCKS = 3: same kernels, same shapes, same operands (only the row stride of the
    last conv's destination differs). Hence torch.equal on corr's first 1024 columns, and the same rois_label. Another
    chunking (chunk = 1: other row counts in the contractions) and a permuted batch are held to the end-to-end bar."""
    m, _ = _build("DAnA", 3, dev, shot, use_BA_block=True)
    inputs = _inputs(dev, shot)
    bank = m.encode_query_bank(inputs[0], chunk=B)
    assert len(bank) == B and bank.nbytes() == B * HW * 1024 * 4 and bank.maps.shape == (B, HW, 1024)
    assert bank.image_hw == (H, W) and bank.map_hw == (8, 10)
    qb = bank.batch(np.arange(B))
    assert qb.index.tolist() == [0, 1] and qb.B == B
    m.save_for_backward = True
    ref = _forward(m, inputs)
    corr_ref = m._ctx["corr"][:, :1024].clone()
    assert len(m._ctx["q_saved"]) == 0 and m._ctx["t"] == 3
    out = _forward(m, [qb] + inputs[1:])
    ctx = m._ctx
    assert torch.equal(ctx["corr"][:, :1024], corr_ref)
    assert torch.equal(bank.maps.view(B * HW, 1024), corr_ref)
    assert len(ctx["q_saved"]) == 0 and len(ctx["s_saved"]) == 0 and len(ctx["m_saved"]) == 0
    assert torch.equal(out[7], ref[7])
    _close(out, ref)
    _losses_agree(out, ref)
    # a plain train-mode forward (nothing saved) takes the batch too
    m.save_for_backward = False
    plain = _forward(m, [qb] + inputs[1:])
    assert m._ctx is None
    _losses_agree(plain, ref)
    m.save_for_backward = True

    # another chunking
    one = m.encode_query_bank(inputs[0], chunk=1)
    print("chunk 1 against one chunk: map-level max |d| %.3e (max |map| %.3e)"
          % ((one.maps - bank.maps).abs().max().item(), bank.maps.abs().max().item()))
    out1 = _forward(m, [one.batch([0, 1])] + inputs[1:])
    _close(out1, ref)
    _losses_agree(out1, ref)
    # a permuted batch: bank rows [1, 0] against the from-images forward over the permuted inputs
    perm = torch.tensor([1, 0], device=dev)
    pin = [t[perm].contiguous() for t in inputs]
    ref_p = _forward(m, pin)
    corr_p = m._ctx["corr"][:, :1024].clone()
    qb.set([1, 0])
    out_p = _forward(m, [qb] + pin[1:])
    print("permuted batch: map-level max |d| %.3e" % (m._ctx["corr"][:, :1024] - corr_p).abs().max().item())
    _close(out_p, ref_p)
    _losses_agree(out_p, ref_p)


@pytest.mark.usefixtures("split_default")
# ---- 3. launch lists --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shot", [1, 2])
def test_query_batch_forward_issues_one_gather_and_no_query_trunk(dev, shot):
    from dana_amd import backward as BW
    m, _ = _build("DAnA", 3, dev, shot, use_BA_block=True)
    pool, draws = _pool_and_draws(dev, shot)
    inputs = _inputs(dev, shot)[:4]
    sup_ims = _support_ims(pool, draws[0])
    qb = m.encode_query_bank(inputs[0], chunk=B).batch(np.arange(B))
    ep = m.encode_support_bank(pool).episode(draws[0])
    m.save_for_backward = True

    def forward(first, sup):
        np.random.seed(33)
        with torch.no_grad():
            m(first, *inputs[1:], sup)
        return m._ctx

    def backward():
        BW.model_backward(m, (1.0, 0.5, 2.0, 1.5))

    forward(inputs[0], sup_ims), backward()  # (warm: plan, role streams, per-shape caches)
    f_img, _ = _recorded(lambda: forward(inputs[0], sup_ims))
    b_img, _ = _recorded(backward)
    f_q, ctx_q = _recorded(lambda: forward(qb, sup_ims))
    saved_q = {k_: len(ctx_q[k_]) for k_ in ("q_saved", "s_saved", "m_saved")}
    b_q, _ = _recorded(backward)
    f_qe, ctx_qe = _recorded(lambda: forward(qb, ep))
    saved_qe = {k_: len(ctx_qe[k_]) for k_ in ("q_saved", "s_saved", "m_saved")}
    b_qe, _ = _recorded(backward)
    plan = m._get_plan()
    corr = torch.empty((B * HW, 2048), dtype=torch.float32, device=dev)
    with torch.no_grad():
        q_trunk, _ = _recorded(lambda: m._rcnn_base(inputs[0], plan, out_stride=2048, out_buf=corr))
        s_trunk, _ = _recorded(lambda: m._rcnn_base(sup_ims.reshape(-1, 3, 320, 320), plan))
    c_img, c_q, c_qe, c_qt, c_st = (Counter(x) for x in (f_img, f_q, f_qe, q_trunk, s_trunk))
    print("forward launches: %d from images, %d from a query batch, %d from both banks; the query trunk alone %d"
          % (len(f_img), len(f_q), len(f_qe), len(q_trunk)))
    conv = [n for n in c_qt if any(w in n for w in ("conv", "winograd", "bottleneck", "gemm"))]
    assert sum(c_qt[n] for n in conv) == 38, [(n, c_qt[n]) for n in conv]
    assert c_img["dana_qbank_gather"] == 0
    want = c_img - c_qt + Counter(["dana_qbank_gather"])
    assert c_q == want, (sorted((c_q - want).items()), sorted((want - c_q).items()))
    want = (c_img - c_qt - c_st - Counter(["dana_avgpool_nhwc", "dana_add_pe", "dana_add_pe_groups"])
            + Counter(["dana_qbank_gather", "dana_bank_gather_episode"]))
    assert c_qe == want, (sorted((c_qe - want).items()), sorted((want - c_qe).items()))
    assert not any(c_qe[n] for n in ("dana_nchw_to_nhwc", "dana_maxpool3x3s2_ceil_nhwc"))  # (no trunk launch at all)
    assert saved_q == dict(q_saved=0, s_saved=0, m_saved=0) and saved_qe == saved_q
    assert b_q == b_img and b_qe == b_img


# ---- 4. Trainer and the launch-program replay ----------------------------------------------------------------------------
@pytest.mark.parametrize("shot", [1, 2])
def test_trainer_and_program_replay_from_both_banks(dev, shot):
    """three Trainer.step iterations from (images, episode) == three from (query batch, episode) naming the same images (same
    np.random seeds, lr 1e-3) by |dp| <= 1e-6 + 1e-4 * max|p|; then a ProgramTrainer recorded on (batch, ..., episode) and
    replayed three times behind batch.set / ep.set == the eager query-bank trainer"""
    from dana_amd import synthetic as S
    from dana_amd.program import ProgramTrainer
    from dana_amd.trainer import Trainer
    pool, draws = _pool_and_draws(dev, shot)
    inputs = _inputs(dev, shot, seed=6)[:4]
    qpool = S.normal("query_pool", (5, 3, H, W), 64.0, 0.0, 17).to(dev)
    qdraws = [np.array(d) for d in ([3, 0], [4, 4], [1, 2])]
    models = [_build("DAnA", 3, dev, shot, sd_seed=5, use_BA_block=True)[0] for _ in range(3)]
    m_img, m_bank, m_prog = models
    start = _params(m_img)
    t_img, t_bank, t_prog = (Trainer(m_, 1e-3) for m_ in models)
    ep_i = m_img.encode_support_bank(pool, chunk=4).episode(draws[0])
    for it, (draw, qd) in enumerate(zip(draws, qdraws)):
        ep_i.set(draw)
        np.random.seed(40 + it)
        t_img.step(qpool[torch.from_numpy(qd).to(dev)].contiguous(), *inputs[1:], ep_i)
    ep = m_bank.encode_support_bank(pool, chunk=4).episode(draws[0])
    qbank = m_bank.encode_query_bank(qpool, chunk=2)
    assert len(qbank) == 5
    qb = qbank.batch(qdraws[0])
    for it, (draw, qd) in enumerate(zip(draws, qdraws)):
        ep.set(draw)
        qb.set(qd)
        np.random.seed(40 + it)
        out_bank = t_bank.step(qb, *inputs[1:], ep)
    torch.cuda.synchronize()
    ref, got = _params(m_img), _params(m_bank)
    d = np.abs(got - ref).max()
    print("eager: max |dp| %.3e between the query-bank and the from-images trainer (bound %.3e), moved %.3e"
          % (d, 1e-6 + 1e-4 * np.abs(ref).max(), np.abs(ref - start).max()))
    assert d <= 1e-6 + 1e-4 * np.abs(ref).max(), d
    assert not np.array_equal(ref, start) and not np.array_equal(got, start)
    assert all(p.grad is None for n, p in m_bank.named_parameters() if n.startswith("RCNN_base."))

    ep_p = m_prog.encode_support_bank(pool, chunk=4).episode(draws[0])
    qb_p = m_prog.encode_query_bank(qpool, chunk=2).batch(qdraws[0])
    pt = ProgramTrainer(t_prog, qb_p, *inputs[1:], ep_p, warmup=0)
    torch.cuda.synchronize()
    assert np.array_equal(_params(m_prog), start) and t_prog.steps == 0
    assert not any(torch.is_tensor(t) and t.dim() == 4 for t in pt.inputs)  # (no im_data holder)
    names = [e[1].__name__ if hasattr(e[1], "__name__") else "" for e in pt.p1.entries if e[0] == 0]
    assert names.count("dana_qbank_gather") == 1 and names.count("dana_bank_gather_episode") == 1
    for it, (draw, qd) in enumerate(zip(draws, qdraws)):
        ep_p.set(draw)
        qb_p.set(qd)
        np.random.seed(40 + it)
        out_prog = pt.step(qb_p, *inputs[1:], ep_p)
    torch.cuda.synchronize()
    rep = _params(m_prog)
    d = np.abs(rep - got).max()
    print("replay: max |dp| %.3e against the eager query-bank trainer (bound %.3e)" % (d, 1e-6 + 1e-4 * np.abs(got).max()))
    assert d <= 1e-6 + 1e-4 * np.abs(got).max(), d
    assert t_prog.steps == 3 and not np.array_equal(rep, start)
    for a, b in zip(out_prog[3:7], out_bank[3:7]):
        assert abs(float(a) - float(b)) <= 1e-4 * max(1.0, abs(float(b)))


# ---- 5. eval ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shot", [1, 2])
def test_eval_forwards_from_a_query_batch(dev, shot):
    """eval-mode forwards from a query batch against the same images: support images, a SupportCache selection, a class sweep"""
    from dana_amd import synthetic as S
    m, _ = _build("DAnA", 3, dev, shot, use_BA_block=True)
    m.eval()
    inputs = _inputs(dev, shot)[:4]
    sup = S.normal("eval_supports", (B, shot, 3, 320, 320), 64.0, 0.0, 9).to(dev)
    with torch.no_grad():
        qb = m.encode_query_bank(inputs[0], chunk=B).batch([0, 1])
        cache = m.encode_supports(sup)
    ref = _forward(m, inputs + [sup])
    out = _forward(m, [qb] + inputs[1:] + [sup])
    assert out[3:] == (0, 0, 0, 0, None)
    _close_eval(out, ref)
    cache.select([1, 0])
    ref = _forward(m, inputs + [cache])
    _close_eval(_forward(m, [qb] + inputs[1:] + [cache]), ref)
    ref = _forward(m, inputs + [cache.sweep([1, 0])])
    out = _forward(m, [qb] + inputs[1:] + [cache.sweep([1, 0])])
    assert out[0].shape[0] == B * 2
    _close_eval(out, ref)


@pytest.mark.usefixtures("split_default")
# ---- 6. refusals and staleness ----------------------------------------------------------------------------------------------
def test_refusals(dev):
    import dana_amd
    from dana_amd import ops, parallel
    from dana_amd.graphs import GraphedDAnA, GraphedTrainer
    from dana_amd.program import ProgramDAnA, ProgramTrainer
    from dana_amd.trainer import Trainer
    shot = 1
    pool, draws = _pool_and_draws(dev, shot)
    inputs = _inputs(dev, shot)
    sup_ims = inputs[4]

    # the trunk not frozen: train mode refuses, eval mode runs (the tensor versions and the weight epoch protect the bank)
    m1, _ = _build("DAnA", 1, dev, shot, use_BA_block=True)
    qb1 = m1.encode_query_bank(inputs[0]).batch([0, 1])
    with pytest.raises(ValueError, match=r"RESNET\.FIXED_BLOCKS"):
        m1(qb1, *inputs[1:])
    m1.eval()
    ev = [inputs[0], *inputs[1:4], sup_ims[:, :shot].contiguous()]
    _close_eval(_forward(m1, [qb1] + ev[1:]), _forward(m1, ev))
    # ... and the weight epoch: layer2-3 train here and the fused optimizer writes them through raw pointers (no tensor
    # version moves), so one Trainer.step makes the bank stale for the validation forward that follows
    m1.train()
    np.random.seed(40)
    Trainer(m1, 1e-3).step(*inputs)
    m1.eval()
    with pytest.raises(RuntimeError, match="re-encode"):
        m1(qb1, *ev[1:])
    fresh = m1.encode_query_bank(inputs[0]).batch([0, 1])
    _close_eval(_forward(m1, [fresh] + ev[1:]), _forward(m1, ev))
    del m1, qb1, fresh

    m, sd = _build("DAnA", 3, dev, shot, use_BA_block=True)
    bank = m.encode_query_bank(inputs[0])
    qb = bank.batch([0, 1])
    # host-side index checks through the public calls
    with pytest.raises(ValueError):
        bank.batch(torch.tensor([0, 1], device=dev))
    with pytest.raises(ValueError):
        bank.batch([[0, 1]])
    with pytest.raises(ValueError):
        qb.set([0, 1, 0])  # (another batch size than the batch's)
    with pytest.raises(IndexError):
        qb.set([0, len(bank)])
    assert qb.index.tolist() == [0, 1]
    # graphs, ProgramDAnA, sharding, attention maps
    tr = Trainer(m, 1e-3)
    with pytest.raises(NotImplementedError, match="QueryBank.*ProgramTrainer"):
        GraphedTrainer(tr, qb, *inputs[1:])
    with pytest.raises(NotImplementedError, match="QueryBank.*ProgramTrainer"):
        GraphedDAnA(m, qb, *inputs[1:])
    with pytest.raises(NotImplementedError, match="QueryBank.*ProgramTrainer"):
        ProgramDAnA(m, qb, *inputs[1:])
    with pytest.raises(TypeError, match="its own bank"):
        parallel.shard_episode((qb,) + tuple(inputs[1:]), 0, 2)
    with pytest.raises(TypeError, match="QueryBatch"):
        m.attention_maps(qb, inputs[1], inputs[2][:, :3, :4].contiguous(), sup_ims)
    # a batch of another bank, another B, or images into a recorded program (and a batch into one recorded on images)
    bank.batch([1, 0])  # (another batch wrote the shared index buffer: the runner puts qb's back before its recording opens)
    pt = ProgramTrainer(tr, qb, *inputs[1:], warmup=0)
    with pytest.raises(RuntimeError, match="re-record"):
        pt.step(m.encode_query_bank(inputs[0]).batch([0, 1]), *inputs[1:])
    with pytest.raises(RuntimeError, match="re-record"):
        pt.step(bank.batch([0]), *[t[:1] for t in inputs[1:]])
    with pytest.raises(RuntimeError, match="re-record"):
        pt.step(*inputs)
    pt_img = ProgramTrainer(tr, *inputs, warmup=0)
    with pytest.raises(RuntimeError, match="re-record"):
        pt_img.step(qb, *inputs[1:])
    del pt_img
    np.random.seed(40)
    pt.step(qb, *inputs[1:])  # (the recorded bank's own batch still replays)
    torch.cuda.synchronize()
    # the bank after the MFMA mode or the weights changed
    prev = ops.set_mfma_mode(0)
    try:
        with pytest.raises(RuntimeError, match="re-encode"):
            m(qb, *inputs[1:])
        with pytest.raises(RuntimeError, match="re-encode"):
            pt.step(qb, *inputs[1:])
    finally:
        ops.set_mfma_mode(prev)
    m.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="re-encode"):
        m(qb, *inputs[1:])
    with pytest.raises(RuntimeError, match="re-encode"):
        pt.step(qb, *inputs[1:])
    # the siblings own their trunk calls
    for name in ("meta", "fsod", "fgn", "frcnn"):
        s = dana_amd.get_model(name, pretrained=False, way=WAY, shot=shot, classes=["fg", "bg"])
        with pytest.raises(NotImplementedError):
            s.encode_query_bank(inputs[0])
