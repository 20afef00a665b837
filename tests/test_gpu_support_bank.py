"""Fine-tuning over a frozen trunk from a support bank (DAnARCNN.encode_support_bank -> SupportBank -> bank.episode(index)):
the gather kernel, the bank rows, the episode forward / backward against the from-images ones, Trainer, the launch-program
replay and the refusals. Small shape of test_gpu_fixed_blocks.py: B 2, way 2, query 128x160, supports 320x320, `test` weight
profile, model built under cfg.RESNET.FIXED_BLOCKS = 3 with the BA block; shot 1 and shot 2 (the positive / negative split and
the shot*L stride of s_pe are trivial at shot 1)."""
from collections import Counter

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, WAY, H, W = 2, 2, 128, 160


def _build(name, k, dev, shot, sd_seed=21, **kw):
    """the model built under cfg.RESNET.FIXED_BLOCKS = k (restored behind the constructor) -> (model on dev in train mode, sd)"""
    import dana_amd
    from dana_amd import synthetic as S
    from dana_amd.config import cfg
    prev = cfg.RESNET.FIXED_BLOCKS
    cfg.RESNET.FIXED_BLOCKS = k
    try:
        m = dana_amd.get_model(name, pretrained=False, way=WAY, shot=shot, classes=["fg", "bg"], **kw)
    finally:
        cfg.RESNET.FIXED_BLOCKS = prev
    sd = S.fill_state_dict(m.state_dict(), seed=sd_seed, profile="test")
    m.load_state_dict(sd)
    m.to(dev).train()
    m.nms_inclusive = True
    return m, sd


def _inputs(dev, shot, seed=23):
    from dana_amd import synthetic as S
    return [t.to(dev) for t in S.episode_inputs(B, WAY, shot, H, W, seed=seed)]


class _Names:
    """a _lib.RECORDER that keeps the C-ABI entry-point names (test_gpu_fixed_blocks.py's _backward_launches)"""

    def __init__(self):
        self.names = []

    def add_call(self, fn, name, args):
        self.names.append(name)


def _recorded(fn):
    from dana_amd import _lib
    rec = _Names()
    _lib.RECORDER = rec
    try:
        out = fn()
    finally:
        _lib.RECORDER = None
    torch.cuda.synchronize()
    return rec.names, out


# ---- 1. the gather alone ------------------------------------------------------------------------------------------------
def _gather_ref(map_pe, pool_pe, idx, shot, s_pe, sp_pe):
    """numpy indexing into prefilled destinations; rows outside [0, N) leave their blocks alone"""
    N, L, P = map_pe.shape[0], map_pe.shape[1], pool_pe.shape[1]
    s_pe, sp_pe = s_pe.copy(), sp_pe.copy()
    for b in range(idx.shape[0]):
        for r in range(idx.shape[1]):
            n, s = idx[b, r], b * idx.shape[1] + r
            if n < 0 or n >= N:
                continue
            sp_pe[s * P:(s + 1) * P] = pool_pe[n]
            if r < shot:
                s_pe[b, r * L:(r + 1) * L] = map_pe[n]
    return s_pe, sp_pe


@pytest.fixture
def split_default():
    """the launch counts and the refusal after a mode change are stated for a process whose default kernel is the bf16x6
    split kernel: pin it, whatever DANA_MFMA_SPLIT says"""
    from dana_amd import ops
    prev = ops.set_mfma_mode(1)
    yield
    ops.set_mfma_mode(prev)


@pytest.mark.parametrize("bws", [(1, 1, 1), (2, 2, 1), (2, 2, 2), (3, 2, 3)], ids=lambda v: "B%d-way%d-shot%d" % v)
@pytest.mark.parametrize("C,L", [(8, 3), (1024, 400)], ids=["c8-L3", "c1024-L400"])
def test_gather_equals_numpy_indexing_bit_for_bit(dev, C, L, bws):
    """dana_bank_gather_episode against numpy indexing: N = 5 rows, the 49-row tensor beside L = 3 / 400 (row counts that are
    no multiple of the kernel's 1024-unit workgroup chunk; at c8-L3 a whole slot is less than one chunk, at c1024-L400 the
    pooled / map boundary falls inside a chunk), repeats, one row positive for image 0 and negative for image 1, and an
    out-of-range entry (N and -1), whose blocks keep the sentinel prefill"""
    from dana_amd import ops
    Bq, way, shot = bws
    N, P, ws = 5, 49, way * shot
    rng = np.random.RandomState(7 + C + 10 * Bq)
    map_pe = rng.standard_normal((N, L, C)).astype(np.float32)
    pool_pe = rng.standard_normal((N, P, C)).astype(np.float32)
    idx = rng.randint(0, N, size=(Bq, ws))
    if Bq > 1 and way > 1:
        idx[1, shot] = idx[0, 0]  # positive of image 0, negative of image 1
    if ws > 1:
        idx[0, ws - 1] = idx[0, 0]  # a repeat inside one image
    d_map, d_pool = torch.from_numpy(map_pe).to(dev), torch.from_numpy(pool_pe).to(dev)
    cases = [idx]
    for bad, slot in ((N, 0), (-1, Bq * ws - 1)):  # a positive slot (both destinations) and the last slot
        j = idx.copy()
        j.reshape(-1)[slot] = bad
        cases.append(j)
    for j in cases:
        s0 = np.full((Bq, shot * L, C), -7.5, dtype=np.float32)
        p0 = np.full((Bq * ws * P, C), -7.5, dtype=np.float32)
        s_pe, sp_pe = ops.bank_gather_episode(d_map, d_pool, torch.from_numpy(j.astype(np.int32).reshape(-1)).to(dev), Bq, way,
                                              shot, s_pe=torch.from_numpy(s0).to(dev), sp_pe=torch.from_numpy(p0).to(dev))
        torch.cuda.synchronize()
        want_s, want_p = _gather_ref(map_pe, pool_pe, j, shot, s0, p0)
        assert np.array_equal(s_pe.cpu().numpy(), want_s), j
        assert np.array_equal(sp_pe.cpu().numpy(), want_p), j
    with pytest.raises(ops.DanaError, match="multiple of 4"):
        ops.bank_gather_episode(torch.zeros((N, L, 6), device=dev), torch.zeros((N, P, 6), device=dev),
                                torch.zeros(Bq * ws, dtype=torch.int32, device=dev), Bq, way, shot)


# ---- 2. bank rows hold what the forward would produce ---------------------------------------------------------------------
@pytest.mark.parametrize("shot", [1, 2])
def test_bank_rows_hold_what_the_from_images_forward_produces(dev, shot):
    """The episode's Ns = B*way*shot images encoded as ONE chunk in episode order, against the from-images saving forward in
    the model's default trunk configuration: merge_trunk False and no Trainer preference (_train_merge unset), i.e. the
    support trunk as its own one-segment walk on the support stream (`_trunk_gen([sup_ims], ...)`, alternated block by block
    with the query trunk's). At FIXED_BLOCKS = 3 that walk saves nothing (save_from = 3), so it issues exactly the launches
    of `_rcnn_base(sup_ims, plan)` -- what encode_support_bank runs for a chunk of the same Ns images: same kernels, same
    shapes, same operands, and the PE / average-pool kernels behind them are elementwise per image. Hence torch.equal.
    Another chunking (chunk = 1) runs the trunk's contractions at other row counts, which may pick other tiles / K splits:
    compared at the float64 bar of test_gpu_backward_ops.py, |d| <= 1e-6 * the summed magnitudes of the terms (map + PE; the
    196 window terms / 196 + PE)."""
    from dana_amd import ops
    m, _ = _build("DAnA", 3, dev, shot, use_BA_block=True)
    assert not m.merge_trunk and getattr(m, "_train_merge", None) is None
    inputs = _inputs(dev, shot)
    Ns, ws = B * WAY * shot, WAY * shot
    pool_ims = inputs[4].reshape(Ns, 3, 320, 320)
    bank = m.encode_support_bank(pool_ims, chunk=Ns)
    assert len(bank) == Ns and bank.nbytes() == Ns * (400 + 49) * 1024 * 4
    assert bank.map_pe.shape == (Ns, 400, 1024) and bank.pool_pe.shape == (Ns, 49, 1024)
    ep = bank.episode(np.arange(Ns).reshape(B, ws))
    s_pe, sp_pe = ops.bank_gather_episode(bank.map_pe, bank.pool_pe, bank._index[(B, ws)], B, WAY, shot)
    m.save_for_backward = True
    np.random.seed(33)
    with torch.no_grad():
        m(*inputs)
    ctx = m._ctx
    assert len(ctx["s_saved"]) == 0 and ctx["t"] == 3
    torch.cuda.synchronize()
    assert torch.equal(ctx["sp_pe"].view(-1), sp_pe.view(-1))
    assert torch.equal(ctx["s_pre"].view(-1), s_pe.view(-1))
    assert ep.index.tolist() == np.arange(Ns).reshape(B, ws).tolist()

    one = m.encode_support_bank(pool_ims, chunk=1)
    pe400, pe49 = m._plan["pe400"].double(), m._plan["pe49"].double()
    ref_map = bank.map_pe.double()
    mag_map = (ref_map - pe400).abs() + pe400.abs()
    amap = (ref_map - pe400).abs().view(Ns, 20, 20, 1024).permute(0, 3, 1, 2)
    mag_pool = torch.nn.functional.avg_pool2d(amap, 14, 1).permute(0, 2, 3, 1).reshape(Ns, 49, 1024) + pe49.abs()
    for name, got, ref, mag in (("map_pe", one.map_pe, bank.map_pe, mag_map), ("pool_pe", one.pool_pe, bank.pool_pe, mag_pool)):
        err = (got.double() - ref.double()).abs()
        worst = (err / (1e-6 * mag + 1e-30)).max().item()
        print("chunk 1 against one chunk, %s: max |d| %.3e, worst |d| / bound %.3f" % (name, err.max().item(), worst))
        assert worst <= 1.0, (name, worst)


# ---- 3. forward parity ------------------------------------------------------------------------------------------------------
def _iou(a, b):
    x1, y1 = np.maximum(a[:, 0], b[:, 0]), np.maximum(a[:, 1], b[:, 1])
    x2, y2 = np.minimum(a[:, 2], b[:, 2]), np.minimum(a[:, 3], b[:, 3])
    inter = np.clip(x2 - x1 + 1, 0, None) * np.clip(y2 - y1 + 1, 0, None)
    aa = (a[:, 2] - a[:, 0] + 1) * (a[:, 3] - a[:, 1] + 1)
    ab = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    return inter / (aa + ab - inter)


def _close(out, ref):
    """test_gpu_support_cache.py's end-to-end bar between two 8-tuples"""
    r, rg = out[0].cpu().numpy().reshape(-1, 5), ref[0].cpu().numpy().reshape(-1, 5)
    assert r.shape == rg.shape and np.array_equal(r[:, 0], rg[:, 0])
    matched = _iou(r[:, 1:], rg[:, 1:]) >= 1 - 1e-3
    assert matched.mean() >= 0.99, "only %.1f%% of rois match by position" % (100 * matched.mean())
    assert np.abs(out[1].cpu().numpy() - ref[1].cpu().numpy())[np.tile(matched, 2)].max() <= 1e-4
    assert np.abs(out[2].cpu().numpy() - ref[2].cpu().numpy())[matched].max() <= 1e-4


def _pool_and_draws(dev, shot, n_pool=6, seed=3):
    """a pool of n_pool support images and three episodes over it that really differ (repeats across images included)"""
    from dana_amd import synthetic as S
    pool = S.normal("support_pool", (n_pool, 3, 320, 320), 64.0, 0.0, seed).to(dev)
    rng = np.random.RandomState(11 + shot)
    draws = [rng.randint(0, n_pool, size=(B, WAY * shot)) for _ in range(3)]
    draws[0][1, shot] = draws[0][0, 0]  # image 0's first positive is a negative of image 1
    assert not np.array_equal(draws[0], draws[1]) and not np.array_equal(draws[1], draws[2])
    return pool, draws


def _support_ims(pool, draw):
    return pool[torch.from_numpy(draw.reshape(-1)).to(pool.device)].reshape(draw.shape[0], draw.shape[1], 3, 320, 320).contiguous()


@pytest.mark.parametrize("shot", [1, 2])
def test_episode_forward_equals_the_from_images_forward(dev, shot):
    """train-mode saving forwards from images and from the episode naming the same images, under the same np.random stream"""
    m, _ = _build("DAnA", 3, dev, shot, use_BA_block=True)
    pool, draws = _pool_and_draws(dev, shot)
    inputs = _inputs(dev, shot)[:4]
    bank = m.encode_support_bank(pool)
    assert len(bank) == 6
    ep = bank.episode(draws[0])
    m.save_for_backward = True
    np.random.seed(33)
    with torch.no_grad():
        ref = m(*inputs, _support_ims(pool, draws[0]))
    np.random.seed(33)
    with torch.no_grad():
        out = m(*inputs, ep)
    torch.cuda.synchronize()
    assert out[1].shape == ref[1].shape and out[1].size(0) == 2 * out[2].size(0)  # (both heads' rows)
    _close(out, ref)
    assert torch.equal(out[7], ref[7])
    for a, b in zip(out[3:7], ref[3:7]):
        print("loss %.6f against %.6f from images" % (float(a), float(b)))
        assert abs(float(a) - float(b)) <= 1e-4 * max(1.0, abs(float(b)))
    # a plain train-mode forward (nothing saved) takes the episode too
    m.save_for_backward = False
    np.random.seed(33)
    with torch.no_grad():
        plain = m(*inputs, ep)
    assert m._ctx is None
    for a, b in zip(plain[3:7], ref[3:7]):
        assert abs(float(a) - float(b)) <= 1e-4 * max(1.0, abs(float(b)))


@pytest.mark.usefixtures("split_default")
# ---- 4. launch list ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shot", [1, 2])
def test_episode_forward_issues_one_gather_and_no_support_trunk(dev, shot):
    from dana_amd import backward as BW
    m, _ = _build("DAnA", 3, dev, shot, use_BA_block=True)
    pool, draws = _pool_and_draws(dev, shot)
    inputs = _inputs(dev, shot)[:4]
    sup_ims = _support_ims(pool, draws[0])
    bank = m.encode_support_bank(pool)
    ep = bank.episode(draws[0])
    m.save_for_backward = True

    def forward(sup):
        np.random.seed(33)
        with torch.no_grad():
            m(*inputs, sup)
        return m._ctx

    def backward():
        BW.model_backward(m, (1.0, 0.5, 2.0, 1.5))

    forward(sup_ims), backward()  # (warm: plan, role streams, per-shape caches)
    f_img, ctx_img = _recorded(lambda: forward(sup_ims))
    assert len(ctx_img["s_saved"]) == 0
    b_img, _ = _recorded(backward)
    f_ep, ctx_ep = _recorded(lambda: forward(ep))
    saved = {k_: len(ctx_ep[k_]) for k_ in ("q_saved", "s_saved", "m_saved", "l4_saved")}
    have = set(ctx_ep)
    b_ep, _ = _recorded(backward)
    # the support trunk's launches, as the from-images forward issues them: one one-segment walk that saves nothing
    with torch.no_grad():
        trunk, _ = _recorded(lambda: m._rcnn_base(sup_ims.reshape(-1, 3, 320, 320), m._get_plan()))
    c_img, c_ep, c_trunk = Counter(f_img), Counter(f_ep), Counter(trunk)
    print("forward launches: %d from images, %d from the episode; the support trunk alone %d" % (len(f_img), len(f_ep), len(trunk)))
    assert c_ep["dana_bank_gather_episode"] == 1 and c_img["dana_bank_gather_episode"] == 0
    assert c_ep["dana_avgpool_nhwc"] == 0 and c_ep["dana_add_pe"] == 0 and c_ep["dana_add_pe_groups"] == 0
    assert c_img["dana_avgpool_nhwc"] == 1 and c_img["dana_add_pe"] == 1 and c_img["dana_add_pe_groups"] == 1
    conv = sorted(n for n in c_trunk if any(w in n for w in ("conv", "winograd", "bottleneck", "gemm")))
    # the stem, then per stage a first block of conv1, conv2, expand + downsample in one contraction and identity blocks of
    # three convs (layer1's: conv1 + the fused conv2 / conv3 tail): 1 + (3 + 2 * 2) + (3 + 3 * 3) + (3 + 5 * 3)
    assert sum(c_trunk[n] for n in conv) == 38, [(n, c_trunk[n]) for n in conv]
    for n in conv:  # the query trunk alone + the RPN + layer4
        assert c_ep[n] == c_img[n] - c_trunk[n], (n, c_ep[n], c_img[n], c_trunk[n])
    # ... and nothing else moved either: the episode forward is the from-images one minus the support trunk and the three
    # support-side pool / PE launches, plus the gather
    want = c_img - c_trunk - Counter(["dana_avgpool_nhwc", "dana_add_pe", "dana_add_pe_groups"]) + Counter(["dana_bank_gather_episode"])
    assert c_ep == want, (sorted((c_ep - want).items()), sorted((want - c_ep).items()))
    assert saved == dict(q_saved=0, s_saved=0, m_saved=0, l4_saved=3)
    assert {"s_pe", "s_pre", "ba_w", "kp", "unary", "sp_pe", "k2", "un2", "sw", "Ns", "sup_map", "sup_pool"} <= have
    assert b_ep == b_img
    assert "dana_avgpool_backward_nhwc" not in b_ep


# ---- 5. Trainer and the launch-program replay ----------------------------------------------------------------------------
def _params(m):
    return np.concatenate([p.detach().float().cpu().numpy().ravel() for _, p in sorted(m.named_parameters())])


@pytest.mark.parametrize("shot", [1, 2])
def test_trainer_and_program_replay_from_a_bank(dev, shot):
    """three Trainer.step iterations from images == three from episodes naming the same images (same np.random seeds, lr
    1e-3: profiles/fixed_blocks.md on why 0.01 is too hot at this shape) by |dp| <= 1e-6 + 1e-4 * max|p|; then a
    ProgramTrainer recorded on an episode and replayed three times behind ep.set(draw) == the eager bank Trainer"""
    from dana_amd.program import ProgramTrainer
    from dana_amd.trainer import Trainer
    pool, draws = _pool_and_draws(dev, shot)
    inputs = _inputs(dev, shot, seed=6)[:4]
    models = [_build("DAnA", 3, dev, shot, sd_seed=5, use_BA_block=True)[0] for _ in range(3)]
    m_img, m_bank, m_prog = models
    start = _params(m_img)
    t_img, t_bank, t_prog = (Trainer(m_, 1e-3) for m_ in models)
    for it, draw in enumerate(draws):
        np.random.seed(40 + it)
        t_img.step(*inputs, _support_ims(pool, draw))
    bank = m_bank.encode_support_bank(pool, chunk=4)
    ep = bank.episode(draws[0])
    for it, draw in enumerate(draws):
        ep.set(draw)
        np.random.seed(40 + it)
        out_bank = t_bank.step(*inputs, ep)
    torch.cuda.synchronize()
    ref, got = _params(m_img), _params(m_bank)
    d = np.abs(got - ref).max()
    print("eager: max |dp| %.3e between the bank and the from-images trainer (bound %.3e), moved %.3e"
          % (d, 1e-6 + 1e-4 * np.abs(ref).max(), np.abs(ref - start).max()))
    assert d <= 1e-6 + 1e-4 * np.abs(ref).max(), d
    assert not np.array_equal(ref, start) and not np.array_equal(got, start)
    assert all(p.grad is None for n, p in m_bank.named_parameters() if n.startswith("RCNN_base."))

    bank_p = m_prog.encode_support_bank(pool, chunk=4)
    ep_p = bank_p.episode(draws[0])
    pt = ProgramTrainer(t_prog, *inputs, ep_p, warmup=0)
    torch.cuda.synchronize()
    assert np.array_equal(_params(m_prog), start) and t_prog.steps == 0
    names = [e[1].__name__ if hasattr(e[1], "__name__") else "" for e in pt.p1.entries if e[0] == 0]
    assert names.count("dana_bank_gather_episode") == 1
    for it, draw in enumerate(draws):
        ep_p.set(draw)
        np.random.seed(40 + it)
        out_prog = pt.step(*inputs, ep_p)
    torch.cuda.synchronize()
    rep = _params(m_prog)
    d = np.abs(rep - got).max()
    print("replay: max |dp| %.3e against the eager bank trainer (bound %.3e)" % (d, 1e-6 + 1e-4 * np.abs(got).max()))
    assert d <= 1e-6 + 1e-4 * np.abs(got).max(), d
    assert t_prog.steps == 3 and not np.array_equal(rep, start)
    for a, b in zip(out_prog[3:7], out_bank[3:7]):
        assert abs(float(a) - float(b)) <= 1e-4 * max(1.0, abs(float(b)))


@pytest.mark.usefixtures("split_default")
# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    import dana_amd
    from dana_amd import ops, parallel
    from dana_amd.graphs import GraphedDAnA, GraphedTrainer
    from dana_amd.program import ProgramTrainer
    from dana_amd.trainer import Trainer
    shot = 1
    pool, draws = _pool_and_draws(dev, shot)
    inputs = _inputs(dev, shot)[:4]

    # the trunk not frozen
    m1, _ = _build("DAnA", 1, dev, shot, use_BA_block=True)
    ep1 = m1.encode_support_bank(pool).episode(draws[0])
    with pytest.raises(ValueError, match=r"RESNET\.FIXED_BLOCKS"):
        m1(*inputs, ep1)
    del m1, ep1

    m, sd = _build("DAnA", 3, dev, shot, use_BA_block=True)
    bank = m.encode_support_bank(pool)
    ep = bank.episode(draws[0])
    # host-side index checks through the public calls
    with pytest.raises(ValueError):
        bank.episode(torch.from_numpy(draws[0]).to(dev))
    with pytest.raises(ValueError):
        bank.episode(draws[0][:, :1])
    with pytest.raises(IndexError):
        ep.set(draws[0] + len(bank))
    with pytest.raises(ValueError):
        ep.set(np.concatenate([draws[0], draws[0]]))  # (another batch size than the episode's)
    assert ep.index.tolist() == draws[0].tolist()
    with pytest.raises(RuntimeError, match="batch of 1"):
        m(*[t[:1] for t in inputs], ep)
    # eval mode: an episode points to encode_supports; a SupportCache in train mode raises as before
    m.eval()
    with pytest.raises(RuntimeError, match="encode_supports"):
        m(*inputs, ep)
    with torch.no_grad():
        cache = m.encode_supports(pool[:2].reshape(2, 1, 3, 320, 320))
    m.train()
    with pytest.raises(RuntimeError, match="eval-mode forwards only"):
        m(*inputs, cache)
    # graphs, sharding
    tr = Trainer(m, 1e-3)
    with pytest.raises(NotImplementedError, match="ProgramTrainer"):
        GraphedTrainer(tr, *inputs, ep)
    with pytest.raises(NotImplementedError, match="SupportBank"):
        GraphedDAnA(m, *inputs, ep)
    with pytest.raises(TypeError, match="its own bank"):
        parallel.shard_episode(tuple(inputs) + (ep,), 0, 2)
    # an episode of another bank into a recorded program
    pt = ProgramTrainer(tr, *inputs, ep, warmup=0)
    other = m.encode_support_bank(pool).episode(draws[0])
    with pytest.raises(RuntimeError, match="re-record"):
        pt.step(*inputs, other)
    with pytest.raises(RuntimeError, match="re-record"):
        pt.step(*inputs, _support_ims(pool, draws[0]))
    np.random.seed(40)
    pt.step(*inputs, ep)  # (the recorded bank's own episode still replays)
    torch.cuda.synchronize()
    # the bank after the MFMA mode or the weights changed
    prev = ops.set_mfma_mode(0)
    try:
        with pytest.raises(RuntimeError, match="re-encode"):
            m(*inputs, ep)
    finally:
        ops.set_mfma_mode(prev)
    m.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="re-encode"):
        m(*inputs, ep)
    with pytest.raises(RuntimeError, match="re-encode"):
        pt.step(*inputs, ep)
    # the siblings own their support encoders
    for name in ("meta", "fsod", "fgn", "frcnn"):
        s = dana_amd.get_model(name, pretrained=False, way=WAY, shot=shot, classes=["fg", "bg"])
        with pytest.raises(NotImplementedError, match="own their support encoders"):
            s.encode_support_bank(pool)
