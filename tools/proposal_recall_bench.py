"""Proposal recall (dana_amd/evaluate.py `ProposalRecallEvaluator`) at validation-set size: the device time of `compute()`
by HIP events, and for comparison on the same box the host route the code without the evaluator forces: a device-to-host
copy of all proposals plus the numpy restatement (`evaluate.proposal_recall_numpy`), by default at a tenth of the images
because it takes minutes at full size.

  python tools/proposal_recall_bench.py                  # 5 000 images x 20 classes x 300 proposals, T = 10, L = 4, A = 8
  python tools/proposal_recall_bench.py --no-others      # target units only
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/proposal_recall_bench.py --profile-run

Prints the AR table of a small synthetic model (a class sweep's `rois` through `add_rois`: the plumbing end to end), then
one JSON line. Synthetic seeded data: 1..7 objects per image with random classes; a list's rows are jittered copies of
the image's objects (of the list's class with probability 0.5, of another class with probability 0.1 -- so the lists are
selective, as the attention in front of the RPN is meant to make them) or random boxes.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dana_amd  # noqa: E402
from dana_amd import evaluate as E  # noqa: E402


def make(n_img, n_cls, n_prop, dev, seed=0):
    """-> (boxes [n_img * n_cls * n_prop, 4] on the device, gt_box, gt_img, gt_cls on the host); list p = i * n_cls + c"""
    rs = np.random.RandomState(seed)
    per = rs.randint(1, 8, n_img)
    g = int(per.sum())
    gt_img = np.repeat(np.arange(n_img), per)
    gt_cls = rs.randint(0, n_cls, g)
    side = np.exp(rs.uniform(np.log(12.), np.log(700.), (g, 2)))  # every one of the eight area ranges gets objects
    xy = rs.uniform(0, 600, (g, 2))
    gt_box = np.concatenate((xy, xy + side), 1).astype(np.float32)
    first = np.concatenate(([0], np.cumsum(per)[:-1]))
    gen = torch.Generator(device=dev).manual_seed(seed)
    shape = (n_img, n_cls, n_prop)
    u = lambda *s: torch.rand(*s, generator=gen, device=dev)
    pick = torch.from_numpy(first).to(dev).view(-1, 1, 1) + (u(*shape) * torch.from_numpy(per).to(dev).view(-1, 1, 1)).long()
    obj = torch.from_numpy(gt_box).to(dev)[pick]                      # [n_img, n_cls, n_prop, 4]
    own = torch.from_numpy(gt_cls).to(dev)[pick] == torch.arange(n_cls, device=dev).view(1, -1, 1)
    near = u(*shape) < torch.where(own, 0.5, 0.1)
    jitter = (u(*shape, 4) - 0.5) * 0.3 * (obj[..., 2:] - obj[..., :2]).repeat(1, 1, 1, 2)
    xy = u(*shape, 2) * 600
    rand = torch.cat((xy, xy + torch.exp(u(*shape, 2) * 3.5 + 2.5)), -1)
    boxes = torch.where(near.unsqueeze(-1), obj + jitter, rand).float().reshape(-1, 4).contiguous()
    return boxes, gt_box, gt_img, gt_cls


def fill(ev, boxes, gt_box, gt_img, gt_cls, n_img, n_cls, n_prop):
    ev.add_ground_truth_packed(gt_box, gt_img, gt_cls)
    step = max((1 << 22) // (n_cls * n_prop), 1)  # appended in pieces of images: the buffer grows by doubling
    for lo in range(0, n_img, step):
        hi = min(lo + step, n_img)
        P = (hi - lo) * n_cls
        ev.add_proposals(boxes[lo * n_cls * n_prop:hi * n_cls * n_prop], np.full(P, n_prop), None,
                         np.repeat(np.arange(lo, hi), n_cls), np.tile(np.arange(n_cls), hi - lo))


def timed(compute, warmup, iters):
    """-> (ms per call by HIP events [iters], the last result)"""
    for _ in range(warmup):
        res = compute()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(iters):
        e0.record()
        res = compute()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return np.asarray(times), res


def synthetic_model_table(dev):
    """a small synthetic eval model, a sweep over three cached support sets, its rois through add_rois -> AR [2,L,A]"""
    from dana_amd import synthetic as S
    m = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=True, way=1, shot=2, classes=["fg", "bg"])
    m.load_state_dict(S.fill_state_dict(m.state_dict(), seed=11, profile="test"))
    m.to(dev).eval()
    im, info, gt, nb, _ = [t.to(dev) for t in S.episode_inputs(2, 1, 2, 192, 256, seed=1996)]
    sup = S.episode_inputs(3, 1, 2, 192, 256, seed=7)[4].to(dev)
    ev = E.ProposalRecallEvaluator(3, dev, limits=(10, 100, 300), area_ranges=["all", "small", "medium", "large"], others=True)
    with torch.no_grad():
        cache = m.encode_supports(sup.reshape(3, -1, 3, sup.size(-2), sup.size(-1)))
        sweep = cache.sweep()
        rois = m(im, info, gt, nb, sweep)[0]
    ev.add_rois(rois, info, [0, 1], sweep.classes)
    scale = info[:, 2].cpu().numpy()
    for b in range(2):
        k = int(nb[b])
        ev.add_ground_truth(b, gt[b, :k, :4].cpu().numpy() / scale[b], [(b + j) % 3 for j in range(k)])
    res = ev.compute()
    ar = res.ar.cpu().numpy()
    print("synthetic model (random weights): %d lists of %d rois; AR by limit (rows) and area (columns)"
          % (rois.size(0), rois.size(1)))
    for role, name in enumerate(("target", "other")):
        print("  %-6s %8s" % (name, "limit") + "".join("%9s" % n for n in res.area_names))
        for li, lim in enumerate(res.limits):
            print("  %-6s %8d" % ("", lim) + "".join("%9.4f" % v for v in ar[role, li]))
    return {"limits": [int(x) for x in res.limits], "areas": list(res.area_names),
            "ar_target": np.round(ar[0], 6).tolist(), "ar_other": np.round(ar[1], 6).tolist()}


def no_nan(x):
    """NaN (a range or role without objects) -> null: the line stays strict JSON"""
    if isinstance(x, dict):
        return {k: no_nan(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [no_nan(v) for v in x]
    return None if isinstance(x, float) and x != x else x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--proposals", type=int, default=300)
    ap.add_argument("--no-others", action="store_true", help="target units only")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-scale", type=float, default=0.1, help="share of the images the host route runs on (0: skip)")
    ap.add_argument("--no-model", action="store_true", help="skip the synthetic model's AR table")
    ap.add_argument("--profile-run", action="store_true", help="five compute() calls and nothing else (for rocprofv3)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("proposal_recall_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    others = not a.no_others
    data = make(a.images, a.classes, a.proposals, dev)
    ev = E.ProposalRecallEvaluator(a.classes, dev, others=others)
    fill(ev, *data, a.images, a.classes, a.proposals)
    tb = ev.tables()
    if a.profile_run:
        for _ in range(5):
            res = ev.compute()
        torch.cuda.synchronize()
        print(json.dumps(no_nan({"profile_run": True, "units": int(tb["unit_tab"].shape[0]), "pairs": tb["n_pairs"],
                                 "ar_target_all": res.ar[0, :, 0].cpu().tolist()})))
        return
    out = {}
    if not a.no_model:
        out["synthetic_model"] = synthetic_model_table(dev)
    times, res = timed(ev.compute, a.warmup, a.iters)
    T, L, A = len(ev.params[0]), len(ev.params[1]), len(ev.params[2])
    # compute() by part: the host tables (numpy), then the C call alone (both launches) on tables already uploaded
    t0 = time.perf_counter()
    for _ in range(5):
        ev.tables()
    tables_ms = (time.perf_counter() - t0) / 5 * 1e3
    U, g = tb["unit_tab"].shape[0], tb["gt_order"].size
    small = torch.from_numpy(np.concatenate((tb["unit_tab"].reshape(-1), tb["gt_order"]))).to(dev)
    gbox, garea, _, _ = ev._ground_truth()
    call = lambda: E.eval_proposal_recall(ev.proposals()[0], small[:9 * U].view(U, 9), gbox, garea, small[9 * U:],
                                          tb["n_pairs"], a.classes, *ev._params_dev)
    ctimes, _ = timed(call, a.warmup, a.iters)
    out.update(images=a.images, classes=a.classes, proposals_per_list=a.proposals, rows=ev.num_rows,
               ground_truth=int(data[1].shape[0]), others=others, units=int(tb["unit_tab"].shape[0]), pairs=tb["n_pairs"],
               thresholds=T, limits=[int(x) for x in ev.params[1]], area_ranges=A,
               compute_ms_median=float(np.median(times)), compute_ms_min=float(times.min()),
               compute_ms_p90=float(np.percentile(times, 90)), iters=a.iters, warmup=a.warmup,
               host_tables_ms=tables_ms, c_call_ms_median=float(np.median(ctimes)),
               workspace_MiB=E.lib().query("dana_eval_proposal_recall_workspace_bytes", ev.num_rows, tb["unit_tab"].shape[0],
                                           tb["n_pairs"], T, L, A) / 2 ** 20,
               ar_target=np.round(res.ar[0].cpu().numpy(), 6).tolist(), ar_other=np.round(res.ar[1].cpu().numpy(), 6).tolist(),
               selectivity_all=np.round(res.selectivity()[:, 0].cpu().numpy(), 4).tolist())
    if a.host_scale > 0:
        hi = max(int(a.images * a.host_scale), 1)
        small = make(hi, a.classes, a.proposals, dev, seed=1)
        ev_small = E.ProposalRecallEvaluator(a.classes, dev, others=others)
        fill(ev_small, *small, hi, a.classes, a.proposals)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows, p_img, p_cls, cnt, off = ev_small.proposals()
        rows = rows.cpu().numpy()  # what the code without the evaluator has to do
        t1 = time.perf_counter()
        ref = E.proposal_recall_numpy(rows, p_img, p_cls, cnt, off, small[1], small[2], small[3], a.classes,
                                      limits=E.RECALL_LIMITS, others=others)
        t2 = time.perf_counter()
        got = ev_small.compute()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        st, _ = timed(ev_small.compute, 3, 10)
        same = bool(np.array_equal(got.hits.cpu().numpy(), ref["hits"]) and np.array_equal(got.npos.cpu().numpy(), ref["npos"])
                    and np.array_equal(got.ov.cpu().numpy(), ref["ov"]))
        out.update(host_images=hi, host_rows=int(rows.shape[0]), host_d2h_s=t1 - t0, host_numpy_s=t2 - t1,
                   device_same_size_wall_s=t3 - t2, device_same_size_ms_median=float(np.median(st)),
                   host_equals_device=same)
    print(json.dumps(no_nan(out)), flush=True)


if __name__ == "__main__":
    main()
