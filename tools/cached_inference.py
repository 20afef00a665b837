"""Cached-support inference (DAnARCNN.encode_supports + the cached forward) against the uncached eval forward, at BASELINE
configs[0]'s eval shape (query 600x1000, 3 supports of 320x320, BA block on).

    python tools/cached_inference.py [--steps 20]

Reports ms per QUERY IMAGE, each the best of eager and launch-program replay (+ hipGraph where the forward supports it: the
uncached one), timed as bench.py's trial(): 3 warm steps, then the median GPU-side interval between consecutive steps:
  uncached_b1            the eval forward, B = 1 (bench.py's eval_b1 shape)
  cached_b1              the cached forward, B = 1, C = 1
  cached_b4_mixed        the cached forward, B = 4 over C = 4 sets, index [2, 0, 3, 0]
  *_pp_loop / *_pp_batched   the last two plus post-processing: the per-image postprocess.detections() loop (one C call +
                         one D2H read per image) vs postprocess.detections_batched() (one call, one read)
plus contraction launches per step (ops.PROFILE, single stream), the gather launch alone, and encode_supports per set.
Class sweep (cache.sweep: every image against C sets, the query trunk once per image), C = 5 sets, each against the
replicated B*C cached forward (cache.select(classes * B), every image repeated C times) in the same rounds, alternated:
  sweep_b1_c5 / repl_b1_c5   one image x 5 sets       sweep_b4_c5 / repl_b4_c5   four images x 5 sets
reported as ms per (image, class), with their contraction launches and the RPN conv's launches (the split conv's two
against the single cin-2048 conv). --only-sweep skips the other cases.
--model meta | fsod | fgn: the sibling detector instead (eager only: launch programs and hipGraphs replay DAnA), C = 5
sets, B = 1 and 4, in ms per (image, class), all four in the same rounds, alternated:
  uncached   the eval forward of B images, image b against set b % C's support images (one class per image)
  cached     the cached forward of the same B images and sets (cache.select)
  repl       the replicated cached forward: B*C images, every image against every set
  sweep      cache.sweep(all C sets): B images x C sets
with their contraction launches per step (ops.PROFILE).
The last line is the JSON record."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def median_interval(marks):
    iv = [a.elapsed_time(b) for a, b in zip(marks[:-1], marks[1:])]
    return statistics.median(iv) if iv else None


def trial(fn, k):
    """bench.py's trial(): ms per step of k steps, the median GPU-side interval between consecutive steps"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True)]
    marks[0].record()
    for _ in range(k):
        fn()
        marks.append(torch.cuda.Event(enable_timing=True))
        marks[-1].record()
    torch.cuda.synchronize()
    return median_interval(marks)


def best_of(cands, k):
    """{mode: fn} -> ({mode: ms per step}, best mode): two interleaved rounds, the better one counts per mode"""
    ms = {n: 1e30 for n in cands}
    for _ in range(2):
        for n, fn in cands.items():
            ms[n] = min(ms[n], trial(fn, k))
    return {n: round(v, 4) for n, v in ms.items()}, min(ms, key=ms.get)


def sweep_cases(m, in1, in4, sets5, k):
    from dana_amd import ops
    from dana_amd.program import ProgramDAnA
    C = sets5.size(0)
    cache = m.encode_supports(sets5)
    classes = list(range(C))
    out = {}
    for B, inp in ((1, in1), (4, in4)):
        q = inp[:4]
        rq = [t.repeat_interleave(C, 0) for t in q]
        sw = cache.sweep(classes)
        cache.select(classes * B)

        def repl(rq=rq):
            return m(*rq, cache)

        def swp(q=q, sw=sw):
            return m(*q, sw)

        # contraction launches and the RPN conv's launches (single stream, ops.PROFILE)
        m._single_stream = True
        prof = {}
        for name, call in (("sweep", swp), ("repl", repl)):
            call()
            ops.PROFILE = []
            call()
            torch.cuda.synchronize()
            rpn = [(e[0], round(e[2].elapsed_time(e[3]) * 1e3, 1)) for e in ops.PROFILE
                   if e[0].startswith(("wino3x3", "conv3x3")) and " N=512 " in e[0]
                   and (" K=%d " % (9 * 1024) in e[0] or " K=%d " % (9 * 2048) in e[0])]
            prof[name] = dict(contraction_launches=len(ops.PROFILE), rpn_conv_launches_us=rpn)
            ops.PROFILE = None
        m._single_stream = False
        p_sw = ProgramDAnA(m, *q, sw)
        p_re = ProgramDAnA(m, *rq, cache)
        ms, _ = best_of({"sweep_eager": swp, "sweep_program": lambda: p_sw(*p_sw.inputs),
                         "repl_eager": repl, "repl_program": lambda: p_re(*p_re.inputs)}, k)
        for name in ("sweep", "repl"):
            best = min(("eager", "program"), key=lambda mode: ms["%s_%s" % (name, mode)])
            tag = "%s_b%d_c%d" % (name, B, C)
            out[tag] = dict(ms_per_image_class=round(ms["%s_%s" % (name, best)] / (B * C), 4), mode=best,
                            ms_per_step={mode: ms["%s_%s" % (name, mode)] for mode in ("eager", "program")}, **prof[name])
            print("%-14s %8.3f ms per (image, class)  (best: %s; ms/step %s; %d contraction launches)"
                  % (tag, out[tag]["ms_per_image_class"], best, out[tag]["ms_per_step"], prof[name]["contraction_launches"]),
                  flush=True)
        del p_sw, p_re
    return out


def sibling_cases(m, name, in1, in4, sets5, k):
    """the four cases of a sibling detector (module docstring) at B = 1 and 4 -> {case_bB_cC: record}"""
    from dana_amd import ops
    C = sets5.size(0)
    classes = list(range(C))
    cache_sel = m.encode_supports(sets5)  # (one cache per selection: select() between steps would copy the index)
    cache_rep = m.encode_supports(sets5)
    extra = (lambda q: [q[2]]) if name == "meta" else (lambda q: [])  # meta: all_cls_gt_boxes (meta.py:48,65)
    out = {}
    for B, inp in ((1, in1), (4, in4)):
        q = inp[:4]
        rq = [t.repeat_interleave(C, 0) for t in q]
        sel = [b % C for b in range(B)]
        sup = sets5[sel].contiguous()
        cache_sel.select(sel)
        cache_rep.select(classes * B)
        sw = cache_sel.sweep(classes)
        cases = {"uncached": (B, lambda q=q, sup=sup: m(*q, sup, *extra(q))),
                 "cached": (B, lambda q=q: m(*q, cache_sel, *extra(q))),
                 "repl": (B * C, lambda rq=rq: m(*rq, cache_rep, *extra(rq))),
                 "sweep": (B * C, lambda q=q, sw=sw: m(*q, sw, *extra(q)))}
        launches = {}
        for case, (_, fn) in cases.items():
            fn()
            ops.PROFILE = []
            fn()
            torch.cuda.synchronize()
            launches[case] = len(ops.PROFILE)
            ops.PROFILE = None
        ms, _ = best_of({case: fn for case, (_, fn) in cases.items()}, k)
        for case, (n, _) in cases.items():
            tag = "%s_b%d_c%d" % (case, B, C)
            out[tag] = dict(ms_per_image_class=round(ms[case] / n, 4), ms_per_step=ms[case], problems=n,
                            contraction_launches=launches[case])
            print("%-16s %8.3f ms per (image, class)  (%.3f ms/step over %d problems; %d contraction launches)"
                  % (tag, ms[case] / n, ms[case], n, launches[case]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--width", type=int, default=1000)
    ap.add_argument("--only-sweep", action="store_true")
    ap.add_argument("--model", choices=["DAnA", "meta", "fsod", "fgn"], default="DAnA")
    args = ap.parse_args()
    import dana_amd
    from dana_amd import ops, postprocess as PP, synthetic as S
    from dana_amd.graphs import GraphedDAnA
    from dana_amd.program import ProgramDAnA
    dev = torch.device("cuda:0")
    shot, H, W, k = 3, args.height, args.width, args.steps
    if args.model != "DAnA":
        m = dana_amd.get_model(args.model, pretrained=False, way=1, shot=shot, classes=["fg", "bg"])
        tame = {"fsod": S.tame_fsod_weights, "fgn": S.tame_fgn_weights}.get(args.model, lambda sd_: sd_)
        m.load_state_dict(tame(S.fill_state_dict(m.state_dict(), seed=5, profile="test")))
        m.to(dev).eval()
        in1 = [t.to(dev) for t in S.episode_inputs(1, 1, shot, H, W, seed=9)]
        in4 = [t.to(dev) for t in S.episode_inputs(4, 1, shot, H, W, seed=10)]
        sets5 = torch.cat([in4[4].reshape(4, shot, 3, 320, 320), in1[4].reshape(1, shot, 3, 320, 320)], 0)
        rec = {"model": args.model, "shape": "query %dx%d, shot %d, supports 320x320" % (H, W, shot), "steps": k}
        with torch.no_grad():
            rec["cases"] = sibling_cases(m, args.model, in1, in4, sets5, k)
        print(json.dumps(rec))
        return
    m = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=True, way=1, shot=shot, classes=["fg", "bg"])
    m.load_state_dict(S.fill_state_dict(m.state_dict(), seed=5, profile="test"))
    m.to(dev).eval()
    in1 = [t.to(dev) for t in S.episode_inputs(1, 1, shot, H, W, seed=9)]
    in4 = [t.to(dev) for t in S.episode_inputs(4, 1, shot, H, W, seed=10)]
    sets1 = in1[4].reshape(1, shot, 3, 320, 320)
    sets4 = in4[4].reshape(4, shot, 3, 320, 320)
    rec = {"shape": "query %dx%d, shot %d, supports 320x320, BA on" % (H, W, shot), "steps": k}
    torch.backends.cudnn.benchmark = False
    with torch.no_grad():
        rec["sweep"] = sweep_cases(m, in1, in4, torch.cat([sets4, sets1], 0), k)
    if args.only_sweep:
        print(json.dumps(rec))
        return
    with torch.no_grad():
        cache1 = m.encode_supports(sets1)
        cache4 = m.encode_supports(sets4)
        cache4.select([2, 0, 3, 0])
        rec["cache_mb_per_set"] = round(cache1.nbytes / 1e6, 3)

        # -- contraction launches per step (single stream, ops.PROFILE) --
        m._single_stream = True
        counts = {}
        for name, call in (("uncached_b1", lambda: m(*in1)), ("cached_b1", lambda: m(*in1[:4], cache1)),
                           ("cached_b4_mixed", lambda: m(*in4[:4], cache4))):
            call()
            ops.PROFILE = []
            call()
            torch.cuda.synchronize()
            counts[name] = len(ops.PROFILE)
            ops.PROFILE = None
        m._single_stream = False
        rec["contraction_launches_per_step"] = counts

        # -- ms per query image --
        p_un = ProgramDAnA(m, *in1)
        g_un = GraphedDAnA(m, *in1)
        p_c1 = ProgramDAnA(m, *in1[:4], cache1)
        p_c4 = ProgramDAnA(m, *in4[:4], cache4)
        cases = {
            "uncached_b1": (1, {"eager": lambda: m(*in1), "program": lambda: p_un(*p_un.inputs),
                                "graph": lambda: g_un(*g_un.inputs)}),
            "cached_b1": (1, {"eager": lambda: m(*in1[:4], cache1), "program": lambda: p_c1(*p_c1.inputs)}),
            "cached_b4_mixed": (4, {"eager": lambda: m(*in4[:4], cache4), "program": lambda: p_c4(*p_c4.inputs)}),
        }

        def loop_pp(out, B):
            rois, prob, pred = out[:3]
            R = rois.size(1)
            info = p_c4.inputs[1] if B == 4 else p_c1.inputs[1]
            return [PP.detections(rois[b:b + 1], prob[b * R:(b + 1) * R], pred[b * R:(b + 1) * R], info[b:b + 1])
                    for b in range(B)]

        def batched_pp(out, B):
            info = p_c4.inputs[1] if B == 4 else p_c1.inputs[1]
            return PP.detections_batched(out[0], out[1], out[2], info)

        cases["cached_b1_pp_loop"] = (1, {"program": lambda: loop_pp(p_c1(*p_c1.inputs), 1)})
        cases["cached_b1_pp_batched"] = (1, {"program": lambda: batched_pp(p_c1(*p_c1.inputs), 1)})
        cases["cached_b4_mixed_pp_loop"] = (4, {"program": lambda: loop_pp(p_c4(*p_c4.inputs), 4)})
        cases["cached_b4_mixed_pp_batched"] = (4, {"program": lambda: batched_pp(p_c4(*p_c4.inputs), 4)})
        res = {}
        for name, (B, cands) in cases.items():
            ms, best = best_of(cands, k)
            res[name] = dict(ms_per_image=round(ms[best] / B, 4), mode=best, ms_per_step=ms)
            print("%-28s %8.3f ms/image  (best: %s; ms/step %s)" % (name, ms[best] / B, best, ms), flush=True)
        rec["cases"] = res
        rec["note_graph"] = "GraphedDAnA does not capture the cached forward (it refuses a SupportCache): eager + program"

        # -- the gather alone (B = 4 of 4 sets) and encode_supports per set --
        rec["gather_b4_us"] = round(1e3 * trial(lambda: cache4._gather(4), max(k, 50)), 2)
        rec["gather_b4_mb_moved"] = round(2 * 4 * cache4.nbytes / 4 / 1e6, 3)  # read + written, 4 images
        rec["encode_ms_per_set"] = round(trial(lambda: m.encode_supports(sets4), 5) / 4, 3)
    print("contraction launches per step: %s" % counts)
    print("gather (B = 4, %.1f MB read + written): %.1f us; encode_supports: %.3f ms per set"
          % (rec["gather_b4_mb_moved"], rec["gather_b4_us"], rec["encode_ms_per_set"]))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
