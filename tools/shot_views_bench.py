"""Shot views of a cached support set (SupportCache.sweep(shots=...)) against the routes they replace, at the shape of
profiles/class_sweep.md: query 600x1000, shot 3, C = 5 cached sets, one image, BA block on, synthetic weights.

    python tools/shot_views_bench.py [--steps 10]

Reports ms per (image, view), timed as bench.py's trial() (3 warm steps, then the median GPU-side interval between
consecutive steps; two interleaved rounds, the better one counts), eager and launch-program replay:
  each_3shot_cache   (a) cache.sweep(shots="each") on the 3-shot cache: 15 one-shot problems, gathered shot block by block
  oneshot_model      (b) the route documented before: a num_shot=1 model with the same weights, the 15 shots encoded as
                     15 one-shot sets, cache1.sweep()
                     (a) and (b) alternate in the same rounds of one process
  mixed_lengths      (c) a sweep of the 5 classes with views of lengths 1, 2, 3, 1, 2 (m = 3: per-segment softmax scales,
                     padding slots attended and scaled by 0) ...
  uniform_m3         ... against the same 5 problems' sets at uniform length 3 (views (0, 1, 2) in another order, so the
                     shot gather runs here too) and
  uniform_m1 / _m2   the K-shot protocol's sweep(shots=k): what the short views cost when they run alone
plus the gather launches alone, back to back (dana_gather_shot_blocks for (a) and (c), dana_gather_blocks for (b)):
interval per launch, bytes read + written, and the share of --hbm-gbs (default 6300: what a plain float4 copy achieves on this chip, 79 % of the 8 TB/s
data-sheet peak; the share is of the achievable figure).
The last line is the JSON record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cached_inference import best_of, trial  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--width", type=int, default=1000)
    ap.add_argument("--hbm-gbs", type=float, default=6300.0)
    args = ap.parse_args()
    import dana_amd
    from dana_amd import ops, synthetic as S
    from dana_amd._lib import lib
    from dana_amd.program import ProgramDAnA
    dev = torch.device("cuda:0")
    shot, C, H, W, k = 3, 5, args.height, args.width, args.steps

    def model(n_shot):
        m_ = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=True, way=1, shot=n_shot, classes=["fg", "bg"])
        m_.load_state_dict(S.fill_state_dict(m_.state_dict(), seed=5, profile="test"))
        return m_.to(dev).eval()

    m3, m1 = model(shot), model(1)
    q = [t.to(dev) for t in S.episode_inputs(1, 1, shot, H, W, seed=9)][:4]
    sets = torch.cat([t.to(dev) for t in (S.episode_inputs(4, 1, shot, H, W, seed=10)[4].reshape(4, shot, 3, 320, 320),
                                          S.episode_inputs(1, 1, shot, H, W, seed=9)[4].reshape(1, shot, 3, 320, 320))], 0)
    rec = {"shape": "query %dx%d, shot %d, C = %d sets, supports 320x320, BA on, one image" % (H, W, shot, C), "steps": k}
    with torch.no_grad():
        cache3 = m3.encode_supports(sets)
        cache1 = m1.encode_supports(sets.reshape(C * shot, 1, 3, 320, 320))
        sw_each = cache3.sweep(shots="each")
        sw_one = cache1.sweep()
        mixed_views = [(0,), (0, 1), (0, 1, 2), (0,), (0, 1)]
        sw_mixed = cache3.sweep(shots=mixed_views)
        sw_m3 = cache3.sweep(shots=(2, 1, 0))
        sw_m1, sw_m2 = cache3.sweep(shots=1), cache3.sweep(shots=2)

        # (a) against (b): the same 15 (class, shot) problems
        p_each, p_one = ProgramDAnA(m3, *q, sw_each), ProgramDAnA(m1, *q, sw_one)
        ms, _ = best_of({"each_eager": lambda: m3(*q, sw_each), "each_program": lambda: p_each(*p_each.inputs),
                         "one_eager": lambda: m1(*q, sw_one), "one_program": lambda: p_one(*p_one.inputs)}, k)
        cases = {}
        for tag, key in (("each_3shot_cache", "each"), ("oneshot_model", "one")):
            best = min(("eager", "program"), key=lambda mode: ms["%s_%s" % (key, mode)])
            cases[tag] = dict(ms_per_image_view=round(ms["%s_%s" % (key, best)] / (C * shot), 4), mode=best, views=C * shot,
                              ms_per_step={mode: ms["%s_%s" % (key, mode)] for mode in ("eager", "program")})
        del p_each, p_one

        # (c): mixed lengths against uniform lengths
        progs = {n: ProgramDAnA(m3, *q, sw) for n, sw in (("mixed_lengths", sw_mixed), ("uniform_m3", sw_m3),
                                                          ("uniform_m2", sw_m2), ("uniform_m1", sw_m1))}
        sweeps = dict(mixed_lengths=sw_mixed, uniform_m3=sw_m3, uniform_m2=sw_m2, uniform_m1=sw_m1)
        cands = {}
        for n, sw in sweeps.items():
            cands[n + "_eager"] = lambda sw=sw: m3(*q, sw)
            cands[n + "_program"] = lambda p=progs[n], sw=sw: p(*p.inputs[:4], sw)
        ms, _ = best_of(cands, k)
        for n in sweeps:
            best = min(("eager", "program"), key=lambda mode: ms["%s_%s" % (n, mode)])
            cases[n] = dict(ms_per_image_view=round(ms["%s_%s" % (n, best)] / C, 4), mode=best, views=C,
                            ms_per_step={mode: ms["%s_%s" % (n, mode)] for mode in ("eager", "program")})
        cases["mixed_lengths"]["view_lengths"] = [len(v) for v in mixed_views]
        cases["mixed_lengths"]["padding_slots_of"] = "%d of %d" % (sum(3 - len(v) for v in mixed_views), 3 * C)
        del progs
        for tag, c_ in cases.items():
            print("%-18s %8.3f ms per (image, view)  (%d views; best: %s; ms/step %s)"
                  % (tag, c_["ms_per_image_view"], c_["views"], c_["mode"], c_["ms_per_step"]), flush=True)
        rec["cases"] = cases

        # the gathers alone. Bytes: what the launch reads plus what it writes (a padding slot is written, not read)
        per_shot = cache3.nbytes // (C * shot)
        gathers = {}
        for tag, cache, idx, views, rd_shots, wr_shots in (
                ("each_shot_gather_p15_m1", cache3, sw_each._index(1), sw_each._views(1), 15, 15),
                ("mixed_shot_gather_p5_m3", cache3, sw_mixed._index(1), sw_mixed._views(1), sum(map(len, mixed_views)), 15),
                ("oneshot_set_gather_p15", cache1, sw_one._index(1), None, 15, 15)):
            cache._gather_views(len(idx), idx, views)  # (index and view table written, buffers allocated)
            st = ops._stream()
            if views is None:  # the launch alone: the cache's own host work would hide a 15 us kernel
                _, tab, n = cache._bufs[len(idx)]
                call = ("dana_gather_blocks", tab[0].data_ptr(), tab[1].data_ptr(), tab[2].data_ptr(), n,
                        cache._index.data_ptr(), len(cache), len(idx), st)
            else:
                m_ = max(map(len, views))
                _, tab, n, w = cache._vbufs[(len(idx), m_)]
                call = ("dana_gather_shot_blocks", tab[0].data_ptr(), tab[1].data_ptr(), tab[2].data_ptr(), tab[3].data_ptr(),
                        n, cache._index.data_ptr(), cache._view.data_ptr(), w.data_ptr(), len(cache), cache.shot, m_,
                        len(idx), st)
            us = 1e3 * trial(lambda: lib().call(*call), max(k, 200))
            mb = (rd_shots + wr_shots) * per_shot / 1e6
            gathers[tag] = dict(us=round(us, 2), mb_read_plus_written=round(mb, 3), gb_per_s=round(mb / us * 1e3, 1),
                                share_of_hbm=round(mb / us * 1e3 / args.hbm_gbs, 3))
            print("%-26s %7.1f us, %.1f MB read + written, %.0f GB/s (%.0f %% of %.0f GB/s)"
                  % (tag, us, mb, mb / us * 1e3, 100 * mb / us * 1e3 / args.hbm_gbs, args.hbm_gbs), flush=True)
        rec["gathers"] = gathers
        rec["cache_mb_per_shot"] = round(per_shot / 1e6, 3)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
