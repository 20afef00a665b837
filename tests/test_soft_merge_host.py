"""CPU suite: Soft-NMS and box voting for merged detection lists (postprocess.merge_detections(method=, vote_thresh=),
csrc/merge.hip). `postprocess.merge_soft_numpy` -- the restatement the GPU tests compare the device against -- does what
the definitions in include/dana_hip.h say on a hand-worked case, equals `merge_numpy` under method="hard", and has the
margins the GPU comparisons rely on for exactly the runs test_gpu_soft_merge.py makes; the entry points are declared,
exported and report argument errors without a GPU."""
import ctypes
import os

import numpy as np
import pytest

import soft_merge_cases as C
from dana_amd import _lib, postprocess as PP

A, B, Cc, D = [0, 0, 9, 9, .9], [0, 0, 9, 4, .8], [0, 5, 9, 9, .7], [20, 20, 29, 29, .6]
WORKED = [np.asarray([A, B, Cc, D], np.float32)]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def test_worked_case():
    """the four boxes of the issue, with its literals: iou(A,B) = iou(A,C) = 0.5, iou(B,C) = 0"""
    assert PP._iou32_rows(A[:4], np.asarray([B[:4], Cc[:4], D[:4]])).tolist() == [0.5, 0.5, 0.0]
    assert PP._iou32_rows(B[:4], np.asarray([Cc[:4]])).tolist() == [0.0]
    hard = PP.merge_soft_numpy(WORKED, 1, 0.3, method="hard")
    assert hard["row"][0].tolist() == [0, 3] and hard["votes"] is None
    lin = PP.merge_soft_numpy(WORKED, 1, 0.3, method="linear", min_score=0.001)
    assert lin["row"][0].tolist() == [0, 3, 1, 2] and lin["group"][0].tolist() == [0, 0, 0, 0]
    assert [float(s) for s in lin["dets"][0][:, 4]] == [0.8999999761581421, 0.6000000238418579, 0.4000000059604645,
                                                        0.3499999940395355]
    assert np.array_equal(lin["dets"][0][:, :4], WORKED[0][[0, 3, 1, 2], :4])  # no voting: the boxes are copies
    assert lin["counts"].tolist() == [4] and lin["offsets"].tolist() == [0, 4]
    for method in ("hard", "linear", "gaussian"):
        v = PP.merge_soft_numpy(WORKED, 1, 0.3, method=method, vote_thresh=0.5)
        assert v["row"][0][:2].tolist() == [0, 3] and v["votes"][0][:2].tolist() == [3, 1]
        assert np.array_equal(v["dets"][0][0, :4], np.asarray([0.0, 1.4583334, 9.0, 7.3333335], np.float32))
        assert np.array_equal(v["dets"][0][1, :4], np.asarray(D[:4], np.float32))
        assert v["margin"]["vote"] == 0.0  # A's voters B and C sit AT the threshold, and >= counts them
    # vote_score="avg": the score becomes the voters' mean original score, (.9 + .8 + .7) / 3 in double, rounded once
    avg = PP.merge_soft_numpy(WORKED, 1, 0.3, method="hard", vote_thresh=0.5, vote_score="avg")
    w = float(np.float32(.9)) + float(np.float32(.8)) + float(np.float32(.7))
    assert avg["dets"][0][:, 4].tolist() == [np.float32(w / 3), np.float32(.6)]
    # gaussian: Nt is not used (None is accepted), every overlapping row decays
    gau = PP.merge_soft_numpy(WORKED, 1, None, method="gaussian", sigma=0.5)
    assert gau["row"][0].tolist() == [0, 3, 1, 2]
    assert gau["dets"][0][2, 4] == np.float32(float(np.float32(.8)) * np.exp(-0.25 / 0.5))


def test_pick_drop_margins_of_the_worked_case():
    m = PP.merge_soft_numpy(WORKED, 1, 0.3, method="linear", min_score=0.001)["margin"]
    # the closest pick is the first: A 0.9 against B 0.8, relative to the best (then D 0.6 / B 0.4, then B 0.4 / C 0.35)
    assert m["pick"] == pytest.approx((0.9 - 0.8) / 0.9, rel=1e-6) and m["vote"] == np.inf
    assert m["drop"] == pytest.approx((0.35 - 0.001) / 0.001, rel=1e-5)
    one = PP.merge_soft_numpy([WORKED[0][:1]], 1, 0.3, method="linear")["margin"]
    assert one == dict(pick=np.inf, drop=np.inf, vote=np.inf)
    # min_score between the decayed scores: C (0.35) is dropped in the middle of the loop, B (0.4) is emitted
    r = PP.merge_soft_numpy(WORKED, 1, 0.3, method="linear", min_score=0.375)
    assert r["row"][0].tolist() == [0, 3, 1]


def _golden_lists(golden_dir):
    g = np.load(os.path.join(golden_dir, "merge_dets.npz"))
    for i in range(int(g["n_cases"])):
        counts = g["c%d_counts" % i]
        yield np.split(g["c%d_dets" % i], np.cumsum(counts)[:-1]), float(g["nms_thresh"])


def _assert_same_merge(soft, ref):
    assert soft["counts"].tolist() == ref["counts"].tolist() and soft["offsets"].tolist() == ref["offsets"].tolist()
    assert soft["counts"].dtype == np.int32 and soft["offsets"].dtype == np.int32
    for l in range(len(ref["dets"])):
        assert np.array_equal(_bits(soft["dets"][l]), _bits(ref["dets"][l])), l
        assert soft["group"][l].tolist() == ref["group"][l].tolist() and soft["row"][l].tolist() == ref["row"][l].tolist()


def test_hard_method_is_merge_numpy(golden_dir):
    n = 0
    for lists, thr in _golden_lists(golden_dir):
        for inclusive in (False, True):
            ref = PP.merge_numpy(lists, len(lists), thr, inclusive)
            assert ref["margin"] >= 1e-4
            _assert_same_merge(PP.merge_soft_numpy(lists, len(lists), thr, inclusive, method="hard"), ref)
            n += 1
    assert n >= 6
    for name, (lists, groups) in C.CASES.items():
        for thr, inclusive, max_dets in ((C.THR, False, 0), (C.THR, True, 0), (C.THR, False, 7), (None, False, 0), (None, False, 7)):
            ref = PP.merge_numpy(lists, groups, thr, inclusive, max_dets)
            if name != "scattered":  # (random IoUs: the float64 margin is whatever it is, and still the two agree)
                assert ref["margin"] >= 1e-4, name
            soft = PP.merge_soft_numpy(lists, groups, thr, inclusive, max_dets, method="hard")
            _assert_same_merge(soft, ref)
            assert soft["votes"] is None and soft["margin"] == dict(pick=np.inf, drop=np.inf, vote=np.inf)


@pytest.mark.parametrize("method", ["hard", "linear", "gaussian"])
def test_emitted_scores_never_increase(method):
    for case in C.CASES:
        for vote in (False, True):
            if case in C.LONG and method == "gaussian":
                continue  # (the per-row Python loop of the Gaussian decay: not run on 600 rows by the GPU file either)
            ref = C.reference(case, method, vote)
            for d in ref["dets"]:
                assert np.all(np.diff(d[:, 4]) <= 0), (case, vote)


def test_lone_voter_keeps_its_coordinates_bit_for_bit():
    """a row whose only voter is itself: X_c / W = (s * x) / s, which is x again only because the division is exact in double
    for float32 inputs (24 + 24 significand bits fit in 53) -- the emitted coordinates must be the input's own bits"""
    rng = np.random.RandomState(5)
    far = np.zeros((40, 5), np.float32)
    far[:, 0] = 1000.0 * np.arange(40) + rng.uniform(0, 1, 40)
    far[:, 1] = rng.uniform(0, 777, 40)
    far[:, 2] = far[:, 0] + rng.uniform(3, 300, 40).astype(np.float32)
    far[:, 3] = far[:, 1] + rng.uniform(3, 300, 40).astype(np.float32)
    far[:, 4] = rng.uniform(0.01, 1, 40)
    far = far[np.argsort(-far[:, 4], kind="stable")]
    for method in ("hard", "linear", "gaussian"):
        r = PP.merge_soft_numpy([far], 1, 0.3, method=method, vote_thresh=0.5)
        assert r["votes"][0].tolist() == [1] * 40
        assert np.array_equal(_bits(r["dets"][0]), _bits(far))
    # ... and D of the worked case
    v = PP.merge_soft_numpy(WORKED, 1, 0.3, method="linear", vote_thresh=0.5)
    assert v["votes"][0].tolist() == [3, 1, 2, 2] and np.array_equal(_bits(v["dets"][0][1]), _bits(WORKED[0][3]))


def test_margins_of_the_gpu_inputs():
    """what makes the GPU file's Gaussian tolerance and discrete equalities meaningful: for every run it makes under
    `gaussian` or with voting, no pick and no removal decision is closer than 1e-4 (relative)"""
    checked = 0
    for case, method, vote, variant, vote_score in C.runs():
        if not C.needs_margin(method, vote):
            continue
        m = C.reference(case, method, vote, variant, vote_score)["margin"]
        assert m["pick"] >= C.MARGIN and m["drop"] >= C.MARGIN, (case, method, vote, variant, m)
        L = max(sum(len(q) for q in C.CASES[case][0][i:i + C.CASES[case][1]])
                for i in range(0, len(C.CASES[case][0]), C.CASES[case][1]))
        assert method != "gaussian" or L <= 80, (case, L)
        checked += 1
    assert checked >= 40


def test_cases_cover_what_they_claim():
    lens = lambda name: [sum(len(q) for q in C.CASES[name][0][i:i + C.CASES[name][1]])  # noqa: E731
                         for i in range(0, len(C.CASES[name][0]), C.CASES[name][1])]
    assert lens("edges") == [0, 1, 2, 63, 64, 65] and lens("long") == [255, 256, 257, 600] and lens("long_groups") == [600, 3]
    assert lens("empty_between") == [14, 0, 70] and lens("empty_middle_group") == [70] and len(C.CASES["empty_middle_group"][0][1]) == 0
    # "drop": rows whose input score was above min_score are removed after a decay, under both soft methods
    for method in ("linear", "gaussian"):
        for case in C.SMALL:
            ref = C.reference(case, method, False, "drop")
            lists, groups = C.CASES[case]
            above = sum(int((q[:, 4] >= 0.05).sum()) for q in lists)
            assert 0 < int(ref["counts"].sum()) < above, (case, method)
    # "max7" cuts inside a list, "max1000" cuts nothing
    assert C.reference("edges", "linear", True, "max7")["counts"].tolist() == [0, 1, 2, 7, 7, 7]
    assert C.reference("edges", "linear", False, "max1000")["counts"].tolist() == C.reference("edges", "linear")["counts"].tolist()
    # the tie rule decides: equal input scores, and B / C decayed to one working score come out in concatenation order
    tie = C.reference("decayed_tie", "linear")
    assert tie["dets"][0][:, 4].tolist() == tie["dets"][1][:, 4].tolist() and tie["dets"][0][2, 4] == tie["dets"][0][3, 4]
    assert list(zip(tie["group"][0].tolist(), tie["row"][0].tolist())) == [(0, 0), (1, 1), (0, 1), (1, 0)]
    assert list(zip(tie["group"][1].tolist(), tie["row"][1].tolist())) == [(0, 0), (1, 1), (0, 1), (1, 0)]
    assert C.reference("decayed_tie", "linear")["margin"]["pick"] == 0.0
    eq = C.reference("equal_scores", "linear")
    g, r, s = eq["group"][0], eq["row"][0], eq["dets"][0][:, 4]
    assert any(s[i] == s[i + 1] for i in range(len(s) - 1))
    for i in range(len(s) - 1):
        if s[i] == s[i + 1]:
            assert (g[i], r[i]) < (g[i + 1], r[i + 1])


def test_argument_errors_are_value_errors_before_any_c_call():
    p = None  # (never looked at: the keywords are checked first)
    for fn in (lambda **kw: PP.merge_detections(p, 1, **kw), lambda **kw: PP.merge_soft_numpy(WORKED, 1, kw.pop("nms_thresh", 0.3), **kw)):
        with pytest.raises(ValueError, match="method"):
            fn(method="soft")
        with pytest.raises(ValueError, match="vote_score"):
            fn(vote_score="max")
        with pytest.raises(ValueError, match="linear"):
            fn(method="linear", nms_thresh=None)
        for sigma in (0.0, -1.0):
            with pytest.raises(ValueError, match="sigma"):
                fn(method="gaussian", sigma=sigma)
        for vt in (0.0, -0.5, 1.5):
            with pytest.raises(ValueError, match="vote_thresh"):
                fn(vote_thresh=vt)
    with pytest.raises(ValueError, match="method"):
        PP.ensemble_shots(p, 3, method="soft")


def test_header_declares_and_library_exports_the_soft_entry_points():
    protos = _lib.parse_header()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("dana_detect_merge_soft_workspace_bytes", "dana_detect_merge_soft"):
        assert name in protos and hasattr(cdll, name), name
    args = [a for _, a in protos["dana_detect_merge_soft"][1]]
    merge_args = [a for _, a in protos["dana_detect_merge"][1]]
    assert set(merge_args) < set(args)
    assert set(args) - set(merge_args) == {"method", "sigma", "min_score", "vote_thresh", "vote_score", "votes_out"}
    assert _lib.lib().query("dana_abi_version") == 1  # the change is additive


def test_soft_argument_and_resource_errors_are_reported_without_a_gpu():
    L = _lib.lib()
    q = lambda *a: L.query("dana_detect_merge_soft_workspace_bytes", *a)  # noqa: E731
    assert q(0, 2, 100) == 0 and q(3, 2, 0) == 0 and q(2, 4, 600) == L.query("dana_detect_merge_workspace_bytes", 2, 4, 600) > 0
    p = 16  # (never dereferenced: every call below returns before its first launch)
    call = lambda cap, method, vt, nb, sigma=0.5, vs=0, n_lists=1: L.call(  # noqa: E731
        "dana_detect_merge_soft", p, p, p, n_lists, 2, cap, 1, 0.3, 0, 0, method, sigma, 0.001, vt, vs, p, p, p, p, p, p, p, nb, None)
    with pytest.raises(_lib.DanaError, match="bad method 3"):
        call(10, 3, -1.0, 1 << 30)
    with pytest.raises(_lib.DanaError, match="vote_score 2"):
        call(10, 1, 0.5, 1 << 30, vs=2)
    with pytest.raises(_lib.DanaError, match="sigma"):
        call(10, 2, -1.0, 1 << 30, sigma=0.0)
    with pytest.raises(_lib.DanaError, match="vote_thresh"):
        call(10, 1, 1.5, 1 << 30)
    with pytest.raises(_lib.DanaError, match="bad shape"):
        call(10, 1, -1.0, 1 << 30, n_lists=-1)
    # the soft loop holds a list in LDS, 21 bytes per row: 3072 rows fit, 3073 are an error and never a launch
    with pytest.raises(_lib.DanaError, match="capacity 3073 above the 3072 rows the soft-NMS kernel holds in LDS"):
        call(3073, 1, -1.0, 1 << 30)
    with pytest.raises(_lib.DanaError, match="capacity 3073 above the 3072 rows"):
        call(3073, 2, 0.5, 1 << 30)
    with pytest.raises(_lib.DanaError, match=r"dana_detect_merge_soft: workspace \d+ < \d+"):
        call(3072, 1, -1.0, q(1, 2, 3072) - 1)
    # the hard method (with voting: chunked, no LDS bound) keeps dana_detect_merge's bound
    with pytest.raises(_lib.DanaError, match=r"dana_detect_merge_soft: workspace \d+ < \d+"):
        call(3073, 0, 0.5, q(1, 2, 3073) - 1)
    with pytest.raises(_lib.DanaError, match="above the 520064 rows dana_nms takes"):
        call(520065, 0, 0.5, 1 << 30)
