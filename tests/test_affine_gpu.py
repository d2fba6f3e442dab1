"""GPU: the batched affine RANSAC (csrc/affine.hip through opp_affine2d_ransac_batch and onepose_plus_plus_amd/detect.py) against the
float64 restatement of tests/affine_reference.py on the case list of tests/affine_cases.py.

The restatement runs once per case and the device once per (iterations, confidence) group, the group's cases being the views of one
call between an empty first view and a 2-match last one.  Sample indices are compared exactly for every case; counts, stop
index, best hypothesis, mask, boxes and the selection exactly for the cases the restatement decides (at most 1 case in 20 may be
undecided); the final map through the displacement it causes at the four image corners, bar 1e-6 px where the refit's (or, without
a refit, the sample's) centred design matrix has a condition number <= 1e3: a float64 normal-equation solve on centred pixel
coordinates is estimated at about 1e-8 px, the bar leaves two orders over that."""
import numpy as np
import pytest
import torch

from tests import affine_cases as AC
from tests import affine_ops as AO
from tests import affine_reference as AR
from tests import hip_ops as ops

pytestmark = pytest.mark.gpu

CORNERS = AC.corners_of(AC.REF_HW)
AFFINE_BAR_PX = 1e-6


def corner_gap(A, B):
    return float(np.abs((CORNERS @ A[:, :2].T + A[:, 2]) - (CORNERS @ B[:, :2].T + B[:, 2])).max())


def compare_groups(cases):
    """-> list of per-case dicts: ref (restatement), dev (the view's device outputs), group results"""
    rows = [None] * len(cases)
    tiny = AC.scene(999, 2, 0.0)
    for (iters, conf), members in AC.groups(cases).items():
        scenes = [AC.scene(cases[i][4], cases[i][0], cases[i][1]) for i in members]
        views = [(np.zeros((0, 2)), np.zeros((0, 2)))] + [(s[0], s[1]) for s in scenes] + [(tiny[0], tiny[1])]
        seeds = [1] + [cases[i][5] for i in members] + [2]
        corners = np.tile(CORNERS, (len(views), 1, 1))
        ref, best_view, best_box, n_tied = AR.estimate_batch(views, seeds, iters, AC.THR, conf, True, corners, AC.FALLBACK)
        dev = AO.run_raw(views, seeds, iters, conf, True, corners, AC.FALLBACK)
        off = AO.concat(views)[2]
        group = {"ref_best_view": best_view, "ref_best_box": best_box, "dev_best_view": int(dev["best_view"][0]),
                 "dev_best_box": dev["best_box"].numpy(), "undecided": any(r["undecided"] for r in ref), "ref": ref, "dev": dev}
        for k, i in enumerate(members):
            v = k + 1
            rows[i] = {"case": cases[i], "ref": ref[v], "group": group,
                       "dev": {"samples": dev["samples"][v].numpy(), "scores": dev["scores"][v].numpy(), "stop": int(dev["stop"][v]),
                               "ok": int(dev["ok"][v]), "n_inliers": int(dev["n_inliers"][v]), "box": dev["boxes"][v].numpy(),
                               "affine": dev["affine"][v].numpy(), "mask": dev["mask"][off[v]:off[v + 1]].numpy()}}
    return rows


@pytest.fixture(scope="module")
def rows():
    return compare_groups(AC.GPU_CASES)


def test_sample_indices_equal_the_restatement(rows):
    for r in rows:
        assert np.array_equal(r["dev"]["samples"], r["ref"]["samples"]), r["case"]


def test_decided_cases_equal_the_restatement(rows):
    skipped = 0
    for r in rows:
        ref, dev = r["ref"], r["dev"]
        if ref["undecided"]:
            skipped += 1
            continue
        assert np.array_equal(dev["scores"], ref["scores"]), r["case"]
        assert dev["stop"] == ref["stop"], (r["case"], dev["stop"], ref["stop"])
        head = dev["scores"][:dev["stop"]]
        best = int(np.argmax(head)) if head.size and head.max() > 2 else -1       # the lowest index of the largest count
        assert best == ref["best"], (r["case"], best, ref["best"])
        assert (dev["ok"], dev["n_inliers"]) == (ref["ok"], ref["n_inliers"]), r["case"]
        assert np.array_equal(dev["mask"], ref["mask"]), r["case"]
        assert np.array_equal(dev["box"], ref["box"]), (r["case"], dev["box"], ref["box"])
    print("undecided: %d of %d" % (skipped, len(rows)))
    assert skipped * 20 <= len(rows), skipped
    groups = {id(r["group"]): r["group"] for r in rows}.values()
    for g in groups:
        ref, dev = g["ref"], g["dev"]
        for v in (0, len(ref) - 1):                                                # the empty first view and the 2-match last one
            assert (int(dev["ok"][v]), int(dev["n_inliers"][v]), int(dev["stop"][v])) == (0, 0, 0)
            assert dev["boxes"][v].tolist() == list(AC.FALLBACK) and np.array_equal(dev["affine"][v].numpy(), np.eye(3)[:2])
            assert (dev["samples"][v] == -1).all() and (dev["scores"][v] == -1).all()
        assert dev["mask"][-2:].tolist() == [0, 0]
        if not g["undecided"]:
            assert g["dev_best_view"] == g["ref_best_view"] and np.array_equal(g["dev_best_box"], g["ref_best_box"])


def test_final_map_within_the_bar(rows):
    worst, checked = 0.0, 0
    for r in rows:
        ref, dev = r["ref"], r["dev"]
        if ref["undecided"] or not ref["ok"]:
            continue
        cond = ref["cond"] if ref["cond"] is not None else ref["sample_cond"]
        gap = corner_gap(dev["affine"], ref["affine"])
        print("%s cond %.3g gap %.3e px" % (r["case"], cond, gap))
        if cond <= 1e3:
            checked += 1
            worst = max(worst, gap)
            assert gap <= AFFINE_BAR_PX, (r["case"], cond, gap)
    print("largest corner displacement %.3e px over %d cases" % (worst, checked))
    assert checked >= len(rows) // 2


def _line_view(n):
    x = 15.0 * np.arange(n)
    return np.stack([x, 2 * x + 3], axis=1).astype(np.float32), np.stack([x + 7, 0.5 * x], axis=1).astype(np.float32)


def test_degenerate_inputs_fail_with_the_fallback_box():
    p0, p1, _, _ = AC.scene(3, 40, 0.0)
    same = (p0[:1].repeat(40, 0), p1[:1].repeat(40, 0))
    for views in ([_line_view(40)], [same], [(p0[:2], p1[:2]), (p0[:0], p1[:0]), (p0[:1], p1[:1])], [_line_view(40), same, (p0[:2], p1[:2])]):
        dev = AO.run_raw(views, list(range(len(views))), 64, 0.99)
        V = len(views)
        assert dev["ok"].tolist() == [0] * V and dev["n_inliers"].tolist() == [0] * V and not dev["mask"].any()
        assert dev["boxes"].tolist() == [list(AC.FALLBACK)] * V and int(dev["best_view"][0]) == -1
        assert dev["best_box"].tolist() == list(AC.FALLBACK)
        assert all(np.array_equal(a, np.eye(3)[:2]) for a in dev["affine"].numpy())
        for v, (q0, _) in enumerate(views):
            assert int(dev["stop"][v]) == (64 if q0.shape[0] >= 3 else 0)
            assert (dev["scores"][v] == -1).all()


def _mixed_views(V):
    sizes = {1: [65], 3: [0, 300, 2], 16: [0, 3, 5, 6, 7, 63, 64, 65, 300, 0, 2, 64, 7, 300, 5, 0]}[V]
    views = []
    for k, n in enumerate(sizes):
        p0, p1, _, _ = AC.scene(500 + k, n, (0.0, 0.3, 0.6)[k % 3])
        views.append((p0, p1))
    return views, [11 + 3 * k for k in range(V)]


def _bits(t):
    return t.reshape(-1).contiguous().view(torch.uint8)


def _same_bits(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


@pytest.mark.parametrize("V", [1, 3, 16])
@pytest.mark.parametrize("iters,conf", [(257, 0.99), (64, 1.0)])
def test_batch_equals_singles_bit_for_bit_and_runs_repeat(V, iters, conf):
    views, seeds = _mixed_views(V)
    corners = np.stack([CORNERS * (1.0 + 0.1 * v) for v in range(V)])
    batch = AO.run_raw(views, seeds, iters, conf, True, corners)
    again = AO.run_raw(views, seeds, iters, conf, True, corners)
    assert _same_bits(batch, again)
    off = AO.concat(views)[2]
    counts = []
    for v in range(V):
        one = AO.run_raw([views[v]], [seeds[v]], iters, conf, True, corners[v:v + 1])
        for k in ("affine", "n_inliers", "ok", "stop", "boxes", "samples", "scores"):
            assert torch.equal(_bits(one[k][0]), _bits(batch[k][v])), (v, k)
        assert torch.equal(one["mask"], batch["mask"][off[v]:off[v + 1]]), v
        counts.append(int(one["n_inliers"][0]) if int(one["ok"][0]) else -1)
        assert int(one["best_view"][0]) == (0 if counts[-1] >= 0 else -1)
        assert one["best_box"].tolist() == one["boxes"][0].tolist()
    want = counts.index(max(counts)) if max(counts) >= 0 else -1
    assert int(batch["best_view"][0]) == want
    assert batch["best_box"].tolist() == (batch["boxes"][want].tolist() if want >= 0 else list(AC.FALLBACK))


def test_offsets_that_are_no_segment_make_empty_views_and_touch_nothing_outside():
    p0, p1, _, _ = AC.scene(41, 80, 0.3)
    bufs = ops.GuardedBuffers("nan")
    dev = AO.run_raw([(p0, p1)], [5, 6, 7, 8, 9], 257, 0.99, offsets=[0, 70, 65, 500, -3, 80], bufs=bufs)
    assert bufs.check() == []
    one = AO.run_raw([(p0[:70], p1[:70])], [5], 257, 0.99)
    assert int(dev["ok"][0]) == 1 and dev["ok"][1:].tolist() == [0, 0, 0, 0] and dev["stop"][1:].tolist() == [0, 0, 0, 0]
    for k in ("affine", "n_inliers", "stop", "boxes", "samples", "scores"):
        assert torch.equal(one[k][0], dev[k][0]), k
    assert torch.equal(one["mask"], dev["mask"][:70]) and not dev["mask"][70:].any()          # matches no view covers: written, zero
    assert dev["boxes"][1:].tolist() == [list(AC.FALLBACK)] * 4 and int(dev["best_view"][0]) == 0


def _exact_view(n, seed, scale=0.375, shift=(200.5, 120.5)):
    """noise-free matches of p1 = scale * p0 + shift: every match is an inlier of every non-degenerate hypothesis"""
    rng = np.random.default_rng(seed)
    p0 = np.round(rng.uniform(0, 1, (n, 2)) * np.array([640, 480]) / 8) * 8           # multiples of 8: the map is exact in float32
    return p0.astype(np.float32), (p0 * scale + np.array(shift)).astype(np.float32)


def test_detect_box_picks_the_most_inliers_and_the_first_on_a_tie():
    from onepose_plus_plus_amd import detect_box, estimate_affine_2d
    a, b, c, d = _exact_view(40, 1), _exact_view(80, 2, 0.5, (100.5, 50.5)), _exact_view(80, 3, 0.25, (300.5, 200.5)), _exact_view(5, 4)
    box, view, n_inl = detect_box([a, b, c, d], AC.REF_HW, AC.QUERY_HW)
    assert (view, n_inl) == (1, 80) and box.dtype == np.int32 and box.tolist() == [100, 50, 420, 290]
    box, view, n_inl = detect_box([d, c, a, b], AC.REF_HW, AC.QUERY_HW)
    assert (view, n_inl) == (1, 80) and box.tolist() == [300, 200, 460, 320]
    cuda = [(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()) for x, y in (a, b)]
    box, view, n_inl = detect_box(cuda, [AC.REF_HW, (240, 320)], AC.QUERY_HW)               # per-view image sizes
    assert (view, n_inl) == (1, 80) and box.tolist() == [100, 50, 260, 170]
    box, view, n_inl = detect_box([d, _exact_view(3, 5)], AC.REF_HW, AC.QUERY_HW)           # fewer than 6 matches: no estimate
    assert (view, n_inl) == (-1, 0) and box.tolist() == [640 - 500, 480 - 500, 640 + 500, 480 + 500]
    M, mask = estimate_affine_2d(b[0], b[1])
    assert M.shape == (2, 3) and M.dtype == np.float64 and mask.shape == (80, 1) and mask.dtype == np.uint8 and mask.all()
    assert np.abs(M - np.array([[0.5, 0, 100.5], [0, 0.5, 50.5]])).max() < 1e-9
    M, mask = estimate_affine_2d(*_line_view(30))
    assert M is None and mask.shape == (30, 1) and not mask.any()


def test_front_end_keeps_tensors_on_the_device():
    from onepose_plus_plus_amd import estimate_affine_2d_batch
    views, seeds = _mixed_views(3)
    p0, p1, off = AO.concat(views)
    ids = np.repeat(np.arange(3), np.diff(off))
    corners = np.tile(CORNERS, (3, 1, 1))
    raw = AO.run_raw(views, seeds, 257, 0.99, True, corners)
    r = estimate_affine_2d_batch(torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda(), view_ids=torch.from_numpy(ids).cuda(), corners=corners,
                                 max_iters=257, seed=seeds, fallback_box=AC.FALLBACK, record=True)
    assert all(t.is_cuda for t in r.values()) and int(r["bad_ids"][0]) == 0 and r["offsets"].cpu().tolist() == off.tolist()
    for k, rk in (("affine", "affine"), ("inliers", "mask"), ("n_inliers", "n_inliers"), ("ok", "ok"), ("stop", "stop"), ("boxes", "boxes"),
                  ("best_view", "best_view"), ("best_box", "best_box"), ("samples", "samples"), ("scores", "scores")):
        assert torch.equal(r[k].cpu(), raw[rk]), k
    r2 = estimate_affine_2d_batch(p0, p1, offsets=off, corners=corners, max_iters=257, seed=seeds, fallback_box=AC.FALLBACK)
    assert torch.equal(r2["affine"].cpu(), raw["affine"]) and "bad_ids" not in r2


def test_tracker_starts_on_its_own_with_the_affine_detector():
    from onepose_plus_plus_amd import AffineBoxDetector, PoseTracker, box_from_pose
    from onepose_plus_plus_amd.bank import ObjectBank
    from tests.test_tracking_gpu import _PlantedMatcher
    rng = np.random.default_rng(2)
    K = np.array([[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1]])
    ext = np.array([0.07, 0.045, 0.1])
    bbox3d = np.array([[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)], np.float64) * ext
    pts3d = rng.uniform(-1, 1, (200, 3)) * ext
    th = 0.4
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    poses = [np.concatenate([R, np.array([[0.01 * i - 0.02], [0.005 * i], [0.6 + 0.01 * i]])], axis=1) for i in range(2)]
    bank = ObjectBank(pts3d, np.zeros((128, 200), np.float32))
    refs = [np.zeros((480, 640), np.uint8), np.ones((480, 640), np.uint8)]
    replay = {0: _exact_view(30, 7, 0.25, (250.5, 180.5)), 1: _exact_view(90, 8)}       # view 1 wins: 0.375 p + (200.5, 120.5)
    seen = []

    def matcher(ref, frame):
        seen.append(int(ref[0, 0]))
        return replay[int(ref[0, 0])]

    detector = AffineBoxDetector(matcher, refs)
    tracker = PoseTracker(_PlantedMatcher(poses, [200, 200], pts3d), bank, K, bbox3d, detector=detector, crop_size=128)
    frames = rng.integers(0, 256, (2, 480, 640), dtype=np.uint8)
    first = tracker.step(frames[0])                                                     # no TrackingLost
    assert first["source"] == "detector" and seen == [0, 1] and detector.last == (1, 90)
    assert first["bbox"].tolist() == [200, 120, 440, 300] and first["state"] and len(first["inliers"]) == 200
    second = tracker.step(frames[1])
    assert second["source"] == "previous_pose" and seen == [0, 1]
    assert np.array_equal(second["bbox"], box_from_pose(K, first["pose"], bbox3d)[0])
