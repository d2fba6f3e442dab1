"""CPU: the numpy restatement of the point-cloud post-processing (tests/pointcloud_reference.py) against results of the reference's
own functions (tests/golden/pointcloud_*.npz, gen_pointcloud_golden.py) -- bit for bit; the margins that make the fixtures
independent of a library's rounding; `get_tkl` / `filter_by_track_length` / `points3D_arrays` of the package (host code); the
refusals that are raised before a device is touched; and the C ABI of the new symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import pointcloud_reference as R
from tests.golden import pointcloud_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PC_SYMBOLS = ("opp_pc_workspace_bytes", "opp_pc_box_mask", "opp_pc_neighbor_count", "opp_pc_neighbor_fill", "opp_pc_select", "opp_pc_emit")


@pytest.fixture(scope="module")
def gold():
    out = {}
    for name in ("merge", "box", "tkl"):
        z = np.load(os.path.join(GOLDEN, "pointcloud_%s.npz" % name))
        out.update({k: z[k] for k in z.files})
    return out


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("name", list(C.MERGE_CASES))
def test_restatement_merge_vs_reference(gold, name):
    xyzs, ids, thr = C.merge_inputs(name)
    assert ids.dtype == np.int64 and ids.min() > 2 ** 31 and len(np.unique(ids)) == len(ids)
    margin = R.boundary_margin(xyzs, thr)
    assert margin >= 1e-6 and margin == float(gold["merge_%s_margin" % name])
    ret_points, ret_idxs = R.merge(xyzs, ids, thr)
    offsets, members = R.csr(ret_idxs)
    assert np.array_equal(offsets, gold["merge_%s_offsets" % name]) and np.array_equal(members, gold["merge_%s_members" % name])
    assert _same_bits(ret_points, gold["merge_%s_points" % name])
    # centres: the selected rows are where the reference's clusters start from
    rows, hoods, dropped = R.merge_walk(xyzs, thr)
    assert len(rows) == len(offsets) - 1 and all(j in h for j, h in zip(rows, hoods))
    assert dropped == len(ids) - len(np.unique(members))


def test_cases_cover_what_they_are_for(gold):
    for name in C.MIXED_CASES:
        offsets, members = gold["merge_%s_offsets" % name], gold["merge_%s_members" % name]
        assert (np.diff(offsets) > 1).sum() > 100 and len(C.merge_inputs(name)[1]) - len(np.unique(members)) >= 5
    assert len(gold["merge_blob40_offsets"]) == 2 and gold["merge_blob40_offsets"][1] == 40
    assert len(gold["merge_n2_close_offsets"]) == 2 and len(gold["merge_n2_far_offsets"]) == 3
    # the line: the walk depends on the order of the points, and the permuted one drops points
    assert len(gold["merge_line200_offsets"]) == 68 and len(np.unique(gold["merge_line200_members"])) == 200
    assert len(np.unique(gold["merge_line200_permuted_members"])) < 200
    assert np.diff(gold["merge_duplicates_offsets"]).max() == 3


@pytest.mark.parametrize("name", list(C.BOX_CASES))
def test_restatement_box_vs_reference(gold, name):
    xyz, corners = C.box_inputs(name)
    margin = R.box_margin(xyz, corners)
    assert margin >= 1e-9 and margin == float(gold["box_%s_margin" % name])
    assert np.array_equal(R.box_mask(xyz, corners), gold["box_%s_keep" % name])


def test_restatement_chain_vs_reference(gold):
    ids, xyz, track_lengths, corners, _, _ = C.postprocess_inputs()
    assert np.array_equal(R.box_mask(xyz, corners), gold["post_keep"])
    ret_points, ret_idxs, track_length = R.postprocess_points(ids, xyz, track_lengths, corners, C.POSTPROCESS["max_num_kp3d"])
    assert track_length == int(gold["post_track_length"])
    offsets, members = R.csr(ret_idxs)
    assert np.array_equal(offsets, gold["post_offsets"]) and np.array_equal(members, gold["post_members"])
    assert _same_bits(ret_points, gold["post_points"])


@pytest.mark.parametrize("name", list(C.TKL_CASES))
def test_get_tkl(gold, name):
    from onepose_plus_plus_amd import pointcloud as P
    tl, thres, percent = C.TKL_CASES[name]
    want = int(gold["track_length"][list(gold["names"]).index(name)])
    assert R.get_tkl(tl, thres, percent) == want
    got = P.get_tkl(np.array(tl), thres, percent_thres=percent)
    assert isinstance(got, int) and got == want
    assert P.get_tkl(tl, thres, percent) == want


def test_get_tkl_empty_raises():
    from onepose_plus_plus_amd import pointcloud as P
    with pytest.raises(ValueError):
        P.get_tkl([], 100)
    with pytest.raises(ValueError):
        R.get_tkl([], 100)


def test_filter_by_track_length_and_points3D_arrays(gold):
    from onepose_plus_plus_amd import pointcloud as P

    class Point3D:
        def __init__(self, xyz, t):
            self.xyz, self.point2D_idxs = xyz, np.arange(t)

    ids, xyz, track_lengths, corners, _, _ = C.postprocess_inputs()
    keep = gold["post_keep"]
    model = {int(i): Point3D(p, t) for i, p, t in zip(ids[keep], xyz[keep], track_lengths[keep])}
    ids2, xyz2, tl2 = P.points3D_arrays(model)
    assert ids2.dtype == np.int64 and xyz2.dtype == np.float64 and tl2.dtype == np.int64
    assert np.array_equal(ids2, ids[keep]) and np.array_equal(xyz2, xyz[keep]) and np.array_equal(tl2, track_lengths[keep])
    xyzs, points_idxs = P.filter_by_track_length(ids2, xyz2, tl2, int(gold["post_track_length"]))
    assert xyzs.dtype == np.float64 and points_idxs.dtype == np.int64
    assert np.array_equal(points_idxs, gold["post_points_idxs"]) and _same_bits(xyzs, gold["post_xyzs"])
    assert np.all(np.diff(points_idxs) > 0)
    rx, ri = R.filter_by_track_length(ids2, xyz2, tl2, int(gold["post_track_length"]))
    assert np.array_equal(ri, points_idxs) and _same_bits(rx, xyzs)
    ex, ei = P.filter_by_track_length(ids2, xyz2, tl2, 1000)
    assert ex.shape == (0, 3) and ei.shape == (0,)


def test_refusals_raise_before_a_device_is_touched(monkeypatch):
    """none of these reaches the library or a device: the loader is replaced by one that fails the test"""
    from onepose_plus_plus_amd import _lib, pointcloud as P

    def no_load():
        raise AssertionError("the refusal came too late: the library was asked for")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(P, "_device", lambda device: no_load())
    xyzs, ids, thr = C.merge_inputs("blob40")
    for fn in (P.merge, P.merge_csr):
        for bad in (0.0, -1e-3, float("inf"), float("nan")):
            with pytest.raises(ValueError, match="dist_threshold"):
                fn(xyzs, ids, bad)
        with pytest.raises(ValueError, match="max_pairs"):
            fn(xyzs, ids, thr, max_pairs=1)
        for bad in (np.nan, np.inf, -np.inf):
            broken = xyzs.copy()
            broken[17, 1] = bad
            with pytest.raises(ValueError, match="non-finite"):
                fn(broken, ids, thr)
        with pytest.raises(ValueError, match=r"2\*\*20"):
            fn(np.zeros((2 ** 20 + 1, 3)), np.arange(2 ** 20 + 1), thr)
        with pytest.raises(ValueError):
            fn(xyzs, ids[:-1], thr)
        with pytest.raises(ValueError):
            fn(xyzs[:, :2], ids, thr)
    broken = xyzs.copy()
    broken[0, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        P.filter_bbox_mask(broken, C.box_corners(False))
    with pytest.raises(ValueError):
        P.filter_bbox_mask(xyzs, C.box_corners(False)[:7])
    corners = C.box_corners(True)
    corners[3, 2] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        P.filter_bbox_mask(xyzs, corners)


def test_module_is_exported():
    import onepose_plus_plus_amd
    assert onepose_plus_plus_amd.pointcloud.merge and "pointcloud" in onepose_plus_plus_amd.__all__


@pytest.fixture(scope="module")
def lib():
    from onepose_plus_plus_amd.build import build
    from onepose_plus_plus_amd import _lib
    build(verbose=False)
    return _lib.load()


def test_header_signatures_and_library_agree(lib):
    from onepose_plus_plus_amd import _lib
    src = open(os.path.join(ROOT, "include", "opp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(opp_pc_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted(PC_SYMBOLS)
    assert sorted(k for k in _lib.SIGNATURES if k.startswith("opp_pc_")) == declared
    for name in declared:
        assert hasattr(lib, name), name
        # the argument count of the ctypes row is the header's
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, re.S).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len(decl.split(",")), name
    from onepose_plus_plus_amd import build
    assert "pointcloud.hip" in build.SOURCES and "-ffp-contract=off" in build.SOURCE_FLAGS["pointcloud.hip"]


def test_workspace_bytes_and_c_level_refusals(lib):
    """host-only entry point, and the argument checks of the launchers, which return before any launch"""
    assert lib.opp_pc_workspace_bytes(0, 0) == 0 and lib.opp_pc_workspace_bytes(2 ** 20 + 1, 2 ** 20 + 1) == 0
    assert lib.opp_pc_workspace_bytes(100, 100 * 100 + 1) == 0
    small, large = lib.opp_pc_workspace_bytes(1000, 1000), lib.opp_pc_workspace_bytes(1000, 64000)
    assert small >= 4 * 1000 + 2 * 1000 and large - small >= 4 * 63000 - 256 and large % 256 == 0
    assert lib.opp_pc_workspace_bytes(2 ** 20, 64 * 2 ** 20) < 300e6          # the default pair limit at the largest cloud: 268 MB, not n^2
    dummy = ctypes.create_string_buffer(64)
    ptr = ctypes.cast(dummy, ctypes.c_void_p)
    assert lib.opp_pc_neighbor_count(ptr, 2 ** 20 + 1, 1e-3, ptr, None) != 0 and b"2^20" in lib.opp_last_error()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.opp_pc_neighbor_count(ptr, 10, bad, ptr, None) != 0 and b"threshold" in lib.opp_last_error()
    assert lib.opp_pc_neighbor_fill(ptr, 10, 1e-3, ptr, 9, ptr, 1 << 20, None) != 0 and b"pairs" in lib.opp_last_error()
    assert lib.opp_pc_neighbor_fill(ptr, 10, 1e-3, ptr, 10, ptr, 16, None) != 0 and b"workspace" in lib.opp_last_error()
    assert lib.opp_pc_select(ptr, 10, 10, ptr, ptr, ptr, ptr, 16, None) != 0 and b"workspace" in lib.opp_last_error()
    corners = (ctypes.c_double * 24)(*([float("nan")] * 24))
    assert lib.opp_pc_box_mask(ptr, 10, corners, ptr, None) != 0 and b"corner" in lib.opp_last_error()
