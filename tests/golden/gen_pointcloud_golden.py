"""Fixtures of the point-cloud post-processing (tests/golden/pointcloud_*.npz), produced by the REFERENCE'S OWN functions: `merge`,
`filter_by_track_length` and `filter_bbox` (whose inner `filter_` decides the box mask) of
src/sfm_utils/postprocess/filter_points.py and `get_tkl` of filter_tkl.py.  The two files are loaded by path from the read-only
reference checkout (OPP_REFERENCE_ROOT, default /root/reference) -- importing their package would pull in h5py -- with empty
stand-ins for cv2, loguru, tqdm, matplotlib and the reference's vis_utils, and with a stand-in for its COLMAP reader / writer that
hands the functions the in-memory `{id: Point3D}` dictionary they would have read and records the one they would have written.
Runs only where the reference and scipy are present:

    python tests/golden/gen_pointcloud_golden.py

Inputs come from the seeds of pointcloud_cases.py, so only results are stored.  The generator refuses to write a case whose
smallest pair margin |d - thr| / thr is below 1e-6 or whose smallest box-face margin is below 1e-9: no stored result then hangs
on a rounding the reference does not define (scipy's pdist and a BLAS dot product may contract into FMAs).  It also asserts what
the cases are for: the mixed clouds give more than 100 multi-member clusters and at least 5 dropped points, the boxes from n = 65
on have points on both sides of every face."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import pointcloud_reference as R  # noqa: E402
from tests.golden import pointcloud_cases as C  # noqa: E402

REF = os.environ.get("OPP_REFERENCE_ROOT", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
PAIR_MARGIN = 1e-6
FACE_MARGIN = 1e-9


class Point3D:
    def __init__(self, xyz, track_length):
        self.xyz = np.asarray(xyz, dtype=np.float64)
        self.image_ids = np.zeros(int(track_length), dtype=np.int64)
        self.point2D_idxs = np.arange(int(track_length), dtype=np.int64)


class _Image:
    def __init__(self):
        self.point3D_ids = np.zeros(64, dtype=np.int64)


class _Colmap:
    """stand-in for src.utils.colmap.read_write_model: the "model path" IS the points3D dictionary"""
    written = None

    @staticmethod
    def read_model(path, ext=""):
        return {}, {0: _Image()}, path

    @classmethod
    def write_model(cls, cameras, images, points3D, path, ext=""):
        cls.written = points3D


def _module(name, **attrs):
    mod = sys.modules.get(name) or types.ModuleType(name)
    for k, v in attrs.items():
        setattr(mod, k, v)
    sys.modules[name] = mod
    return mod


def load_reference():
    post = os.path.join(REF, "src", "sfm_utils", "postprocess")
    if not os.path.isdir(post):
        raise RuntimeError("reference tree not found at %s" % REF)
    for name in ("cv2", "tqdm", "matplotlib"):
        if name not in sys.modules:
            _module(name)
    _module("loguru", logger=None)
    _module("matplotlib.pyplot")
    rw = _module("src.utils.colmap.read_write_model", read_model=_Colmap.read_model, write_model=_Colmap.write_model)
    _module("src.utils.colmap", read_write_model=rw)
    _module("src.utils.vis_utils", add_pointcloud_to_vis3d=None)
    _module("src.utils")
    _module("src")
    mods = []
    for fname in ("filter_points.py", "filter_tkl.py"):
        spec = importlib.util.spec_from_file_location("opp_ref_" + fname[:-3], os.path.join(post, fname))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods


def as_points3D(ids, xyz, track_lengths):
    return {int(i): Point3D(p, t) for i, p, t in zip(ids, xyz, track_lengths)}


def reference_box_keep(fp, ids, xyz, corners, tmp):
    """filter_bbox on the in-memory model -> boolean keep mask in input order"""
    box = os.path.join(tmp, "box.txt")
    np.savetxt(box, corners, fmt="%.17g")
    assert np.array_equal(np.loadtxt(box), corners)
    fp.filter_bbox(as_points3D(ids, xyz, np.full(len(ids), 2)), os.path.join(tmp, "model"), box)
    kept = set(_Colmap.written)
    return np.array([int(i) in kept for i in ids], dtype=bool)


def main():
    fp, ft = load_reference()
    out = {}
    # merge
    for name in C.MERGE_CASES:
        xyzs, ids, thr = C.merge_inputs(name)
        margin = R.boundary_margin(xyzs, thr)
        assert margin >= PAIR_MARGIN, "%s: a pair distance within %.1e of the threshold" % (name, margin)
        ret_points, ret_idxs = fp.merge(xyzs, ids, dist_threshold=thr)
        offsets, members = R.csr(ret_idxs)
        assert ret_points.dtype == np.float64 and all(ret_idxs[c].dtype == np.int64 for c in ret_idxs)
        dropped = len(ids) - len(np.unique(members))
        multi = int((np.diff(offsets) > 1).sum())
        if name in C.MIXED_CASES:
            assert multi > 100 and dropped >= 5, (name, multi, dropped)
        out.update({"merge_%s_points" % name: ret_points, "merge_%s_offsets" % name: offsets, "merge_%s_members" % name: members,
                    "merge_%s_margin" % name: np.float64(margin)})
        print("merge %-20s n = %4d -> %4d clusters (%3d multi-member), %2d dropped, margin %.2e" % (name, len(ids), len(offsets) - 1, multi,
                                                                                                    dropped, margin))
    np.savez(os.path.join(OUT, "pointcloud_merge.npz"), **out)
    # box
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in C.BOX_CASES:
            xyz, corners = C.box_inputs(name)
            margin = R.box_margin(xyz, corners)
            assert margin >= FACE_MARGIN, "%s: a point within %.1e of a face" % (name, margin)
            keep = reference_box_keep(fp, np.arange(len(xyz)) + C.ID_BASE, xyz, corners, tmp)
            if len(xyz) >= 65:
                origin, edges = R._edges(corners)
                for v in edges:
                    m = R._dot3(xyz - origin, v)
                    assert (m < 0).any() and (m > R._dot3(v, v)).any() and keep.any()
            out.update({"box_%s_keep" % name: keep, "box_%s_margin" % name: np.float64(margin)})
            print("box %-14s %4d of %4d inside, margin %.2e" % (name, keep.sum(), len(keep), margin))
        # the chain of run.py:335-363 on one cloud
        ids, xyz, track_lengths, corners, _, _ = C.postprocess_inputs()
        assert R.box_margin(xyz, corners) >= FACE_MARGIN
        keep = reference_box_keep(fp, ids, xyz, corners, tmp)
        survivors = as_points3D(ids[keep], xyz[keep], track_lengths[keep])
        track_length, counts = ft.get_tkl(survivors, thres=C.POSTPROCESS["max_num_kp3d"])
        assert counts == [int(t) for t in track_lengths[keep]]
        xyzs, points_idxs = fp.filter_by_track_length(survivors, track_length)
        assert R.boundary_margin(xyzs, C.THR) >= PAIR_MARGIN
        ret_points, ret_idxs = fp.merge(xyzs, points_idxs)
        offsets, members = R.csr(ret_idxs)
        assert 0 < keep.sum() < len(keep) and 0 < len(xyzs) < keep.sum() and (np.diff(offsets) > 1).sum() >= 10
        out.update(post_keep=keep, post_track_length=np.int64(track_length), post_xyzs=xyzs, post_points_idxs=points_idxs.astype(np.int64),
                   post_points=ret_points, post_offsets=offsets, post_members=members)
        print("postprocess: %d points, %d in the box, track length %d leaves %d, %d clusters" % (len(ids), keep.sum(), track_length, len(xyzs),
                                                                                                len(offsets) - 1))
    np.savez(os.path.join(OUT, "pointcloud_box.npz"), **out)
    # get_tkl
    names = list(C.TKL_CASES)
    values = []
    for name in names:
        tl, thres, percent = C.TKL_CASES[name]
        model = as_points3D(np.arange(len(tl)) + C.ID_BASE, np.zeros((len(tl), 3)), tl)
        values.append(ft.get_tkl(model, thres, percent_thres=percent)[0])
    np.savez(os.path.join(OUT, "pointcloud_tkl.npz"), names=np.array(names), track_length=np.array(values, dtype=np.int64))
    print("get_tkl:", dict(zip(names, values)))


if __name__ == "__main__":
    main()
