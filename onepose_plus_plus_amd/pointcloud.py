"""SfM point-cloud post-processing: what the reference runs between COLMAP's `points3D` and the descriptor bank
(run.py:335-363), the step BEFORE `bankbuild.build_object_bank`:

    filter_points.filter_bbox           :172-234   keep the points strictly inside the annotated 3D box
    filter_tkl.get_tkl                  :37-56     smallest track length that leaves at most max_num_kp3d points
    filter_points.filter_track_length   :10-27     cut by it, points ordered by id
    filter_points.merge                 :265-297   average every point with its neighbours closer than 1e-3

All coordinates are float64 end to end.  The box mask and the merge run on the device (csrc/pointcloud.hip); the merge never forms
the reference's n x n distance matrix: a tiled pair search keeps the pairs below the threshold, a deterministic selection
reproduces the reference's row walk, and one kernel emits the clusters.  `merge` returns exactly the reference's values, so
run.py can call it in place of `filter_points.merge`; `postprocess_points` strings the four steps together and its outputs go
straight into `bankbuild.build_object_bank`.  The COLMAP readers stay the reference's: `points3D_arrays` takes their
`{id: Point3D}` dictionary.  There is no CPU path: without the HIP library every device step raises.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib

MAX_POINTS = 1 << 20
DEFAULT_PAIRS_PER_POINT = 64


def _device(device):
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def _checked_xyz(xyz):
    """host-side refusals, before a device is touched: shape, the 2**20 limit, non-finite coordinates"""
    if not isinstance(xyz, torch.Tensor):
        xyz = np.asarray(xyz, dtype=np.float64)
    if len(xyz.shape) != 2 or xyz.shape[1] != 3:
        raise ValueError("points must have shape (n, 3), got %s" % (tuple(xyz.shape),))
    if xyz.shape[0] > MAX_POINTS:
        raise ValueError("%d points: more than the 2**20 the all-pairs search is built for" % xyz.shape[0])
    finite = bool(torch.isfinite(xyz).all()) if isinstance(xyz, torch.Tensor) else bool(np.isfinite(xyz).all())
    if not finite:
        raise ValueError("non-finite point coordinates")
    return xyz


def _xyz_to_device(xyz, device):
    """checked points -> float64 [N,3] contiguous device tensor"""
    if isinstance(xyz, torch.Tensor):
        return xyz.to(device=device, dtype=torch.float64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(xyz)).to(device)


def filter_bbox_mask(xyz, corners, device=None):
    """bool [N] device tensor: True where the point lies strictly inside the box of `corners` [8,3] (filter_bbox's inner
    `filter_`, numpy branch): 0 < (p - c4) . v < v . v for v = c5 - c4, c0 - c4, c7 - c4."""
    corners = np.ascontiguousarray(np.asarray(corners, dtype=np.float64))
    if corners.shape != (8, 3):
        raise ValueError("box corners must have shape (8, 3), got %s" % (corners.shape,))
    if not np.isfinite(corners).all():
        raise ValueError("non-finite box corners")
    xyz = _checked_xyz(xyz)
    device = _device(device)
    pts = _xyz_to_device(xyz, device)
    n = int(pts.shape[0])
    lib = _lib.load()
    mask = torch.empty(n, dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        _lib.check(lib.opp_pc_box_mask(pts.data_ptr(), n, corners.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), mask.data_ptr(), stream),
                   "opp_pc_box_mask")
    return mask.bool()


def get_tkl(track_lengths, thres, percent_thres=1.0):
    """The track length that limits the number of 3D points to `thres` (filter_tkl.get_tkl): walking the distinct lengths
    upwards and taking their points away, the first length at which at most min(N * percent_thres, thres) points are left."""
    tl = np.asarray(track_lengths).reshape(-1)
    n = int(tl.shape[0])
    if n == 0:
        raise ValueError("get_tkl: no 3D points")       # upstream ends in an unbound local here
    thres = min(n * percent_thres, thres)
    keys, counts = np.unique(tl, return_counts=True)
    left = n
    for key, count in zip(keys.tolist(), counts.tolist()):
        left -= count
        if left <= thres:
            return int(key)
    raise ValueError("get_tkl: no track length leaves at most %r points" % (thres,))   # thres < 0 only: the walk ends at 0 points


def filter_by_track_length(ids, xyz, track_lengths, track_length):
    """-> (xyzs [n,3] float64, points_idxs [n] int64): the points whose track has at least `track_length` observations, in
    ascending id (filter_points.filter_by_track_length)."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    tl = np.asarray(track_lengths).reshape(-1)
    if not (len(ids) == len(xyz) == len(tl)):
        raise ValueError("ids, xyz and track_lengths disagree in length: %d, %d, %d" % (len(ids), len(xyz), len(tl)))
    order = np.argsort(ids, kind="stable")
    order = order[tl[order] >= track_length]
    return np.ascontiguousarray(xyz[order]), np.ascontiguousarray(ids[order])


def merge_csr(xyzs, points_idxs, dist_threshold=1e-3, device=None, max_pairs=None):
    """`merge` without the dictionary -> (ret_points [M,3] float64, offsets [M+1] int64, members [T] int64) on the device:
    cluster c averages the points whose ids are members[offsets[c]:offsets[c+1]].

    Refused before anything is allocated or launched: more than 2**20 points, a threshold that is not finite and positive,
    non-finite coordinates, a `max_pairs` below n (every point is its own neighbour).  A pair total above `max_pairs` (default
    64 per point) is refused once the counting pass has produced it, before the neighbour lists are allocated."""
    thr = float(dist_threshold)
    if not math.isfinite(thr) or thr <= 0.0:
        raise ValueError("dist_threshold must be finite and positive, got %r" % (dist_threshold,))
    xyzs = _checked_xyz(xyzs)
    n = int(xyzs.shape[0])
    if len(points_idxs) != n:
        raise ValueError("%d points but %d ids" % (n, len(points_idxs)))
    max_pairs = DEFAULT_PAIRS_PER_POINT * n if max_pairs is None else int(max_pairs)
    if max_pairs < n:
        raise ValueError("max_pairs = %d is below the %d points, each of which is its own neighbour" % (max_pairs, n))
    device = _device(device)
    pts = _xyz_to_device(xyzs, device)
    ids = (points_idxs.to(device=device, dtype=torch.int64) if isinstance(points_idxs, torch.Tensor)
           else torch.from_numpy(np.ascontiguousarray(np.asarray(points_idxs, dtype=np.int64))).to(device)).contiguous()
    if n == 0:
        return (torch.empty((0, 3), dtype=torch.float64, device=device), torch.zeros(1, dtype=torch.int64, device=device),
                torch.empty(0, dtype=torch.int64, device=device))
    lib = _lib.load()
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        counts = torch.empty(n, dtype=torch.int32, device=device)
        _lib.check(lib.opp_pc_neighbor_count(pts.data_ptr(), n, thr, counts.data_ptr(), stream), "opp_pc_neighbor_count")
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=device)
        torch.cumsum(counts, 0, dtype=torch.int64, out=offsets[1:])
        pairs = int(offsets[n].item())                                  # the one read-back between the two passes
        if pairs > max_pairs:
            raise ValueError("%d point pairs are closer than %g, more than max_pairs = %d: a degenerate cloud (or a threshold of the "
                             "cloud's own size)" % (pairs, thr, max_pairs))
        ws_bytes = int(lib.opp_pc_workspace_bytes(n, pairs))
        ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=device)
        _lib.check(lib.opp_pc_neighbor_fill(pts.data_ptr(), n, thr, offsets.data_ptr(), pairs, ws.data_ptr(), ws_bytes, stream),
                   "opp_pc_neighbor_fill")
        sel = torch.empty(n, dtype=torch.int32, device=device)
        selcnt = torch.empty(n, dtype=torch.int32, device=device)
        status = torch.zeros(1, dtype=torch.int32, device=device)
        _lib.check(lib.opp_pc_select(offsets.data_ptr(), n, pairs, sel.data_ptr(), selcnt.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                     ws_bytes, stream), "opp_pc_select")
        rank = torch.cumsum(sel, 0, dtype=torch.int64)
        mem_end = torch.cumsum(selcnt, 0, dtype=torch.int64)
        n_clusters, n_members, st = torch.stack([rank[-1], mem_end[-1], status[0].to(torch.int64)]).tolist()
        if st != 0:
            raise _lib.OppError("opp_pc_select: the selection did not settle within its bound of %d rounds" % n)
        ret_points = torch.empty((n_clusters, 3), dtype=torch.float64, device=device)
        cl_offsets = torch.zeros(n_clusters + 1, dtype=torch.int64, device=device)
        members = torch.empty(n_members, dtype=torch.int64, device=device)
        _lib.check(lib.opp_pc_emit(pts.data_ptr(), ids.data_ptr(), n, pairs, offsets.data_ptr(), sel.data_ptr(), rank.data_ptr(),
                                   mem_end.data_ptr(), n_clusters, n_members, ret_points.data_ptr(), cl_offsets.data_ptr(),
                                   members.data_ptr(), ws.data_ptr(), ws_bytes, stream), "opp_pc_emit")
    return ret_points, cl_offsets, members


def merge(xyzs, points_idxs, dist_threshold=1e-3, device=None, max_pairs=None):
    """Merge points which are close to others -> (ret_points [M,3] float64 ndarray, ret_idxs {new point: int64 ndarray of the
    old ids}), the return values of filter_points.merge."""
    ret_points, offsets, members = merge_csr(xyzs, points_idxs, dist_threshold, device=device, max_pairs=max_pairs)
    offsets = offsets.cpu().numpy()
    members = members.cpu().numpy()
    ret_idxs = {c: members[offsets[c]:offsets[c + 1]] for c in range(len(offsets) - 1)}
    return ret_points.cpu().numpy(), ret_idxs


def points3D_arrays(points3D):
    """COLMAP's {id: Point3D} (anything with `.xyz` and `.point2D_idxs`) -> (ids [N] int64, xyz [N,3] float64,
    track_lengths [N] int64), in the dictionary's order."""
    n = len(points3D)
    ids = np.empty(n, dtype=np.int64)
    xyz = np.empty((n, 3), dtype=np.float64)
    track_lengths = np.empty(n, dtype=np.int64)
    for row, (pid, point) in enumerate(points3D.items()):
        ids[row] = pid
        xyz[row] = np.asarray(point.xyz, dtype=np.float64).reshape(3)
        track_lengths[row] = len(point.point2D_idxs)
    return ids, xyz, track_lengths


def postprocess_points(ids, xyz, track_lengths, box_corners=None, max_num_kp3d=15000, dist_threshold=1e-3, device=None):
    """run.py:335-363 in one call -> (merge_xyzs, merge_idxs, track_length): box mask (skipped when `box_corners` is None),
    get_tkl on the survivors, the track-length cut, the merge.  merge_xyzs / merge_idxs are `build_object_bank`'s inputs."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    track_lengths = np.asarray(track_lengths).reshape(-1)
    if box_corners is not None:
        keep = filter_bbox_mask(xyz, box_corners, device=device).cpu().numpy()
        ids, xyz, track_lengths = ids[keep], xyz[keep], track_lengths[keep]
    track_length = get_tkl(track_lengths, max_num_kp3d)
    xyzs, points_idxs = filter_by_track_length(ids, xyz, track_lengths, track_length)
    merge_xyzs, merge_idxs = merge(xyzs, points_idxs, dist_threshold, device=device)
    return merge_xyzs, merge_idxs, track_length
