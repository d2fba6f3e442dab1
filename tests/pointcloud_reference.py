"""float64 numpy restatement of the reference's point-cloud post-processing (src/sfm_utils/postprocess/filter_points.py
filter_bbox :172-234, filter_by_track_length :10-27, merge :265-297; filter_tkl.py get_tkl :37-56), TEST INFRASTRUCTURE ONLY: no
scipy, no n x n matrix kept (rows are formed a block at a time), every multiply and add rounded on its own.  Pinned against the
reference's own results by tests/test_pointcloud_cpu.py (tests/golden/pointcloud_*.npz).

Two places where the reference's libraries may round differently (a BLAS dot product or scipy's pdist may contract into FMAs) are
kept away from every fixture by the margins below: no stored pair distance lies within 1e-6 (relative) of the threshold and no
stored point within 1e-9 of a box face, so both roundings decide alike."""
import numpy as np


def _edges(corners):
    c = np.asarray(corners, dtype=np.float64)
    return c[4], [c[5] - c[4], c[0] - c[4], c[7] - c[4]]


def _dot3(p, v):
    return (p[..., 0] * v[0] + p[..., 1] * v[1]) + p[..., 2] * v[2]


def box_mask(xyz, corners):
    """filter_bbox's inner filter_ (numpy branch): strictly inside on all six faces"""
    origin, edges = _edges(corners)
    p = np.asarray(xyz, dtype=np.float64).reshape(-1, 3) - origin
    keep = np.ones(len(p), dtype=bool)
    for v in edges:
        m = _dot3(p, v)
        keep &= (0 < m) & (m < _dot3(v, v))
    return keep


def box_margin(xyz, corners):
    """smallest min(|m|, |m - v.v|) / v.v over the points and the three edge directions: relative distance to the nearest face"""
    origin, edges = _edges(corners)
    p = np.asarray(xyz, dtype=np.float64).reshape(-1, 3) - origin
    best = np.inf
    for v in edges:
        m, vv = _dot3(p, v), _dot3(v, v)
        if len(m):
            best = min(best, float(np.min(np.minimum(np.abs(m), np.abs(m - vv)) / vv)))
    return best


def _distance_rows(xyzs, block=512):
    """yields (first row, distances [rows, n]) with d = sqrt((dx dx + dy dy) + dz dz)"""
    for s in range(0, len(xyzs), block):
        d = xyzs[s:s + block, None, :] - xyzs[None, :, :]
        sq = d * d
        yield s, np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2])


def neighbours(xyzs, thr):
    """N(j) = ascending positions i with distance < thr (j included), for every j"""
    xyzs = np.asarray(xyzs, dtype=np.float64).reshape(-1, 3)
    out = []
    for _, dist in _distance_rows(xyzs):
        out.extend(np.nonzero(row)[0] for row in dist < thr)
    return out


def boundary_margin(xyzs, thr):
    """smallest |d - thr| / thr over all pairs"""
    xyzs = np.asarray(xyzs, dtype=np.float64).reshape(-1, 3)
    best = np.inf
    for _, dist in _distance_rows(xyzs):
        best = min(best, float(np.min(np.abs(dist - thr))) / thr)
    return best


def merge_walk(xyzs, thr):
    """-> (selected rows, their neighbourhoods, number of points in no cluster): row j is taken iff no member of N(j) belongs to
    the N(i) of an earlier taken row"""
    nb = neighbours(xyzs, thr)
    recorded = np.zeros(len(nb), dtype=bool)
    rows = []
    for j, idx in enumerate(nb):
        if recorded[idx].any():
            continue
        rows.append(j)
        recorded[idx] = True
    return rows, [nb[j] for j in rows], int((~recorded).sum())


def merge(xyzs, points_idxs, dist_threshold=1e-3):
    """-> (ret_points [M,3], ret_idxs {c: ids}) like filter_points.merge; the mean spelled out the way numpy reduces axis 0:
    the members added one after the other, one division"""
    xyzs = np.asarray(xyzs, dtype=np.float64).reshape(-1, 3)
    points_idxs = np.asarray(points_idxs)
    rows, members, _ = merge_walk(xyzs, dist_threshold)
    ret_points = np.empty((len(rows), 3))
    ret_idxs = {}
    for c, idx in enumerate(members):
        acc = xyzs[idx[0]].copy()
        for i in idx[1:]:
            acc = acc + xyzs[i]
        ret_points[c] = acc / float(len(idx))
        ret_idxs[c] = points_idxs[idx]
    return ret_points, ret_idxs


def csr(ret_idxs):
    """{c: ids} -> (offsets [M+1], members) int64"""
    sizes = [len(ret_idxs[c]) for c in range(len(ret_idxs))]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    members = np.concatenate([ret_idxs[c] for c in range(len(ret_idxs))]).astype(np.int64) if sizes else np.empty(0, np.int64)
    return offsets, members


def get_tkl(track_lengths, thres, percent_thres=1.0):
    tl = [int(t) for t in track_lengths]
    if not tl:
        raise ValueError("no 3D points")
    thres = min(len(tl) * percent_thres, thres)
    left = len(tl)
    for key in sorted(set(tl)):
        left -= tl.count(key)
        if left <= thres:
            return key
    raise ValueError("no track length leaves at most %r points" % (thres,))


def filter_by_track_length(ids, xyz, track_lengths, track_length):
    rows = [r for r in sorted(range(len(ids)), key=lambda r: ids[r]) if track_lengths[r] >= track_length]
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    return xyz[rows].reshape(-1, 3), np.asarray(ids, dtype=np.int64)[rows]


def postprocess_points(ids, xyz, track_lengths, box_corners=None, max_num_kp3d=15000, dist_threshold=1e-3):
    """run.py:335-363: box, get_tkl on the survivors, cut, merge"""
    ids, xyz, track_lengths = np.asarray(ids, dtype=np.int64), np.asarray(xyz, dtype=np.float64), np.asarray(track_lengths)
    if box_corners is not None:
        keep = box_mask(xyz, box_corners)
        ids, xyz, track_lengths = ids[keep], xyz[keep], track_lengths[keep]
    track_length = get_tkl(track_lengths, max_num_kp3d)
    xyzs, points_idxs = filter_by_track_length(ids, xyz, track_lengths, track_length)
    ret_points, ret_idxs = merge(xyzs, points_idxs, dist_threshold)
    return ret_points, ret_idxs, track_length
