"""A training sample's tensors, built on the device from the small annotation arrays.

Mirror of the training branch of `OnePosePlusDataset.read_anno` (src/datasets/OnePosePlus_dataset.py:341-437) and of the padding of
`read_anno3d` for `split == "train"` (:105-146, src/utils/data_utils.py:93-209), in front of `build_assignmatrix` (assignmatrix.py):

    project the matched 3D points with the GT pose and intrinsics            opp_project_pairs
    image_warp_adapt: SAP homography (src/utils/sample_homo.py) on the image   opp_homography_warp   (kornia 0.4.1 homography_warp, restated)
                      and on the projected keypoints, out-of-bounds filter     opp_project_pairs / opp_select_pairs
    snap to the 1/8 grid, drop invalid points, one pair per cell (np.unique),  opp_select_pairs
    write the survivors into keypoints2d_coarse / keypoints2d_fine
    conf_matrix_gt / fine_location_matrix_gt                                    opp_build_assignmatrix (unchanged)

The index bookkeeping of the 3D padding runs on the host with upstream's torch global-RNG calls in upstream's order (so
`torch.manual_seed(s)` gives upstream's indices and pad points); the homography is sampled with upstream's `np.random.uniform` draws in
upstream's order.  The gathers, the padding values and everything per pixel / per pair run on the device, on the current stream.
There is no CPU fallback: a non-CUDA device raises RuntimeError.

kornia is not a dependency of this package; `normal_transform_pixel`, `normalize_homography` and the warp are restated from kornia
0.4.1 (the `(w - 1)`, `(h - 1)` convention) and that parity is NOT pinned against the library.
"""
import ctypes

import numpy as np
import torch

from . import _lib

# ---- src/utils/sample_homo.py: similarity-affinity-perspective (SAP) homographies ---------------------------------------------------


def _similarity(angle, tx, ty, s):
    th = np.deg2rad(angle)
    return np.array([[s * np.cos(th), -s * np.sin(th), tx], [s * np.sin(th), s * np.cos(th), ty], [0, 0, 1]])


def compute_homography_sap(h, w, angle=0, tx=0, ty=0, scale=1, k0=1, k1=0, v0=0, v1=0):
    """sample_homo.py:18-42, same products in the same order (float64): H = M_denorm HS HA HP M_norm on the image centred and scaled
    by its half long side.  angle in degrees; tx, ty shift; scale zoom; k0 / k1 squeeze / skew; v0 / v1 perspective."""
    half = max(w / 2, h / 2)
    m_norm = _similarity(0, 0, 0, 1 / half).dot(_similarity(0, -w / 2, -h / 2, 1))
    m_denorm = _similarity(0, w / 2, h / 2, 1).dot(_similarity(0, 0, 0, half))
    hs = _similarity(angle, tx, ty, scale)
    ha = np.array([[k0, k1, 0], [0, 1 / k0, 0], [0, 0, 1]])
    hp = np.array([[1, 0, 0], [0, 1, 0], [v0, v1, 1]])
    return m_denorm.dot(hs).dot(ha).dot(hp).dot(m_norm)


def sample_homography_sap(h, w):
    """sample_homo.py:45-59: seven `np.random.uniform` draws in upstream's order (angle, tx, ty, scale, k1, v0, v1; k0 = 1), so that
    `np.random.seed(s)` gives upstream's matrix."""
    angle = np.random.uniform(-180, 180)
    tx = np.random.uniform(-0.25, 0.25)
    ty = np.random.uniform(-0.25, 0.25)
    scale = np.random.uniform(0.25, 1)
    k1 = np.random.uniform(-0.1, 0.1)
    v0 = np.random.uniform(-0.5, 0.5)
    v1 = np.random.uniform(-0.5, 0.5)
    return compute_homography_sap(h, w, angle, tx, ty, scale, 1, k1, v0, v1)


# ---- kornia 0.4.1 geometry helpers, restated ----------------------------------------------------------------------------------------


def normal_transform_pixel(height, width, dtype=torch.float32):
    """kornia 0.4.1 `normal_transform_pixel`: pixel coordinates -> [-1, 1] with -1 at pixel 0 and +1 at pixel n - 1.  -> [1, 3, 3]"""
    m = torch.tensor([[1.0, 0.0, -1.0], [0.0, 1.0, -1.0], [0.0, 0.0, 1.0]], dtype=dtype)
    m[0, 0] = m[0, 0] * 2.0 / (1e-14 if width == 1 else width - 1.0)
    m[1, 1] = m[1, 1] * 2.0 / (1e-14 if height == 1 else height - 1.0)
    return m.unsqueeze(0)


def normalize_homography(dst_pix_trans_src_pix, dsize_src, dsize_dst):
    """kornia 0.4.1 `normalize_homography`: [B, 3, 3] between pixel coordinates -> between normalised coordinates."""
    H = torch.as_tensor(dst_pix_trans_src_pix)
    if H.dim() != 3 or H.shape[-2:] != (3, 3):
        raise ValueError("normalize_homography expects [B, 3, 3]")
    src_norm_trans_src_pix = normal_transform_pixel(dsize_src[0], dsize_src[1], H.dtype)
    dst_norm_trans_dst_pix = normal_transform_pixel(dsize_dst[0], dsize_dst[1], H.dtype)
    return dst_norm_trans_dst_pix @ (H @ torch.inverse(src_norm_trans_src_pix))


def _device(device):
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("train_sample runs on the device: the HIP path has no CPU fallback")
    return device


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def homography_warp(images, src_homo_dst, align_corners=False):
    """kornia 0.4.1 `homography_warp(images, src_homo_dst, (h, w))` for device images [B, 1, h, w] fp32 (rows may be strided), one
    launch for the batch.  src_homo_dst [B, 3, 3]: the NORMALISED matrix, as read_anno passes `torch.linalg.inv(homo_sampled_normed)`.
    `align_corners=False` is our reading of kornia 0.4.1's default (unpinned: kornia is not at hand; the flag is there to check both)."""
    if not (isinstance(images, torch.Tensor) and images.dim() == 4 and images.shape[1] == 1 and images.dtype == torch.float32):
        raise ValueError("homography_warp expects a [B, 1, h, w] float32 tensor")
    device = _device(images.device)
    lib = _lib.load()
    B, _, h, w = images.shape
    if images.stride(3) != 1 or images.stride(2) < w or (B > 1 and images.stride(0) < (h - 1) * images.stride(2) + w):
        images = images.contiguous()
    mats = torch.as_tensor(src_homo_dst, dtype=torch.float32).to(device).contiguous()
    if mats.shape != (B, 3, 3):
        raise ValueError("homography_warp: src_homo_dst must be [%d, 3, 3]" % B)
    out = torch.empty((B, 1, h, w), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _lib.check(lib.opp_homography_warp(images.data_ptr(), B, h, w, images.stride(2), images.stride(0), mats.data_ptr(),
                                           1 if align_corners else 0, out.data_ptr(), _stream(device)), "opp_homography_warp")
    return out


# ---- read_anno3d's padding for split == "train" -------------------------------------------------------------------------------------


def _append_random_points(keypoints, n_pad):
    """data_utils.py:101-114 / :160-173: uniform points in [-0.5, 0.5)^3 that are not already keypoints, three torch.rand calls a round"""
    while n_pad > 0:
        rand = torch.cat([torch.rand(n_pad, 1) - 0.5, torch.rand(n_pad, 1) - 0.5, torch.rand(n_pad, 1) - 0.5], dim=1)
        exist = (rand[:, None, :] == keypoints[None, :, :]).all(-1).any(1)
        kept = rand[~exist]
        n_pad -= len(kept)
        if len(kept) > 0:
            keypoints = torch.cat([keypoints, kept], dim=0)
    return keypoints


def pad_points_for_training(keypoints3d, descriptors3d, scores3d, coarse_descriptors3d, assign_matrix, shape3d, device=None):
    """`read_anno3d(pad=True)` with `split == "train"` (:105-146): -> (keypoints3d [shape3d, 3], descriptors3d [dim, shape3d],
    scores3d [shape3d, 1], coarse_descriptors3d [dim_c, shape3d] or None, assign_matrix [2, k] int64 on the host or None), the four
    tensors on the device.

    More points than shape3d and an assignment: all matched points stay, the rest is drawn from the unmatched ones
    (`torch.randint`), the result is shuffled (`torch.randperm`) and row 1 of the assignment re-indexed.  Fewer: random pad points
    (`torch.rand` rejection loop), descriptors padded with ones, scores with zeros.  No assignment: the first shape3d points, or the
    same padding.  The index work is done on the host with these global-RNG calls in upstream's order; the gathers and the ones /
    zeros padding run on the device."""
    device = _device(device)
    n = int(shape3d)
    kp = torch.as_tensor(keypoints3d, dtype=torch.float32).cpu()
    if kp.dim() != 2 or kp.shape[1] != 3:
        raise ValueError("keypoints3d must be [m, 3]")
    m = kp.shape[0]
    n_pad = n - m
    index = None
    am = None if assign_matrix is None else torch.as_tensor(assign_matrix).cpu().long().clone()
    if am is not None and n_pad < 0:
        unmatched = torch.ones(m, dtype=torch.bool)
        unmatched[am[1]] = False
        matched_points = kp[am[1]]
        num_of_pad = n - matched_points.shape[0]
        if num_of_pad < 0:
            raise AssertionError("shape3d = %d cannot hold the %d matched points (upstream asserts here)" % (n, matched_points.shape[0]))
        unmatched_idx = torch.arange(m)[unmatched]
        pick = torch.randint(unmatched_idx.shape[0], (num_of_pad,))
        shuffle = torch.randperm(n)
        inverse = torch.zeros(n, dtype=torch.long)
        inverse[shuffle] = torch.arange(n)
        index = torch.cat([am[1], unmatched_idx[pick]])[shuffle]
        kp = kp[index]
        am[1, :] = inverse[: matched_points.shape[0]]
    elif am is None and n_pad < 0:
        index = torch.arange(n)
        kp = kp[:n]
    else:
        kp = _append_random_points(kp, n_pad)
    n_pad = max(n_pad, 0)

    def features(desc):
        if desc is None:
            return None
        d = torch.as_tensor(desc, dtype=torch.float32).to(device)
        if index is not None:
            return d.index_select(1, index.to(device))
        return torch.cat([d, torch.ones((d.shape[0], n_pad), dtype=torch.float32, device=device)], dim=-1)

    sc = torch.as_tensor(scores3d, dtype=torch.float32).to(device)
    sc = sc.index_select(0, index.to(device)) if index is not None else torch.cat([sc, torch.zeros((n_pad, 1), dtype=torch.float32, device=device)], dim=0)
    return kp.to(device), features(descriptors3d), sc, features(coarse_descriptors3d), am


# ---- the pair chain -----------------------------------------------------------------------------------------------------------------


def _host_floats(x, shape):
    a = np.ascontiguousarray(torch.as_tensor(x).detach().cpu().to(torch.float32).numpy().reshape(shape))
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def pixel_homography(homo_sampled_normed, h, w):
    """The matrix read_anno applies to the projected keypoints (:373-386): norm_pixel_mat^-1 . H_normed . norm_pixel_mat, formed in
    float64 from upstream's three fp32 matrices.  -> [3, 3] float32"""
    norm = normal_transform_pixel(h, w)[0]
    return (norm.inverse().double() @ torch.as_tensor(homo_sampled_normed, dtype=torch.float32).double() @ norm.double()).float()


def project_pairs(keypoints3d, assign_matrix, pose_gt, K_crop, homography_px=None, status=None):
    """mkpts_proj [k, 2] fp32 on the device: K (R X + t), x / (z + 1e-6) of the 3D point of every pair (:343-354), then the pixel-space
    homography with the division by its third row (:373-391) when one is given.  keypoints3d [n, 3] and assign_matrix [2, k] are
    taken to the device of keypoints3d (or the current one)."""
    device = _device(keypoints3d.device if isinstance(keypoints3d, torch.Tensor) and keypoints3d.is_cuda else None)
    lib = _lib.load()
    kp = torch.as_tensor(keypoints3d, dtype=torch.float32).to(device).contiguous()
    am = torch.as_tensor(assign_matrix).long().to(device).contiguous()
    if am.dim() != 2 or am.shape[0] != 2 or kp.dim() != 2 or kp.shape[1] != 3:
        raise ValueError("project_pairs: keypoints3d must be [n, 3] and assign_matrix [2, k]")
    k = int(am.shape[1])
    pose = torch.as_tensor(pose_gt)
    _rt, rt_p = _host_floats(pose[:3, :4], (12,))
    _kk, kk_p = _host_floats(torch.as_tensor(K_crop)[:3, :3], (9,))
    _hh, hh_p = (None, None) if homography_px is None else _host_floats(homography_px, (9,))
    out = torch.empty((k, 2), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _lib.check(lib.opp_project_pairs(kp.data_ptr(), int(kp.shape[0]), am.data_ptr(), k, rt_p, kk_p, hh_p, out.data_ptr(),
                                         None if status is None else status.data_ptr(), _stream(device)), "opp_project_pairs")
    return out


def select_pairs(mkpts_proj, assign_matrix, hw, keypoints2d_coarse, warped, coarse_scale=1.0 / 8, status=None):
    """The discrete half of read_anno (:393-433) on the device, exact.  -> (assign_out [2, k] int64, n_out [1] int32, keypoints2d_coarse
    [n2d, 2], keypoints2d_fine [n2d, 2]), all on the device: the first n_out columns of assign_out are upstream's compacted assignment
    in upstream's order, the rest is padding that `opp_build_assignmatrix` drops; keypoints2d_coarse is a copy of the input with the
    survivors' rounded points written in, keypoints2d_fine zeros with their unrounded points."""
    h, w = int(hw[0]), int(hw[1])
    cell = int(1 / coarse_scale)
    if cell <= 0 or h % cell or w % cell:
        raise ValueError("image %d x %d is not a multiple of the coarse cell %d: upstream floors silently, and the model cannot take such an "
                         "image" % (h, w, cell))
    device = _device(mkpts_proj.device if isinstance(mkpts_proj, torch.Tensor) and mkpts_proj.is_cuda else None)
    lib = _lib.load()
    proj = torch.as_tensor(mkpts_proj, dtype=torch.float32).to(device).contiguous()
    am = torch.as_tensor(assign_matrix).long().to(device).contiguous()
    kc = torch.as_tensor(keypoints2d_coarse, dtype=torch.float32).to(device).clone().contiguous()
    if am.dim() != 2 or am.shape[0] != 2 or proj.shape != (am.shape[1], 2) or kc.dim() != 2 or kc.shape[1] != 2:
        raise ValueError("select_pairs: mkpts_proj must be [k, 2], assign_matrix [2, k] and keypoints2d_coarse [n, 2]")
    k, n2d = int(am.shape[1]), int(kc.shape[0])
    kf = torch.zeros((n2d, 2), dtype=torch.float32, device=device)
    out = torch.empty((2, k), dtype=torch.int64, device=device)
    n_out = torch.empty(1, dtype=torch.int32, device=device)
    scratch = torch.empty((h // cell + 1) * (w // cell + 1) + n2d, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.check(lib.opp_select_pairs(proj.data_ptr(), am.data_ptr(), k, h, w, cell, 1 if warped else 0, n2d, kc.data_ptr(), kf.data_ptr(),
                                        out.data_ptr(), n_out.data_ptr(), scratch.data_ptr(), None if status is None else status.data_ptr(),
                                        _stream(device)), "opp_select_pairs")
    return out, n_out, kc, kf


# ---- read_anno's data dict ----------------------------------------------------------------------------------------------------------


def _prepare(query_image, keypoints3d, descriptors3d, scores3d, coarse_descriptors3d, assign_matrix, keypoints2d_coarse, pose_gt, K_crop,
             query_img_scale, warp=False, shape3d=7000, coarse_scale=1.0 / 8, strict=True, homography=None, align_corners=False,
             conf_out=None, floc_out=None):
    """everything of one sample except the image warp -> (data, src_homo_dst or None, status)"""
    if not (isinstance(query_image, torch.Tensor) and query_image.dim() == 3 and query_image.shape[0] == 1):
        raise ValueError("query_image must be a [1, h, w] tensor")
    h, w = int(query_image.shape[1]), int(query_image.shape[2])
    cell = int(1 / coarse_scale)
    if h % cell or w % cell:
        raise ValueError("query image %d x %d is not a multiple of %d (1 / coarse_scale): upstream floors the coarse grid silently, and the "
                         "model cannot take such an image" % (h, w, cell))
    device = _device(query_image.device)
    lib = _lib.load()
    if assign_matrix is None:
        raise ValueError("a training sample needs its assign_matrix")
    h_c, w_c = int(h * coarse_scale), int(w * coarse_scale)
    n, L = int(shape3d), int(h_c * w_c)
    with torch.cuda.device(device):
        kp3d, desc, scores, desc_c, am = pad_points_for_training(keypoints3d, descriptors3d, scores3d, coarse_descriptors3d, assign_matrix,
                                                                 n, device)
        pose = torch.as_tensor(pose_gt)
        K = torch.as_tensor(K_crop)
        scale = torch.as_tensor(query_img_scale, dtype=torch.float32).flatten()
        status = torch.zeros(2, dtype=torch.int32, device=device)          # [0]: projection / selection, [1]: build_assignmatrix
        am_dev = am.to(device)
        intrinsic, src_homo_dst, h_px = K, None, None
        if warp:
            homo = sample_homography_sap(h, w) if homography is None else np.asarray(homography, dtype=np.float64)
            normed = normalize_homography(torch.from_numpy(homo[None]).to(torch.float32), (h, w), (h, w))
            src_homo_dst = torch.linalg.inv(normed)
            h_px = pixel_homography(normed[0], h, w)
            # upstream :401-403 -- "FIXME: incorrect! Shouldn't H \times K directly" -- kept as upstream computes it
            intrinsic = torch.from_numpy(homo).to(torch.float32) @ K.to(torch.float32)
        proj = project_pairs(kp3d, am_dev, pose, K, h_px, status[0:1])
        assign_out, n_out, kc, kf = select_pairs(proj, am_dev, (h, w), keypoints2d_coarse, warp, coarse_scale, status[0:1])
        k = int(am_dev.shape[1])
        conf = torch.empty((n, L), dtype=torch.int16, device=device) if conf_out is None else conf_out
        floc = torch.empty((n, L, 2), dtype=torch.float32, device=device) if floc_out is None else floc_out
        keys = torch.empty(max(k, 1), dtype=torch.int64, device=device)
        _lib.check(lib.opp_build_assignmatrix(kc.data_ptr(), kf.data_ptr(), int(kc.shape[0]), assign_out.data_ptr(), k, n, L, w_c,
                                              float(scale[1]), float(scale[0]), float(coarse_scale), conf.data_ptr(), floc.data_ptr(),
                                              keys.data_ptr(), status[1:2].data_ptr(), _stream(device)), "opp_build_assignmatrix")
    data = {
        "keypoints3d": kp3d,                       # [shape3d, 3]
        "descriptors3d_db": desc,                  # [dim, shape3d]
        "scores3d_db": scores.squeeze(1),          # [shape3d]
        "query_image": query_image,                # [1, h, w]; replaced by the warped image
        "query_image_scale": scale.to(device),
        "query_intrinsic": intrinsic.to(device),
        "query_pose_gt": pose.to(device),
        "conf_matrix_gt": conf,                    # [shape3d, h_c * w_c] int16
        "fine_location_matrix_gt": floc,           # [shape3d, h_c * w_c, 2]
        "n_pairs": n_out,                          # [1] int32 on the device: the pairs that survived the filters
    }
    if desc_c is not None:
        data["descriptors3d_coarse_db"] = desc_c
    return data, src_homo_dst, (status if strict else None)


def _raise_if_flagged(status):
    if status is not None:
        st = status.cpu()
        if int(st[0]) & 1 or int(st[1]) & 1:
            raise IndexError("make_train_sample: a keypoint / point / grid index is out of range or a projection is not finite (the "
                             "reference raises here as well)")


def make_train_sample(query_image, keypoints3d, descriptors3d, scores3d, coarse_descriptors3d, assign_matrix, keypoints2d_coarse, pose_gt,
                      K_crop, query_img_scale, warp=False, shape3d=7000, coarse_scale=1.0 / 8, strict=True, homography=None,
                      align_corners=False):
    """The data dict of `read_anno` for one training sample, made on the device of `query_image` ([1, h, w] fp32, e.g. from
    `ingest.read_grayscale_u8`), on the current stream: `query_image`, `query_intrinsic`, `keypoints3d`, `descriptors3d_db`,
    `descriptors3d_coarse_db` (when coarse descriptors are given), `scores3d_db`, `conf_matrix_gt`, `fine_location_matrix_gt`, beside the
    small `query_image_scale`, `query_pose_gt` and `n_pairs`.

    keypoints3d [m, 3], descriptors3d [dim, m], scores3d [m, 1], coarse_descriptors3d [dim_c, m] or None: the object's averaged
    annotation; assign_matrix [2, k] and keypoints2d_coarse [n2d, 2]: the image's coarse annotation; pose_gt [4, 4] (or [3, 4]), K_crop
    [3, 3]; query_img_scale [2].  warp=True is upstream's `image_warp_adapt` sample: a homography from `sample_homography_sap(h, w)`
    (numpy global RNG), or `homography=` [3, 3] in pixels; `query_intrinsic` is then `H @ K` as upstream forms it.  strict: raise
    IndexError where upstream's indexing would (the only host synchronisation)."""
    data, src_homo_dst, status = _prepare(query_image, keypoints3d, descriptors3d, scores3d, coarse_descriptors3d, assign_matrix,
                                          keypoints2d_coarse, pose_gt, K_crop, query_img_scale, warp, shape3d, coarse_scale, strict, homography,
                                          align_corners)
    if src_homo_dst is not None:
        data["query_image"] = homography_warp(data["query_image"][None], src_homo_dst, align_corners)[0]
    _raise_if_flagged(status)
    return data


def make_train_batch(samples):
    """A collated batch from a list of `make_train_sample` keyword dicts (same image size and shape3d): the two ground-truth matrices
    are written straight into their [B, ...] tensors and all warped images go through ONE `opp_homography_warp` launch."""
    if not samples:
        raise ValueError("make_train_batch: no samples")
    first = samples[0]["query_image"]
    device = _device(first.device)
    h, w = int(first.shape[1]), int(first.shape[2])
    cs = [s.get("coarse_scale", 1.0 / 8) for s in samples]
    n = int(samples[0].get("shape3d", 7000))
    if any(tuple(s["query_image"].shape) != (1, h, w) or int(s.get("shape3d", 7000)) != n or c != cs[0] for s, c in zip(samples, cs)):
        raise ValueError("make_train_batch: the samples of a batch share image size, shape3d and coarse_scale")
    B, L = len(samples), int(h * cs[0]) * int(w * cs[0])
    conf = torch.empty((B, n, L), dtype=torch.int16, device=device)
    floc = torch.empty((B, n, L, 2), dtype=torch.float32, device=device)
    parts = [_prepare(conf_out=conf[b], floc_out=floc[b], **s) for b, s in enumerate(samples)]
    images = torch.stack([d["query_image"].to(torch.float32) for d, _, _ in parts])
    warped = [b for b, (_, m, _) in enumerate(parts) if m is not None]
    if warped:
        flags = {bool(samples[b].get("align_corners", False)) for b in warped}
        if len(flags) != 1:
            raise ValueError("make_train_batch: one align_corners setting per batch")
        images[warped] = homography_warp(images[warped], torch.cat([parts[b][1] for b in warped]), flags.pop())
    for _, _, status in parts:
        _raise_if_flagged(status)
    batch = {"query_image": images, "conf_matrix_gt": conf, "fine_location_matrix_gt": floc}
    for key in parts[0][0]:
        if key not in batch:
            vals = [d[key] for d, _, _ in parts]
            batch[key] = torch.stack([v.to(torch.float64) if key == "query_intrinsic" else v for v in vals])
    return batch
