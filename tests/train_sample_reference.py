"""Host restatement of a training sample's construction: the training branch of `OnePosePlusDataset.read_anno`
(src/datasets/OnePosePlus_dataset.py:341-437), `read_anno3d`'s padding for split == "train" (:105-146, src/utils/data_utils.py:93-209),
`src/utils/sample_homo.py` and the three kornia 0.4.1 functions read_anno imports (restated: kornia is not installed anywhere this
project runs, so that part is our reading of 0.4.1 and is not pinned against the library).  TEST INFRASTRUCTURE ONLY: the yardstick of
`onepose_plus_plus_amd.train_sample`, itself pinned against fixtures made by the reference's own statements
(tests/golden/gen_train_sample_golden.py).  numpy + torch on the CPU, nothing else.

`dtype=torch.float32` follows upstream's statements literally (the chain a user of the reference runs); `dtype=torch.float64` runs the same
statements in double: the yardstick for the approximate half.  The discrete half (`select_pairs`) is dtype-agnostic and exact.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import assignmatrix_oracle as AO

# ---- sample_homo.py -----------------------------------------------------------------------------------------------------------------


def _sim(angle, tx, ty, s):
    th = np.deg2rad(angle)
    return np.array([[s * np.cos(th), -s * np.sin(th), tx], [s * np.sin(th), s * np.cos(th), ty], [0, 0, 1]])


def compute_homography_sap(h, w, angle=0, tx=0, ty=0, scale=1, k0=1, k1=0, v0=0, v1=0):
    ms = max(w / 2, h / 2)
    m_norm = _sim(0, 0, 0, 1 / ms).dot(_sim(0, -w / 2, -h / 2, 1))
    m_denorm = _sim(0, w / 2, h / 2, 1).dot(_sim(0, 0, 0, ms))
    return m_denorm.dot(_sim(angle, tx, ty, scale)).dot(np.array([[k0, k1, 0], [0, 1 / k0, 0], [0, 0, 1]])).dot(
        np.array([[1, 0, 0], [0, 1, 0], [v0, v1, 1]])).dot(m_norm)


def sample_homography_sap(h, w):
    u = np.random.uniform
    angle, tx, ty, scale = u(-180, 180), u(-0.25, 0.25), u(-0.25, 0.25), u(0.25, 1)
    k1, v0, v1 = u(-0.1, 0.1), u(-0.5, 0.5), u(-0.5, 0.5)
    return compute_homography_sap(h, w, angle, tx, ty, scale, 1, k1, v0, v1)


# ---- kornia 0.4.1, restated ---------------------------------------------------------------------------------------------------------


def normal_transform_pixel(height, width, dtype=torch.float32):
    tr = torch.tensor([[1.0, 0.0, -1.0], [0.0, 1.0, -1.0], [0.0, 0.0, 1.0]], dtype=dtype)
    tr[0, 0] = tr[0, 0] * 2.0 / (width - 1.0)
    tr[1, 1] = tr[1, 1] * 2.0 / (height - 1.0)
    return tr.unsqueeze(0)


def normalize_homography(dst_pix_trans_src_pix, dsize_src, dsize_dst):
    dt = dst_pix_trans_src_pix.dtype
    src_pix_trans_src_norm = torch.inverse(normal_transform_pixel(dsize_src[0], dsize_src[1], dt))
    return normal_transform_pixel(dsize_dst[0], dsize_dst[1], dt) @ (dst_pix_trans_src_pix @ src_pix_trans_src_norm)


def homography_warp(patch_src, src_homo_dst, dsize, mode="bilinear", padding_mode="zeros", align_corners=False):
    """grid linspace(-1, 1) -> transform_points (scale 1 / z where |z| > 1e-8, else 1) -> grid_sample; dtype of patch_src"""
    h, w = dsize
    dt = patch_src.dtype
    xs, ys = torch.linspace(-1, 1, w, dtype=dt), torch.linspace(-1, 1, h, dtype=dt)
    grid = torch.stack(torch.meshgrid(xs, ys, indexing="xy"), dim=-1)[None]                  # [1, h, w, 2] (x, y)
    pts = torch.cat([grid, torch.ones_like(grid[..., :1])], dim=-1)                           # homogeneous
    out = torch.matmul(src_homo_dst.to(dt)[:, None, None], pts[..., None]).squeeze(-1)         # [B, h, w, 3]
    z = out[..., -1:]
    scale = torch.where(z.abs() > 1e-8, 1.0 / z, torch.ones_like(z))
    return F.grid_sample(patch_src, scale * out[..., :2], mode=mode, padding_mode=padding_mode, align_corners=align_corners)


# ---- data_utils.py: padding for split == "train" ------------------------------------------------------------------------------------


def _random_pad(keypoints, n_pad):
    while n_pad > 0:
        rand = torch.cat([torch.rand(n_pad, 1) - 0.5 for _ in range(3)], dim=1)
        kept = rand[~(rand[:, None, :] == keypoints[None, :, :]).all(-1).any(1)]
        n_pad -= len(kept)
        if len(kept) > 0:
            keypoints = torch.cat([keypoints, kept], dim=0)
    return keypoints


def pad_points(keypoints3d, descriptors3d, scores3d, coarse_descriptors3d, assign_matrix, shape3d):
    """-> keypoints3d [shape3d, 3], descriptors3d [dim, shape3d], scores3d [shape3d, 1], coarse descriptors or None, assign_matrix
    (long, row 1 re-indexed) or None, index [shape3d] of the kept points or None when padded"""
    n_pad = shape3d - keypoints3d.shape[0]
    index = None
    if assign_matrix is not None:
        assign_matrix = assign_matrix.long().clone()
    if n_pad < 0 and assign_matrix is not None:
        unmatched = torch.ones(keypoints3d.shape[0], dtype=torch.bool)
        unmatched[assign_matrix[1]] = False
        k = assign_matrix.shape[1]
        assert shape3d - k >= 0
        rand_idx = torch.randint(int(unmatched.sum()), (shape3d - k,))
        shuffle = torch.randperm(shape3d)
        inv = torch.zeros(shape3d, dtype=torch.long)
        inv[shuffle] = torch.arange(shape3d)
        index = torch.cat([assign_matrix[1], torch.arange(keypoints3d.shape[0])[unmatched][rand_idx]])[shuffle]
        keypoints3d = keypoints3d[index]
        assign_matrix[1, :] = inv[:k]
    elif n_pad < 0:
        index = torch.arange(shape3d)
        keypoints3d = keypoints3d[:shape3d]
    else:
        keypoints3d = _random_pad(keypoints3d, n_pad)

    def feat(d):
        if d is None:
            return None
        return d[:, index] if index is not None else torch.cat([d, torch.ones(d.shape[0], n_pad)], dim=-1)

    scores3d = scores3d[index] if index is not None else torch.cat([scores3d, torch.zeros(n_pad, 1)], dim=0)
    return keypoints3d, feat(descriptors3d), scores3d, feat(coarse_descriptors3d), assign_matrix, index


# ---- read_anno, training branch -----------------------------------------------------------------------------------------------------


def project(keypoints3d, assign_matrix, pose_gt, K_crop, homo_sampled, hw, dtype):
    """mkpts_proj [k, 2] BEFORE any filter (:343-391); homo_sampled: pixel-space [3, 3] float64 numpy or None"""
    h, w = hw
    npdt = np.float32 if dtype == torch.float32 else np.float64
    mkpts_3d = keypoints3d.to(dtype)[assign_matrix.long()[1, :]]
    R, t, K = pose_gt[:3, :3].to(dtype), pose_gt[:3, [3]].to(dtype), K_crop.to(dtype)
    proj = (K @ (R @ mkpts_3d.transpose(1, 0) + t)).transpose(1, 0)
    proj = proj[:, :2] / (proj[:, [2]] + 1e-6)
    if homo_sampled is None:
        return proj
    normed_h = normalize_homography(torch.from_numpy(homo_sampled[None]).to(dtype), (h, w), (h, w))
    norm = normal_transform_pixel(h, w, dtype)
    pts = (norm[0].numpy() @ np.concatenate([proj.numpy(), np.ones((proj.shape[0], 1))], axis=-1).T).astype(npdt)
    warped = ((norm[0].inverse() @ normed_h[0]).numpy() @ pts).T
    warped[:, :2] /= warped[:, [2]]                      # "NOTE: Important! [:, 2] is not all 1!"
    return torch.from_numpy(np.ascontiguousarray(warped[:, :2]))


def select_pairs(mkpts_proj, assign_matrix, hw, warped, keypoints2d_coarse, cell=8, diagnostics=True):
    """The discrete half (:393-433) on given points.  -> dict: assign [2, k'], keypoints2d_coarse / keypoints2d_fine (float32, the
    latter zeros where not written), and how many pairs each rule dropped"""
    h, w = hw
    proj = mkpts_proj.clone()
    am = assign_matrix.long().clone()
    kc = keypoints2d_coarse.clone()
    kf = torch.zeros((kc.shape[0], 2), dtype=torch.float)
    drops = {"oob": 0}
    if warped:
        oob = (proj[:, 0] < 0) | (proj[:, 0] > (w - 1)) | (proj[:, 1] < 0) | (proj[:, 1] > (h - 1))
        drops["oob"] = int(oob.sum())
        proj, am = proj[~oob], am[:, ~oob]
    rounded = (proj / cell).round() * cell
    invalid = (rounded[:, 0] < 0) | (rounded[:, 0] > w - 1) | (rounded[:, 1] < 0) | (rounded[:, 1] > h - 1)
    drops["invalid"] = int(invalid.sum())
    rounded, proj, am = rounded[~invalid], proj[~invalid], am[:, ~invalid]
    _, index = np.unique(rounded.numpy(), return_index=True, axis=0)
    drops["duplicate"] = int(rounded.shape[0] - len(index))
    first_not_lex_first = False
    if diagnostics and len(index):
        # a repeated cell whose kept (first) occurrence is not the smallest row under a full lexicographic sort of the unrounded points
        for i in index:
            same = (rounded == rounded[i]).all(-1).nonzero().flatten()
            if len(same) > 1 and int(same[np.lexsort((proj[same, 1].numpy(), proj[same, 0].numpy()))[0]]) != int(i):
                first_not_lex_first = True
    index = torch.from_numpy(index)
    rounded, proj, am = rounded[index], proj[index], am[:, index]
    kc[am[0, :]] = rounded.to(kc.dtype)
    kf[am[0, :]] = proj.to(kf.dtype)
    drops["repeated_2d"] = int(am.shape[1] - len(torch.unique(am[0])))
    return {"assign": am, "keypoints2d_coarse": kc, "keypoints2d_fine": kf, "drops": drops, "first_not_lex_first": first_not_lex_first}


def read_anno_train(inp, dtype=torch.float32, align_corners=False, reseed=True, diagnostics=True):
    """The whole chain for one sample `inp` (see make_case): padding under torch.manual_seed(inp["torch_seed"]), a homography under
    np.random.seed(inp["np_seed"]) when inp["warp"] (reseed=False: both global generators are used as they stand, as for the later
    samples of a batch).  -> the data dict of read_anno plus the intermediate results"""
    h, w = inp["hw"]
    cs = 1.0 / 8
    if reseed:
        torch.manual_seed(inp["torch_seed"])
    kp3d, desc, scores, desc_c, am, index = pad_points(inp["keypoints3d"], inp["descriptors3d"], inp["scores3d"], inp["coarse_descriptors3d"],
                                                       inp["assign_matrix"], inp["shape3d"])
    homo = None
    image, intrinsic = inp["query_image"], inp["K_crop"]
    if inp["warp"]:
        if reseed:
            np.random.seed(inp["np_seed"])
        homo = sample_homography_sap(h, w)
        normed = normalize_homography(torch.from_numpy(homo[None]).to(dtype), (h, w), (h, w))
        image = homography_warp(image[None].to(dtype), torch.linalg.inv(normed), (h, w), align_corners=align_corners)[0]
        intrinsic = torch.from_numpy(homo).to(torch.float32) @ inp["K_crop"].to(torch.float32)
    proj = project(kp3d, am, inp["pose_gt"], inp["K_crop"], homo, (h, w), dtype)
    sel = select_pairs(proj, am, (h, w), inp["warp"], inp["keypoints2d_coarse"], int(1 / cs), diagnostics)
    conf, floc = AO.build_assignmatrix(sel["keypoints2d_coarse"], sel["keypoints2d_fine"], sel["assign"], inp["shape3d"], (h // 8) * (w // 8), w // 8,
                                       inp["query_img_scale"], cs)
    return {"keypoints3d": kp3d, "descriptors3d_db": desc, "descriptors3d_coarse_db": desc_c, "scores3d_db": scores.squeeze(1),
            "query_image": image, "query_intrinsic": intrinsic, "conf_matrix_gt": conf, "fine_location_matrix_gt": floc,
            "mkpts_proj": proj, "assign_padded": am, "padding_index": index, "homography": homo, **sel}


# ---- inputs -------------------------------------------------------------------------------------------------------------------------

BOUNDARY_MARGIN = 1e-2       # px: no decision of a fixture case is closer than this to its boundary (ten times the fp32 bar of the projection)

# name -> (hw, number of 3D points, shape3d, k pairs, number of 2D keypoints, warp, input seed, torch seed, numpy seed)
CASES = {
    "train_sample_nowarp_pad": ((64, 96), 150, 200, 100, 80, False, 11, 101, 0),
    "train_sample_nowarp_trunc": ((64, 96), 150, 120, 100, 80, False, 12, 102, 0),
    "train_sample_warp_pad": ((64, 96), 150, 200, 100, 80, True, 13, 103, 3),
    "train_sample_warp_trunc": ((64, 96), 150, 120, 100, 80, True, 14, 104, 5),
}


def boundary_distance(coords, hw):
    """smallest distance of any coordinate [n, 2] (x, y) to 0, w - 1 / h - 1 and the rounding edges 8 m + 4"""
    c = np.asarray(coords, dtype=np.float64)
    lim = np.array([hw[1] - 1.0, hw[0] - 1.0])
    d = np.minimum(np.abs(c), np.abs(c - lim))
    return np.minimum(d, np.abs(np.mod(c, 8.0) - 4.0)).min(axis=-1)


def make_case(name, fine_dim=8, coarse_dim=16):
    """the stand-in annotation arrays of fixture case `name` (make_inputs)"""
    return make_inputs(*CASES[name], fine_dim=fine_dim, coarse_dim=coarse_dim)


def make_inputs(hw, n3d, shape3d, k, n2d, warp, seed, torch_seed, np_seed, fine_dim=8, coarse_dim=16):
    """Stand-in annotation arrays of one sample.  The 3D points are back-projected in float64 from chosen pixels of the FINAL image (the
    warped one for a warp case, through the inverse of the case's homography), drawn on a domain 6 px larger than the image so that every
    filter has something to drop, and only pixels whose float64 re-projection keeps BOUNDARY_MARGIN from every decision boundary are used."""
    h, w = hw
    rng = np.random.default_rng(seed)
    ax = rng.standard_normal(3)
    ax = ax / np.linalg.norm(ax) * 0.4
    th = np.linalg.norm(ax)
    kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]]) / th
    R = np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * kx @ kx
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = R, [0.1, -0.05, 2.0]
    K = np.array([[110.0, 0, w / 2 - 0.7], [0, 105.0, h / 2 + 0.4], [0, 0, 1]])
    homo = None
    if warp:
        state = np.random.get_state()
        np.random.seed(np_seed)
        homo = sample_homography_sap(h, w)
        np.random.set_state(state)
    pose_t, K_t = torch.from_numpy(pose), torch.from_numpy(K)
    pts = np.zeros((0, 3), dtype=np.float32)
    while len(pts) < n3d:
        pix = rng.uniform([-6.0, -6.0], [w + 5.0, h + 5.0], size=(4 * n3d, 2))
        src = pix
        if warp:
            q = np.linalg.inv(homo) @ np.concatenate([pix, np.ones((len(pix), 1))], axis=-1).T
            src = (q[:2] / q[2]).T
        z = rng.uniform(1.5, 3.0, size=(len(src), 1))
        cam = (np.linalg.inv(K) @ np.concatenate([src, np.ones((len(src), 1))], axis=-1).T).T * z
        X = ((cam - pose[:3, 3]) @ R).astype(np.float32)              # R^T (cam - t), rounded to what the loader stores
        idx = torch.arange(len(X))[None].repeat(2, 1)
        back = project(torch.from_numpy(X), idx, pose_t, K_t, homo, hw, torch.float64).numpy()
        good = (boundary_distance(back, hw) >= 2 * BOUNDARY_MARGIN) & np.isfinite(back).all(-1) & (np.abs(back - pix).max(-1) < 1e-2)
        pts = np.concatenate([pts, X[good]])
    pts = pts[:n3d]
    g = torch.Generator().manual_seed(seed)
    am = torch.stack([torch.randint(0, n2d, (k,), generator=g), torch.randint(0, n3d, (k,), generator=g)]).float()
    am[:, k // 2: k // 2 + k // 10] = am[:, : k // 10]                   # repeated pairs: duplicate cells by construction
    return {
        "hw": hw, "shape3d": shape3d, "warp": warp, "torch_seed": torch_seed, "np_seed": np_seed,
        "query_image": torch.rand(1, h, w, generator=g),
        "keypoints3d": torch.from_numpy(pts),
        "descriptors3d": torch.randn(fine_dim, n3d, generator=g),
        "scores3d": torch.rand(n3d, 1, generator=g),
        "coarse_descriptors3d": torch.randn(coarse_dim, n3d, generator=g),
        "assign_matrix": am,                                             # float, as read_anno2d returns it
        "keypoints2d_coarse": torch.rand(n2d, 2, generator=g) * torch.tensor([w - 1.0, h - 1.0]),
        "pose_gt": pose_t, "K_crop": K_t, "query_img_scale": torch.ones(2),
    }


WARP_SHAPES = [(8, 8), (64, 96), (72, 104)]
WARP_SEEDS = {1: [3], 3: [0, 5, 7]}          # batch size -> numpy seeds of its homographies


def warp_inputs(hw, batch, kind):
    """-> images [B, 1, h, w] float32 in [0, 1] ("sinusoid": smooth, "noise": uniform), src_homo_dst [B, 3, 3] float32 as read_anno
    forms it (inverse of the normalised fp32 homography), the pixel-space homographies [B, 3, 3] float64"""
    h, w = hw
    g = torch.Generator().manual_seed(1000 * h + w + batch)
    if kind == "noise":
        images = torch.rand(batch, 1, h, w, generator=g)
    else:
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
        images = torch.stack([(0.5 + 0.25 * torch.sin(0.37 * (b + 1) * xx + 0.3 * b) + 0.25 * torch.cos(0.23 * yy * (b + 1) + 0.11 * xx))
                              for b in range(batch)])[:, None].float()
    homos = []
    state = np.random.get_state()
    for s in WARP_SEEDS[batch]:
        np.random.seed(s)
        homos.append(sample_homography_sap(h, w))
    np.random.set_state(state)
    homos = np.stack(homos)
    src_homo_dst = torch.linalg.inv(normalize_homography(torch.from_numpy(homos).to(torch.float32), (h, w), (h, w)))
    return images, src_homo_dst, homos


def warp_yardstick(images, src_homo_dst, align_corners=False):
    """-> (float64 restatement of the warp of these fp32 inputs, the distance of torch's own fp32 chain from it: max |difference|)"""
    hw = images.shape[-2:]
    ref = homography_warp(images.double(), src_homo_dst.double(), hw, align_corners=align_corners)
    f32 = homography_warp(images, src_homo_dst, hw, align_corners=align_corners)
    return ref, float((f32.double() - ref).abs().max())


def coverage(out, inp):
    """the conditions every fixture case meets (asserted by the generator and by the CPU test)"""
    d = out["drops"]
    ok = d["invalid"] > 0 and d["duplicate"] > 0 and out["assign"].shape[1] >= 20 and d["repeated_2d"] > 0
    if inp["warp"]:
        ok = ok and d["oob"] > 0
    used = out["mkpts_proj"].numpy()
    return bool(ok) and float(boundary_distance(used, inp["hw"]).min()) >= BOUNDARY_MARGIN
