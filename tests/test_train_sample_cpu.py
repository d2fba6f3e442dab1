"""Host side of the training-sample builder (onepose_plus_plus_amd/train_sample.py): the restatement the GPU tests compare with
(tests/train_sample_reference.py) against fixtures made by the reference's own statements (tests/golden/gen_train_sample_golden.py), the
host functions of the package against both, and the fp32-vs-fp64 distances that serve as yardsticks on the GPU."""
import os

import numpy as np
import pytest
import torch

from onepose_plus_plus_amd import train_sample as TS
from tests import helpers as H
from tests import test_train_sample_gpu as G
from tests import train_sample_reference as TR


def _dense(gold):
    n, L = [int(v) for v in gold["conf_shape"]]
    conf = torch.zeros(n, L, dtype=torch.int16)
    floc = torch.full((n, L, 2), -50.0)
    pos, fpos = torch.from_numpy(gold["conf_pos"]), torch.from_numpy(gold["floc_pos"])
    conf[pos[:, 0], pos[:, 1]] = 1
    floc[fpos[:, 0], fpos[:, 1]] = torch.from_numpy(gold["floc_val"])
    return conf, floc


@pytest.mark.parametrize("name", list(TR.CASES))
def test_restatement_matches_reference_fixture(name):
    gold = H.load_golden(name)
    inp = TR.make_case(name)
    for key in ("keypoints3d", "assign_matrix", "keypoints2d_coarse", "query_image", "pose_gt", "K_crop"):
        assert np.array_equal(gold["in_" + key], inp[key].numpy()), key        # the fixture's inputs are the ones the seeds regenerate
    out = TR.read_anno_train(inp)
    gconf, gfloc = _dense(gold)
    # discrete outputs and everything that is an index or a copy: bit for bit
    assert np.array_equal(out["assign"].numpy(), gold["out_assign"])
    assert np.array_equal(out["assign_padded"].numpy(), gold["out_assign_padded"])
    assert torch.equal(out["conf_matrix_gt"], gconf)
    assert np.array_equal(out["keypoints3d"].numpy(), gold["out_keypoints3d"])
    assert np.array_equal(out["descriptors3d_db"].numpy(), gold["out_descriptors3d"])
    assert np.array_equal(out["descriptors3d_coarse_db"].numpy(), gold["out_descriptors3d_coarse"])
    assert np.array_equal(out["scores3d_db"].numpy(), gold["out_scores3d"][:, 0])
    assert np.array_equal(out["query_intrinsic"].numpy(), gold["out_query_intrinsic"])
    # the fp32 chain is upstream's statement for statement, so its values agree too
    assert torch.equal(out["fine_location_matrix_gt"], gfloc)
    idx = out["assign"][0]
    assert np.array_equal(out["keypoints2d_coarse"][idx].numpy(), gold["out_keypoints2d_coarse"][idx.numpy()])
    assert np.array_equal(out["keypoints2d_fine"].numpy(), gold["out_keypoints2d_fine"])


@pytest.mark.parametrize("name", list(TR.CASES))
def test_fixture_cases_cover_every_rule(name):
    """every case drops pairs by every rule it can, keeps >= 20, repeats a 2D index, and no decision is within BOUNDARY_MARGIN of its
    boundary -- in the fp32 chain and in the float64 one, which therefore take the same decisions"""
    inp = TR.make_case(name)
    a, b = TR.read_anno_train(inp), TR.read_anno_train(inp, torch.float64)
    assert TR.coverage(a, inp) and TR.coverage(b, inp)
    assert torch.equal(a["assign"], b["assign"]) and torch.equal(a["conf_matrix_gt"], b["conf_matrix_gt"])
    assert (inp["shape3d"] < inp["keypoints3d"].shape[0]) == (a["padding_index"] is not None)


def test_top_n_padding_matches_reference_fixture():
    gold = H.load_golden("train_sample_topn")
    inp = TR.make_case("train_sample_nowarp_pad")
    for tag in ("trunc", "pad"):
        torch.manual_seed(int(gold["torch_seed"]))
        kp, desc, sc, desc_c, am, _ = TR.pad_points(inp["keypoints3d"], inp["descriptors3d"], inp["scores3d"], inp["coarse_descriptors3d"], None,
                                                    int(gold[tag + "_shape3d"]))
        assert am is None
        assert np.array_equal(kp.numpy(), gold[tag + "_keypoints3d"]) and np.array_equal(desc.numpy(), gold[tag + "_descriptors3d"])
        assert np.array_equal(sc.numpy(), gold[tag + "_scores3d"]) and np.array_equal(desc_c.numpy(), gold[tag + "_descriptors3d_coarse"])


def test_sample_homography_sap_matches_upstream_draws():
    gold = H.load_golden("train_sample_homographies")
    assert len(gold) >= 18
    live = None
    from tests.golden.gen_train_sample_golden import REF
    path = os.path.join(REF, "src", "utils", "sample_homo.py")
    if os.path.exists(path):                       # the live module, where the reference checkout is present
        live = {}
        exec(compile(open(path).read(), path, "exec"), live)
    for key, want in gold.items():
        hw, seed = key[1:].split("_s")
        h, w = [int(v) for v in hw.split("x")]
        for fn in (TS.sample_homography_sap, TR.sample_homography_sap) + ((live["sample_homography_sap"],) if live else ()):
            np.random.seed(int(seed))
            got = fn(h, w)
            assert got.dtype == np.float64 and np.array_equal(got, want), key
    assert np.array_equal(TS.compute_homography_sap(64, 96), TR.compute_homography_sap(64, 96))
    assert np.allclose(TS.compute_homography_sap(64, 96), np.eye(3), atol=1e-12)


def test_kornia_helpers_of_the_package_match_the_restatement():
    for h, w in ((64, 96), (512, 512), (72, 104)):
        assert torch.equal(TS.normal_transform_pixel(h, w), TR.normal_transform_pixel(h, w))
        np.random.seed(3)
        homo = torch.from_numpy(TR.sample_homography_sap(h, w)[None]).float()
        normed = TS.normalize_homography(homo, (h, w), (h, w))
        assert torch.equal(normed, TR.normalize_homography(homo, (h, w), (h, w)))
        # the keypoints' matrix norm^-1 . H_normed . norm is the pixel-space homography again, up to fp32 rounding of its factors
        hp = TS.pixel_homography(normed[0], h, w)
        assert hp.dtype == torch.float32 and torch.allclose(hp / hp[2, 2], homo[0] / homo[0, 2, 2], rtol=1e-4, atol=1e-4)
    m = TR.normal_transform_pixel(5, 9)[0]
    assert float(m[0, 0]) == np.float32(2.0) / np.float32(8.0) and float(m[1, 1]) == 0.5 and float(m[0, 2]) == -1.0


def test_no_cpu_fallback_and_size_refusal():
    inp = TR.make_case("train_sample_nowarp_pad")
    kw = dict(query_image=inp["query_image"], keypoints3d=inp["keypoints3d"], descriptors3d=inp["descriptors3d"], scores3d=inp["scores3d"],
              coarse_descriptors3d=None, assign_matrix=inp["assign_matrix"], keypoints2d_coarse=inp["keypoints2d_coarse"],
              pose_gt=inp["pose_gt"], K_crop=inp["K_crop"], query_img_scale=inp["query_img_scale"], shape3d=200)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TS.make_train_sample(**kw)                                        # a CPU image
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TS.homography_warp(torch.zeros(1, 1, 8, 8), torch.eye(3)[None])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TS.pad_points_for_training(inp["keypoints3d"], inp["descriptors3d"], inp["scores3d"], None, None, 200, device="cpu")
    kw["query_image"] = torch.zeros(1, 60, 96)
    with pytest.raises(ValueError, match="not a multiple of 8"):
        TS.make_train_sample(**kw)
    with pytest.raises(ValueError, match="not a multiple"):
        TS.select_pairs(torch.zeros(1, 2), torch.zeros(2, 1), (64, 100), torch.zeros(1, 2), False)


@pytest.mark.parametrize("hw", TR.WARP_SHAPES)
def test_warp_yardstick_is_the_quoted_one(hw):
    """torch's fp32 grid_sample chain against the float64 restatement on the GPU test's cases: the distance the GPU bar is 4 x of stays in
    the range quoted in test_train_sample_gpu's docstring, and every case samples and pads at least 5 % of its pixels."""
    lo, hi = G.QUOTED_WARP_DISTANCE[hw]
    for batch in (1, 3):
        for kind in ("sinusoid", "noise"):
            images, mats, _ = TR.warp_inputs(hw, batch, kind)
            ref, d32 = TR.warp_yardstick(images, mats)
            assert lo <= d32 <= hi, (hw, batch, kind, d32)
            for b in range(batch):
                frac = float((ref[b] != 0).double().mean())
                assert 0.05 <= frac <= 0.95, (hw, batch, b, frac)
    # what the identity test on the GPU is worth: torch's own fp32 chain does NOT return the image bit for bit
    im = torch.rand(1, 1, 64, 96, generator=torch.Generator().manual_seed(1))
    assert not torch.equal(TR.homography_warp(im, torch.eye(3)[None], (64, 96), align_corners=True), im)


@pytest.mark.parametrize("name", list(TR.CASES))
def test_projection_yardstick_is_the_quoted_one(name):
    inp = TR.make_case(name)
    a, b = TR.read_anno_train(inp), TR.read_anno_train(inp, torch.float64)
    d32 = float((a["mkpts_proj"].double() - b["mkpts_proj"]).abs().max())
    print("%s: fp32 chain vs float64, max |d mkpts_proj| = %.3e px" % (name, d32))
    assert G.QUOTED_PROJECTION_DISTANCE[0] <= d32 <= G.QUOTED_PROJECTION_DISTANCE[1]
    assert d32 < 1e-3
