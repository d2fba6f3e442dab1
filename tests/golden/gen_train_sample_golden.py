"""Fixtures for the device-side training-sample builder (onepose_plus_plus_amd/train_sample.py), produced by the REFERENCE'S OWN
statements.  Read from the reference checkout at generation time and compiled unchanged with `ast` (the modules cannot be imported
here: pycocotools / kornia / cv2 are absent):

  * the `if self.split == "train":` block at the end of `OnePosePlusDataset.read_anno` and the method `build_assignmatrix`
    (src/datasets/OnePosePlus_dataset.py), run with a stand-in `self` and stand-in locals;
  * the `if self.split == "train":` block of `read_anno3d` with the four `pad_*` functions it calls (src/utils/data_utils.py, whose
    top-level `import cv2` prevents a plain import);
  * src/utils/sample_homo.py as a whole (it imports cleanly).

The three kornia functions of the warp branch are the restated ones of tests/train_sample_reference.py (kornia is not installed): the
fixtures pin everything around them, not kornia itself.  Runs only where the reference checkout is:

    python tests/golden/gen_train_sample_golden.py

Stores the inputs, the RNG seeds and the outputs (the two matrices in sparse form).  Asserts the coverage conditions of
`train_sample_reference.coverage` before writing.
"""
import ast
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import train_sample_reference as TR  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("OPP_REFERENCE_ROOT", "/root/reference")
HOMOGRAPHY_SEEDS = [0, 1, 2, 3, 5, 7]
HOMOGRAPHY_SIZES = [(64, 96), (512, 512), (72, 104)]


def _is_train_test(node):
    return isinstance(node, ast.If) and ast.unparse(node.test) == "self.split == 'train'"


def _method(cls, name):
    return next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == name)


def load_reference():
    """-> (run_pad(ns), run_train(ns), sample_homo module namespace): the reference's statements as callables over a namespace"""
    ds_path = os.path.join(REF, "src", "datasets", "OnePosePlus_dataset.py")
    cls = next(n for n in ast.parse(open(ds_path).read()).body if isinstance(n, ast.ClassDef) and n.name == "OnePosePlusDataset")
    pad_block = next(n for n in ast.walk(_method(cls, "read_anno3d")) if _is_train_test(n))
    train_block = [n for n in _method(cls, "read_anno").body if _is_train_test(n)][-1]
    assert ast.unparse(train_block.body[0]) == "assign_matrix = assign_matrix.long()"
    build = ast.Module(body=[_method(cls, "build_assignmatrix")], type_ignores=[])

    du_path = os.path.join(REF, "src", "utils", "data_utils.py")
    pads = [n for n in ast.parse(open(du_path).read()).body if isinstance(n, ast.FunctionDef) and n.name in (
        "pad_keypoints3d_top_n", "pad_keypoints3d_according_to_assignmatrix", "pad_features3d_top_n", "pad_features3d_according_to_assignmatrix")]
    assert len(pads) == 4
    du = {"torch": torch, "np": np}
    exec(compile(ast.Module(body=pads, type_ignores=[]), du_path, "exec"), du)
    data_utils = types.SimpleNamespace(**{k: v for k, v in du.items() if k.startswith("pad_")})

    sh_path = os.path.join(REF, "src", "utils", "sample_homo.py")
    sh = {}
    exec(compile(open(sh_path).read(), sh_path, "exec"), sh)

    pad_code = compile(ast.Module(body=pad_block.body, type_ignores=[]), ds_path, "exec")
    train_code = compile(ast.Module(body=train_block.body, type_ignores=[]), ds_path, "exec")
    logger = types.SimpleNamespace(warning=lambda *a, **k: None)
    bns = {"torch": torch, "np": np, "logger": logger}
    exec(compile(build, ds_path, "exec"), bns)

    def run_pad(ns):
        ns.update({"torch": torch, "np": np, "data_utils": data_utils})
        exec(pad_code, ns)
        return ns

    def run_train(ns):
        ns.update({"torch": torch, "np": np, "sample_homography_sap": sh["sample_homography_sap"], "normalize_homography": TR.normalize_homography,
                   "homography_warp": TR.homography_warp, "normal_transform_pixel": TR.normal_transform_pixel})
        ns["self"].build_assignmatrix = lambda *a, **k: bns["build_assignmatrix"](ns["self"], *a, **k)
        exec(train_code, ns)
        return ns

    return run_pad, run_train, sh


def reference_sample(run_pad, run_train, inp):
    """one sample through the reference's statements, in read_anno's order: read_anno3d's padding, then the training block"""
    h, w = inp["hw"]
    self = types.SimpleNamespace(split="train", shape3d=inp["shape3d"], pad=True, coarse_scale=1 / 8, h_i=h, w_i=w, w_c=int(w / 8),
                                 n_query_coarse_grid=int(int(h / 8) * int(w / 8)), query_img_scale=inp["query_img_scale"])
    torch.manual_seed(inp["torch_seed"])
    p = run_pad({"self": self, "keypoints3d": inp["keypoints3d"].clone(), "avg_descriptors3d": inp["descriptors3d"].clone(),
                 "avg_scores": inp["scores3d"].clone(), "avg_coarse_descriptors3d": inp["coarse_descriptors3d"].clone(),
                 "avg_coarse_scores": inp["scores3d"].clone(), "assignmatrix": inp["assign_matrix"].clone()})
    np.random.seed(inp["np_seed"])
    data = {"query_image": inp["query_image"].clone()}
    t = run_train({"self": self, "assign_matrix": p["assignmatrix"], "keypoints3d": p["keypoints3d"], "pose_gt": inp["pose_gt"],
                   "K_crop": inp["K_crop"], "keypoints2d_coarse": inp["keypoints2d_coarse"].clone(), "image_warp_adapt": inp["warp"],
                   "data": data, "query_img": inp["query_image"]})
    return p, t


def main():
    run_pad, run_train, sh = load_reference()
    for name in TR.CASES:
        inp = TR.make_case(name)
        mine = TR.read_anno_train(inp)
        assert TR.coverage(mine, inp), (name, mine["drops"], mine["assign"].shape)
        assert TR.coverage(TR.read_anno_train(inp, torch.float64), inp), name
        p, t = reference_sample(run_pad, run_train, inp)
        conf, floc = t["data"]["conf_matrix_gt"], t["data"]["fine_location_matrix_gt"]
        pos = torch.nonzero(conf)
        fpos = torch.nonzero((floc != -50).any(-1))
        out = {
            "out_keypoints3d": p["keypoints3d"].numpy(), "out_descriptors3d": p["avg_descriptors3d"].numpy(),
            "out_descriptors3d_coarse": p["avg_coarse_descriptors3d"].numpy(), "out_scores3d": p["avg_scores"].numpy(),
            "out_assign_padded": p["assignmatrix"].long().numpy(), "out_assign": t["assign_matrix"].numpy(),
            "out_keypoints2d_coarse": torch.as_tensor(t["keypoints2d_coarse"]).numpy(),
            "out_keypoints2d_fine": torch.as_tensor(t["keypoints2d_fine"]).numpy(),
            "conf_shape": np.array(conf.shape), "conf_pos": pos.numpy(), "floc_pos": fpos.numpy(),
            "floc_val": floc[fpos[:, 0], fpos[:, 1]].numpy(),
            "out_query_intrinsic": t["data"]["query_intrinsic"].numpy() if inp["warp"] else inp["K_crop"].numpy(),
        }
        ins = {"in_" + k: (v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in inp.items()}
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **ins, **out)
        print(name, "pairs kept:", out["out_assign"].shape[1], "ones:", len(pos), "drops:", mine["drops"])

    # the top-n branch (no assignment) of read_anno3d, truncating and padding
    inp = TR.make_case("train_sample_nowarp_pad")
    topn = {}
    for tag, shape3d in (("trunc", 90), ("pad", 170)):
        self = types.SimpleNamespace(split="train", shape3d=shape3d)
        torch.manual_seed(7)
        p = run_pad({"self": self, "keypoints3d": inp["keypoints3d"].clone(), "avg_descriptors3d": inp["descriptors3d"].clone(),
                     "avg_scores": inp["scores3d"].clone(), "avg_coarse_descriptors3d": inp["coarse_descriptors3d"].clone(),
                     "avg_coarse_scores": inp["scores3d"].clone(), "assignmatrix": None})
        topn.update({tag + "_shape3d": np.array(shape3d), tag + "_keypoints3d": p["keypoints3d"].numpy(),
                     tag + "_descriptors3d": p["avg_descriptors3d"].numpy(), tag + "_scores3d": p["avg_scores"].numpy(),
                     tag + "_descriptors3d_coarse": p["avg_coarse_descriptors3d"].numpy()})
    np.savez_compressed(os.path.join(HERE, "train_sample_topn.npz"), torch_seed=np.array(7), **topn)

    # sample_homography_sap under fixed numpy seeds
    homos = {}
    for hw in HOMOGRAPHY_SIZES:
        for s in HOMOGRAPHY_SEEDS:
            np.random.seed(s)
            homos["h%dx%d_s%d" % (hw[0], hw[1], s)] = sh["sample_homography_sap"](hw[0], hw[1])
    np.savez_compressed(os.path.join(HERE, "train_sample_homographies.npz"), **homos)
    print("homographies:", len(homos))


if __name__ == "__main__":
    main()
