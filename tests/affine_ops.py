"""`opp_affine2d_ransac_batch` called directly, with every byte of device memory taken from a `tests.hip_ops.Buffers` object, for
tests/test_affine_gpu.py and tests/test_affine_contract_gpu.py."""
import ctypes

import numpy as np
import torch

from onepose_plus_plus_amd import _lib
from tests import affine_cases as AC
from tests import hip_ops as ops


def concat(views):
    """list of (p0 [n,2], p1 [n,2]) -> (p0 [N,2] float32, p1 [N,2] float32, offsets [V+1] int32)"""
    p0 = np.concatenate([np.asarray(v[0], np.float32).reshape(-1, 2) for v in views]) if views else np.zeros((0, 2), np.float32)
    p1 = np.concatenate([np.asarray(v[1], np.float32).reshape(-1, 2) for v in views]) if views else np.zeros((0, 2), np.float32)
    off = np.concatenate([[0], np.cumsum([np.asarray(v[0]).reshape(-1, 2).shape[0] for v in views])]).astype(np.int32)
    return p0, p1, off


def run_raw(views, seeds, iterations, confidence=0.99, refine=True, corners=None, fallback=AC.FALLBACK, thr=AC.THR, offsets=None,
            record=True, bufs=None):
    """-> dict of CPU tensors: affine [V,2,3], mask [N], n_inliers, ok, stop [V], boxes [V,4], best_view [1], best_box [4] and, with
    `record`, samples [V,I,3] and scores [V,I].  offsets: replaces the ones of the concatenation (V = len(offsets) - 1)."""
    lib = _lib.load()
    bufs = bufs or ops.DEFAULT_BUFFERS
    p0, p1, off = concat(views)
    if offsets is not None:
        off = np.asarray(offsets, np.int32)
    V, N = off.shape[0] - 1, p0.shape[0]
    cor = np.tile(AC.corners_of(AC.REF_HW), (V, 1, 1)) if corners is None else np.asarray(corners, np.float64).reshape(V, 4, 2)
    i32 = torch.int32
    d0 = bufs.input(torch.from_numpy(p0 if N else np.zeros((1, 2), np.float32)), "pts0")
    d1 = bufs.input(torch.from_numpy(p1 if N else np.zeros((1, 2), np.float32)), "pts1")
    doff = bufs.input(torch.from_numpy(off), "offsets")
    dseed = bufs.input(torch.from_numpy((np.asarray(seeds, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32).copy()), "seeds")
    dcor = bufs.input(torch.from_numpy(np.ascontiguousarray(cor)), "corners")
    out = {"affine": bufs.output((V, 2, 3), torch.float64, name="affine"), "mask": bufs.output(max(N, 1), i32, fill=-7, name="mask"),
           "n_inliers": bufs.output(V, i32, fill=-7, name="n_inliers"), "ok": bufs.output(V, i32, fill=-7, name="ok"),
           "stop": bufs.output(V, i32, fill=-7, name="stop"), "boxes": bufs.output((V, 4), i32, fill=-7, name="boxes"),
           "best_view": bufs.output(1, i32, fill=-7, name="best_view"), "best_box": bufs.output(4, i32, fill=-7, name="best_box")}
    if record:
        out["samples"] = bufs.output((V, iterations, 3), i32, fill=-7, name="samples")
        out["scores"] = bufs.output((V, iterations), i32, fill=-7, name="scores")
    ws = bufs.workspace(lib.opp_affine2d_batch_workspace_bytes(iterations, V, N))
    fb = (ctypes.c_int * 4)(*[int(x) for x in fallback])
    stream = torch.cuda.current_stream().cuda_stream
    bufs.call(lib.opp_affine2d_ransac_batch(
        d0.data_ptr(), d1.data_ptr(), doff.data_ptr(), V, N, dseed.data_ptr(), dcor.data_ptr(), float(thr), int(iterations), float(confidence),
        1 if refine else 0, fb, out["affine"].data_ptr(), out["mask"].data_ptr(), out["n_inliers"].data_ptr(), out["ok"].data_ptr(),
        out["stop"].data_ptr(), out["boxes"].data_ptr(), out["best_view"].data_ptr(), out["best_box"].data_ptr(),
        out["samples"].data_ptr() if record else None, out["scores"].data_ptr() if record else None, ws.data_ptr(), bufs.ws_bytes(ws), stream),
        "opp_affine2d_ransac_batch")
    torch.cuda.synchronize()
    res = {k: v.cpu() for k, v in out.items()}
    res["mask"] = res["mask"][:N]
    return res
