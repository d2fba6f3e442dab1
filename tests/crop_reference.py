"""Numpy restatement of the tracking crop (`crop_img_by_bbox`, src/local_feature_object_detector/local_feature_2D_detector.py:133-159:
two `get_image_crop_resize` = `get_affine_transform` + `cv2.warpAffine(INTER_LINEAR)`, src/utils/data_utils.py:22-52, :239-255),
in two forms that tests/test_tracking_cpu.py holds against each other bytewise:

  warp_generic   what the reference runs, step by step: the three point pairs of `get_affine_transform` in float32,
                 cv2.getAffineTransform as a float64 solve of the 6 x 6 system, then OpenCV's 8-bit warpAffine as we read it
                 (the matrix inverted in float64, cvRound(. * 1024) column / row tables, rounding offset 16, 5 fractional bits,
                 bilinear weights scaled to 2^15, (sum + 2^14) >> 15, constant border 0), applied as TWO passes with the uint8
                 image of the first as the input of the second;
  warp_closed    the integer closed form the kernel evaluates (csrc/track.hip), one pass.

OpenCV's source is not available here and cv2 is not installed: parity with OpenCV itself is unpinned (like oracle/ingest_oracle.py).
Known simplifications against OpenCV: the weight table is not passed through `short` (OpenCV stores 2^15 as a short after a
correction step), and coordinates are not saturated to `short` (the library refuses sizes at or beyond 32767)."""
import numpy as np

AB_BITS = 10
AB_SCALE = 1 << AB_BITS
INTER_BITS = 5
INTER_TAB_SIZE = 1 << INTER_BITS
ROUND_DELTA = AB_SCALE // INTER_TAB_SIZE // 2          # 16
COEF_BITS = 15


def _third_point(a, b):
    d = a - b
    return b + np.array([-d[1], d[0]], dtype=np.float32)


def affine_from_box(box, out_w, out_h):
    """`get_affine_transform(center, scale, 0, [out_w, out_h])` for the centre / scale `get_image_crop_resize` derives from `box`:
    source and destination triangles in float32, the 2 x 3 matrix from a float64 solve (cv2.getAffineTransform)."""
    x0, y0, x1, y1 = [float(v) for v in box]
    center = np.array([(x0 + x1) / 2.0, (y0 + y1) / 2.0])
    src_w = x1 - x0                                       # the scale comes from the width only
    src = np.zeros((3, 2), np.float32)
    dst = np.zeros((3, 2), np.float32)
    src[0] = center
    src[1] = center + np.array([0.0, src_w * -0.5])
    dst[0] = [out_w * 0.5, out_h * 0.5]
    dst[1] = np.array([out_w * 0.5, out_h * 0.5], np.float32) + np.array([0, out_w * -0.5], np.float32)
    src[2] = _third_point(src[0], src[1])
    dst[2] = _third_point(dst[0], dst[1])
    A = np.zeros((6, 6))
    b = np.zeros(6)
    for i in range(3):
        A[i, 0:3] = [src[i, 0], src[i, 1], 1.0]
        A[i + 3, 3:6] = [src[i, 0], src[i, 1], 1.0]
        b[i], b[i + 3] = dst[i, 0], dst[i, 1]
    return np.linalg.solve(A, b).reshape(2, 3)


def _invert_affine(M):
    """the inversion warpAffine applies to a forward matrix"""
    M = np.array(M, np.float64)
    D = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[1, 1] * D, M[0, 0] * D
    M[0, 0], M[0, 1], M[1, 0], M[1, 1] = A11, M[0, 1] * -D, M[1, 0] * -D, A22
    b1 = -M[0, 0] * M[0, 2] - M[0, 1] * M[1, 2]
    b2 = -M[1, 0] * M[0, 2] - M[1, 1] * M[1, 2]
    M[0, 2], M[1, 2] = b1, b2
    return M


def _cv_round(a):
    return np.rint(a).astype(np.int64)                   # round half to even


def _taps(img, sx, sy):
    h, w = img.shape
    ok = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    return np.where(ok, img[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)], 0).astype(np.int64)


def warp_affine_u8(img, M, out_w, out_h):
    """8-bit warpAffine(img, M, (out_w, out_h), INTER_LINEAR, BORDER_CONSTANT 0)"""
    iM = _invert_affine(M)
    x = np.arange(out_w, dtype=np.float64)
    y = np.arange(out_h, dtype=np.float64)
    adelta = _cv_round(iM[0, 0] * x * AB_SCALE)
    bdelta = _cv_round(iM[1, 0] * x * AB_SCALE)
    X0 = _cv_round((iM[0, 1] * y + iM[0, 2]) * AB_SCALE) + ROUND_DELTA
    Y0 = _cv_round((iM[1, 1] * y + iM[1, 2]) * AB_SCALE) + ROUND_DELTA
    X = (X0[:, None] + adelta[None, :]) >> (AB_BITS - INTER_BITS)
    Y = (Y0[:, None] + bdelta[None, :]) >> (AB_BITS - INTER_BITS)
    sx, sy = X >> INTER_BITS, Y >> INTER_BITS
    fx = (X & (INTER_TAB_SIZE - 1)).astype(np.float32) / np.float32(INTER_TAB_SIZE)
    fy = (Y & (INTER_TAB_SIZE - 1)).astype(np.float32) / np.float32(INTER_TAB_SIZE)
    one = np.float32(1)
    scale = np.float32(1 << COEF_BITS)
    w00 = _cv_round((one - fy) * (one - fx) * scale)
    w10 = _cv_round((one - fy) * fx * scale)
    w01 = _cv_round(fy * (one - fx) * scale)
    w11 = _cv_round(fy * fx * scale)
    acc = w00 * _taps(img, sx, sy) + w10 * _taps(img, sx + 1, sy) + w01 * _taps(img, sx, sy + 1) + w11 * _taps(img, sx + 1, sy + 1)
    v = (acc + (1 << (COEF_BITS - 1))) >> COEF_BITS
    return np.clip(v, 0, 255).astype(np.uint8)


def warp_generic(frame, box, S):
    x0, y0, x1, y1 = [int(v) for v in box]
    w, h = x1 - x0, y1 - y0
    stage1 = warp_affine_u8(frame, affine_from_box([x0, y0, x1, y1], w, h), w, h)
    return warp_affine_u8(stage1, affine_from_box([0, 0, w, h], S, S), S, S)


def warp_closed(frame, box, S):
    """[S, S] uint8; S a power of two <= 1024"""
    x0, y0, x1, y1 = [int(v) for v in box]
    w, h = x1 - x0, y1 - y0
    assert w >= 1 and h >= 1 and S & (S - 1) == 0 and S <= 1024
    k = 1024 // S
    fh, fw = frame.shape
    x = np.arange(S, dtype=np.int64)[None, :]
    y = np.arange(S, dtype=np.int64)[:, None]
    X = (w * k * x + 16) >> 5
    Y = (w * k * y + 512 * (h - w) + 16) >> 5
    X, Y = np.broadcast_arrays(X, Y)
    sx, fx, sy, fy = X >> 5, X & 31, Y >> 5, Y & 31

    def tap(i, j):
        ok = (i >= 0) & (i < w) & (j >= 0) & (j < h)
        u, v = x0 + i, y0 + j
        ok &= (u >= 0) & (u < fw) & (v >= 0) & (v < fh)
        return np.where(ok, frame[np.clip(v, 0, fh - 1), np.clip(u, 0, fw - 1)], 0).astype(np.int64)

    acc = 32 * ((32 - fx) * (32 - fy) * tap(sx, sy) + fx * (32 - fy) * tap(sx + 1, sy) + (32 - fx) * fy * tap(sx, sy + 1)
                + fx * fy * tap(sx + 1, sy + 1))
    return ((acc + 16384) >> 15).astype(np.uint8)


def to_float(crop_u8):
    """`image_crop.astype(np.float32) / 255` of the reference"""
    return crop_u8.astype(np.float32) / np.float32(255)
