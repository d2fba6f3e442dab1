// Tracking crop: 8-bit grayscale frame + 2D boxes -> S x S crops, fp32 / 255, on the device.  Replaces, per frame,
// cv2.imread + two cv2.warpAffine + the fp32 upload of
//   crop_img_by_bbox        src/local_feature_object_detector/local_feature_2D_detector.py:133-159
//   get_image_crop_resize   src/utils/data_utils.py:239-255   (get_affine_transform :22-52)
// so that the tracking loop of demo.py:98-134 keeps the frame on the device.
//
// Upstream warps twice.  Stage 1 maps the box [x0, y0, x1, y1] to an image of h x w (w = x1 - x0, h = y1 - y0): a pure
// translation, i.e. a copy of the window with zeros outside the frame.  Stage 2 maps that image to S x S with ONE uniform scale
// S / w (get_affine_transform takes the scale from the width only) and sends the centre (w/2, h/2) to (S/2, S/2): a box that is
// not square is cut or zero-padded vertically, never stretched.
//
// Arithmetic restated from OpenCV's 8-bit warpAffine(INTER_LINEAR, BORDER_CONSTANT 0) (imgproc/imgwarp.cpp; the reference pins
// opencv-python, the library itself is not vendored -> parity unpinned, like ingest.hip): AB_BITS 10, INTER_BITS 5, rounding
// offset 16, bilinear weights = products of 5-bit fractions scaled to 2^15, result (sum + 2^14) >> 15.  With S a power of two
// every fixed-point quantity of both stages is an exact integer (tests/crop_reference.py checks the closed form against the
// generic float64 formulation), so with k = 1024 / S and the output pixel (x, y):
//   X = (w k x + 16) >> 5 ; Y = (w k y + 512 (h - w) + 16) >> 5      (arithmetic shifts)
//   sx = X >> 5, fx = X & 31 ; sy = Y >> 5, fy = Y & 31
//   tap (i, j) of the stage-1 image: 0 unless 0 <= i < w and 0 <= j < h (even where the frame has pixels there), else
//   frame[y0 + j][x0 + i] if that lies inside the frame, else 0
//   v = (32 (32-fx)(32-fy) t00 + 32 fx (32-fy) t10 + 32 (32-fx) fy t01 + 32 fx fy t11 + 16384) >> 15 ; out = (float)v / 255.f
// Launch-bound byte work: one thread per output pixel, grid z = box, at most 4 source bytes in, 4 (+1) bytes out.
#include "opp_common.h"

namespace {

__device__ __forceinline__ int crop_tap(const unsigned char* __restrict__ src, int fh, int fw, int src_stride, int x0, int y0,
                                        int w, int h, int i, int j) {
  if (i < 0 || i >= w || j < 0 || j >= h) return 0;      // stage 2's constant border
  const int fx = x0 + i, fy = y0 + j;
  if (fx < 0 || fx >= fw || fy < 0 || fy >= fh) return 0;  // stage 1's constant border: never read outside the frame
  return (int)src[(size_t)fy * src_stride + fx];
}

__global__ __launch_bounds__(256) void crop_warp_u8_kernel(const unsigned char* __restrict__ src, int fh, int fw, int src_stride,
                                                           const int* __restrict__ boxes, int S, int k, float* __restrict__ dst,
                                                           unsigned char* __restrict__ dst_u8) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= S || y >= S) return;
  const int b = blockIdx.z;
  const int x0 = boxes[4 * b], y0 = boxes[4 * b + 1];
  int w = boxes[4 * b + 2] - x0, h = boxes[4 * b + 3] - y0;
  // the host refuses such boxes before the launch; a device copy that disagrees with it still produces zeros, not an overflow
  if (w < 1 || h < 1 || w > 65535 || h > 65535) w = h = 0;
  const int X = (w * k * x + 16) >> 5;
  const int Y = (w * k * y + 512 * (h - w) + 16) >> 5;
  const int sx = X >> 5, fx = X & 31, sy = Y >> 5, fy = Y & 31;
  const int t00 = crop_tap(src, fh, fw, src_stride, x0, y0, w, h, sx, sy);
  const int t10 = crop_tap(src, fh, fw, src_stride, x0, y0, w, h, sx + 1, sy);
  const int t01 = crop_tap(src, fh, fw, src_stride, x0, y0, w, h, sx, sy + 1);
  const int t11 = crop_tap(src, fh, fw, src_stride, x0, y0, w, h, sx + 1, sy + 1);
  const int sum = 32 * ((32 - fx) * (32 - fy) * t00 + fx * (32 - fy) * t10 + (32 - fx) * fy * t01 + fx * fy * t11);
  const int v = (sum + 16384) >> 15;
  const size_t o = ((size_t)b * S + y) * S + x;
  if (dst) dst[o] = (float)v / 255.f;
  if (dst_u8) dst_u8[o] = (unsigned char)v;
}

}  // namespace

extern "C" int opp_crop_warp_u8(const unsigned char* src, int h, int w, int src_stride, const int* boxes, const int* boxes_host,
                                int n_boxes, int crop_size, float* dst, unsigned char* dst_u8, void* stream) {
  OPP_CHECK_ARG(src && boxes && boxes_host && (dst || dst_u8), "crop_warp: null argument");
  OPP_CHECK_ARG(crop_size >= 64 && crop_size <= 1024 && (crop_size & (crop_size - 1)) == 0,
                "crop_warp: crop_size %d is not a power of two in [64, 1024]", crop_size);
  OPP_CHECK_ARG(h > 0 && w > 0 && h < 32767 && w < 32767 && src_stride >= w, "crop_warp: bad frame %dx%d (stride %d)", h, w,
                src_stride);
  OPP_CHECK_ARG(n_boxes >= 1 && n_boxes <= 65535, "crop_warp: %d boxes", n_boxes);
  for (int b = 0; b < n_boxes; ++b) {
    const int* q = boxes_host + 4 * b;
    for (int c = 0; c < 4; ++c)
      OPP_CHECK_ARG(q[c] > -32767 && q[c] < 32767, "crop_warp: box %d coordinate %d beyond the 16-bit range", b, q[c]);
    OPP_CHECK_ARG(q[2] - q[0] >= 1 && q[3] - q[1] >= 1, "crop_warp: box %d is empty (%d x %d)", b, q[2] - q[0], q[3] - q[1]);
  }
  hipLaunchKernelGGL(crop_warp_u8_kernel, dim3(opp_cdiv(crop_size, 64), opp_cdiv(crop_size, 4), n_boxes), dim3(256), 0,
                     (hipStream_t)stream, src, h, w, src_stride, boxes, crop_size, 1024 / crop_size, dst, dst_u8);
  OPP_CHECK_LAUNCH("crop_warp_u8_kernel");
  return OPP_OK;
}
