/* libpmf_amd.so -- the A2D2 frame loader (csrc/undistort.hip, csrc/a2d2.hip).  Fourth header of the C ABI: pmf_amd.h,
 * pmf_amd_sensat.h and pmf_amd_wide.h keep their prototypes, this one adds the three entry points that replace the two
 * per-frame host steps of the reference's A2D2 path (pc_processor/dataset/a2d2/dataset_a2d2.py): the OpenCV undistortion of
 * the camera image (:158-186) and the per-point Python loop that turns label-image colours into classes (:244-254).  Same
 * conventions as pmf_amd.h (every call enqueues on the given stream and returns without synchronising, 0 / hipError_t /
 * negative PMF_E_*), read by the same strict reader (pmf_amd/_lib.py).  Pointers are DEVICE memory unless named `_host`.
 *
 * Undistortion follows OpenCV's published algorithm (initUndistortRectifyMap, fisheye::initUndistortRectifyMap, and
 * remap(INTER_LINEAR, BORDER_CONSTANT 0) in its fixed-point form: 5 fractional coordinate bits, 15-bit weight table).
 * Parity with OpenCV's own output is unpinned -- no fixture could be made with it.  One known deviation: OpenCV's `short`
 * map wraps beyond +-32767 px, this map saturates at the int32 range. */
#ifndef PMF_AMD_A2D2_H
#define PMF_AMD_A2D2_H
#include "pmf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* lens kinds of pmf_undistort_map */
#define PMF_LENS_TELECAM 0
#define PMF_LENS_FISHEYE 1

/* Once per camera: map i32[h][w][2].  Entry (i, j) is the source coordinate (iu, iv) = (rint(u * 32), rint(v * 32)) of
 * destination pixel (row i, column j), round-half-even, saturated to the int32 range (a NaN coordinate gives the int32
 * minimum, which lies outside every source).  (u, v) in float64:
 *   (x, y, w') = ir_host . (j, i, 1), x /= w', y /= w'      ir_host: 9 doubles, row-major inverse of the NEW camera matrix
 *   lens 0 (Telecam), dist_host = k1, k2, p1, p2, k3:  r2 = x*x + y*y, kr = 1 + ((k3*r2 + k2)*r2 + k1)*r2,
 *       xd = x*kr + p1*2xy + p2*(r2 + 2x*x),  yd = y*kr + p1*(r2 + 2y*y) + p2*2xy
 *   lens 1 (Fisheye), dist_host = k1, k2, k3, k4 (the fifth is not read):  r = sqrt(x*x + y*y), t = atan(r),
 *       td = t*(1 + k1 t^2 + k2 t^4 + k3 t^6 + k4 t^8),  s = r == 0 ? 1 : td / r,  xd = x*s, yd = y*s
 *   u = fx*xd + cx, v = fy*yd + cy                          the ORIGINAL camera matrix
 * ir_host and dist_host (5 doubles) are HOST arrays, read before the call returns.
 * PMF_E_ARG without a launch: a null pointer, h < 1, w < 1, lens outside {0, 1}; PMF_E_UNSUPPORTED: h * w > 2^31 - 1. */
int pmf_undistort_map(int32_t lens, const double* ir_host, double fx, double fy, double cx, double cy,
                      const double* dist_host, int32_t h, int32_t w, int32_t* map, pmf_stream_t s);

/* Per frame: src u8[sh][sw][3], map i32[h][w][2] -> dst u8[h][w][3], integer arithmetic only.  With (iu, iv) the map entry,
 * sx = iu >> 5 (arithmetic), a = iu & 31, sy = iv >> 5, b = iv & 31:
 *   dst = (S(sy,sx)(32-b)(32-a) + S(sy,sx+1)(32-b)a + S(sy+1,sx)b(32-a) + S(sy+1,sx+1)ba + 512) >> 10   per channel,
 * a neighbour outside [0,sh) x [0,sw) reads 0.  Nothing outside src is read, whatever the map holds.  dst must not
 * overlap src.  A lane takes four consecutive destination pixels: 32 bytes of map, three whole dwords of output, so map
 * must sit on 16 bytes and dst on 4 (a device allocation does); the last h * w % 4 pixels are stored byte by byte.
 * PMF_E_ARG without a launch: a null pointer, sh / sw / h / w < 1, map or dst off that alignment; PMF_E_UNSUPPORTED: h * w
 * or sh * sw > 2^31 - 1. */
int pmf_remap_u8c3(const uint8_t* src, int32_t sh, int32_t sw, const int32_t* map, int32_t h, int32_t w, uint8_t* dst,
                   pmf_stream_t s);

/* Per frame: what perspective_view_loader_v2.py:72-101 and dataset_a2d2.py:244-254 compute per point, for all P points.
 *   in:  points f64[P][3], reflectance f64[P], rows / cols i32[P] (the host's (row + 0.5).astype(int32) and the same of
 *        col), rgb u8[P][3] (label-image pixel of each point) or null, keys u32[n] (r << 16 | g << 8 | b) with their
 *        classes cls i32[n], img_scale
 *   out: pts f32[P][4] = x, y, z, reflectance, each rounded once from float64
 *        depth f32[P] = float32 of sqrt((x*x + y*y) + z*z), every operation rounded in float64 (no fused multiply-add)
 *        xy f64[P][2] = (rows * img_scale, cols * img_scale); x_data, y_data i32[P] = their truncation toward zero
 *        sem i32[P] = class of the point's colour; 0 where the colour is not in the table, and everywhere when rgb is null
 *        meta i32[6] = row_min, row_max, col_min, col_max (over x_data / y_data), n_unknown (points whose colour is not in
 *        the table), first_unknown (the smallest such point index, 2^31 - 1 if there is none)
 * PMF_E_ARG without a launch: a null pointer other than rgb / keys / cls, P < 1, img_scale not > 0 or not finite, pts off
 * 16 bytes; with rgb given: keys or cls null, n outside [1, 64]. */
int pmf_a2d2_index(const double* points, const double* reflectance, const int32_t* rows, const int32_t* cols,
                   const uint8_t* rgb, int32_t P, const uint32_t* keys, const int32_t* cls, int32_t n, double img_scale,
                   float* pts, float* depth, double* xy, int32_t* x_data, int32_t* y_data, int32_t* sem, int32_t* meta,
                   pmf_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
