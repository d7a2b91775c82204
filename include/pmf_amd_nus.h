/* libpmf_amd.so -- the nuScenes projection chain (csrc/nus_project.hip).  Fifth header of the C ABI: pmf_amd.h,
 * pmf_amd_sensat.h, pmf_amd_wide.h and pmf_amd_a2d2.h keep their prototypes, this one adds the one entry point that
 * replaces the per-view host step of the reference's nuScenes readers (pc_processor/dataset/nuScenes/dataset_nuscenes.py:
 * 204-282 mapLidar2Camera, dataset_nuscenes_v2.py:222-375 mapLidar2Camera / mapLidar2CameraCropYaw): four rigid
 * transforms of the devkit's float32 point cloud, the pinhole, the keep mask and the order-preserving crop.  It is the index
 * pass in front of pmf_project_v2_scatter, the place pmf_project_v2_index has for SemanticKITTI and pmf_a2d2_index for
 * A2D2.  Same conventions as pmf_amd.h (the call enqueues on the given stream and returns without synchronising, 0 /
 * hipError_t / negative PMF_E_*), read by the same strict reader (pmf_amd/_lib.py).  Pointers are DEVICE memory unless
 * named `_host`.
 *
 * Parity with the devkit's own output is unpinned -- no fixture could be made with it.  Two known sources of difference:
 * np.dot's BLAS summation order in the rotations, and NumPy < 2 rounding the translation vector to float32 before the
 * addition (at most one float32 ulp per step). */
#ifndef PMF_AMD_NUS_H
#define PMF_AMD_NUS_H
#include "pmf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* points per workgroup (one lane per point): blk_cnt holds one count per workgroup */
#define PMF_NUS_BLOCK 256
/* doubles in chain_host */
#define PMF_NUS_CHAIN 57
/* modes of pmf_nus_project */
#define PMF_NUS_IMAGE 0
#define PMF_NUS_YAW 1

/* One camera view of one sweep, three launches (count, scan, compact), no copy, no synchronisation.
 *   in:  points f32[P][stride], stride 4 or 5 floats per row (x, y, z, intensity[, ring]: the raw .pcd.bin rows go up as
 *        they are, the fifth float is never read)
 *        chain_host: PMF_NUS_CHAIN HOST doubles, read before the call returns and handed to the kernels by value:
 *            R1[9] t1[3] R2[9] t2[3] t3[3] R3[9] t4[3] R4[9] K[9], matrices row-major.
 *            R1, t1: lidar -> ego at the sweep's time (calibrated_sensor of the lidar); R2, t2: ego -> global (ego_pose of
 *            the sweep); t3 = -(ego_pose translation of the image), R3 = its rotation TRANSPOSED; t4 = -(camera
 *            calibrated_sensor translation), R4 = its rotation TRANSPOSED; K = camera_intrinsic.  Transposing and negating
 *            are exact, the host does them.
 *        mode, min_dist, fov_lo / fov_hi (radians, mode 1), bound_h / bound_w (mode 0), row_scale, col_scale, img_scale
 *        blk_cnt i32[ceil(P / PMF_NUS_BLOCK) + 1]: workspace
 *   The formula (every product and sum below is one IEEE operation, nothing is fused):
 *     Rot(R, p)_i = (float)((R[i][0] * (double)p_x + R[i][1] * (double)p_y) + R[i][2] * (double)p_z)
 *     Tr(t, p)_i  = (float)((double)p_i + t_i)
 *     p = Tr(t1, Rot(R1, p));  p = Tr(t2, Rot(R2, p));  p = Rot(R3, Tr(t3, p));  p = Rot(R4, Tr(t4, p))
 *        -- the point is a float32 triple after every step, as in the devkit's float32 LidarPointCloud
 *     x, y, z = the float32 camera-frame point widened to double
 *     a = (K00 x + K01 y) + K02 z,  b = (K10 x + K11 y) + K12 z,  c = (K20 x + K21 y) + K22 z,  u = a / c,  v = b / c
 *     xy = ((v * row_scale) * img_scale, (u * col_scale) * img_scale);  x_data, y_data = their truncation toward zero
 *     mode 1 (mapLidar2CameraCropYaw): keep = z_f32 > (float)min_dist && yaw >= fov_lo && yaw <= fov_hi with
 *        yaw = -atan2f(z_f32, x_f32) (both sides widened to double, as pmf_project_v2_index compares);
 *        depth = sqrtf((x*x + y*y) + z*z) in float32 of the CAMERA-frame point
 *     mode 0 (mapLidar2Camera): keep = z_f32 > (float)min_dist && u > 1 && u < bound_h - 1 && v > 1 && v < bound_w - 1
 *        (the reference's callers pass the image WIDTH as img_h, hence the names); depth is the same expression of the
 *        LIDAR-frame input point.  A point with c == 0 is never kept in mode 0.  Mode 1 does not look at u, v: for a kept
 *        point whose scaled coordinates are not finite or lie outside the int32 range (c == 0, which a camera matrix with the
 *        last row 0 0 1 and min_dist >= 0 excludes, or a huge scale) xy holds them as computed, and its x_data, y_data and
 *        the box in meta are unspecified.
 *   out: keep u8[P]; for the K kept points in file order: src_idx i32[K] (position in the sweep), crop f32[K][4] =
 *        camera-frame x, y, z and the untouched intensity, xy f64[K][2], x_data / y_data i32[K], depth f32[K];
 *        meta i32[5] = K, row_min, row_max, col_min, col_max (over x_data / y_data).  Every per-point output array holds P
 *        entries.  K = 0 is not an error: meta[0] = 0 and nothing else but keep is written.
 * PMF_E_ARG without a launch: a null pointer, P < 1, stride outside {4, 5}, mode outside {0, 1}, row_scale / col_scale /
 * img_scale not finite or not > 0. */
int pmf_nus_project(const float* points, int32_t P, int32_t stride, const double* chain_host, int32_t mode, double min_dist,
                    float fov_lo, float fov_hi, double bound_h, double bound_w, double row_scale, double col_scale,
                    double img_scale, uint8_t* keep, int32_t* src_idx, float* crop, double* xy, int32_t* x_data,
                    int32_t* y_data, float* depth, int32_t* meta, int32_t* blk_cnt, pmf_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
