/* libpmf_amd.so -- the SensatUrban training loader (csrc/bev_train.hip).  Second header of the C ABI: pmf_amd.h keeps its
 * prototypes, this one adds the sample struct and the two entry points of the device-side SensatLoader.  Same conventions
 * as pmf_amd.h (caller-owned DEVICE pointers, every call enqueues on the given stream and returns without synchronising,
 * 0 / hipError_t / negative PMF_E_*), and it is read by the same strict reader (pmf_amd/_lib.py).
 *
 * The reference's loader (pc_processor/dataset/sensat_urban/sensat_loader.py:17-27,64-71) runs, per item and on the host,
 *   RandomCrop(2H,2W) -> RandomRotation(360) -> RandomCrop(H,W) -> RandomHorizontalFlip -> RandomVerticalFlip
 * over the nine planes of a whole frame, again and again until 10 % of the label plane is >= 0, then two scalar jitters.
 * The chain is one map from an output pixel to one frame pixel or to zero; here the frames stay on the device and a batch
 * is one count launch per acceptance round plus one gather launch. */
#ifndef PMF_AMD_SENSAT_H
#define PMF_AMD_SENSAT_H
#include "pmf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* bits of pmf_bev_sample_t.flags */
#define PMF_BEV_HFLIP 1
#define PMF_BEV_VFLIP 2

/* One candidate draw.  An array of these sits in DEVICE memory (samples_dev).
 *   feat     the frame's features, pixel-major f32[h][w][8] (32 bytes per pixel, 16-byte aligned): the .float() of the
 *            reference's float64 frame, laid out so that one gathered pixel is two 16-byte loads
 *   label    the frame's labels, int8[h][w], -1 = unlabelled
 *   top1, left1   the first crop, 2H x 2W, inside the frame
 *   m0 m1 m3 m4   the inverse rotation matrix [cos r, sin r, -sin r, cos r], r = radians(-angle), about the centre of the
 *                 first crop (torchvision's tensor rotate: nearest, zero fill)
 *   top2, left2   the second crop, H x W, inside the rotated 2H x 2W image
 *   flags    PMF_BEV_HFLIP | PMF_BEV_VFLIP, applied after the second crop
 *   jit_rgb, jit_h   the two scalar jitters (sensat_loader.py:70-71) */
typedef struct {
  const float* feat;
  const int8_t* label;
  int32_t h, w;
  int32_t top1, left1;
  float m0, m1, m3, m4;
  int32_t top2, left2;
  int32_t flags;
  float jit_rgb, jit_h;
} pmf_bev_sample_t;

/* sizeof(pmf_bev_sample_t), for bindings to self-check */
int pmf_sizeof_sensat(void);

/* counts_dev[i] = number of the H x W output pixels of candidate i whose label is >= 0; a pixel that falls outside the
 * rotated first crop is zero-filled and therefore counts (the reference tests tmp_map[8].ge(0) after the zero fill).  The
 * flips permute the pixels and are not applied.  Reads the label planes only; counts_dev (int32[n]) is zeroed first.
 * PMF_E_ARG without a launch: a null pointer, n / H / W <= 0, n > 65535, H * W > 2^31 - 1. */
int pmf_bev_sample_count(const pmf_bev_sample_t* samples_dev, int32_t n, int32_t H, int32_t W, int32_t* counts_dev,
                         pmf_stream_t s);

/* feature_out f32[B][8][H][W], label_out f32[B][H][W]: output pixel (oy, ox) of sample b is pixel
 * (top2 + cy, left2 + cx) of the rotated first crop, cx = W-1-ox under PMF_BEV_HFLIP, cy = H-1-oy under PMF_BEV_VFLIP;
 * its source (sy, sx) in the first crop follows pmf_flip_rotate_crop's float32 arithmetic with w := 2W, h := 2H; outside
 * the crop OR outside the frame all nine values are 0, inside they are frame pixel (top1 + sy, left1 + sx).  Then with
 * m = channel 4: channels 5..7 = (v + jit_rgb) * m, channels 0..2 = (v + jit_h) * m (two float32 roundings each), channels
 * 3, 4 and the label as gathered.  Nothing outside [0,h) x [0,w) of a frame is read, whatever the struct holds.
 * PMF_E_ARG without a launch: a null pointer, B / H / W <= 0, B > 65535, H * W > 2^31 - 1, B * 8 * H * W * 4 bytes past
 * 2^63 - 1. */
int pmf_bev_sample_gather(const pmf_bev_sample_t* samples_dev, int32_t B, int32_t H, int32_t W, float* feature_out,
                          float* label_out, pmf_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
