/*
 * include/popsift_c.h -- flat C binding of the C++ extraction API (PopSift / SiftJob / FeaturesHost).
 *
 * The reference exposes only C++ classes (popsift.h:44-317).  Hosts that cannot include C++ headers
 * (ctypes, cgo, JNI ...) bind these functions instead; bench.py drives the product's real end-to-end
 * path (host image in -> PopSift::enqueue -> SiftJob::get -> FeaturesHost out) through them.  Each
 * function is a one-line forward to the class method it names; exceptions become a NULL / negative
 * return plus popsift_c_last_error().
 */
#ifndef POPSIFT_C_H
#define POPSIFT_C_H

#include "popsift_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct popsift_c_handle   popsift_c_handle;     /* PopSift            */
typedef struct popsift_c_job      popsift_c_job;        /* SiftJob            */
typedef struct popsift_c_features popsift_c_features;   /* popsift::FeaturesHost */

/* PopSift::PopSift(config, mode, imode, device), popsift.h:166-168.  cfg is translated into a
 * popsift::Config through its public setters.  image_mode: 0 ByteImages, 1 FloatImages;
 * processing_mode: 0 ExtractingMode (MatchingMode results are device resident and have no C view). */
popsift_c_handle* popsift_c_create(const psx_config* cfg, int image_mode, int device);
/* popsift_c_create with Config::setDescriptorFormat (sift_conf.h): descriptor_format PSX_DESCFMT_F32 (as
 * popsift_c_create) or PSX_DESCFMT_U8 (SiftJob::get returns byte descriptors, include/popsift_hip.h); any other
 * value returns NULL before a device is touched. */
popsift_c_handle* popsift_c_create_fmt(const psx_config* cfg, int image_mode, int device, int descriptor_format);
/* PopSift::uninit + destructor */
void popsift_c_destroy(popsift_c_handle* h);
/* PopSift::enqueue, popsift.h:219-232: deep-copies the image; NULL when the image is refused */
popsift_c_job* popsift_c_enqueue_u8(popsift_c_handle* h, int w, int hgt, const unsigned char* img);
popsift_c_job* popsift_c_enqueue_f32(popsift_c_handle* h, int w, int hgt, const float* img);
/* PopSift::enqueue with caller-supplied keypoints (psx_keypoint, include/popsift_hip.h): the detector does not run, the
 * n records are deep-copied and described; kps NULL or n 0 gives an empty result */
popsift_c_job* popsift_c_enqueue_u8_kp(popsift_c_handle* h, int w, int hgt, const unsigned char* img, const psx_keypoint* kps, int n);
popsift_c_job* popsift_c_enqueue_f32_kp(popsift_c_handle* h, int w, int hgt, const float* img, const psx_keypoint* kps, int n);
/* PopSift::enqueue with a detection mask (psx_set_mask, include/popsift_hip.h): a tight mask_w x mask_h plane of bytes,
 * non-zero = keypoints allowed, deep-copied.  mask NULL with mask_w = mask_h = 0 runs unmasked.  NULL for a NULL handle
 * and for a mask whose size is not the image's (refused before a device is touched). */
popsift_c_job* popsift_c_enqueue_u8_mask(popsift_c_handle* h, int w, int hgt, const unsigned char* img, const unsigned char* mask, int mask_w, int mask_h);
popsift_c_job* popsift_c_enqueue_f32_mask(popsift_c_handle* h, int w, int hgt, const float* img, const unsigned char* mask, int mask_w, int mask_h);
/* FeaturesHost::getSourceIndices: the input record of every feature of a keypoint job.  Returns their number (0 for a
 * detector job, -1 for NULL) and copies at most capacity of them into out (may be NULL). */
int popsift_c_source_indices(const popsift_c_features* f, int* out, int capacity);
/* SiftJob::get + delete job, popsift.h:75-81: blocks until the frame is done.  NULL on error. */
popsift_c_features* popsift_c_get(popsift_c_job* job);
/* FeaturesHost::getFeatureCount / getDescriptorCount */
int popsift_c_feature_count(const popsift_c_features* f);
int popsift_c_descriptor_count(const popsift_c_features* f);
/* Copies the keypoints as psx_feature records (Descriptor* turned into indices into the descriptor
 * array) and the descriptors (128 floats each); either pointer may be NULL. */
int popsift_c_copy(const popsift_c_features* f, psx_feature* features, float* descriptors);
/* direct view of the FeaturesHost descriptor array (getDescriptors()), valid until popsift_c_free; NULL for a
 * byte result.  popsift_c_copy with a non-NULL descriptor pointer fails on a byte result (PSX_ERR_STATE). */
const float* popsift_c_descriptors(const popsift_c_features* f);
/* PSX_DESCFMT_F32 or PSX_DESCFMT_U8: the form of the result's descriptors (FeaturesHost::hasByteDescriptors) */
int popsift_c_descriptor_format(const popsift_c_features* f);
/* popsift_c_copy for a byte result: records (desc_idx = rows of 128 bytes) and num_descriptors * 128 bytes; either
 * pointer may be NULL; PSX_ERR_STATE with a byte pointer on a float result */
int popsift_c_copy_u8(const popsift_c_features* f, psx_feature* features, unsigned char* descriptors);
/* direct view of the byte descriptors (FeaturesHost::getDescriptorBytes), valid until popsift_c_free; NULL for a
 * float result */
const unsigned char* popsift_c_descriptor_bytes(const popsift_c_features* f);
/* delete the FeaturesHost */
void popsift_c_free(popsift_c_features* f);
/* message of the last failure on the calling thread */
const char* popsift_c_last_error(void);
/* Diagnostics (no reference counterpart): counters of the library's pinned result / job-image pool of one device
 * (device < 0: all pools summed): out[0] = buffers ever allocated (hipHostMalloc), out[1] = buffers really freed
 * (hipHostFree), out[2] = requests served from the free list, out[3] = buffers on the free list, out[4] = bytes on the
 * free list, out[5] = bytes handed out.  A steady stream of frames must not move out[0] / out[1] after warm-up. */
void popsift_c_pool_stats(int device, long long out[6]);

#ifdef __cplusplus
}
#endif
#endif
