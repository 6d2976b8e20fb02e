// Where the pseudo-label kernels find their small per-image arguments: in device arrays (the entry points that take them as
// pointers) or by value in the kernel arguments (semidetr_teacher_pseudo_labels_f32, semidetr_transform_bboxes_table_f32,
// semidetr_hip.h).  The kernels are templates over the source and read nothing else differently, so both give the same bits.
#pragma once
#include "common.h"

namespace semidetr {

// (height, width) of image b
struct DeviceHw {
    const float *img_hw;
    __device__ __forceinline__ float h(int b) const { return img_hw[2 * b]; }
    __device__ __forceinline__ float w(int b) const { return img_hw[2 * b + 1]; }
};
struct ValueHw {
    semidetr_image_sizes s;
    __device__ __forceinline__ float h(int b) const { return s.hw[b][0]; }
    __device__ __forceinline__ float w(int b) const { return s.hw[b][1]; }
};

// first proposal row of image b and how many rows it has
struct DeviceRows {
    const int32_t *offs, *counts;      // counts may be NULL: offs[b + 1] - offs[b]
    __device__ __forceinline__ int start(int b) const { return offs[b]; }
    __device__ __forceinline__ int count(int b) const { return counts ? counts[b] : offs[b + 1] - offs[b]; }
};
struct PaddedRows {
    int stride;                        // image b's rows start at b * stride (the padded layout of the NMS)
    const int32_t *counts;
    __device__ __forceinline__ int start(int b) const { return b * stride; }
    __device__ __forceinline__ int count(int b) const { return counts[b]; }
};

static_assert(sizeof(semidetr_box_table) + 64 <= 4096 && sizeof(semidetr_image_sizes) + 128 <= 4096,
              "SEMIDETR_IMAGE_TABLE: the tables do not fit the kernel arguments");

// the filter launch of semidetr_teacher_pseudo_labels_f32 (pseudo_label.hip); arguments checked by the caller
int launch_pseudo_filter_padded(hipStream_t st, const float *proposals, const int64_t *labels, int stride, const int32_t *counts,
                                int num_images, float *out_boxes, int64_t *out_labels, float *out_scores, int32_t *out_count,
                                float *out_thr);

}  // namespace semidetr
