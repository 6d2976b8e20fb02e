// Where the matcher's kernels find problem b's ground truths: in the concatenated arrays of the three-call entry points (device
// offsets and image sizes), or through the by-value table of semidetr_hungarian_assign_f32 (semidetr_hip.h).  The kernels are
// templates over the source and read nothing else differently, so both give the same bits.
#pragma once
#include "common.h"

namespace semidetr {

struct FlatGt {
    const float *gt_bboxes;
    const int64_t *gt_labels;
    const int32_t *gt_offsets;
    const float *img_wh;
    __device__ __forceinline__ int start(int b) const { return gt_offsets[b]; }
    __device__ __forceinline__ int count(int b) const { return gt_offsets[b + 1] - gt_offsets[b]; }
    __device__ __forceinline__ const float *boxes(int b) const { return gt_bboxes + (int64_t)gt_offsets[b] * 4; }
    __device__ __forceinline__ const int64_t *labels(int b) const { return gt_labels + gt_offsets[b]; }
    __device__ __forceinline__ float img_w(int b) const { return img_wh[2 * b]; }
    __device__ __forceinline__ float img_h(int b) const { return img_wh[2 * b + 1]; }
};

struct TableGt {
    semidetr_match_table t;
    __device__ __forceinline__ int start(int b) const { return t.offsets[b]; }
    __device__ __forceinline__ int count(int b) const { return t.count[b]; }
    __device__ __forceinline__ const float *boxes(int b) const { return t.boxes[b]; }
    __device__ __forceinline__ const int64_t *labels(int b) const { return t.labels[b]; }
    __device__ __forceinline__ float img_w(int b) const { return t.img_wh[b][0]; }
    __device__ __forceinline__ float img_h(int b) const { return t.img_wh[b][1]; }
};

// the 4096 bytes of kernel arguments a launch may carry, less the other arguments of the assignment kernel
static_assert(sizeof(semidetr_match_table) + 128 <= 4096, "SEMIDETR_MATCH_TABLE: the table does not fit the kernel arguments");

// The launches of semidetr_hungarian_assign_f32, each in the file of its kernel; sizes and pointers are checked by the caller.
int launch_match_cost_table(hipStream_t st, const float *bbox_pred, const float *cls_pred, const semidetr_match_table &table,
                            int num_query, int num_classes, const semidetr_cost_params &params, float *cost);
int launch_lsap_table(hipStream_t st, const float *cost, const semidetr_match_table &table, int num_query, int max_gt,
                      int64_t *match_row, int64_t *match_col, int64_t *assigned_gt_inds, int64_t *assigned_labels, int32_t *status,
                      void *workspace);
int launch_build_targets_table(hipStream_t st, const int64_t *assigned_gt_inds, const semidetr_match_table &table, int num_query,
                               int64_t num_classes, int64_t *labels, float *label_weights, float *bbox_targets, float *bbox_weights,
                               int32_t *num_pos);

}  // namespace semidetr
