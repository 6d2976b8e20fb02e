// semidetr_hungarian_assign_f32: cost matrix, assignment and (where asked) training targets of a batch of problems in one call,
// the ground truths read in place through a table that travels in the kernel arguments (semidetr_hip.h, match_table.h).  The
// kernels are those of match_cost.hip and lsap.hip; this file checks the table and issues the launches back to back.
#include <hip/hip_runtime.h>

#include "common.h"
#include "match_table.h"

extern "C" int semidetr_hungarian_assign_f32(void *stream, const float *bbox_pred, const float *cls_pred,
                                             const semidetr_match_table *table, int num_query, int num_classes,
                                             const semidetr_cost_params *params, float *cost, int64_t *match_row,
                                             int64_t *match_col, int64_t *assigned_gt_inds, int64_t *assigned_labels,
                                             int32_t *status, void *workspace, int64_t target_num_classes, int64_t *target_labels,
                                             float *label_weights, float *bbox_targets, float *bbox_weights, int32_t *num_pos)
{
    SEMIDETR_REQUIRE(table && params, SEMIDETR_E_BADARG, "hungarian_assign: null table / params");
    const int B = table->num_problems;
    SEMIDETR_REQUIRE(B >= 1 && B <= SEMIDETR_MATCH_TABLE, SEMIDETR_E_BADARG,
                     "hungarian_assign: %d problems (1 .. %d fit the table)", B, SEMIDETR_MATCH_TABLE);
    SEMIDETR_REQUIRE(num_query >= 0 && num_classes > 0, SEMIDETR_E_BADARG, "hungarian_assign: bad sizes (Q=%d C=%d)", num_query,
                     num_classes);
    int64_t total = 0;
    int max_gt = 0;
    for (int b = 0; b < B; ++b) {
        const int n = table->count[b];
        SEMIDETR_REQUIRE(n >= 0 && table->offsets[b] == total, SEMIDETR_E_BADARG,
                         "hungarian_assign: problem %d: count %d, offset %d (expected %lld)", b, n, table->offsets[b],
                         (long long)total);
        SEMIDETR_REQUIRE(n == 0 || (table->boxes[b] && table->labels[b]), SEMIDETR_E_BADARG,
                         "hungarian_assign: problem %d: null boxes / labels", b);
        SEMIDETR_REQUIRE(((uintptr_t)table->boxes[b] & 15) == 0 && ((uintptr_t)table->labels[b] & 7) == 0, SEMIDETR_E_BADARG,
                         "hungarian_assign: problem %d: boxes must be 16-byte, labels 8-byte aligned", b);
        total += n;
        max_gt = n > max_gt ? n : max_gt;
        SEMIDETR_REQUIRE((int64_t)num_query * total < INT32_MAX, SEMIDETR_E_TOOLARGE, "hungarian_assign: matrix too large");
    }
    SEMIDETR_REQUIRE(table->offsets[B] == total, SEMIDETR_E_BADARG, "hungarian_assign: offsets[%d] = %d, the counts sum to %lld", B,
                     table->offsets[B], (long long)total);
    SEMIDETR_REQUIRE(status, SEMIDETR_E_BADARG, "hungarian_assign: null status");
    const bool has_cost = num_query > 0 && total > 0;
    SEMIDETR_REQUIRE(!has_cost || (bbox_pred && cls_pred && cost), SEMIDETR_E_BADARG, "hungarian_assign: null pointer argument");
    SEMIDETR_REQUIRE(((uintptr_t)bbox_pred & 15) == 0, SEMIDETR_E_BADARG, "hungarian_assign: bbox_pred must be 16-byte aligned");
    if (target_labels)
        SEMIDETR_REQUIRE(assigned_gt_inds && label_weights && bbox_targets && bbox_weights && num_pos, SEMIDETR_E_BADARG,
                         "hungarian_assign: targets need assigned_gt_inds and all five target outputs");
    hipStream_t st = semidetr::as_stream(stream);
    if (has_cost)
        if (int rc = semidetr::launch_match_cost_table(st, bbox_pred, cls_pred, *table, num_query, num_classes, *params, cost))
            return rc;
    if (int rc = semidetr::launch_lsap_table(st, cost, *table, num_query, max_gt, match_row, match_col, assigned_gt_inds,
                                             assigned_labels, status, workspace))
        return rc;
    if (target_labels)
        return semidetr::launch_build_targets_table(st, assigned_gt_inds, *table, num_query, target_num_classes, target_labels,
                                                    label_weights, bbox_targets, bbox_weights, num_pos);
    return SEMIDETR_OK;
}
