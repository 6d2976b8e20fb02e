// Compiled Python module `MultiScaleDeformableAttention` -- the drop-in for the reference's pybind module
// (detr_od/models/utils/ops/src/vision.cpp:13-16, signatures of src/ms_deform_attn.h:20-61, host code of
// src/cuda/ms_deform_attn_cuda.cu:20-153): same two entry points, same argument order, same precondition errors
// (AT_ASSERTM -> RuntimeError), outputs freshly allocated on the inputs' device, launches on the CURRENT stream, no
// synchronisation.  It holds no kernels: it validates at::Tensors and calls the C ABI of libsemidetr_hip.so
// (include/semidetr_hip.h), which is where the hand-written gfx950 code lives.  Host-only C++ (g++), built by
// csrc/Makefile; a ctypes call of the same ABI cost ~16 us per forward against a 4.7 us kernel (BENCH_r01), this
// path costs the launch plus ~2 us.
//
// Besides the reference's two functions it exports the fused MSDeformAttn prologue/epilogue pair (SURVEY.md
// section 8(f) row 1) and `pyramid_check`, the cached test behind SEMIDETR_MSDA_QUERIES_ARE_PIXELS.
#include <torch/extension.h>

// ROCm builds of torch present their devices as DeviceType::CUDA; these are the guard / stream types for that view
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <mutex>
#include <vector>

#include "semidetr_hip.h"

namespace {

void check_rc(int rc, const char *what)
{
    TORCH_CHECK(rc == 0, what, " failed (code ", rc, "): ", semidetr_last_error());
}

const char *scalar_name(at::ScalarType t) { return c10::toString(t); }

// ms_deform_attn.h:27-38 (CPU tensors only raise) and ms_deform_attn_cuda.cu:28-38 / :93-105
void check_tensor(const at::Tensor &t, const at::Tensor &value, const char *name)
{
    TORCH_CHECK(t.is_contiguous(), name, " tensor has to be contiguous");
    TORCH_CHECK(t.is_cuda(), name, " must be a CUDA tensor");
    TORCH_CHECK(t.device() == value.device(), name, " must be on the same device as value");
}

struct Dims {
    int N, S, M, D, L, Lq, P;
};

Dims op_dims(const at::Tensor &value, const at::Tensor &shapes, const at::Tensor &starts, const at::Tensor &loc,
             const at::Tensor &attn, int64_t im2col_step, const char *what)
{
    TORCH_CHECK(value.is_cuda(), "Not implemented on the CPU");
    check_tensor(value, value, "value");
    check_tensor(shapes, value, "spatial_shapes");
    check_tensor(starts, value, "level_start_index");
    check_tensor(loc, value, "sampling_loc");
    check_tensor(attn, value, "attn_weight");
    TORCH_CHECK(value.dim() == 4 && loc.dim() == 6 && attn.dim() == 5, what,
                ": expected value (N,S,M,D), sampling_loc (N,Lq,M,L,P,2), attn_weight (N,Lq,M,L,P)");
    Dims d;
    d.N = (int)value.size(0); d.S = (int)value.size(1); d.M = (int)value.size(2); d.D = (int)value.size(3);
    d.L = (int)shapes.size(0); d.Lq = (int)loc.size(1); d.P = (int)loc.size(4);
    const int64_t step = std::min<int64_t>(d.N, im2col_step);           // ms_deform_attn_cuda.cu:50-52
    TORCH_CHECK(step > 0 && d.N % step == 0, "batch(", d.N, ") must divide im2col_step(", step, ")");
    // the reference reads .data<int64_t>() of both index tensors -> anything but int64 raises
    TORCH_CHECK(shapes.scalar_type() == at::kLong, "expected scalar type Long for spatial_shapes");
    TORCH_CHECK(starts.scalar_type() == at::kLong, "expected scalar type Long for level_start_index");
    TORCH_CHECK(value.scalar_type() == at::kFloat || value.scalar_type() == at::kDouble, "\"", what,
                "\" not implemented for '", scalar_name(value.scalar_type()), "'");
    TORCH_CHECK(loc.scalar_type() == value.scalar_type() && attn.scalar_type() == value.scalar_type(), what,
                ": value, sampling_loc and attn_weight must share one dtype");
    TORCH_CHECK(loc.size(0) == d.N && loc.size(2) == d.M && loc.size(3) == d.L && loc.size(5) == 2 &&
                    attn.size(0) == d.N && attn.size(1) == d.Lq && attn.size(2) == d.M && attn.size(3) == d.L &&
                    attn.size(4) == d.P && starts.numel() == d.L && shapes.dim() == 2 && shapes.size(1) == 2,
                what, ": inconsistent tensor shapes");
    return d;
}

// ---- is the level table an exact tiling of [0, S)?  The answer needs the table on the host (one blocking copy), so
// it is cached per (spatial_shapes, level_start_index) tensor pair and version: a training step passes the same two
// tensors to all twelve layers, so this is at most one synchronisation per step where the reference's module has one
// per layer call (`assert (...).sum() == Len_in`, modules/ms_deform_attn.py:90).
struct PyramidEntry {
    c10::weak_intrusive_ptr<c10::TensorImpl> shapes, starts;
    uint32_t v_shapes, v_starts;
    const void *p_shapes, *p_starts;
    int64_t S;
    int result;
    int levels;               // rows of `table` (0: the table is not kept -- more than kTableLevels levels)
    int64_t table[2 * 32];    // the host copy of spatial_shapes the verdict was computed from
};
constexpr int kTableLevels = 32;
// the host copy of spatial_shapes for the `_v2` entry points of the C ABI (they choose the encoder kernels' region grids from it)
struct HostTable {
    int levels = 0;
    int64_t hw[2 * kTableLevels];
    const int64_t *ptr() const { return levels > 0 ? hw : nullptr; }
};
std::mutex g_pyr_mutex;
std::vector<PyramidEntry> g_pyr_cache;

// bit 0: sum(H*W) == S (the reference's assert); bit 1: level_start tiles [0, S) contiguously
// table (optional): receives the host copy the verdict rests on -- what the check fetched anyway, no further copy or synchronisation
int pyramid_lookup(const at::Tensor &shapes, const at::Tensor &starts, int64_t S, HostTable *table)
{
    if (table) table->levels = 0;
    auto *is = shapes.unsafeGetTensorImpl();
    auto *it = starts.unsafeGetTensorImpl();
    // Inference tensors have no version counter (torch.inference_mode(): "Inference tensors do not track version
    // counter"): the cache cannot tell whether they changed, so they are checked on every call.
    const bool cacheable = !shapes.is_inference() && !starts.is_inference();
    if (cacheable) {
        std::lock_guard<std::mutex> lock(g_pyr_mutex);
        for (auto &e : g_pyr_cache) {
            if (e.S != S || e.shapes._unsafe_get_target() != is || e.starts._unsafe_get_target() != it) continue;
            auto a = e.shapes.lock();      // expired (address reused by a new tensor) -> nullptr
            auto b = e.starts.lock();
            // also keyed on the storage address: `t.data = other` re-points a tensor without touching its version.
            // (In-place writes through `t.data` itself bump no counter anyone can see -- as for torch's own autograd
            // checks, that is outside what a version-based cache can notice.)
            if (a && b && e.v_shapes == is->version_counter().current_version() &&
                e.v_starts == it->version_counter().current_version() && e.p_shapes == shapes.data_ptr() &&
                e.p_starts == starts.data_ptr()) {
                if (table && e.levels > 0) {
                    table->levels = e.levels;
                    std::copy(e.table, e.table + 2 * e.levels, table->hw);
                }
                return e.result;
            }
        }
    }
    TORCH_CHECK(shapes.scalar_type() == at::kLong && starts.scalar_type() == at::kLong && shapes.dim() == 2 &&
                    shapes.size(1) == 2 && starts.numel() == shapes.size(0),
                "pyramid_check: expected spatial_shapes (L,2) and level_start_index (L,) of dtype int64");
    if (shapes.is_cuda()) {      // a table not seen before costs a device-to-host copy, which a stream capture does not allow:
        // answer "nothing known" (the kernels that assume nothing) and do not cache it
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        hipStream_t cur = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(shapes.device().index()).stream();
        if (hipStreamIsCapturing(cur, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) return 0;
    }
    const at::Tensor hs = shapes.to(at::kCPU).contiguous(), hl = starts.to(at::kCPU).contiguous();
    const int64_t *ps = hs.data_ptr<int64_t>(), *pl = hl.data_ptr<int64_t>();
    int64_t sum = 0;
    bool tiles = true;
    for (int64_t l = 0; l < hs.size(0); ++l) {
        // (height / width <= 32766: the region-window forward packs a sample's top-left pixel into 15 + 15 bits, semidetr_hip.h)
        tiles = tiles && pl[l] == sum && ps[2 * l] > 0 && ps[2 * l + 1] > 0 && ps[2 * l] <= 32766 && ps[2 * l + 1] <= 32766;
        sum += ps[2 * l] * ps[2 * l + 1];
    }
    const int result = (sum == S ? 1 : 0) | (tiles && sum == S ? 2 : 0);
    const int levels = hs.size(0) <= kTableLevels ? (int)hs.size(0) : 0;
    if (table && levels > 0) {
        table->levels = levels;
        std::copy(ps, ps + 2 * levels, table->hw);
    }
    if (!cacheable) return result;
    std::lock_guard<std::mutex> lock(g_pyr_mutex);
    if (g_pyr_cache.size() >= 16) g_pyr_cache.erase(g_pyr_cache.begin());
    g_pyr_cache.push_back({c10::weak_intrusive_ptr<c10::TensorImpl>(shapes.getIntrusivePtr()),
                           c10::weak_intrusive_ptr<c10::TensorImpl>(starts.getIntrusivePtr()),
                           is->version_counter().current_version(), it->version_counter().current_version(),
                           shapes.data_ptr(), starts.data_ptr(), S, result, levels, {0}});
    std::copy(ps, ps + 2 * levels, g_pyr_cache.back().table);
    return result;
}

int pyramid_check(const at::Tensor &shapes, const at::Tensor &starts, int64_t S) { return pyramid_lookup(shapes, starts, S, nullptr); }

// `flags` of the f32 entry points: the self-attention statement, the call site's slot of the forward-kernel choice, and -- while
// torch.use_deterministic_algorithms(True) is in force -- a forward kernel that does not depend on earlier launches
int self_attention_flags(const at::Tensor &shapes, const at::Tensor &starts, int Lq, int S, int64_t policy_slot = 0,
                         HostTable *table = nullptr)
{
    // (the backward calls may carry, OR-ed into the slot number, what gather_choice(slot) answered when the matching forward ran:
    //  SEMIDETR_MSDA_GATHER_WINDOW / _PATCH, bits 16 / 17 -- the autograd functions do that)
    constexpr int64_t kGather = SEMIDETR_MSDA_GATHER_WINDOW | SEMIDETR_MSDA_GATHER_PATCH;
    TORCH_CHECK(policy_slot >= 0 && (policy_slot & ~kGather) <= 255 && (policy_slot & kGather) != kGather,
                "policy_slot must be 0..255 (optionally | gather_choice(slot)), got ", policy_slot);
    return ((Lq == S && (pyramid_lookup(shapes, starts, S, table) & 2)) ? SEMIDETR_MSDA_QUERIES_ARE_PIXELS : 0) |
           SEMIDETR_MSDA_POLICY_SLOT((int)(policy_slot & 0xff)) | (int)(policy_slot & kGather) |
           (at::globalContext().deterministicAlgorithms() ? SEMIDETR_MSDA_FIXED_FORWARD : 0);
}

void *stream_of(const at::Tensor &t) { return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream(); }

// extra_flags: OR-ed into the f32 call's flags (the exact route's forward: SEMIDETR_MSDA_FIXED_FORWARD whatever torch's switch says)
at::Tensor forward_with_flags(const at::Tensor &value, const at::Tensor &spatial_shapes,
                              const at::Tensor &level_start_index, const at::Tensor &sampling_loc,
                              const at::Tensor &attn_weight, int64_t im2col_step, int64_t policy_slot, int extra_flags)
{
    const Dims d = op_dims(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step,
                           "ms_deform_attn_forward_cuda");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(value.device());
    at::Tensor out = at::empty({d.N, d.Lq, (int64_t)d.M * d.D}, value.options());      // the kernel writes all of it
    if (out.numel() == 0 || value.numel() == 0) return out.zero_();
    const int64_t *sh = spatial_shapes.data_ptr<int64_t>(), *ls = level_start_index.data_ptr<int64_t>();
    int rc;
    if (value.scalar_type() == at::kDouble)
        rc = semidetr_msda_forward_f64(stream_of(value), value.data_ptr<double>(), sh, ls, sampling_loc.data_ptr<double>(),
                                       attn_weight.data_ptr<double>(), d.N, d.S, d.M, d.D, d.L, d.Lq, d.P,
                                       out.data_ptr<double>());
    else {
        HostTable ht;
        const int flags = self_attention_flags(spatial_shapes, level_start_index, d.Lq, d.S, policy_slot, &ht) | extra_flags;
        rc = semidetr_msda_forward_f32_v2(stream_of(value), value.data_ptr<float>(), sh, ls, sampling_loc.data_ptr<float>(),
                                          attn_weight.data_ptr<float>(), d.N, d.S, d.M, d.D, d.L, d.Lq, d.P, flags,
                                          out.data_ptr<float>(), ht.ptr());
    }
    check_rc(rc, "ms_deform_attn_forward");
    return out;
}

at::Tensor ms_deform_attn_forward(const at::Tensor &value, const at::Tensor &spatial_shapes,
                                  const at::Tensor &level_start_index, const at::Tensor &sampling_loc,
                                  const at::Tensor &attn_weight, int64_t im2col_step, int64_t policy_slot)
{
    return forward_with_flags(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step, policy_slot, 0);
}

// ---- the exact route (not part of the reference's pybind surface; include/semidetr_hip.h: semidetr_msda_backward_exact_f32) ----
// what the C entry takes, so that a caller can route a call it would refuse elsewhere: fp32 / 16-bit value (the module up-casts a
// 16-bit one first) with 32 channels per head, <= 32 heads, num_levels * num_point <= 62
bool exact_supported(const at::Tensor &value, int64_t num_levels, int64_t num_point)
{
    return value.is_cuda() && value.dim() == 4 && value.size(3) == 32 && value.size(2) <= 32 && num_levels >= 1 && num_levels <= 32 &&
           num_point >= 1 && num_levels * num_point <= 62 &&
           (value.scalar_type() == at::kFloat || value.scalar_type() == at::kHalf || value.scalar_type() == at::kBFloat16) &&
           value.size(1) * value.size(2) * 128 < (int64_t)0xFFFFF000u &&
           semidetr_msda_exact_workspace_bytes(1, 1, 1, (int)num_levels, 1, (int)num_point) != 0;
}

// the forward whose kernel is a function of the arguments alone (SEMIDETR_MSDA_FIXED_FORWARD: the patch / strips kernel)
at::Tensor ms_deform_attn_exact_forward(const at::Tensor &value, const at::Tensor &spatial_shapes,
                                        const at::Tensor &level_start_index, const at::Tensor &sampling_loc,
                                        const at::Tensor &attn_weight, int64_t im2col_step, int64_t policy_slot)
{
    TORCH_CHECK(value.scalar_type() == at::kFloat, "ms_deform_attn_exact_forward: fp32 only, got '", scalar_name(value.scalar_type()), "'");
    return forward_with_flags(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step, policy_slot,
                              SEMIDETR_MSDA_FIXED_FORWARD);
}

// grad_value as the exact sum of its contributions, rounded once; the two small gradients from the atomics-free gather
std::vector<at::Tensor> ms_deform_attn_exact_backward(const at::Tensor &value, const at::Tensor &spatial_shapes,
                                                      const at::Tensor &level_start_index, const at::Tensor &sampling_loc,
                                                      const at::Tensor &attn_weight, const at::Tensor &grad_output,
                                                      int64_t im2col_step, int64_t policy_slot)
{
    const Dims d = op_dims(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step,
                           "ms_deform_attn_exact_backward");
    TORCH_CHECK(value.scalar_type() == at::kFloat, "ms_deform_attn_exact_backward: fp32 only, got '", scalar_name(value.scalar_type()), "'");
    check_tensor(grad_output, value, "grad_output");
    TORCH_CHECK(grad_output.scalar_type() == value.scalar_type() && grad_output.numel() == (int64_t)d.N * d.Lq * d.M * d.D,
                "ms_deform_attn_exact_backward: grad_output must be (N, Lq, M*D) of value's dtype");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(value.device());
    at::Tensor gv = at::empty_like(value);            // every element is written by the reduce kernel: no fill
    at::Tensor gl = at::empty_like(sampling_loc);
    at::Tensor ga = at::empty_like(attn_weight);
    if (value.numel() == 0 || gl.numel() == 0) return {gv.zero_(), gl.zero_(), ga.zero_()};
    const size_t bytes = semidetr_msda_exact_workspace_bytes(d.N, d.S, d.M, d.L, d.Lq, d.P);
    TORCH_CHECK(bytes != 0, "ms_deform_attn_exact_backward: num_query * num_levels * num_point * 4 must be below 2^32");
    at::Tensor work = at::empty({(int64_t)bytes}, value.options().dtype(at::kByte));
    const int flags = self_attention_flags(spatial_shapes, level_start_index, d.Lq, d.S, policy_slot);
    const int rc = semidetr_msda_backward_exact_f32(stream_of(value), grad_output.data_ptr<float>(), value.data_ptr<float>(),
                                                    spatial_shapes.data_ptr<int64_t>(), level_start_index.data_ptr<int64_t>(),
                                                    sampling_loc.data_ptr<float>(), attn_weight.data_ptr<float>(), d.N, d.S, d.M, d.D, d.L,
                                                    d.Lq, d.P, flags, work.data_ptr(), bytes, gv.data_ptr<float>(), gl.data_ptr<float>(),
                                                    ga.data_ptr<float>());
    check_rc(rc, "ms_deform_attn_exact_backward");
    return {gv, gl, ga};
}

std::vector<at::Tensor> ms_deform_attn_backward(const at::Tensor &value, const at::Tensor &spatial_shapes,
                                                const at::Tensor &level_start_index, const at::Tensor &sampling_loc,
                                                const at::Tensor &attn_weight, const at::Tensor &grad_output,
                                                int64_t im2col_step, int64_t policy_slot)
{
    const Dims d = op_dims(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step,
                           "ms_deform_attn_backward_cuda");
    check_tensor(grad_output, value, "grad_output");
    TORCH_CHECK(grad_output.scalar_type() == value.scalar_type() &&
                    grad_output.numel() == (int64_t)d.N * d.Lq * d.M * d.D,
                "ms_deform_attn_backward_cuda: grad_output must be (N, Lq, M*D) of value's dtype");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(value.device());
    at::Tensor gv = at::empty_like(value);            // zero-filled inside the call where the kernels need it
    at::Tensor gl = at::empty_like(sampling_loc);     // fully written by the kernels
    at::Tensor ga = at::empty_like(attn_weight);
    if (value.numel() == 0 || gl.numel() == 0) return {gv.zero_(), gl.zero_(), ga.zero_()};
    const int64_t *sh = spatial_shapes.data_ptr<int64_t>(), *ls = level_start_index.data_ptr<int64_t>();
    int rc;
    if (value.scalar_type() == at::kDouble)
        rc = semidetr_msda_backward_f64(stream_of(value), grad_output.data_ptr<double>(), value.data_ptr<double>(), sh, ls,
                                        sampling_loc.data_ptr<double>(), attn_weight.data_ptr<double>(), d.N, d.S, d.M,
                                        d.D, d.L, d.Lq, d.P, gv.data_ptr<double>(), gl.data_ptr<double>(),
                                        ga.data_ptr<double>());
    else {
        HostTable ht;
        const int flags = self_attention_flags(spatial_shapes, level_start_index, d.Lq, d.S, policy_slot, &ht);
        rc = semidetr_msda_backward_f32_v2(stream_of(value), grad_output.data_ptr<float>(), value.data_ptr<float>(), sh, ls,
                                           sampling_loc.data_ptr<float>(), attn_weight.data_ptr<float>(), d.N, d.S, d.M, d.D,
                                           d.L, d.Lq, d.P, flags, gv.data_ptr<float>(), gl.data_ptr<float>(), ga.data_ptr<float>(),
                                           ht.ptr());
    }
    check_rc(rc, "ms_deform_attn_backward");
    return {gv, gl, ga};
}

// ---- fp16 / bf16 value maps (not part of the reference's pybind surface): what autocast hands MSDeformAttn, without the fp32
// copies of the reference's "for amp" branch (ops/modules/ms_deform_attn.py:113-120).  value / grad_output / out / grad_value
// are Half or BFloat16, locations and weights (and their gradients) Float; include/semidetr_hip.h states the contract.
bool h16_supported(const at::Tensor &value, const at::Tensor &loc, const at::Tensor &attn)
{
    return value.is_cuda() && (value.scalar_type() == at::kHalf || value.scalar_type() == at::kBFloat16) && value.dim() == 4 &&
           loc.scalar_type() == at::kFloat && attn.scalar_type() == at::kFloat;
}

Dims h16_dims(const at::Tensor &value, const at::Tensor &shapes, const at::Tensor &starts, const at::Tensor &loc,
              const at::Tensor &attn, int64_t im2col_step, const char *what)
{
    TORCH_CHECK(value.is_cuda(), "Not implemented on the CPU");
    check_tensor(value, value, "value");
    check_tensor(shapes, value, "spatial_shapes");
    check_tensor(starts, value, "level_start_index");
    check_tensor(loc, value, "sampling_loc");
    check_tensor(attn, value, "attn_weight");
    TORCH_CHECK(value.dim() == 4 && loc.dim() == 6 && attn.dim() == 5, what,
                ": expected value (N,S,M,D), sampling_loc (N,Lq,M,L,P,2), attn_weight (N,Lq,M,L,P)");
    Dims d;
    d.N = (int)value.size(0); d.S = (int)value.size(1); d.M = (int)value.size(2); d.D = (int)value.size(3);
    d.L = (int)shapes.size(0); d.Lq = (int)loc.size(1); d.P = (int)loc.size(4);
    const int64_t step = std::min<int64_t>(d.N, im2col_step);
    TORCH_CHECK(step > 0 && d.N % step == 0, "batch(", d.N, ") must divide im2col_step(", step, ")");
    TORCH_CHECK(shapes.scalar_type() == at::kLong, "expected scalar type Long for spatial_shapes");
    TORCH_CHECK(starts.scalar_type() == at::kLong, "expected scalar type Long for level_start_index");
    TORCH_CHECK(value.scalar_type() != at::kFloat && value.scalar_type() != at::kDouble, what, ": value is '",
                scalar_name(value.scalar_type()), "' -- the fp32 / fp64 entry is ms_deform_attn_forward / ms_deform_attn_backward");
    TORCH_CHECK(value.scalar_type() == at::kHalf || value.scalar_type() == at::kBFloat16, "\"", what, "\" not implemented for '",
                scalar_name(value.scalar_type()), "'");
    TORCH_CHECK(loc.scalar_type() == at::kFloat && attn.scalar_type() == at::kFloat, what,
                ": sampling_loc and attn_weight must be Float (locations and weights are never narrowed to 16 bits), got '",
                scalar_name(loc.scalar_type()), "' and '", scalar_name(attn.scalar_type()), "'");
    TORCH_CHECK(loc.size(0) == d.N && loc.size(2) == d.M && loc.size(3) == d.L && loc.size(5) == 2 &&
                    attn.size(0) == d.N && attn.size(1) == d.Lq && attn.size(2) == d.M && attn.size(3) == d.L &&
                    attn.size(4) == d.P && starts.numel() == d.L && shapes.dim() == 2 && shapes.size(1) == 2,
                what, ": inconsistent tensor shapes");
    return d;
}

int h16_dtype(const at::Tensor &value) { return value.scalar_type() == at::kHalf ? SEMIDETR_H16_FP16 : SEMIDETR_H16_BF16; }

at::Tensor ms_deform_attn_h16_forward(const at::Tensor &value, const at::Tensor &spatial_shapes,
                                      const at::Tensor &level_start_index, const at::Tensor &sampling_loc,
                                      const at::Tensor &attn_weight, int64_t im2col_step)
{
    const Dims d = h16_dims(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step,
                            "ms_deform_attn_h16_forward");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(value.device());
    at::Tensor out = at::empty({d.N, d.Lq, (int64_t)d.M * d.D}, value.options());      // the kernel writes all of it
    if (out.numel() == 0 || value.numel() == 0) return out.zero_();
    const int rc = semidetr_msda_forward_h16(stream_of(value), h16_dtype(value), value.data_ptr(), spatial_shapes.data_ptr<int64_t>(),
                                             level_start_index.data_ptr<int64_t>(), sampling_loc.data_ptr<float>(),
                                             attn_weight.data_ptr<float>(), d.N, d.S, d.M, d.D, d.L, d.Lq, d.P, out.data_ptr());
    check_rc(rc, "ms_deform_attn_h16_forward");
    return out;
}

std::vector<at::Tensor> ms_deform_attn_h16_backward(const at::Tensor &value, const at::Tensor &spatial_shapes,
                                                    const at::Tensor &level_start_index, const at::Tensor &sampling_loc,
                                                    const at::Tensor &attn_weight, const at::Tensor &grad_output,
                                                    int64_t im2col_step)
{
    const Dims d = h16_dims(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step,
                            "ms_deform_attn_h16_backward");
    check_tensor(grad_output, value, "grad_output");
    TORCH_CHECK(grad_output.scalar_type() == value.scalar_type(), "ms_deform_attn_h16_backward: value ('",
                scalar_name(value.scalar_type()), "') and grad_output ('", scalar_name(grad_output.scalar_type()),
                "') must share one dtype");
    TORCH_CHECK(grad_output.numel() == (int64_t)d.N * d.Lq * d.M * d.D,
                "ms_deform_attn_h16_backward: grad_output must be (N, Lq, M*D)");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(value.device());
    at::Tensor gv = at::empty_like(value);            // every element written by the conversion kernel
    at::Tensor gl = at::empty_like(sampling_loc);     // fully written by the kernels
    at::Tensor ga = at::empty_like(attn_weight);
    if (value.numel() == 0 || gl.numel() == 0) return {gv.zero_(), gl.zero_(), ga.zero_()};
    // grad_value is summed in fp32 and rounded once: the sums live in this workspace, cleared on the current stream
    at::Tensor ws = at::empty({(int64_t)(semidetr_msda_backward_h16_workspace_bytes(d.N, d.S, d.M, d.D) / sizeof(float))},
                              value.options().dtype(at::kFloat));
    ws.zero_();
    const int rc = semidetr_msda_backward_h16(stream_of(value), h16_dtype(value), grad_output.data_ptr(), value.data_ptr(),
                                              spatial_shapes.data_ptr<int64_t>(), level_start_index.data_ptr<int64_t>(),
                                              sampling_loc.data_ptr<float>(), attn_weight.data_ptr<float>(), d.N, d.S, d.M, d.D,
                                              d.L, d.Lq, d.P, ws.data_ptr(), gv.data_ptr(), gl.data_ptr<float>(),
                                              ga.data_ptr<float>());
    check_rc(rc, "ms_deform_attn_h16_backward");
    return {gv, gl, ga};
}

// ---- fused prologue / epilogue (not part of the reference's pybind surface) ----------------------------------
bool fused_supported(const at::Tensor &value, const at::Tensor &ref, const at::Tensor &off, const at::Tensor &logits)
{
    return value.is_cuda() && value.scalar_type() == at::kFloat && value.dim() == 4 && value.size(3) == 32 &&
           value.size(2) <= 32 && (ref.size(-1) == 2 || ref.size(-1) == 4) && off.scalar_type() == at::kFloat &&
           logits.scalar_type() == at::kFloat && ref.scalar_type() == at::kFloat;
}

Dims fused_dims(const at::Tensor &value, const at::Tensor &shapes, const at::Tensor &starts, const at::Tensor &ref,
                const at::Tensor &off, const at::Tensor &logits)
{
    TORCH_CHECK(value.is_cuda(), "Not implemented on the CPU");
    check_tensor(value, value, "value");
    check_tensor(shapes, value, "spatial_shapes");
    check_tensor(starts, value, "level_start_index");
    check_tensor(ref, value, "reference_points");
    check_tensor(off, value, "sampling_offsets");
    check_tensor(logits, value, "attention logits");
    TORCH_CHECK(shapes.scalar_type() == at::kLong && starts.scalar_type() == at::kLong,
                "expected scalar type Long for spatial_shapes / level_start_index");
    TORCH_CHECK(value.dim() == 4 && off.dim() == 6 && logits.dim() == 4 && ref.dim() == 4,
                "ms_deform_attn_fused: expected sampling_offsets (N,Lq,M,L,P,2), logits (N,Lq,M,L*P), reference "
                "(N,Lq,L,2|4)");
    TORCH_CHECK(value.scalar_type() == at::kFloat && off.scalar_type() == at::kFloat &&
                    logits.scalar_type() == at::kFloat && ref.scalar_type() == at::kFloat,
                "ms_deform_attn_fused: fp32 tensors only");
    Dims d;
    d.N = (int)value.size(0); d.S = (int)value.size(1); d.M = (int)value.size(2); d.D = (int)value.size(3);
    d.Lq = (int)off.size(1); d.L = (int)off.size(3); d.P = (int)off.size(4);
    TORCH_CHECK(off.size(0) == d.N && off.size(2) == d.M && off.size(5) == 2 && logits.size(0) == d.N &&
                    logits.size(1) == d.Lq && logits.size(2) == d.M && logits.size(3) == (int64_t)d.L * d.P &&
                    ref.size(0) == d.N && ref.size(1) == d.Lq && ref.size(2) == d.L && shapes.size(0) == d.L,
                "ms_deform_attn_fused: inconsistent tensor shapes");
    if (ref.size(-1) != 2 && ref.size(-1) != 4)
        throw py::value_error("Last dim of reference_points must be 2 or 4, but get " + std::to_string(ref.size(-1)) +
                              " instead.");
    return d;
}

// The library reads reference points with 16-byte loads: a contiguous VIEW at an odd 8-byte offset (a batch slice of 2-d points
// with an odd Lq * L) is copied into a fresh, aligned allocation -- small and rare.
at::Tensor aligned16(const at::Tensor &t)
{
    return (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0 ? t : t.clone();
}

// input_padding_mask (N, S) bool / uint8, True = padding, or None: handed to the kernels as bytes
const unsigned char *mask_ptr(const c10::optional<at::Tensor> &mask, const at::Tensor &value, const Dims &d)
{
    if (!mask.has_value() || !mask->defined()) return nullptr;
    const at::Tensor &m = *mask;
    TORCH_CHECK(m.is_cuda() && m.device() == value.device() && m.is_contiguous() && m.dim() == 2 && m.size(0) == d.N &&
                    m.size(1) == d.S && (m.scalar_type() == at::kBool || m.scalar_type() == at::kByte),
                "ms_deform_attn_fused: padding_mask must be a contiguous (N, S) bool / uint8 tensor on value's device");
    return static_cast<const unsigned char *>(m.data_ptr());
}

// ---- the mask's per-(image, level) extents (include/semidetr_hip.h: semidetr_msda_mask_extents), cached like the pyramid
// check: the reference builds ONE mask per batch and hands it to all twelve layers of a pass (transformer.py:1309,1380), so
// one small launch per batch serves 12 forward + 12 backward calls.  Keyed on the mask / level-table tensors (weak references +
// versions + addresses) and the stream the summary was queued on -- a call on another stream queues its own.
struct ExtentsEntry {
    c10::weak_intrusive_ptr<c10::TensorImpl> mask, shapes;
    uint32_t v_mask, v_shapes;
    const void *p_mask, *p_shapes, *p_starts, *stream;
    at::Tensor ext;
};
std::mutex g_ext_mutex;
std::vector<ExtentsEntry> g_ext_cache;

at::Tensor mask_extents(const at::Tensor &m, const at::Tensor &shapes, const at::Tensor &starts)
{
    TORCH_CHECK(m.is_cuda() && m.is_contiguous() && m.dim() == 2 && (m.scalar_type() == at::kBool || m.scalar_type() == at::kByte),
                "mask_extents: padding_mask must be a contiguous (N, S) bool / uint8 CUDA tensor");
    TORCH_CHECK(shapes.is_cuda() && starts.is_cuda() && shapes.scalar_type() == at::kLong && starts.scalar_type() == at::kLong &&
                    shapes.is_contiguous() && starts.is_contiguous() && shapes.dim() == 2 && shapes.size(1) == 2 &&
                    starts.numel() == shapes.size(0),
                "mask_extents: expected contiguous int64 spatial_shapes (L,2) and level_start_index (L,) on the mask's device");
    // (the kernel indexes mask[n * S + starts[l] + i] for i < H * W -- the level table has to be on the mask's device
    //  and has to describe exactly S pixels; the cached pyramid check answers that without a copy after the first call)
    TORCH_CHECK(shapes.device() == m.device() && starts.device() == m.device(),
                "mask_extents: spatial_shapes / level_start_index must be on the mask's device");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(m.device());
    TORCH_CHECK((pyramid_check(shapes, starts, m.size(1)) & 1) != 0,
                "mask_extents: sum(H * W) of spatial_shapes must equal padding_mask.size(1) (and level_start_index must be readable "
                "outside a stream capture)");
    void *stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(m.device().index()).stream();
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(static_cast<hipStream_t>(stream), &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
    // (inference tensors carry no version counter; a summary computed inside a capture lives in the graph's memory pool)
    const bool cacheable = !m.is_inference() && !shapes.is_inference() && !capturing;
    auto *im = m.unsafeGetTensorImpl();
    auto *is = shapes.unsafeGetTensorImpl();
    if (cacheable) {
        std::lock_guard<std::mutex> lock(g_ext_mutex);
        for (auto &e : g_ext_cache) {
            if (e.mask._unsafe_get_target() != im || e.shapes._unsafe_get_target() != is || e.stream != stream) continue;
            auto a = e.mask.lock();
            auto b = e.shapes.lock();
            if (a && b && e.v_mask == im->version_counter().current_version() && e.v_shapes == is->version_counter().current_version() &&
                e.p_mask == m.data_ptr() && e.p_shapes == shapes.data_ptr() && e.p_starts == starts.data_ptr())
                return e.ext;
        }
    }
    const int N = (int)m.size(0), S = (int)m.size(1), L = (int)shapes.size(0);
    at::Tensor ext = at::empty({N, L}, m.options().dtype(at::kInt));
    if (ext.numel() == 0) return ext;
    check_rc(semidetr_msda_mask_extents(stream, static_cast<const unsigned char *>(m.data_ptr()), shapes.data_ptr<int64_t>(),
                                        starts.data_ptr<int64_t>(), N, S, L, ext.data_ptr<int>()),
             "mask_extents");
    if (cacheable) {
        std::lock_guard<std::mutex> lock(g_ext_mutex);
        if (g_ext_cache.size() >= 16) g_ext_cache.erase(g_ext_cache.begin());
        g_ext_cache.push_back({c10::weak_intrusive_ptr<c10::TensorImpl>(m.getIntrusivePtr()),
                               c10::weak_intrusive_ptr<c10::TensorImpl>(shapes.getIntrusivePtr()),
                               im->version_counter().current_version(), is->version_counter().current_version(), m.data_ptr(),
                               shapes.data_ptr(), starts.data_ptr(), stream, ext});
    }
    return ext;
}

at::Tensor ms_deform_attn_fused_forward(const at::Tensor &value, const at::Tensor &spatial_shapes,
                                        const at::Tensor &level_start_index, const at::Tensor &reference_points,
                                        const at::Tensor &sampling_offsets, const at::Tensor &attn_logits,
                                        const c10::optional<at::Tensor> &padding_mask, int64_t policy_slot)
{
    const Dims d = fused_dims(value, spatial_shapes, level_start_index, reference_points, sampling_offsets, attn_logits);
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(value.device());
    at::Tensor out = at::empty({d.N, d.Lq, (int64_t)d.M * d.D}, value.options());
    if (out.numel() == 0 || value.numel() == 0) return out.zero_();
    const at::Tensor ref = aligned16(reference_points);
    const unsigned char *mask = mask_ptr(padding_mask, value, d);
    at::Tensor ext;      // (kept alive until the launch is queued; the allocator orders its reuse on this stream)
    if (mask) ext = mask_extents(*padding_mask, spatial_shapes, level_start_index);
    HostTable ht;      // (the host copy of the level table the pyramid check holds anyway: the library chooses the region grids from it)
    const int flags = self_attention_flags(spatial_shapes, level_start_index, d.Lq, d.S, policy_slot, &ht);
    const int rc = semidetr_msda_fused_forward_f32_v2(
        stream_of(value), value.data_ptr<float>(), spatial_shapes.data_ptr<int64_t>(), level_start_index.data_ptr<int64_t>(),
        ref.data_ptr<float>(), (int)reference_points.size(-1), sampling_offsets.data_ptr<float>(),
        attn_logits.data_ptr<float>(), mask, mask ? ext.data_ptr<int>() : nullptr, d.N, d.S, d.M, d.D, d.L, d.Lq, d.P,
        flags, out.data_ptr<float>(), ht.ptr());
    check_rc(rc, "ms_deform_attn_fused_forward");
    return out;
}

std::vector<at::Tensor> ms_deform_attn_fused_backward(const at::Tensor &value, const at::Tensor &spatial_shapes,
                                                      const at::Tensor &level_start_index,
                                                      const at::Tensor &reference_points,
                                                      const at::Tensor &sampling_offsets, const at::Tensor &attn_logits,
                                                      const at::Tensor &grad_output,
                                                      const c10::optional<at::Tensor> &padding_mask, int64_t policy_slot)
{
    const Dims d = fused_dims(value, spatial_shapes, level_start_index, reference_points, sampling_offsets, attn_logits);
    TORCH_CHECK(grad_output.is_contiguous() && grad_output.numel() == (int64_t)d.N * d.Lq * d.M * d.D &&
                    grad_output.scalar_type() == at::kFloat && grad_output.device() == value.device(),
                "ms_deform_attn_fused_backward: grad_output must be a contiguous (N, Lq, M*D) tensor of value's dtype");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(value.device());
    at::Tensor gv = at::empty_like(value), go = at::empty_like(sampling_offsets), gl = at::empty_like(attn_logits);
    if (value.numel() == 0 || go.numel() == 0) return {gv.zero_(), go.zero_(), gl.zero_()};
    const at::Tensor ref = aligned16(reference_points);
    const unsigned char *mask = mask_ptr(padding_mask, value, d);
    at::Tensor ext;
    if (mask) ext = mask_extents(*padding_mask, spatial_shapes, level_start_index);
    HostTable ht;
    const int flags = self_attention_flags(spatial_shapes, level_start_index, d.Lq, d.S, policy_slot, &ht);
    const int rc = semidetr_msda_fused_backward_f32_v2(
        stream_of(value), grad_output.data_ptr<float>(), value.data_ptr<float>(), spatial_shapes.data_ptr<int64_t>(),
        level_start_index.data_ptr<int64_t>(), ref.data_ptr<float>(), (int)reference_points.size(-1),
        sampling_offsets.data_ptr<float>(), attn_logits.data_ptr<float>(), mask, mask ? ext.data_ptr<int>() : nullptr, d.N, d.S, d.M,
        d.D, d.L, d.Lq, d.P, flags, gv.data_ptr<float>(), go.data_ptr<float>(), gl.data_ptr<float>(), ht.ptr());
    check_rc(rc, "ms_deform_attn_fused_backward");
    return {gv, go, gl};
}

// ---- the fused prologue / epilogue on a 16-bit value map (include/semidetr_hip.h: semidetr_msda_fused_forward_h16): value Half /
// BFloat16, offsets and logits of value's dtype (what the Linear layers produce under autocast or in a .half() module) or Float,
// reference points Float -- or value's dtype, then up-cast here, exactly (locations are never narrowed).
bool is_h16(const at::Tensor &t) { return t.scalar_type() == at::kHalf || t.scalar_type() == at::kBFloat16; }
bool aligned_to(const at::Tensor &t, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(t.data_ptr()) & (bytes - 1)) == 0; }

bool fused_h16_supported(const at::Tensor &value, const at::Tensor &ref, const at::Tensor &off, const at::Tensor &logits)
{
    if (!(value.is_cuda() && is_h16(value) && value.dim() == 4 && value.size(3) == 32 && value.size(2) <= 32)) return false;
    if (!(ref.dim() == 4 && (ref.size(-1) == 2 || ref.size(-1) == 4) && off.dim() == 6 && logits.dim() == 4)) return false;
    if (!(ref.scalar_type() == at::kFloat || ref.scalar_type() == value.scalar_type())) return false;
    if (off.scalar_type() != logits.scalar_type() || !(off.scalar_type() == at::kFloat || off.scalar_type() == value.scalar_type()))
        return false;
    if (off.size(3) > 32 || off.size(3) * off.size(4) > 64) return false;
    // (a tensor that is not contiguous is made so by the caller: its copy is a fresh, aligned allocation)
    return (!value.is_contiguous() || aligned_to(value, 8)) && (!off.is_contiguous() || aligned_to(off, 8)) &&
           (!logits.is_contiguous() || aligned_to(logits, 4));
}

Dims fused_h16_dims(const at::Tensor &value, const at::Tensor &shapes, const at::Tensor &starts, const at::Tensor &ref,
                    const at::Tensor &off, const at::Tensor &logits, const char *what)
{
    TORCH_CHECK(value.is_cuda(), "Not implemented on the CPU");
    check_tensor(value, value, "value");
    check_tensor(shapes, value, "spatial_shapes");
    check_tensor(starts, value, "level_start_index");
    check_tensor(ref, value, "reference_points");
    check_tensor(off, value, "sampling_offsets");
    check_tensor(logits, value, "attention logits");
    TORCH_CHECK(shapes.scalar_type() == at::kLong && starts.scalar_type() == at::kLong,
                "expected scalar type Long for spatial_shapes / level_start_index");
    TORCH_CHECK(value.dim() == 4 && off.dim() == 6 && logits.dim() == 4 && ref.dim() == 4, what,
                ": expected value (N,S,M,D), sampling_offsets (N,Lq,M,L,P,2), logits (N,Lq,M,L*P), reference (N,Lq,L,2|4)");
    TORCH_CHECK(is_h16(value), what, ": value must be Half or BFloat16, got '", scalar_name(value.scalar_type()),
                "' -- the fp32 entry is ms_deform_attn_fused_forward / ms_deform_attn_fused_backward");
    TORCH_CHECK(off.scalar_type() == logits.scalar_type() && (off.scalar_type() == at::kFloat || off.scalar_type() == value.scalar_type()),
                what, ": sampling_offsets and attention logits must both be Float or both be value's dtype ('",
                scalar_name(value.scalar_type()), "'), got '", scalar_name(off.scalar_type()), "' and '",
                scalar_name(logits.scalar_type()), "'");
    TORCH_CHECK(ref.scalar_type() == at::kFloat || ref.scalar_type() == value.scalar_type(), what,
                ": reference_points must be Float or value's dtype, got '", scalar_name(ref.scalar_type()), "'");
    Dims d;
    d.N = (int)value.size(0); d.S = (int)value.size(1); d.M = (int)value.size(2); d.D = (int)value.size(3);
    d.Lq = (int)off.size(1); d.L = (int)off.size(3); d.P = (int)off.size(4);
    TORCH_CHECK(off.size(0) == d.N && off.size(2) == d.M && off.size(5) == 2 && logits.size(0) == d.N &&
                    logits.size(1) == d.Lq && logits.size(2) == d.M && logits.size(3) == (int64_t)d.L * d.P &&
                    ref.size(0) == d.N && ref.size(1) == d.Lq && ref.size(2) == d.L && shapes.dim() == 2 && shapes.size(0) == d.L &&
                    shapes.size(1) == 2 && starts.numel() == d.L,
                what, ": inconsistent tensor shapes");
    if (ref.size(-1) != 2 && ref.size(-1) != 4)
        throw py::value_error("Last dim of reference_points must be 2 or 4, but get " + std::to_string(ref.size(-1)) +
                              " instead.");
    TORCH_CHECK(d.D == 32 && d.M <= 32, what, ": the fused 16-bit kernels take 32 channels per head and at most 32 heads (got ", d.D,
                " and ", d.M, "); there is no generic fused kernel -- see fused_h16_supported");
    TORCH_CHECK(aligned_to(value, 8) && aligned_to(off, 8) && aligned_to(logits, 4), what,
                ": value and sampling_offsets must be 8-byte aligned, attention logits 4-byte aligned");
    return d;
}

int prologue_type_of(const at::Tensor &off)
{
    return off.scalar_type() == at::kFloat ? SEMIDETR_ROW_F32 : (off.scalar_type() == at::kHalf ? SEMIDETR_ROW_FP16 : SEMIDETR_ROW_BF16);
}

// fp32 reference points in 8-byte aligned storage: an exact up-cast of 16-bit points (small: N * Lq * L * 2|4 numbers)
at::Tensor ref_f32(const at::Tensor &ref)
{
    const at::Tensor r = ref.scalar_type() == at::kFloat ? ref : ref.to(at::kFloat);
    return aligned_to(r, 8) ? r : r.clone();
}

at::Tensor ms_deform_attn_h16_fused_forward(const at::Tensor &value, const at::Tensor &spatial_shapes,
                                            const at::Tensor &level_start_index, const at::Tensor &reference_points,
                                            const at::Tensor &sampling_offsets, const at::Tensor &attn_logits,
                                            const c10::optional<at::Tensor> &padding_mask)
{
    const char *what = "ms_deform_attn_h16_fused_forward";
    const Dims d = fused_h16_dims(value, spatial_shapes, level_start_index, reference_points, sampling_offsets, attn_logits, what);
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(value.device());
    at::Tensor out = at::empty({d.N, d.Lq, (int64_t)d.M * d.D}, value.options());      // the kernel writes all of it
    if (out.numel() == 0 || value.numel() == 0) return out.zero_();
    // the kernels index the mask and the value map through the level table: it has to describe exactly S pixels
    TORCH_CHECK((pyramid_check(spatial_shapes, level_start_index, d.S) & 1) != 0, what,
                ": sum(H * W) of spatial_shapes must equal value.size(1)");
    const at::Tensor ref = ref_f32(reference_points);
    const int rc = semidetr_msda_fused_forward_h16(
        stream_of(value), h16_dtype(value), value.data_ptr(), spatial_shapes.data_ptr<int64_t>(), level_start_index.data_ptr<int64_t>(),
        ref.data_ptr<float>(), (int)ref.size(-1), sampling_offsets.data_ptr(), attn_logits.data_ptr(), prologue_type_of(sampling_offsets),
        mask_ptr(padding_mask, value, d), d.N, d.S, d.M, d.D, d.L, d.Lq, d.P, out.data_ptr());
    check_rc(rc, what);
    return out;
}

std::vector<at::Tensor> ms_deform_attn_h16_fused_backward(const at::Tensor &value, const at::Tensor &spatial_shapes,
                                                          const at::Tensor &level_start_index, const at::Tensor &reference_points,
                                                          const at::Tensor &sampling_offsets, const at::Tensor &attn_logits,
                                                          const at::Tensor &grad_output,
                                                          const c10::optional<at::Tensor> &padding_mask)
{
    const char *what = "ms_deform_attn_h16_fused_backward";
    const Dims d = fused_h16_dims(value, spatial_shapes, level_start_index, reference_points, sampling_offsets, attn_logits, what);
    check_tensor(grad_output, value, "grad_output");
    TORCH_CHECK(grad_output.scalar_type() == value.scalar_type(), what, ": value ('", scalar_name(value.scalar_type()),
                "') and grad_output ('", scalar_name(grad_output.scalar_type()), "') must share one dtype");
    TORCH_CHECK(grad_output.numel() == (int64_t)d.N * d.Lq * d.M * d.D && aligned_to(grad_output, 8), what,
                ": grad_output must be (N, Lq, M*D), 8-byte aligned");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(value.device());
    at::Tensor gv = at::empty_like(value);      // every element written by the conversion kernel
    at::Tensor go = at::empty_like(sampling_offsets), gl = at::empty_like(attn_logits);      // fully written by the kernel
    if (value.numel() == 0 || go.numel() == 0) return {gv.zero_(), go.zero_(), gl.zero_()};
    TORCH_CHECK((pyramid_check(spatial_shapes, level_start_index, d.S) & 1) != 0, what,
                ": sum(H * W) of spatial_shapes must equal value.size(1)");
    const at::Tensor ref = ref_f32(reference_points);
    // grad_value is summed in fp32 and rounded once: the sums live in this workspace, cleared on the current stream
    at::Tensor ws = at::empty({(int64_t)(semidetr_msda_backward_h16_workspace_bytes(d.N, d.S, d.M, d.D) / sizeof(float))},
                              value.options().dtype(at::kFloat));
    ws.zero_();
    const int rc = semidetr_msda_fused_backward_h16(
        stream_of(value), h16_dtype(value), grad_output.data_ptr(), value.data_ptr(), spatial_shapes.data_ptr<int64_t>(),
        level_start_index.data_ptr<int64_t>(), ref.data_ptr<float>(), (int)ref.size(-1), sampling_offsets.data_ptr(),
        attn_logits.data_ptr(), prologue_type_of(sampling_offsets), mask_ptr(padding_mask, value, d), d.N, d.S, d.M, d.D, d.L, d.Lq,
        d.P, ws.data_ptr(), gv.data_ptr(), go.data_ptr(), gl.data_ptr());
    check_rc(rc, what);
    return {gv, go, gl};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.doc() = "MultiScaleDeformableAttention for MI355X (gfx950): at::Tensor front end of libsemidetr_hip.so";
    // the reference's surface (src/vision.cpp:13-16)
    // (+ an optional trailing `policy_slot`: the call site's slot of the encoder forward-kernel choice, semidetr_hip.h)
    m.def("ms_deform_attn_forward", &ms_deform_attn_forward, "ms_deform_attn_forward", py::arg("value"), py::arg("spatial_shapes"),
          py::arg("level_start_index"), py::arg("sampling_loc"), py::arg("attn_weight"), py::arg("im2col_step"),
          py::arg("policy_slot") = 0);
    m.def("ms_deform_attn_backward", &ms_deform_attn_backward, "ms_deform_attn_backward", py::arg("value"), py::arg("spatial_shapes"),
          py::arg("level_start_index"), py::arg("sampling_loc"), py::arg("attn_weight"), py::arg("grad_output"), py::arg("im2col_step"),
          py::arg("policy_slot") = 0);
    // additions
    m.def("ms_deform_attn_exact_forward", &ms_deform_attn_exact_forward, py::arg("value"), py::arg("spatial_shapes"),
          py::arg("level_start_index"), py::arg("sampling_loc"), py::arg("attn_weight"), py::arg("im2col_step"), py::arg("policy_slot") = 0,
          "ms_deform_attn_forward with SEMIDETR_MSDA_FIXED_FORWARD semantics: the kernel is a function of the arguments alone");
    m.def("ms_deform_attn_exact_backward", &ms_deform_attn_exact_backward, py::arg("value"), py::arg("spatial_shapes"),
          py::arg("level_start_index"), py::arg("sampling_loc"), py::arg("attn_weight"), py::arg("grad_output"), py::arg("im2col_step"),
          py::arg("policy_slot") = 0, "backward with grad_value as the exact, order-independent sum of its contributions (fp32, D = 32)");
    m.def("exact_supported", &exact_supported, py::arg("value"), py::arg("num_levels"), py::arg("num_point"));
    m.def("ms_deform_attn_fused_forward", &ms_deform_attn_fused_forward, py::arg("value"), py::arg("spatial_shapes"),
          py::arg("level_start_index"), py::arg("reference_points"), py::arg("sampling_offsets"), py::arg("attn_logits"),
          py::arg("padding_mask") = py::none(), py::arg("policy_slot") = 0);
    m.def("ms_deform_attn_fused_backward", &ms_deform_attn_fused_backward, py::arg("value"), py::arg("spatial_shapes"),
          py::arg("level_start_index"), py::arg("reference_points"), py::arg("sampling_offsets"), py::arg("attn_logits"),
          py::arg("grad_output"), py::arg("padding_mask") = py::none(), py::arg("policy_slot") = 0);
    m.def("fused_supported", &fused_supported);
    // fp16 / bf16 value maps with fp32 locations and weights (include/semidetr_hip.h: semidetr_msda_forward_h16)
    m.def("ms_deform_attn_h16_forward", &ms_deform_attn_h16_forward, py::arg("value"), py::arg("spatial_shapes"),
          py::arg("level_start_index"), py::arg("sampling_loc"), py::arg("attn_weight"), py::arg("im2col_step") = 64);
    m.def("ms_deform_attn_h16_backward", &ms_deform_attn_h16_backward, py::arg("value"), py::arg("spatial_shapes"),
          py::arg("level_start_index"), py::arg("sampling_loc"), py::arg("attn_weight"), py::arg("grad_output"),
          py::arg("im2col_step") = 64);
    m.def("h16_supported", &h16_supported, py::arg("value"), py::arg("sampling_loc"), py::arg("attn_weight"),
          "value is a 16-bit (Half / BFloat16) CUDA map and locations / weights are Float: the mixed-precision op takes the call");
    // ... and with the fused prologue / epilogue inside those kernels (semidetr_msda_fused_forward_h16)
    m.def("ms_deform_attn_h16_fused_forward", &ms_deform_attn_h16_fused_forward, py::arg("value"), py::arg("spatial_shapes"),
          py::arg("level_start_index"), py::arg("reference_points"), py::arg("sampling_offsets"), py::arg("attn_logits"),
          py::arg("padding_mask") = py::none());
    m.def("ms_deform_attn_h16_fused_backward", &ms_deform_attn_h16_fused_backward, py::arg("value"), py::arg("spatial_shapes"),
          py::arg("level_start_index"), py::arg("reference_points"), py::arg("sampling_offsets"), py::arg("attn_logits"),
          py::arg("grad_output"), py::arg("padding_mask") = py::none());
    m.def("fused_h16_supported", &fused_h16_supported, py::arg("value"), py::arg("reference_points"), py::arg("sampling_offsets"),
          py::arg("attn_logits"),
          "value is a 16-bit CUDA map of 32 channels per head, offsets / logits are both Float or both value's dtype, reference points "
          "Float or value's dtype: the fused 16-bit kernels take the call");
    m.def("gather_choice", [](int64_t slot) { return semidetr_msda_gather_choice((int)slot); }, py::arg("policy_slot") = 0,
          "What an encoder backward of this slot issued now would pick for grad_sampling_loc / grad_attn_weight (SEMIDETR_MSDA_GATHER_WINDOW "
          "or _PATCH): OR it into the backward call's policy_slot and the backward follows what was known at forward time.");
    m.def("mask_extents", &mask_extents, py::arg("padding_mask"), py::arg("spatial_shapes"), py::arg("level_start_index"),
          "(N, L) int32 words vh | vw << 16: level l of image n is padded exactly on rows >= vh / columns >= vw, or -1.  Cached per "
          "(mask, level table) tensors, version and stream; the fused calls fetch it themselves.");
    m.def("pyramid_check", &pyramid_check,
          "bit 0: sum(H*W) == S; bit 1: level_start_index tiles [0, S) exactly.  Cached per tensor pair / version.");
    m.def("abi_version", []() { return SEMIDETR_ABI_VERSION; });      // the header this front end was compiled against
}
