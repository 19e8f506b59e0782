// pfa_qk_norm_capi.hip -- C ABI of QK-norm fused with the rotary embedding of the training calls (include/pfa_hip_qk_norm.h,
// pfa_qk_norm*, pfa_qk_norm_bwd*): validation and the launches of qk_norm_kernel.h.  No allocation, no synchronisation, no process-wide
// state; the backward's workspace is the caller's.
// Compiled with -ffp-contract=off (csrc/Makefile), as pfa_rotary_capi is: the kernels' products and sums round separately.
#include "pfa_hip_qk_norm.h"

#include <math.h>
#include <stdio.h>

#include "pfa_rows_host.h"
#include "qk_norm_kernel.h"

namespace {

namespace rows = pfa::rows;
using rows::in_place;
using rows::kLim;
using rows::kPiece;
constexpr uint32_t kFlags = PFA_QKNORM_INTERLEAVED | PFA_QKNORM_UNIT_OFFSET;

// ---- what both blocks add to the rules of pfa_rows_host.h ------------------------------------------------------------------------------
template <typename A>
int64_t units(const A* a) { return rows::units(a, a->D); }
template <typename A>
bool head_dims_ok(const A* a) { return (a->D == 64 || a->D == 128) && rows::rot_dim_ok(a, true); }
// the rules of both blocks between the pointer rules and the stride rules, in their order
template <typename A>
int check_shape_dims_dtypes(const A* a) {
    if (!rows::shape_ok(a, true) || !(a->eps >= 0.f) || !isfinite(a->eps)) return PFA_ERR_SHAPE;
    if (!head_dims_ok(a)) return PFA_ERR_HEAD_DIM;
    if (a->dtype != PFA_DTYPE_BF16 && a->dtype != PFA_DTYPE_FP16) return PFA_ERR_DTYPE;
    if (a->w_dtype != a->dtype && a->w_dtype != PFA_DTYPE_FP32) return PFA_ERR_DTYPE;
    return PFA_OK;
}

// ---- forward -------------------------------------------------------------------------------------------------------------------------
int64_t workgroups(const pfa_qk_norm_args* a) { return rows::workgroups(a, units(a), pfa::QKNORM_THREADS); }

int check(const pfa_qk_norm_args* a) {
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_qk_norm_args)) return PFA_ERR_STRUCT_SIZE;
    if (a->flags & ~kFlags) return PFA_ERR_FLAGS;
    if (!rows::positions_exclusive(a) || !rows::in_place_consistent(a)) return PFA_ERR_FLAGS;
    if (!a->x0 || !a->x0_out || !a->w0) return PFA_ERR_NULL;
    if (!rows::null_iff(a->H1 == 0, {a->x1, a->x1_out, a->w1}) || !rows::null_iff(a->rot_dim == 0, {a->cos, a->sin})) return PFA_ERR_NULL;
    const int st = check_shape_dims_dtypes(a);
    if (st != PFA_OK) return st;
    if (!rows::fwd_strides_ok(a) || (in_place(a) && !rows::in_place_strides_equal(a)) || !rows::tables_ok(a)) return PFA_ERR_STRIDE;
    if (!rows::all_aligned16({a->x0, a->x0_out, a->x1, a->x1_out, a->w0, a->w1, a->cos, a->sin}) || !rows::ints_aligned(a)) return PFA_ERR_ALIGN;
    // a sequence's item index and the grid inside 32 bits
    if (!rows::items_fit(a, units(a), pfa::QKNORM_THREADS) || workgroups(a) > kLim) return PFA_ERR_SHAPE;
    return PFA_OK;
}

// ---- backward ------------------------------------------------------------------------------------------------------------------------
int64_t nrc(const pfa_qk_norm_bwd_args* a) { return ((int64_t)a->S + pfa::QKNORM_BWD_ROWS - 1) / pfa::QKNORM_BWD_ROWS; }
int64_t partials(const pfa_qk_norm_bwd_args* a) {   // stage-1 workgroups (after the shape rules: all factors >= 1)
    return (a->H1 > 0 ? 2 : 1) * (int64_t)a->B * nrc(a);
}
bool limits_ok(const pfa_qk_norm_bwd_args* a) { return rows::items_fit(a, units(a), pfa::QKNORM_THREADS) && partials(a) <= kLim; }
size_t workspace_bytes(const pfa_qk_norm_bwd_args* a) { return (size_t)partials(a) * (size_t)a->D * sizeof(float); }

int check(const pfa_qk_norm_bwd_args* a) {
    using pfa::aligned4;
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_qk_norm_bwd_args)) return PFA_ERR_STRUCT_SIZE;
    if (a->flags & ~kFlags) return PFA_ERR_FLAGS;
    if (!rows::positions_exclusive(a)) return PFA_ERR_FLAGS;
    if (a->dx0 && (a->dx0 == a->x0 || a->dx0 == a->dy0)) return PFA_ERR_FLAGS;      // in place is refused in the backward
    if (a->dx1 && (a->dx1 == a->x1 || a->dx1 == a->dy1)) return PFA_ERR_FLAGS;
    if (!a->x0 || !a->dy0 || !a->dx0 || !a->w0 || !a->dw0 || !a->workspace) return PFA_ERR_NULL;
    if (!rows::null_iff(a->H1 == 0, {a->x1, a->dy1, a->dx1, a->w1, a->dw1}) || !rows::null_iff(a->rot_dim == 0, {a->cos, a->sin}))
        return PFA_ERR_NULL;
    const int st = check_shape_dims_dtypes(a);
    if (st != PFA_OK) return st;
    if (!pfa::multiples_of(8, {a->x0_stride_s, a->x0_stride_h, a->dy0_stride_s, a->dy0_stride_h, a->dx0_stride_s, a->dx0_stride_h,
                               a->x1_stride_s, a->x1_stride_h, a->dy1_stride_s, a->dy1_stride_h, a->dx1_stride_s, a->dx1_stride_h}))
        return PFA_ERR_STRIDE;
    if (!a->cu_seqlens && !pfa::multiples_of(8, {a->x0_stride_b, a->dy0_stride_b, a->dx0_stride_b, a->x1_stride_b, a->dy1_stride_b, a->dx1_stride_b}))
        return PFA_ERR_STRIDE;
    if (!rows::tables_ok(a)) return PFA_ERR_STRIDE;
    if (!rows::all_aligned16({a->x0, a->dy0, a->dx0, a->x1, a->dy1, a->dx1, a->w0, a->w1, a->cos, a->sin})) return PFA_ERR_ALIGN;
    if (!aligned4(a->dw0) || !aligned4(a->dw1) || !aligned4(a->workspace) || !rows::ints_aligned(a)) return PFA_ERR_ALIGN;
    if (!limits_ok(a)) return PFA_ERR_SHAPE;
    if (a->workspace_bytes < workspace_bytes(a)) return PFA_ERR_NULL;
    return PFA_OK;
}

// ---- the kernel names and tables, each in one place ----------------------------------------------------------------------------------
template <typename A>
void name_of(const A* a, const char* stem, const char* tail, bool inplace, char* buf, size_t n) {
    snprintf(buf, n, "%s_%s_d%d%s%s%s%s%s%s%s", stem, a->dtype == PFA_DTYPE_BF16 ? "bf16" : "fp16", a->D, a->cu_seqlens ? "_packed" : "",
             (a->flags & PFA_QKNORM_INTERLEAVED) ? "_interleaved" : "", a->rot_dim ? "_rot" : "", (a->flags & PFA_QKNORM_UNIT_OFFSET) ? "_unit" : "",
             a->w_dtype == PFA_DTYPE_FP32 ? "_w32" : "", inplace ? "_inplace" : "", tail);
}

template <typename T, int G>
pfa::KernelFn<pfa::QkNormParams> fwd_of(bool packed, bool interleaved) {
    return pfa::dispatch_bools(
        [](auto pk, auto il) -> pfa::KernelFn<pfa::QkNormParams> { return &pfa::qk_norm_kernel<T, G, pk.value, il.value>; }, packed, interleaved);
}
template <typename T, int G>
pfa::KernelFn<pfa::QkNormBwdParams> bwd_of(bool packed, bool interleaved) {
    return pfa::dispatch_bools(
        [](auto pk, auto il) -> pfa::KernelFn<pfa::QkNormBwdParams> { return &pfa::qk_norm_bwd_kernel<T, G, pk.value, il.value>; }, packed,
        interleaved);
}

}  // namespace

extern "C" {

int pfa_qk_norm_check(const pfa_qk_norm_args* a) { return check(a); }

int pfa_qk_norm_describe(const pfa_qk_norm_args* a, char* buf, size_t n) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    if (buf && n) name_of(a, "qk_norm", "", in_place(a), buf, n);
    return (int)workgroups(a);
}

int pfa_qk_norm(const pfa_qk_norm_args* a, void* stream) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    const bool packed = a->cu_seqlens != nullptr;
    pfa::QkNormParams p;
    rows::fill_fwd(p, a, units(a), pfa::QKNORM_THREADS);
    p.w0 = a->w0; p.w1 = a->w1;
    p.eps = a->eps; p.inv_d = 1.0f / (float)a->D;
    p.w_fp32 = a->w_dtype == PFA_DTYPE_FP32;
    p.unit_offset = (a->flags & PFA_QKNORM_UNIT_OFFSET) ? 1 : 0;

    const bool il = (a->flags & PFA_QKNORM_INTERLEAVED) != 0;
    const auto fn = pfa::dispatch_elem_dim(a->dtype, a->D, [&](auto tag) {
        using Tag = decltype(tag);
        return fwd_of<typename Tag::type, Tag::D / kPiece>(packed, il);
    });
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    return pfa::launch(fn, dim3((unsigned)workgroups(a)), pfa::QKNORM_THREADS, p, 0, stream);
}

size_t pfa_qk_norm_bwd_workspace_bytes(const pfa_qk_norm_bwd_args* a) {
    if (!a || a->size != sizeof(pfa_qk_norm_bwd_args)) return 0;
    if (a->B < 1 || a->S < 1 || a->H0 < 1 || a->H1 < 0 || (a->cu_seqlens && (a->total < 1 || a->S > a->total))) return 0;
    if (!head_dims_ok(a) || !limits_ok(a)) return 0;
    return workspace_bytes(a);
}

int pfa_qk_norm_bwd_check(const pfa_qk_norm_bwd_args* a) { return check(a); }

int pfa_qk_norm_bwd_describe(const pfa_qk_norm_bwd_args* a, char* buf, size_t n) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    if (buf && n) {
        char tail[32];
        snprintf(tail, sizeof(tail), "_r%d+dw", pfa::QKNORM_BWD_ROWS);
        name_of(a, "qk_norm_bwd", tail, false, buf, n);
    }
    return (int)partials(a);
}

int pfa_qk_norm_bwd(const pfa_qk_norm_bwd_args* a, void* stream) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    const bool packed = a->cu_seqlens != nullptr;
    pfa::QkNormBwdParams p;
    p.x0 = a->x0; p.dy0 = a->dy0; p.dx0 = a->dx0; p.x1 = a->x1; p.dy1 = a->dy1; p.dx1 = a->dx1;
    p.w0 = a->w0; p.w1 = a->w1; p.dw0 = a->dw0; p.dw1 = a->dw1;
    p.partial = (float*)a->workspace;
    rows::fill_common(p, a);
    PFA_FILL_STRIDES(p, a, x0); PFA_FILL_STRIDES(p, a, dy0); PFA_FILL_STRIDES(p, a, dx0);
    PFA_FILL_STRIDES(p, a, x1); PFA_FILL_STRIDES(p, a, dy1); PFA_FILL_STRIDES(p, a, dx1);
    p.eps = a->eps; p.inv_d = 1.0f / (float)a->D;
    p.nrc = (int32_t)nrc(a);
    p.B = a->B; p.H1 = a->H1;
    p.w_fp32 = a->w_dtype == PFA_DTYPE_FP32;
    p.unit_offset = (a->flags & PFA_QKNORM_UNIT_OFFSET) ? 1 : 0;

    const bool il = (a->flags & PFA_QKNORM_INTERLEAVED) != 0;
    const auto stage1 = pfa::dispatch_elem_dim(a->dtype, a->D, [&](auto tag) {
        using Tag = decltype(tag);
        return bwd_of<typename Tag::type, Tag::D / kPiece>(packed, il);
    });
    const pfa::KernelFn<pfa::QkNormBwdParams> stage2 = a->D == 128 ? &pfa::qk_norm_dw_kernel<128> : &pfa::qk_norm_dw_kernel<64>;
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    const int st1 = pfa::launch(stage1, dim3((unsigned)partials(a)), pfa::QKNORM_THREADS, p, 0, stream);
    if (st1 != PFA_OK) return st1;
    return pfa::launch(stage2, dim3((a->H1 > 0 ? 2u : 1u) * (unsigned)(a->D / kPiece)), pfa::QKNORM_THREADS, p, 0, stream);
}

}  // extern "C"
