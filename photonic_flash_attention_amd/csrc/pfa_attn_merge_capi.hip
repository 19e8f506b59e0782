// pfa_attn_merge_capi.hip -- C ABI of the merge of partial attention results (include/pfa_hip.h, pfa_attn_merge*): validation and the
// launch of attn_merge_kernel.  No allocation, no synchronisation, no process-wide state, no workspace.
#include "pfa_hip.h"

#include <hip/hip_runtime.h>
#include <stdio.h>

#include "attn_merge_kernel.h"
#include "pfa_host.h"

static_assert(PFA_MERGE_MAX_PARTS == pfa::ATTN_MERGE_MAX_PARTS, "the header's part limit is the kernel's");

namespace {

// 16-byte (16-bit output) or 32-byte (fp32) work items: 8 elements of one (row, head)
// (after the shape rules: all factors >= 1), saturated past 32 bits so that the product cannot wrap
int64_t items(const pfa_attn_merge_args* a) {
    const int64_t lim = 0x7fffffffLL, rows = (int64_t)a->B * a->Sq;
    if (rows > lim || rows * a->H > lim) return lim;
    return rows * a->H * (a->D / 8);
}

// workgroups: from host shapes only, so a captured graph stays valid while the tensors' contents change
int64_t workgroups(const pfa_attn_merge_args* a) { return (items(a) + pfa::ATTN_MERGE_THREADS - 1) / pfa::ATTN_MERGE_THREADS; }

bool known_dtype(int32_t d) { return d == PFA_DTYPE_BF16 || d == PFA_DTYPE_FP16 || d == PFA_DTYPE_FP32; }
const char* dtype_name(int32_t d) { return d == PFA_DTYPE_BF16 ? "bf16" : d == PFA_DTYPE_FP16 ? "fp16" : "fp32"; }

int check(const pfa_attn_merge_args* a) {
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_attn_merge_args)) return PFA_ERR_STRUCT_SIZE;
    if (a->flags != 0 || a->reserved0 != 0 || a->reserved1 != 0) return PFA_ERR_FLAGS;
    if (!a->o) return PFA_ERR_NULL;
    const int parts = a->n_parts < 0 ? 0 : a->n_parts > PFA_MERGE_MAX_PARTS ? PFA_MERGE_MAX_PARTS : a->n_parts;      // those that can be looked at
    for (int n = 0; n < parts; ++n)
        if (!a->o_part[n] || !a->lse_part[n]) return PFA_ERR_NULL;
    if (a->n_parts < 2 || a->n_parts > PFA_MERGE_MAX_PARTS || a->B <= 0 || a->H <= 0 || a->Sq <= 0) return PFA_ERR_SHAPE;
    if (a->D < 8 || a->D % 8 != 0 || a->D > 256) return PFA_ERR_HEAD_DIM;
    if (!known_dtype(a->dtype_part) || !known_dtype(a->dtype_out)) return PFA_ERR_DTYPE;
    if (a->dtype_part != PFA_DTYPE_FP32 && a->dtype_out != a->dtype_part && a->dtype_out != PFA_DTYPE_FP32) return PFA_ERR_DTYPE;
    const int part_mult = a->dtype_part == PFA_DTYPE_FP32 ? 4 : 8;
    for (int n = 0; n < a->n_parts; ++n)
        if (!pfa::multiples_of(part_mult, {a->op_stride_b[n], a->op_stride_h[n], a->op_stride_s[n]})) return PFA_ERR_STRIDE;
    if (!pfa::multiples_of(a->dtype_out == PFA_DTYPE_FP32 ? 4 : 8, {a->o_stride_b, a->o_stride_h, a->o_stride_s})) return PFA_ERR_STRIDE;
    if (!pfa::aligned16(a->o) || !pfa::aligned4(a->lse_out)) return PFA_ERR_ALIGN;
    for (int n = 0; n < a->n_parts; ++n)
        if (!pfa::aligned16(a->o_part[n]) || !pfa::aligned4(a->lse_part[n])) return PFA_ERR_ALIGN;
    // the grid, and the item index inside 32 bits
    if (items(a) + pfa::ATTN_MERGE_THREADS > 0x7fffffffLL) return PFA_ERR_SHAPE;
    return PFA_OK;
}

using MergeFn = pfa::KernelFn<pfa::AttnMergeParams>;

template <typename TP, typename TO>
MergeFn kernel_for_parts(int n) {
    switch (n) {
        case 2: return &pfa::attn_merge_kernel<TP, TO, 2>;
        case 3: return &pfa::attn_merge_kernel<TP, TO, 3>;
        case 4: return &pfa::attn_merge_kernel<TP, TO, 4>;
        case 5: return &pfa::attn_merge_kernel<TP, TO, 5>;
        case 6: return &pfa::attn_merge_kernel<TP, TO, 6>;
        case 7: return &pfa::attn_merge_kernel<TP, TO, 7>;
        default: return &pfa::attn_merge_kernel<TP, TO, 8>;
    }
}

template <typename TP>
MergeFn kernel_for_out(int dtype_out, int n) {
    return dtype_out == PFA_DTYPE_FP32 ? kernel_for_parts<TP, float>(n)
         : dtype_out == PFA_DTYPE_BF16 ? kernel_for_parts<TP, __bf16>(n) : kernel_for_parts<TP, _Float16>(n);
}

// the instantiation of a checked call: 16-bit parts keep their type or widen to fp32, fp32 parts go to any of the three
MergeFn kernel(const pfa_attn_merge_args* a) {
    if (a->dtype_part == PFA_DTYPE_FP32) return kernel_for_out<float>(a->dtype_out, a->n_parts);
    if (a->dtype_part == PFA_DTYPE_BF16)
        return a->dtype_out == PFA_DTYPE_FP32 ? kernel_for_parts<__bf16, float>(a->n_parts) : kernel_for_parts<__bf16, __bf16>(a->n_parts);
    return a->dtype_out == PFA_DTYPE_FP32 ? kernel_for_parts<_Float16, float>(a->n_parts) : kernel_for_parts<_Float16, _Float16>(a->n_parts);
}

}  // namespace

extern "C" {

int pfa_attn_merge_check(const pfa_attn_merge_args* a) { return check(a); }

int pfa_attn_merge_describe(const pfa_attn_merge_args* a, char* buf, size_t n) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    if (buf && n) snprintf(buf, n, "attn_merge_%s_%s_d%d_n%d", dtype_name(a->dtype_part), dtype_name(a->dtype_out), a->D, a->n_parts);
    return (int)workgroups(a);
}

int pfa_attn_merge(const pfa_attn_merge_args* a, void* stream) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    pfa::AttnMergeParams p = {};
    for (int n = 0; n < a->n_parts; ++n) {
        pfa::AttnMergePart& q = p.part[n];
        q.o = a->o_part[n]; q.lse = a->lse_part[n];
        q.o_sb = a->op_stride_b[n]; q.o_sh = a->op_stride_h[n]; q.o_ss = a->op_stride_s[n];
        q.l_sb = a->lp_stride_b[n]; q.l_sh = a->lp_stride_h[n]; q.l_ss = a->lp_stride_s[n];
    }
    p.o = a->o; p.lse_out = a->lse_out;
    p.o_sb = a->o_stride_b; p.o_sh = a->o_stride_h; p.o_ss = a->o_stride_s;
    p.lo_sb = a->lo_stride_b; p.lo_sh = a->lo_stride_h; p.lo_ss = a->lo_stride_s;
    p.items = (int32_t)items(a); p.H = a->H; p.Sq = a->Sq; p.dchunks = a->D / 8;

    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    return pfa::launch(kernel(a), dim3((unsigned)workgroups(a)), pfa::ATTN_MERGE_THREADS, p, 0, stream);
}

}  // extern "C"
