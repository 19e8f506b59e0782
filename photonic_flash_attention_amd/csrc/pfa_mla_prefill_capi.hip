// pfa_mla_prefill_capi.hip -- C ABI of the non-absorbed MLA prefill over packed sequences (include/pfa_hip_mla_prefill.h, ABI v9 additive):
// the entry points and the 8 instantiations of fa3_mla_prefill_kernel (bf16 / fp16 x causal x output).  One or H rotary key heads is a
// stride (0 between the heads of a shared one), not an instantiation.  A file of its own: every other object is built from what it was
// built from.
// No allocation, no synchronisation, no process-wide state, no workspace, a grid from host shapes only.
#include <stdio.h>

#include "fa3_mla_prefill_kernel.h"
#include "pfa_host.h"
#include "pfa_hip_mla_prefill.h"

using pfa::mlap::Params;

static_assert(pfa::mlap::DN == PFA_MLA_PREFILL_D_NOPE && pfa::mlap::DR == PFA_MLA_PREFILL_D_ROPE && pfa::mlap::DV == PFA_MLA_PREFILL_D_V,
              "the header and the kernel agree on the widths");

namespace {

// fp32 output: P carried as a 16-bit hi + lo pair (SPLITP)
pfa::KernelFn<Params> kernel_mla_prefill(int dtype, bool causal, bool out32) {
    return pfa::dispatch_bools([](auto bf, auto c, auto o32) -> pfa::KernelFn<Params> {
        using T = std::conditional_t<bf.value, __bf16, _Float16>;
        return &pfa::mlap::fa3_mla_prefill_kernel<T, c.value, o32.value, pfa::out_t<o32.value, T>>;
    }, dtype == PFA_DTYPE_BF16, causal, out32);
}

// a 64-key tile's rows are addressed by 32-bit offsets from a per-tile buffer descriptor that ends `width` elements into its last row, and
// a row behind a sequence's last key must start past that end
bool key_stride_ok(int64_t stride_s, int width) { return stride_s >= width && stride_s * 2 * pfa::BLOCK_N + width * 2 <= 0x7fffffffLL; }

// the field rules of include/pfa_hip_mla_prefill.h in the order their errors are reported -> PFA_OK and the workgroups of the launch in *grid
int check(const pfa_mla_prefill_args* a, int64_t* grid) {
    using namespace pfa::mlap;
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_mla_prefill_args)) return PFA_ERR_STRUCT_SIZE;
    if (a->flags != 0 || a->reserved != 0) return PFA_ERR_FLAGS;
    if (!a->q || !a->k_nope || !a->k_rope || !a->v || !a->o || !a->cu_seqlens_q || !a->cu_seqlens_k) return PFA_ERR_NULL;
    if (a->B < 1 || a->H < 1 || a->total_q < 1 || a->total_k < 1 || (a->rope_heads != 1 && a->rope_heads != a->H)) return PFA_ERR_SHAPE;
    if (a->max_seqlen_q < 1 || a->max_seqlen_q > a->total_q || a->max_seqlen_k < 1 || a->max_seqlen_k > a->total_k) return PFA_ERR_SHAPE;
    if (!pfa::scale_ok(a->softmax_scale)) return PFA_ERR_SHAPE;
    if (a->dtype_in != PFA_DTYPE_BF16 && a->dtype_in != PFA_DTYPE_FP16) return PFA_ERR_DTYPE;
    if (a->dtype_out != a->dtype_in && a->dtype_out != PFA_DTYPE_FP32) return PFA_ERR_DTYPE;
    if (!pfa::multiples_of(8, {a->q_stride_s, a->q_stride_h, a->kn_stride_s, a->kn_stride_h, a->kr_stride_s, a->v_stride_s, a->v_stride_h}))
        return PFA_ERR_STRIDE;
    if (a->rope_heads != 1 && a->kr_stride_h % 8 != 0) return PFA_ERR_STRIDE;
    if (!pfa::multiples_of(4, {a->o_stride_s, a->o_stride_h})) return PFA_ERR_STRIDE;
    if (a->q_stride_s < DN + DR || a->o_stride_s < DV) return PFA_ERR_STRIDE;
    if (!key_stride_ok(a->kn_stride_s, DN) || !key_stride_ok(a->kr_stride_s, DR) || !key_stride_ok(a->v_stride_s, DV)) return PFA_ERR_STRIDE;
    if (!pfa::aligned16(a->q) || !pfa::aligned16(a->k_nope) || !pfa::aligned16(a->k_rope) || !pfa::aligned16(a->v) || !pfa::aligned16(a->o))
        return PFA_ERR_ALIGN;
    if (!pfa::aligned4(a->lse) || !pfa::aligned4(a->cu_seqlens_q) || !pfa::aligned4(a->cu_seqlens_k)) return PFA_ERR_ALIGN;
    *grid = (int64_t)a->B * a->H * ((a->max_seqlen_q + BLOCK_M - 1) / BLOCK_M);
    return *grid > 0x7fffffffLL ? PFA_ERR_SHAPE : PFA_OK;
}

}  // namespace

extern "C" {

int pfa_mla_prefill_check(const pfa_mla_prefill_args* a) {
    int64_t grid;
    return check(a, &grid);
}

int pfa_mla_prefill_describe(const pfa_mla_prefill_args* a, char* buf, size_t n) {
    int64_t grid;
    const int st = check(a, &grid);
    if (st != PFA_OK) return st;
    if (buf && n)
        snprintf(buf, n, "mla_prefill_%s_%s_%s_%s", a->dtype_in == PFA_DTYPE_BF16 ? "bf16" : "fp16", a->dtype_out == PFA_DTYPE_FP32 ? "o32" : "o16",
                 a->causal ? "causal" : "full", a->rope_heads == 1 ? "rope1" : "ropeH");
    return (int)grid;
}

int pfa_mla_prefill(const pfa_mla_prefill_args* a, void* stream) {
    int64_t grid;
    const int st = check(a, &grid);
    if (st != PFA_OK) return st;
    Params p;
    p.q = a->q; p.kn = a->k_nope; p.kr = a->k_rope; p.v = a->v; p.o = a->o; p.lse = a->lse;
    p.cu_q = a->cu_seqlens_q; p.cu_k = a->cu_seqlens_k;
    p.q_ss = a->q_stride_s; p.q_sh = a->q_stride_h;
    p.kn_ss = a->kn_stride_s; p.kn_sh = a->kn_stride_h;
    p.kr_ss = a->kr_stride_s; p.kr_sh = a->rope_heads == 1 ? 0 : a->kr_stride_h;     // one rotary key head serves every query head
    p.v_ss = a->v_stride_s; p.v_sh = a->v_stride_h;
    p.o_ss = a->o_stride_s; p.o_sh = a->o_stride_h;
    p.B = a->B; p.H = a->H; p.total_q = a->total_q; p.total_k = a->total_k; p.max_q = a->max_seqlen_q; p.max_k = a->max_seqlen_k;
    p.nqblk = (a->max_seqlen_q + pfa::mlap::BLOCK_M - 1) / pfa::mlap::BLOCK_M;
    p.scale_log2 = a->softmax_scale * pfa::LOG2E;
    const auto fn = kernel_mla_prefill(a->dtype_in, a->causal != 0, a->dtype_out == PFA_DTYPE_FP32);
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    return pfa::launch(fn, dim3((unsigned)grid), pfa::mlap::THREADS, p, pfa::mlap::LDS_BYTES, stream);
}

}  // extern "C"
