// pfa_kv_append_fp8_capi.hip -- C ABI of the quantising KV-cache append (include/pfa_hip.h, pfa_kv_append_q8*): the rules of
// pfa_fa3_kv_quant, then everything pfa_kv_append says of the same argument block, and the launch of the QUANT instantiations of
// kv_append_kernel.  Built with -ffp-contract=off (csrc/Makefile), as the rotary object is: the plain-torch model is bit-equal.
// No allocation, no synchronisation, no process-wide state, no workspace.
#include "pfa_hip.h"

#include <hip/hip_runtime.h>

#include "kv_append_kernel.h"
#include "pfa_fp8_host.h"

namespace {

// 16-element work items of one sequence, at most, and the workgroups: from host shapes only, as pfa_kv_append's
int64_t items(const pfa_kv_append_args* a) { return (int64_t)a->max_seqlen_q * a->Hkv * (a->D / 16); }
int64_t workgroups(const pfa_kv_append_args* a) {
    return (int64_t)a->B * ((items(a) + pfa::KV_APPEND_THREADS - 1) / pfa::KV_APPEND_THREADS);
}

int check(const pfa_kv_append_args* a, const pfa_fa3_kv_quant* quant) {
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_kv_append_args)) return PFA_ERR_STRUCT_SIZE;
    const int st = pfa::check_kv_quant(quant, a);
    if (st != PFA_OK) return st;
    if (a->D % 16 != 0) return PFA_ERR_HEAD_DIM;
    return pfa_kv_append_check(a);       // its grid has twice the items of this one
}

template <typename T>
const void* kernel_of(bool varlen, bool paged) {
    return varlen ? (paged ? (const void*)&pfa::kv_append_kernel<true, true, true, T> : (const void*)&pfa::kv_append_kernel<true, false, true, T>)
                  : (paged ? (const void*)&pfa::kv_append_kernel<false, true, true, T> : (const void*)&pfa::kv_append_kernel<false, false, true, T>);
}

}  // namespace

extern "C" {

int pfa_kv_append_q8_check(const pfa_kv_append_args* a, const pfa_fa3_kv_quant* quant) { return check(a, quant); }

int pfa_kv_append_q8(const pfa_kv_append_args* a, const pfa_fa3_kv_quant* quant, void* stream) {
    const int st = check(a, quant);
    if (st != PFA_OK) return st;
    pfa::KvAppendQ8Params p;
    p.k_new = a->k_new; p.v_new = a->v_new; p.k_cache = a->k_cache; p.v_cache = a->v_cache;
    p.cu_seqlens_q = a->cu_seqlens_q;
    p.kn_sb = a->kn_stride_b; p.kn_ss = a->kn_stride_s; p.kn_sh = a->kn_stride_h;
    p.vn_sb = a->vn_stride_b; p.vn_ss = a->vn_stride_s; p.vn_sh = a->vn_stride_h;
    pfa::fill_cache_params(p, a);
    p.nchunk = (int32_t)(workgroups(a) / a->B);
    p.Sq = a->max_seqlen_q; p.total_new = a->total_new;
    p.dchunks = a->D / 16; p.units = a->Hkv * (a->D / 16);
    p.k_descale = quant->k_descale; p.v_descale = quant->v_descale; p.ds_sb = quant->descale_stride_b;

    const bool varlen = a->cu_seqlens_q != nullptr, paged = a->block_table != nullptr;
    const void* fn = a->dtype == PFA_DTYPE_BF16 ? kernel_of<__bf16>(varlen, paged) : kernel_of<_Float16>(varlen, paged);
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    return pfa::launch(fn, dim3((unsigned)workgroups(a)), pfa::KV_APPEND_THREADS, p, 0, stream);
}

}  // extern "C"
