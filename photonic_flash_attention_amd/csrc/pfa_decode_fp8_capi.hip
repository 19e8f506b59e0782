// pfa_decode_fp8_capi.hip -- C ABI of the split-KV decode over an FP8 (e4m3fn) KV cache (include/pfa_hip.h, pfa_fa3_decode_q8*): the
// rules of pfa_fa3_kv_quant, then everything pfa_fa3_decode_ex says of the same argument block, and the launch of the KV8 instantiations of
// fa3_decode_kernel.  Validation is asked of the 16-bit call; the split count, the workgroups, the workspace layout and the launches are
// pfa_decode_host.h's, which both units share, so the two cannot drift apart.  A file of its own: the 16-bit decode's object is built
// from what it was built from.  No allocation, no synchronisation, no process-wide state.
#include <stdio.h>

#include "pfa_decode_host.h"
#include "pfa_fp8_host.h"

namespace {

// of arguments that pass, the plan is the window-less 16-bit call's: pfa::decode::plan(a, 0)
int check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant) {
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_fa3_decode_args)) return PFA_ERR_STRUCT_SIZE;
    const int st = pfa::check_kv_quant(quant, a);
    if (st != PFA_OK) return st;
    if (pfa::fp8_refuses_window(ext)) return PFA_ERR_FLAGS;
    return pfa_fa3_decode_check_ex(a, ext);
}

}  // namespace

extern "C" {

size_t pfa_fa3_decode_q8_workspace_bytes(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant) {
    if (!a || a->size != sizeof(pfa_fa3_decode_args) || pfa::check_kv_quant(quant, a, false) != PFA_OK) return 0;
    if (pfa::fp8_refuses_window(ext)) return 0;
    return pfa_fa3_decode_workspace_bytes_ex(a, ext);
}

int pfa_fa3_decode_q8_check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant) { return check(a, ext, quant); }

int pfa_fa3_decode_q8_describe(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant, char* buf, size_t n,
                               int32_t* nsplit) {
    const int st = check(a, ext, quant);
    if (st != PFA_OK) return st;
    const pfa::decode::Plan pl = pfa::decode::plan(a, 0);
    if (buf && n)
        snprintf(buf, n, "fa3_decode_%s_d%d_%s_kv8%s%s", a->dtype_in == PFA_DTYPE_BF16 ? "bf16" : "fp16", a->D,
                 a->dtype_out == PFA_DTYPE_FP32 ? "o32" : "o16", pl.nsplit > 1 ? "+combine" : "", a->block_table ? "_paged" : "");
    if (nsplit) *nsplit = pl.nsplit;
    return (int)pl.items;
}

int pfa_fa3_decode_q8(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant, void* stream) {
    const int st = check(a, ext, quant);
    if (st != PFA_OK) return st;
    const pfa::decode::Plan pl = pfa::decode::plan(a, 0);
    pfa::dec::DecodeQ8Params p;
    pfa::decode::fill_params(p, a, pl);
    p.k_descale = quant->k_descale; p.v_descale = quant->v_descale; p.ds_sb = quant->descale_stride_b;
    return pfa::decode::launch<false, false, true>(a, pl, p, stream);
}

}  // extern "C"
