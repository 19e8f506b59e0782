// pfa_prefill_varlen_fp8_capi.hip -- C ABI of the ragged forward over an FP8 (e4m3fn) KV cache (include/pfa_hip.h,
// pfa_fa3_prefill_varlen_q8*): the rules of pfa_fa3_kv_quant, then everything pfa_fa3_prefill_varlen_check_ex says of the same argument
// block, and the launch of the KV8 + VARLEN instantiations of fa3_prefill_kernel.  Built and laid out as pfa_prefill_fp8_capi.hip.
// No allocation, no synchronisation, no process-wide state, no workspace.
#include "pfa_prefill_host.h"

namespace {

int check(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant) {
    const int st = pfa::prefill::check_q8_front(a, ext, quant);
    return st != PFA_OK ? st : pfa_fa3_prefill_varlen_check_ex(a, ext);
}

}  // namespace

extern "C" {

int pfa_fa3_prefill_varlen_q8_check(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant) {
    return check(a, ext, quant);
}

int pfa_fa3_prefill_varlen_q8_describe(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant,
                                       char* buf, size_t n) {
    const int st = pfa::prefill::check_q8_front(a, ext, quant);
    if (st != PFA_OK) return st;
    char name[160];
    const int items = pfa_fa3_prefill_varlen_describe_ex(a, ext, name, sizeof name);
    if (items >= 0) pfa::prefill::name_q8(name, buf, n);
    return items;
}

int pfa_fa3_prefill_varlen_q8(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant, void* stream) {
    const int st = check(a, ext, quant);
    return st != PFA_OK ? st : pfa::prefill::launch_q8<true>(a, quant, stream);
}

}  // extern "C"
