// pfa_prefill_varlen_fp8_capi.hip -- C ABI of the ragged forward over an FP8 (e4m3fn) KV cache (include/pfa_hip.h,
// pfa_fa3_prefill_varlen_q8*): the entry points and the KV8 + VARLEN instantiations of fa3_prefill_kernel.  Built and laid out as
// pfa_prefill_fp8_capi.hip.  No allocation, no synchronisation, no process-wide state, no workspace.
#include "pfa_prefill_host.h"

using namespace pfa::prefill;

extern "C" {

int pfa_fa3_prefill_varlen_q8_check(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant) {
    return entry_check<true>(a, ext, quant, nullptr);
}

int pfa_fa3_prefill_varlen_q8_describe(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant,
                                       char* buf, size_t n) {
    return entry_describe<true>(a, ext, quant, nullptr, buf, n);
}

int pfa_fa3_prefill_varlen_q8(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant, void* stream) {
    return entry_run<pfa::MODE_KV8>(a, ext, quant, nullptr, stream);
}

}  // extern "C"
