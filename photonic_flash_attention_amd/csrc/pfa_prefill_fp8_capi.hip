// pfa_prefill_fp8_capi.hip -- C ABI of the forward over an FP8 (e4m3fn) KV cache (include/pfa_hip.h, pfa_fa3_prefill_q8*): the entry
// points and the uniform KV8 instantiations of fa3_prefill_kernel.  The rules of pfa_fa3_kv_quant come first, then everything
// pfa_fa3_prefill_check_ex says of the same argument block: one check in pfa_prefill_host.h, so the two cannot drift apart.  A file of
// its own: the 16-bit objects are built from what they were built from, and the 32 kernels compile side by side with theirs.
// No allocation, no synchronisation, no process-wide state, no workspace.
#include "pfa_prefill_host.h"

using namespace pfa::prefill;

extern "C" {

int pfa_fa3_prefill_q8_check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant) {
    return entry_check<true>(a, ext, quant, nullptr);
}

int pfa_fa3_prefill_q8_describe(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant, char* buf, size_t n) {
    return entry_describe<true>(a, ext, quant, nullptr, buf, n);
}

int pfa_fa3_prefill_q8(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant, void* stream) {
    return entry_run<pfa::MODE_KV8>(a, ext, quant, nullptr, stream);
}

}  // extern "C"
