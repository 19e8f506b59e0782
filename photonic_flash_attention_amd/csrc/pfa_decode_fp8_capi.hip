// pfa_decode_fp8_capi.hip -- C ABI of the split-KV decode over an FP8 (e4m3fn) KV cache (include/pfa_hip.h, pfa_fa3_decode_q8*): the
// entry points and the KV8 instantiations of fa3_decode_kernel.  The rules of pfa_fa3_kv_quant come first, then everything pfa_fa3_decode_ex
// says of the same blocks: one check, one plan and one launch in pfa_decode_host.h, which the three decode units share, so they cannot
// drift apart.  A file of its own: the 16-bit decode's object is built from what it was built from.  No allocation, no synchronisation,
// no process-wide state.
#include "pfa_decode_host.h"

using namespace pfa::decode;

extern "C" {

size_t pfa_fa3_decode_q8_workspace_bytes(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant) {
    return workspace_bytes<true>(a, {ext, nullptr, quant});
}

int pfa_fa3_decode_q8_check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant) {
    return check_only<true>(a, {ext, nullptr, quant});
}

int pfa_fa3_decode_q8_describe(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant, char* buf, size_t n,
                               int32_t* nsplit) {
    return describe<true>(a, {ext, nullptr, quant}, buf, n, nsplit);
}

int pfa_fa3_decode_q8(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant, void* stream) {
    return run<pfa::MODE_KV8>(a, {ext, nullptr, quant}, stream);
}

}  // extern "C"
