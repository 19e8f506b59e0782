// pfa_prefill_capi.hip -- C ABI of the forward over a KV cache (include/pfa_hip.h, pfa_fa3_prefill*): the entry points and the uniform
// instantiations of fa3_prefill_kernel, plain and windowed; the bodies are pfa_prefill_host.h's.
// No allocation, no synchronisation, no process-wide state, no workspace.
#include "pfa_prefill_host.h"

using namespace pfa::prefill;

extern "C" {

int pfa_fa3_prefill_check_ex(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext) { return entry_check(a, ext, nullptr, nullptr); }

int pfa_fa3_prefill_describe_ex(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, char* buf, size_t n) {
    return entry_describe(a, ext, nullptr, nullptr, buf, n);
}

int pfa_fa3_prefill_ex(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, void* stream) {
    return entry_run<0, pfa::MODE_WINDOW>(a, ext, nullptr, nullptr, stream);
}

// the calls without the extension block
int pfa_fa3_prefill_check(const pfa_fa3_decode_args* a) { return pfa_fa3_prefill_check_ex(a, nullptr); }
int pfa_fa3_prefill_describe(const pfa_fa3_decode_args* a, char* buf, size_t n) { return pfa_fa3_prefill_describe_ex(a, nullptr, buf, n); }
int pfa_fa3_prefill(const pfa_fa3_decode_args* a, void* stream) { return pfa_fa3_prefill_ex(a, nullptr, stream); }

}  // extern "C"
