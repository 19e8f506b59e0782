// pfa_prefill_varlen_capi.hip -- C ABI of the ragged forward over a KV cache (include/pfa_hip.h, pfa_fa3_prefill_varlen*): the entry
// points and fa3_prefill_kernel's VARLEN instantiations, plain and windowed; the bodies are pfa_prefill_host.h's.
// No allocation, no synchronisation, no process-wide state, no workspace.
#include "pfa_prefill_host.h"

using namespace pfa::prefill;

extern "C" {

int pfa_fa3_prefill_varlen_check_ex(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext) { return entry_check(a, ext, nullptr, nullptr); }

int pfa_fa3_prefill_varlen_describe_ex(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, char* buf, size_t n) {
    return entry_describe(a, ext, nullptr, nullptr, buf, n);
}

int pfa_fa3_prefill_varlen_ex(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, void* stream) {
    return entry_run<0, pfa::MODE_WINDOW>(a, ext, nullptr, nullptr, stream);
}

// the calls without the extension block
int pfa_fa3_prefill_varlen_check(const pfa_fa3_prefill_varlen_args* a) { return pfa_fa3_prefill_varlen_check_ex(a, nullptr); }
int pfa_fa3_prefill_varlen_describe(const pfa_fa3_prefill_varlen_args* a, char* buf, size_t n) { return pfa_fa3_prefill_varlen_describe_ex(a, nullptr, buf, n); }
int pfa_fa3_prefill_varlen(const pfa_fa3_prefill_varlen_args* a, void* stream) { return pfa_fa3_prefill_varlen_ex(a, nullptr, stream); }

}  // extern "C"
