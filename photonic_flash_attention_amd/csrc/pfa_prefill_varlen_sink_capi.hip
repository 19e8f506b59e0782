// pfa_prefill_varlen_sink_capi.hip -- C ABI of the ragged forward over a KV cache with attention sinks (include/pfa_hip.h,
// pfa_fa3_prefill_varlen_sink*): the entry points and fa3_prefill_kernel's VARLEN SINK instantiations, plain and windowed.  Laid out as
// pfa_prefill_sink_capi.hip.  No allocation, no synchronisation, no process-wide state, no workspace.
#include "pfa_prefill_host.h"

using namespace pfa::prefill;

extern "C" {

int pfa_fa3_prefill_varlen_sink_check(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks) {
    return entry_check(a, ext, nullptr, sinks);
}

int pfa_fa3_prefill_varlen_sink_describe(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks, char* buf,
                                         size_t n) {
    return entry_describe(a, ext, nullptr, sinks, buf, n);
}

int pfa_fa3_prefill_varlen_sink(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks, void* stream) {
    return entry_run<pfa::MODE_SINK, pfa::MODE_WINDOW>(a, ext, nullptr, sinks, stream);
}

}  // extern "C"
