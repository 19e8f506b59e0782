// pfa_prefill_sink_capi.hip -- C ABI of the forward over a KV cache with attention sinks (include/pfa_hip.h, pfa_fa3_prefill_sink*): the
// entry points and fa3_prefill_kernel's uniform SINK instantiations, plain and windowed.  The rules of pfa_fa3_sinks come first, then
// everything pfa_fa3_prefill_ex says of the same blocks; the bodies are pfa_prefill_host.h's.  A NULL block is the sink-less call itself.
// A file of its own, as the FP8 units are.  No allocation, no synchronisation, no process-wide state, no workspace.
#include "pfa_prefill_host.h"

using namespace pfa::prefill;

extern "C" {

int pfa_fa3_prefill_sink_check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks) {
    return entry_check(a, ext, nullptr, sinks);
}

int pfa_fa3_prefill_sink_describe(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks, char* buf, size_t n) {
    return entry_describe(a, ext, nullptr, sinks, buf, n);
}

int pfa_fa3_prefill_sink(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks, void* stream) {
    return entry_run<pfa::MODE_SINK, pfa::MODE_WINDOW>(a, ext, nullptr, sinks, stream);
}

}  // extern "C"
