// pfa_prefill_split_sink_capi.hip -- C ABI of the forward over a KV cache with the keys split over workgroups and attention sinks
// (include/pfa_hip.h, pfa_fa3_prefill_split_sink*): the entry points and fa3_prefill_kernel's SPLIT SINK instantiations, in which split 0
// of every q block carries the sink into the unchanged pfa_attn_merge.  The rules of pfa_fa3_sinks come first, then everything
// pfa_fa3_prefill_split says of the same arguments; the bodies are pfa_prefill_split_host.h's.  A NULL block is the sink-less call itself;
// a count that resolves to 1 is pfa_fa3_prefill_sink.  A file of its own, as the FP8 units are.  No allocation, no synchronisation, no
// process-wide state, no atomics.
#include "pfa_prefill_split_host.h"

using namespace pfa::prefill_split;

extern "C" {

size_t pfa_fa3_prefill_split_sink_workspace_bytes(const pfa_fa3_decode_args* a, int32_t key_splits, const pfa_fa3_sinks* sinks) {
    return entry_workspace_bytes(a, key_splits, sinks);
}

int pfa_fa3_prefill_split_sink_check(const pfa_fa3_decode_args* a, int32_t key_splits, const pfa_fa3_sinks* sinks) { return entry_check(a, key_splits, sinks); }

int pfa_fa3_prefill_split_sink_describe(const pfa_fa3_decode_args* a, int32_t key_splits, const pfa_fa3_sinks* sinks, char* buf, size_t n,
                                        int32_t* nsplit) {
    return entry_describe(a, key_splits, sinks, buf, n, nsplit);
}

int pfa_fa3_prefill_split_sink(const pfa_fa3_decode_args* a, int32_t key_splits, const pfa_fa3_sinks* sinks, void* stream) {
    return entry_run<pfa::MODE_SPLIT | pfa::MODE_SINK>(a, key_splits, sinks, stream);
}

}  // extern "C"
