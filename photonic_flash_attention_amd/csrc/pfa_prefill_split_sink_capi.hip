// pfa_prefill_split_sink_capi.hip -- C ABI of the forward over a KV cache with the keys split over workgroups and attention sinks
// (include/pfa_hip.h, pfa_fa3_prefill_split_sink*): the rules of pfa_fa3_sinks, then everything pfa_fa3_prefill_split says of the same
// arguments, and the launch of fa3_prefill_kernel's SPLIT SINK instantiations, in which split 0 of every q block carries the sink into
// the unchanged pfa_attn_merge.  Validation, the plan and the workspace are asked of the sink-less call; layout, merge block and launch
// are pfa_prefill_split_host.h's.  A NULL block is the sink-less call itself; a count that resolves to 1 is pfa_fa3_prefill_sink.  A file
// of its own, as the FP8 units are.  No allocation, no synchronisation, no process-wide state, no atomics.
#include "pfa_prefill_split_host.h"

namespace {

int check(const pfa_fa3_decode_args* a, int32_t key_splits, const pfa_fa3_sinks* sinks) {
    if (sinks) {
        const int st = pfa::check_sinks(sinks);
        if (st != PFA_OK) return st;
    }
    return pfa_fa3_prefill_split_check(a, key_splits);
}

}  // namespace

extern "C" {

size_t pfa_fa3_prefill_split_sink_workspace_bytes(const pfa_fa3_decode_args* a, int32_t key_splits, const pfa_fa3_sinks* sinks) {
    if (sinks && pfa::check_sinks(sinks, false) != PFA_OK) return 0;
    return pfa_fa3_prefill_split_workspace_bytes(a, key_splits);
}

int pfa_fa3_prefill_split_sink_check(const pfa_fa3_decode_args* a, int32_t key_splits, const pfa_fa3_sinks* sinks) { return check(a, key_splits, sinks); }

int pfa_fa3_prefill_split_sink_describe(const pfa_fa3_decode_args* a, int32_t key_splits, const pfa_fa3_sinks* sinks, char* buf, size_t n,
                                        int32_t* nsplit) {
    const int st = check(a, key_splits, sinks);
    if (st != PFA_OK) return st;
    const int wgs = pfa_fa3_prefill_split_describe(a, key_splits, buf, n, nsplit);
    if (sinks && wgs >= 0) pfa::name_sink(buf, n);
    return wgs;
}

int pfa_fa3_prefill_split_sink(const pfa_fa3_decode_args* a, int32_t key_splits, const pfa_fa3_sinks* sinks, void* stream) {
    if (!sinks) return pfa_fa3_prefill_split(a, key_splits, stream);
    const int st = check(a, key_splits, sinks);
    if (st != PFA_OK) return st;
    const int ns = pfa_fa3_prefill_split_plan(a, key_splits);     // passed above: 1 .. 8
    if (ns == 1) return pfa_fa3_prefill_sink(a, nullptr, sinks, stream);      // the unsplit call with sinks: kernel function, grid and bits
    return pfa::prefill_split::run<true>(a, ns, sinks, stream);
}

}  // extern "C"
