// pfa_prefill_varlen_sink_capi.hip -- C ABI of the ragged forward over a KV cache with attention sinks (include/pfa_hip.h,
// pfa_fa3_prefill_varlen_sink*): the rules of pfa_fa3_sinks, then everything pfa_fa3_prefill_varlen_ex says of the same blocks, and the launch
// of fa3_prefill_kernel's VARLEN SINK instantiations, plain and windowed.  Validation and the describe are asked of the sink-less call;
// grid, fill and launch are pfa_prefill_host.h's.  A NULL block is the sink-less call itself.  A file of its own, as the FP8 units are.
// No allocation, no synchronisation, no process-wide state, no workspace.
#include "pfa_prefill_host.h"

namespace {

int check(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks) {
    if (sinks) {
        const int st = pfa::check_sinks(sinks);
        if (st != PFA_OK) return st;
    }
    return pfa_fa3_prefill_varlen_check_ex(a, ext);
}

}  // namespace

extern "C" {

int pfa_fa3_prefill_varlen_sink_check(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks) {
    return check(a, ext, sinks);
}

int pfa_fa3_prefill_varlen_sink_describe(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks, char* buf,
                                         size_t n) {
    const int st = check(a, ext, sinks);
    if (st != PFA_OK) return st;
    const int wgs = pfa_fa3_prefill_varlen_describe_ex(a, ext, buf, n);
    if (sinks && wgs >= 0) pfa::name_sink(buf, n);
    return wgs;
}

int pfa_fa3_prefill_varlen_sink(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks, void* stream) {
    if (!sinks) return pfa_fa3_prefill_varlen_ex(a, ext, stream);
    const int st = check(a, ext, sinks);
    if (st != PFA_OK) return st;
    int window;
    (void)pfa::check_cache_ext(ext, a->causal, a->Smax, &window);      // passed above: the window of the blocks
    return pfa::prefill::launch_windowed_sink<true>(a, window, sinks, stream);
}

}  // extern "C"
