// pfa_decode_sink_capi.hip -- C ABI of the split-KV decode with attention sinks (include/pfa_hip.h, pfa_fa3_decode_sink*): the rules of
// pfa_fa3_sinks, then everything pfa_fa3_decode_ex says of the same argument and extension blocks, and the launch of the SINK instantiations
// of fa3_decode_kernel, plain and windowed.  Validation is asked of the sink-less call; the split count, the workgroups, the workspace
// layout and the launches are pfa_decode_host.h's, which the three decode units share, so they cannot drift apart.  A NULL block is the
// sink-less call itself.  A file of its own: the other decode objects are built from what they were built from.  No allocation, no
// synchronisation, no process-wide state.
#include "pfa_decode_host.h"
#include "pfa_sink_host.h"

namespace {

// of arguments that pass, the plan is the sink-less call's: pfa::decode::plan(a, window)
int check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks) {
    if (sinks) {
        const int st = pfa::check_sinks(sinks);
        if (st != PFA_OK) return st;
    }
    return pfa_fa3_decode_check_ex(a, ext);
}

// the window of blocks that passed check()
int window_of(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext) {
    int window;
    (void)pfa::check_cache_ext(ext, a->causal, a->Smax, &window);
    return window;
}

}  // namespace

extern "C" {

size_t pfa_fa3_decode_sink_workspace_bytes(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks) {
    if (sinks && pfa::check_sinks(sinks, false) != PFA_OK) return 0;
    return pfa_fa3_decode_workspace_bytes_ex(a, ext);
}

int pfa_fa3_decode_sink_check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks) { return check(a, ext, sinks); }

int pfa_fa3_decode_sink_describe(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks, char* buf, size_t n,
                                 int32_t* nsplit) {
    const int st = check(a, ext, sinks);
    if (st != PFA_OK) return st;
    const int wgs = pfa_fa3_decode_describe_ex(a, ext, buf, n, nsplit);
    if (sinks && wgs >= 0) pfa::name_sink(buf, n);
    return wgs;
}

int pfa_fa3_decode_sink(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks, void* stream) {
    if (!sinks) return pfa_fa3_decode_ex(a, ext, stream);
    const int st = check(a, ext, sinks);
    if (st != PFA_OK) return st;
    const int window = window_of(a, ext);
    const pfa::decode::Plan pl = pfa::decode::plan(a, window);
    if (window) {
        pfa::dec::DecodeWinSinkParams p;
        pfa::decode::fill_params(p, a, pl);
        p.window = window; p.sinks = sinks->sinks;
        return pfa::decode::launch<true, false, false, true>(a, pl, p, stream);
    }
    pfa::dec::DecodeSinkParams p;
    pfa::decode::fill_params(p, a, pl);
    p.sinks = sinks->sinks;
    return pfa::decode::launch<false, false, false, true>(a, pl, p, stream);
}

}  // extern "C"
