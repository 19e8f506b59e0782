// pfa_decode_sink_capi.hip -- C ABI of the split-KV decode with attention sinks (include/pfa_hip.h, pfa_fa3_decode_sink*): the entry
// points and the SINK instantiations of fa3_decode_kernel, plain and windowed.  The rules of pfa_fa3_sinks come first, then everything
// pfa_fa3_decode_ex says of the same argument and extension blocks: one check, one plan and one launch in pfa_decode_host.h, which the
// three decode units share, so they cannot drift apart.  A NULL block is the sink-less call itself, whose kernels are the other unit's.
// A file of its own: the other decode objects are built from what they were built from.  No allocation, no synchronisation, no
// process-wide state.
#include "pfa_decode_host.h"

using namespace pfa::decode;

extern "C" {

size_t pfa_fa3_decode_sink_workspace_bytes(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks) {
    return workspace_bytes(a, {ext, nullptr, nullptr, sinks});
}

int pfa_fa3_decode_sink_check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks) {
    return check_only(a, {ext, nullptr, nullptr, sinks});
}

int pfa_fa3_decode_sink_describe(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks, char* buf, size_t n,
                                 int32_t* nsplit) {
    return describe(a, {ext, nullptr, nullptr, sinks}, buf, n, nsplit);
}

int pfa_fa3_decode_sink(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks, void* stream) {
    if (!sinks) return pfa_fa3_decode_ex(a, ext, stream);
    return run<pfa::MODE_SINK, pfa::MODE_WINDOW>(a, {ext, nullptr, nullptr, sinks}, stream);
}

}  // extern "C"
