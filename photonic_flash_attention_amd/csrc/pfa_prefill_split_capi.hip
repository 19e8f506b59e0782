// pfa_prefill_split_capi.hip -- C ABI of the forward over a KV cache with the keys split over workgroups (include/pfa_hip.h,
// pfa_fa3_prefill_split*): the entry points and fa3_prefill_kernel's SPLIT instantiations; the plan, validation, the launch into the caller's
// workspace and the call of pfa_attn_merge that joins the parts are pfa_prefill_split_host.h's, which the sink unit shares.  No allocation, no synchronisation, no process-wide state, no atomics.
#include "pfa_prefill_split_host.h"

using namespace pfa::prefill_split;

extern "C" {

int pfa_fa3_prefill_split_plan(const pfa_fa3_decode_args* a, int32_t key_splits) { return resolve_from_shapes(a, key_splits); }

size_t pfa_fa3_prefill_split_workspace_bytes(const pfa_fa3_decode_args* a, int32_t key_splits) { return entry_workspace_bytes(a, key_splits, nullptr); }

int pfa_fa3_prefill_split_check(const pfa_fa3_decode_args* a, int32_t key_splits) { return entry_check(a, key_splits, nullptr); }

int pfa_fa3_prefill_split_describe(const pfa_fa3_decode_args* a, int32_t key_splits, char* buf, size_t n, int32_t* nsplit) {
    return entry_describe(a, key_splits, nullptr, buf, n, nsplit);
}

int pfa_fa3_prefill_split(const pfa_fa3_decode_args* a, int32_t key_splits, void* stream) {
    return entry_run<pfa::MODE_SPLIT>(a, key_splits, nullptr, stream);
}

}  // extern "C"
