// pfa_prefill_split_capi.hip -- C ABI of the forward over a KV cache with the keys split over workgroups (include/pfa_hip.h,
// pfa_fa3_prefill_split*): the entry points; the plan, validation, the launch of fa3_prefill_kernel's SPLIT instantiations into the caller's
// workspace and the call of pfa_attn_merge that joins the parts are pfa_prefill_split_host.h's, which the sink unit shares.  No allocation, no synchronisation, no process-wide state, no atomics.
#include "pfa_prefill_split_host.h"

using namespace pfa::prefill_split;

extern "C" {

int pfa_fa3_prefill_split_plan(const pfa_fa3_decode_args* a, int32_t key_splits) { return resolve_from_shapes(a, key_splits); }

size_t pfa_fa3_prefill_split_workspace_bytes(const pfa_fa3_decode_args* a, int32_t key_splits) {
    const int ns = resolve_from_shapes(a, key_splits);
    return ns < 0 ? 0 : workspace_bytes(a, ns);
}

int pfa_fa3_prefill_split_check(const pfa_fa3_decode_args* a, int32_t key_splits) {
    int ns;
    return check(a, key_splits, &ns);
}

int pfa_fa3_prefill_split_describe(const pfa_fa3_decode_args* a, int32_t key_splits, char* buf, size_t n, int32_t* nsplit) {
    int ns;
    const int st = check(a, key_splits, &ns);
    if (st != PFA_OK) return st;
    if (nsplit) *nsplit = ns;
    if (ns == 1) return pfa_fa3_prefill_describe(a, buf, n);
    char mode[24];
    snprintf(mode, sizeof(mode), "_split%d+merge", ns);
    return pfa::prefill::describe<false>(a, 0, buf, n, mode) * ns;
}

int pfa_fa3_prefill_split(const pfa_fa3_decode_args* a, int32_t key_splits, void* stream) {
    int ns;
    const int st = check(a, key_splits, &ns);
    if (st != PFA_OK) return st;
    if (ns == 1) return pfa_fa3_prefill(a, stream);      // the same kernel function, grid and bits
    return run<false>(a, ns, nullptr, stream);
}

}  // extern "C"
