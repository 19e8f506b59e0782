// pfa_prefill_varlen_capi.hip -- C ABI of the ragged forward over a KV cache (include/pfa_hip.h, pfa_fa3_prefill_varlen*): validation
// and the launch of fa3_prefill_kernel's VARLEN instantiations.  No allocation, no synchronisation, no process-wide state, no workspace.
#include "pfa_prefill_host.h"

namespace {

// -> PFA_OK and the kernel's window (0: none) in *window
int check(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, int* window) {
    *window = 0;
    const int st = pfa::check_cache_args(a, INT_MAX);          // max_seqlen_q < 1 is its Sq < 1
    if (st != PFA_OK) return st;
    if (!a->cu_seqlens_q) return PFA_ERR_NULL;
    if (!pfa::aligned4(a->cu_seqlens_q)) return PFA_ERR_ALIGN;
    if (a->total_q < 1 || a->max_seqlen_q > a->total_q) return PFA_ERR_SHAPE;
    return pfa::prefill::check_grid_and_ext(a, ext, window);
}

}  // namespace

extern "C" {

int pfa_fa3_prefill_varlen_check_ex(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext) {
    int window;
    return check(a, ext, &window);
}

int pfa_fa3_prefill_varlen_describe_ex(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, char* buf, size_t n) {
    int window;
    const int st = check(a, ext, &window);
    return st != PFA_OK ? st : pfa::prefill::describe<true>(a, window, buf, n);
}

int pfa_fa3_prefill_varlen_ex(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, void* stream) {
    int window;
    const int st = check(a, ext, &window);
    return st != PFA_OK ? st : pfa::prefill::launch_windowed<true>(a, window, stream);
}

// the calls without the extension block
int pfa_fa3_prefill_varlen_check(const pfa_fa3_prefill_varlen_args* a) { return pfa_fa3_prefill_varlen_check_ex(a, nullptr); }
int pfa_fa3_prefill_varlen_describe(const pfa_fa3_prefill_varlen_args* a, char* buf, size_t n) { return pfa_fa3_prefill_varlen_describe_ex(a, nullptr, buf, n); }
int pfa_fa3_prefill_varlen(const pfa_fa3_prefill_varlen_args* a, void* stream) { return pfa_fa3_prefill_varlen_ex(a, nullptr, stream); }

}  // extern "C"
