// pfa_prefill_capi.hip -- C ABI of the forward over a KV cache (include/pfa_hip.h, pfa_fa3_prefill*): validation and the launch.
// No allocation, no synchronisation, no process-wide state, no workspace.
#include "pfa_prefill_host.h"

namespace {

// -> PFA_OK and the kernel's window (0: none) in *window
int check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, int* window) {
    *window = 0;
    const int st = pfa::check_cache_args(a, INT_MAX);
    if (st != PFA_OK) return st;
    if (a->key_mask) return PFA_ERR_FLAGS;           // key masks over the cache: pfa_fa3_decode only
    return pfa::prefill::check_grid_and_ext(a, ext, window);
}

}  // namespace

extern "C" {

int pfa_fa3_prefill_check_ex(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext) {
    int window;
    return check(a, ext, &window);
}

int pfa_fa3_prefill_describe_ex(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, char* buf, size_t n) {
    int window;
    const int st = check(a, ext, &window);
    return st != PFA_OK ? st : pfa::prefill::describe<false>(a, window, buf, n);
}

int pfa_fa3_prefill_ex(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, void* stream) {
    int window;
    const int st = check(a, ext, &window);
    return st != PFA_OK ? st : pfa::prefill::launch_windowed<false>(a, window, stream);
}

// the calls without the extension block
int pfa_fa3_prefill_check(const pfa_fa3_decode_args* a) { return pfa_fa3_prefill_check_ex(a, nullptr); }
int pfa_fa3_prefill_describe(const pfa_fa3_decode_args* a, char* buf, size_t n) { return pfa_fa3_prefill_describe_ex(a, nullptr, buf, n); }
int pfa_fa3_prefill(const pfa_fa3_decode_args* a, void* stream) { return pfa_fa3_prefill_ex(a, nullptr, stream); }

}  // extern "C"
