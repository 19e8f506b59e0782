// pfa_decode_capi.hip -- C ABI of the split-KV decode path (include/pfa_hip.h, ABI v9): the entry points and the instantiations plain,
// WINDOW and TREE of fa3_decode_kernel; validation, the split rule, the describe, the kernel table, the parameter fill and the launches are
// pfa_decode_host.h's, which the FP8 and the sink unit share.
// One body per entry point: the *_tree calls; the *_ex calls are those with no tree, the plain calls those with no extension either.
// No allocation, no synchronisation, no process-wide state.
#include "pfa_decode_host.h"

using namespace pfa::decode;

extern "C" {

size_t pfa_fa3_decode_tree_workspace_bytes(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_tree_mask* tree) {
    return workspace_bytes(a, {ext, tree});
}

int pfa_fa3_decode_tree_check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_tree_mask* tree) {
    return check_only(a, {ext, tree});
}

int pfa_fa3_decode_tree_describe(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_tree_mask* tree, char* buf, size_t n,
                                 int32_t* nsplit) {
    return describe(a, {ext, tree}, buf, n, nsplit);
}

int pfa_fa3_decode_tree(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_tree_mask* tree, void* stream) {
    return run<0, pfa::MODE_WINDOW | pfa::MODE_TREE>(a, {ext, tree}, stream);
}

// the calls without a tree
size_t pfa_fa3_decode_workspace_bytes_ex(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext) {
    return pfa_fa3_decode_tree_workspace_bytes(a, ext, nullptr);
}
int pfa_fa3_decode_check_ex(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext) { return pfa_fa3_decode_tree_check(a, ext, nullptr); }
int pfa_fa3_decode_describe_ex(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, char* buf, size_t n, int32_t* nsplit) {
    return pfa_fa3_decode_tree_describe(a, ext, nullptr, buf, n, nsplit);
}
int pfa_fa3_decode_ex(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, void* stream) { return pfa_fa3_decode_tree(a, ext, nullptr, stream); }

// ... and without the extension block
size_t pfa_fa3_decode_workspace_bytes(const pfa_fa3_decode_args* a) { return pfa_fa3_decode_workspace_bytes_ex(a, nullptr); }
int pfa_fa3_decode_check(const pfa_fa3_decode_args* a) { return pfa_fa3_decode_check_ex(a, nullptr); }
int pfa_fa3_decode_describe(const pfa_fa3_decode_args* a, char* buf, size_t n, int32_t* nsplit) {
    return pfa_fa3_decode_describe_ex(a, nullptr, buf, n, nsplit);
}
int pfa_fa3_decode(const pfa_fa3_decode_args* a, void* stream) { return pfa_fa3_decode_ex(a, nullptr, stream); }

}  // extern "C"
