// pfa_mla_decode_capi.hip -- C ABI of the MLA decode over a latent KV cache (include/pfa_hip_mla.h, ABI v9 additive): the entry points
// and the 8 instantiations of fa3_mla_decode_kernel (bf16 / fp16 x output x paged) with the 4 of the combine kernel at D = 512.  The
// argument block is this call's own; behind its check it is restated as the pfa_fa3_decode_args of one K/V head at D = 512
// (pfa_mla_decode_host.h, shared with the unit over an FP8 cache), so that the split rule, the workspace layout and the parameter fill are
// pfa_decode_host.h's, which every decode unit shares.  A file of its own: the other decode objects are built from what they were built from.
// No allocation, no synchronisation, no process-wide state, a grid from host shapes only.
#include "pfa_mla_decode_host.h"

using namespace pfa::decode;
using namespace pfa::mla;
using pfa::dec::DecodeParams;

namespace {

pfa::KernelFn<DecodeParams> kernel_mla(int dtype, bool out32, bool paged) {
    return pfa::dispatch_bools([](auto bf, auto o32, auto pg) -> pfa::KernelFn<DecodeParams> {
        using T = std::conditional_t<bf.value, __bf16, _Float16>;
        return &pfa::dec::fa3_mla_decode_kernel<T, pfa::out_t<o32.value, T>, pg.value>;
    }, dtype == PFA_DTYPE_BF16, out32, paged);
}

}  // namespace

extern "C" {

size_t pfa_mla_decode_workspace_bytes(const pfa_mla_decode_args* a) {
    if (check_shape(a) != PFA_OK) return 0;
    const pfa_fa3_decode_args d = as_decode(a);
    return plan(&d, 0).ws_bytes;
}

int pfa_mla_decode_check(const pfa_mla_decode_args* a) {
    pfa_fa3_decode_args d;
    Plan pl;
    int64_t grid;
    return pfa::mla::check(a, &d, &pl, &grid);
}

int pfa_mla_decode_describe(const pfa_mla_decode_args* a, char* buf, size_t n, int32_t* nsplit) {
    pfa_fa3_decode_args d;
    Plan pl;
    int64_t grid;
    const int st = pfa::mla::check(a, &d, &pl, &grid);
    if (st != PFA_OK) return st;
    return pfa::mla::describe(a, pl, grid, "", buf, n, nsplit);
}

int pfa_mla_decode(const pfa_mla_decode_args* a, void* stream) {
    pfa_fa3_decode_args d;
    Plan pl;
    int64_t grid;
    const int st = pfa::mla::check(a, &d, &pl, &grid);
    if (st != PFA_OK) return st;
    DecodeParams p;
    fill_params(p, &d, pl);
    const bool out32 = a->dtype_out == PFA_DTYPE_FP32;
    const auto fn = kernel_mla(a->dtype_in, out32, a->block_table != nullptr);
    const auto cfn = combine_at<GeoMla::DV>(a->dtype_in, out32);
    return launch_with_combine(fn, cfn, p, &d, pl, grid, GeoMla::LDS, stream);
}

}  // extern "C"
