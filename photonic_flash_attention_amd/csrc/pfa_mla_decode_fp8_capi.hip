// pfa_mla_decode_fp8_capi.hip -- C ABI of the MLA decode over an FP8 (e4m3fn) latent cache (include/pfa_hip_mla_cache.h,
// pfa_mla_decode_q8*): the rules of pfa_mla_kv_quant and of a cache of one-byte elements, then everything pfa_mla_decode says of the same
// argument block (pfa_mla_decode_host.h), and the 8 instantiations of fa3_mla_decode_kv8_kernel (bf16 / fp16 x output x paged).  Plan,
// grid, workspace and parameter fill are the 16-bit call's; the combine kernel at D = 512 is the one it launches.  Built with
// pfa_mla_decode_capi's flags (csrc/Makefile), whose bits it returns when the descales are powers of two.
// No allocation, no synchronisation, no process-wide state, a grid from host shapes only.
#include "fa3_mla_decode_fp8_kernel.h"
#include "pfa_hip_mla_cache.h"
#include "pfa_mla_cache_host.h"
#include "pfa_mla_decode_host.h"

using namespace pfa::decode;
using pfa::dec::GeoMla;
using pfa::dec::MlaKv8Params;

namespace {

pfa::KernelFn<MlaKv8Params> kernel_kv8(int dtype, bool out32, bool paged) {
    return pfa::dispatch_bools([](auto bf, auto o32, auto pg) -> pfa::KernelFn<MlaKv8Params> {
        using T = std::conditional_t<bf.value, __bf16, _Float16>;
        return &pfa::dec::fa3_mla_decode_kv8_kernel<T, pfa::out_t<o32.value, T>, pg.value>;
    }, dtype == PFA_DTYPE_BF16, out32, paged);
}

// include/pfa_hip_mla_cache.h, pfa_mla_decode_q8, in the order the errors are reported
int check(const pfa_mla_decode_args* a, const pfa_mla_kv_quant* quant, pfa_fa3_decode_args* d, Plan* pl, int64_t* grid) {
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_mla_decode_args)) return PFA_ERR_STRUCT_SIZE;
    const int st = pfa::mla::check_kv_quant(quant);
    if (st != PFA_OK) return st;
    // one-byte elements: the 8-byte loads of a tile, and rows a 16-byte store can fill
    if (!pfa::multiples_of(16, {a->kv_stride_b, a->kv_stride_s})) return PFA_ERR_STRIDE;
    if (!pfa::aligned16(a->kv_cache)) return PFA_ERR_ALIGN;
    return pfa::mla::check(a, d, pl, grid);
}

}  // namespace

extern "C" {

size_t pfa_mla_decode_q8_workspace_bytes(const pfa_mla_decode_args* a, const pfa_mla_kv_quant* quant) {
    if (pfa::mla::check_shape(a) != PFA_OK || pfa::mla::check_kv_quant(quant, false) != PFA_OK) return 0;
    const pfa_fa3_decode_args d = pfa::mla::as_decode(a);
    return plan(&d, 0).ws_bytes;
}

int pfa_mla_decode_q8_check(const pfa_mla_decode_args* a, const pfa_mla_kv_quant* quant) {
    pfa_fa3_decode_args d;
    Plan pl;
    int64_t grid;
    return check(a, quant, &d, &pl, &grid);
}

int pfa_mla_decode_q8_describe(const pfa_mla_decode_args* a, const pfa_mla_kv_quant* quant, char* buf, size_t n, int32_t* nsplit) {
    pfa_fa3_decode_args d;
    Plan pl;
    int64_t grid;
    const int st = check(a, quant, &d, &pl, &grid);
    if (st != PFA_OK) return st;
    return pfa::mla::describe(a, pl, grid, "_q8", buf, n, nsplit);
}

int pfa_mla_decode_q8(const pfa_mla_decode_args* a, const pfa_mla_kv_quant* quant, void* stream) {
    pfa_fa3_decode_args d;
    Plan pl;
    int64_t grid;
    const int st = check(a, quant, &d, &pl, &grid);
    if (st != PFA_OK) return st;
    MlaKv8Params p;
    fill_params(p, &d, pl);
    p.kv_descale = quant->kv_descale; p.ds_sb = quant->descale_stride_b;
    const bool out32 = a->dtype_out == PFA_DTYPE_FP32;
    const auto fn = kernel_kv8(a->dtype_in, out32, a->block_table != nullptr);
    const auto cfn = combine_at<GeoMla::DV>(a->dtype_in, out32);
    return launch_with_combine(fn, cfn, p, &d, pl, grid, GeoMla::LDS, stream);
}

}  // extern "C"
