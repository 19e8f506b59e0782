// pfa_prefill_capi.hip -- C ABI of the forward over a KV cache (include/pfa_hip.h, pfa_fa3_prefill*): validation and the launch.
// No allocation, no synchronisation, no process-wide state, no workspace.
#include "pfa_hip.h"

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdio.h>

#include "fa3_prefill_kernel.h"
#include "pfa_host.h"

namespace {

// workgroups: from shapes only, so a captured graph stays valid while cache_seqlens, the block table and the cache change
int64_t workgroups(const pfa_fa3_decode_args* a) {
    return (int64_t)a->B * a->H * (((int64_t)a->Sq + pfa::FWD_BLOCK_M - 1) / pfa::FWD_BLOCK_M);
}

// -> PFA_OK and the kernel's window (0: none) in *window
int check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, int* window) {
    *window = 0;
    const int st = pfa::check_cache_args(a, INT_MAX);
    if (st != PFA_OK) return st;
    if (a->key_mask) return PFA_ERR_FLAGS;           // key masks over the cache: pfa_fa3_decode only
    if (workgroups(a) > 0x7fffffffLL) return PFA_ERR_SHAPE;
    return pfa::check_cache_ext(ext, a->causal, a->Smax, window);
}

// fp32 output: P carried as a 16-bit hi + lo pair (SPLITP), as the forward does for its <= 1e-3 mode
template <typename T, int D, bool CAUSAL, bool PAGED, bool WINDOW = false>
const void* fn_out(bool out32) {
    return out32 ? (const void*)&pfa::fa3_prefill_kernel<T, D, CAUSAL, true, PAGED, float, false, WINDOW>
                 : (const void*)&pfa::fa3_prefill_kernel<T, D, CAUSAL, false, PAGED, T, false, WINDOW>;
}
// the windowed instantiations exist under the causal flag only
template <typename T, int D>
const void* fn_td(bool causal, bool paged, bool out32, bool window) {
    if (window) return paged ? fn_out<T, D, true, true, true>(out32) : fn_out<T, D, true, false, true>(out32);
    if (causal) return paged ? fn_out<T, D, true, true>(out32) : fn_out<T, D, true, false>(out32);
    return paged ? fn_out<T, D, false, true>(out32) : fn_out<T, D, false, false>(out32);
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
    if (st != PFA_OK) return st;
    if (buf && n)
        snprintf(buf, n, "fa3_prefill_%s_d%d_%s%s%s%s", a->dtype_in == PFA_DTYPE_BF16 ? "bf16" : "fp16", a->D,
                 a->dtype_out == PFA_DTYPE_FP32 ? "o32" : "o16", a->causal ? "_causal" : "", window ? "_win" : "", a->block_table ? "_paged" : "");
    return (int)workgroups(a);
}

int pfa_fa3_prefill_ex(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, void* stream) {
    int window;
    const int st = check(a, ext, &window);
    if (st != PFA_OK) return st;
    pfa::PrefillWinParams p;         // the window-less kernels take its PrefillParams base, unchanged
    p.q = a->q; p.k = a->k_cache; p.v = a->v_cache; p.o = a->o;
    p.lse = a->lse; p.seqlens = a->cache_seqlens;
    p.q_sb = a->q_stride_b; p.q_sh = a->q_stride_h; p.q_ss = a->q_stride_s;
    p.k_sb = a->k_stride_b; p.k_sh = a->k_stride_h; p.k_ss = a->k_stride_s;
    p.v_sb = a->v_stride_b; p.v_sh = a->v_stride_h; p.v_ss = a->v_stride_s;
    p.o_sb = a->o_stride_b; p.o_sh = a->o_stride_h; p.o_ss = a->o_stride_s;
    p.B = a->B; p.H = a->H; p.Sq = a->Sq; p.Smax = a->Smax;
    p.nqblk = (a->Sq + pfa::FWD_BLOCK_M - 1) / pfa::FWD_BLOCK_M;
    p.kv_group = a->H / a->Hkv;
    p.scale_log2 = a->softmax_scale * 1.4426950408889634f;
    p.block_table = a->block_table; p.bt_sb = a->block_table_stride_b; p.page_size = a->page_size; p.num_pages = a->num_pages;
    p.window = window;

    const bool bf = a->dtype_in == PFA_DTYPE_BF16, out32 = a->dtype_out == PFA_DTYPE_FP32, paged = a->block_table != nullptr;
    const bool causal = a->causal != 0;
    const bool win = window != 0;
    const void* fn = bf ? (a->D == 128 ? fn_td<__bf16, 128>(causal, paged, out32, win) : fn_td<__bf16, 64>(causal, paged, out32, win))
                        : (a->D == 128 ? fn_td<_Float16, 128>(causal, paged, out32, win) : fn_td<_Float16, 64>(causal, paged, out32, win));
    const int lds = 2 * 2 * pfa::BLOCK_N * a->D * 2;      // two buffers of a K and a V tile image (<= 64 KiB)
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    void* kargs[] = {&p};           // a kernel copies as many bytes as its parameter type has: the base, or all of it
    const hipError_t e = hipLaunchKernel(fn, dim3((unsigned)workgroups(a)), dim3(pfa::FWD_THREADS), kargs, (size_t)lds, (hipStream_t)stream);
    return pfa::hip_failed(e) ? PFA_ERR_LAUNCH : PFA_OK;
}

// the calls without the extension block
int pfa_fa3_prefill_check(const pfa_fa3_decode_args* a) { return pfa_fa3_prefill_check_ex(a, nullptr); }
int pfa_fa3_prefill_describe(const pfa_fa3_decode_args* a, char* buf, size_t n) { return pfa_fa3_prefill_describe_ex(a, nullptr, buf, n); }
int pfa_fa3_prefill(const pfa_fa3_decode_args* a, void* stream) { return pfa_fa3_prefill_ex(a, nullptr, stream); }

}  // extern "C"
