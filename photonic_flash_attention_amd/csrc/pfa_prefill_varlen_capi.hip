// pfa_prefill_varlen_capi.hip -- C ABI of the ragged forward over a KV cache (include/pfa_hip.h, pfa_fa3_prefill_varlen*): validation
// and the launch of fa3_prefill_kernel's VARLEN instantiations.  No allocation, no synchronisation, no process-wide state, no workspace.
#include "pfa_hip.h"

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdio.h>

#include "fa3_prefill_kernel.h"
#include "pfa_host.h"

namespace {

// workgroups: from host shapes only (max_seqlen_q, never cu_seqlens_q), so a captured graph stays valid while the device data changes
int64_t workgroups(const pfa_fa3_prefill_varlen_args* a) {
    return (int64_t)a->B * a->H * (((int64_t)a->max_seqlen_q + pfa::FWD_BLOCK_M - 1) / pfa::FWD_BLOCK_M);
}

// The fields the ragged call has in common with pfa_fa3_decode_args, in that form, so that check_cache_args states their rules once:
// the packed tensors have no batch stride (0 passes every stride rule) and max_seqlen_q stands where Sq does.
pfa_fa3_decode_args as_cache_args(const pfa_fa3_prefill_varlen_args* a) {
    pfa_fa3_decode_args c = {};
    c.size = sizeof(c); c.flags = a->flags; c.reserved0 = a->reserved0;
    c.q = a->q; c.k_cache = a->k_cache; c.v_cache = a->v_cache; c.o = a->o; c.lse = a->lse; c.cache_seqlens = a->cache_seqlens;
    c.q_stride_h = a->q_stride_h; c.q_stride_s = a->q_stride_s; c.o_stride_h = a->o_stride_h; c.o_stride_s = a->o_stride_s;
    c.k_stride_b = a->k_stride_b; c.k_stride_h = a->k_stride_h; c.k_stride_s = a->k_stride_s;
    c.v_stride_b = a->v_stride_b; c.v_stride_h = a->v_stride_h; c.v_stride_s = a->v_stride_s;
    c.B = a->B; c.H = a->H; c.Hkv = a->Hkv; c.Sq = a->max_seqlen_q; c.Smax = a->Smax; c.D = a->D;
    c.dtype_in = a->dtype_in; c.dtype_out = a->dtype_out; c.causal = a->causal; c.softmax_scale = a->softmax_scale;
    c.device_id = a->device_id;
    c.block_table = a->block_table; c.block_table_stride_b = a->block_table_stride_b; c.page_size = a->page_size; c.num_pages = a->num_pages;
    return c;
}

// -> PFA_OK and the kernel's window (0: none) in *window
int check(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, int* window) {
    *window = 0;
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_fa3_prefill_varlen_args)) return PFA_ERR_STRUCT_SIZE;
    const pfa_fa3_decode_args c = as_cache_args(a);
    const int st = pfa::check_cache_args(&c, INT_MAX);         // max_seqlen_q < 1 is its Sq < 1
    if (st != PFA_OK) return st;
    if (!a->cu_seqlens_q) return PFA_ERR_NULL;
    if (reinterpret_cast<uintptr_t>(a->cu_seqlens_q) & 3u) return PFA_ERR_ALIGN;
    if (a->total_q < 1 || a->max_seqlen_q > a->total_q) return PFA_ERR_SHAPE;
    if (workgroups(a) > 0x7fffffffLL) return PFA_ERR_SHAPE;
    return pfa::check_cache_ext(ext, a->causal, a->Smax, window);
}

// fp32 output: P carried as a 16-bit hi + lo pair (SPLITP), as pfa_fa3_prefill does
template <typename T, int D, bool CAUSAL, bool PAGED, bool WINDOW = false>
const void* fn_out(bool out32) {
    return out32 ? (const void*)&pfa::fa3_prefill_kernel<T, D, CAUSAL, true, PAGED, float, true, WINDOW>
                 : (const void*)&pfa::fa3_prefill_kernel<T, D, CAUSAL, false, PAGED, T, true, WINDOW>;
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

int pfa_fa3_prefill_varlen_check_ex(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext) {
    int window;
    return check(a, ext, &window);
}

int pfa_fa3_prefill_varlen_describe_ex(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, char* buf, size_t n) {
    int window;
    const int st = check(a, ext, &window);
    if (st != PFA_OK) return st;
    if (buf && n)
        snprintf(buf, n, "fa3_prefill_%s_d%d_%s%s%s_varlen%s", a->dtype_in == PFA_DTYPE_BF16 ? "bf16" : "fp16", a->D,
                 a->dtype_out == PFA_DTYPE_FP32 ? "o32" : "o16", a->causal ? "_causal" : "", window ? "_win" : "", a->block_table ? "_paged" : "");
    return (int)workgroups(a);
}

int pfa_fa3_prefill_varlen_ex(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, void* stream) {
    int window;
    const int st = check(a, ext, &window);
    if (st != PFA_OK) return st;
    pfa::PrefillVarlenWinParams p;   // the window-less kernels take its PrefillVarlenParams base, unchanged
    p.q = a->q; p.k = a->k_cache; p.v = a->v_cache; p.o = a->o;
    p.lse = a->lse; p.seqlens = a->cache_seqlens;
    p.q_sb = 0; p.q_sh = a->q_stride_h; p.q_ss = a->q_stride_s;
    p.k_sb = a->k_stride_b; p.k_sh = a->k_stride_h; p.k_ss = a->k_stride_s;
    p.v_sb = a->v_stride_b; p.v_sh = a->v_stride_h; p.v_ss = a->v_stride_s;
    p.o_sb = 0; p.o_sh = a->o_stride_h; p.o_ss = a->o_stride_s;
    p.B = a->B; p.H = a->H; p.Sq = a->max_seqlen_q; p.Smax = a->Smax;
    p.nqblk = (a->max_seqlen_q + pfa::FWD_BLOCK_M - 1) / pfa::FWD_BLOCK_M;
    p.kv_group = a->H / a->Hkv;
    p.scale_log2 = a->softmax_scale * 1.4426950408889634f;
    p.block_table = a->block_table; p.bt_sb = a->block_table_stride_b; p.page_size = a->page_size; p.num_pages = a->num_pages;
    p.cu_seqlens_q = a->cu_seqlens_q; p.total_q = a->total_q;
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
int pfa_fa3_prefill_varlen_check(const pfa_fa3_prefill_varlen_args* a) { return pfa_fa3_prefill_varlen_check_ex(a, nullptr); }
int pfa_fa3_prefill_varlen_describe(const pfa_fa3_prefill_varlen_args* a, char* buf, size_t n) { return pfa_fa3_prefill_varlen_describe_ex(a, nullptr, buf, n); }
int pfa_fa3_prefill_varlen(const pfa_fa3_prefill_varlen_args* a, void* stream) { return pfa_fa3_prefill_varlen_ex(a, nullptr, stream); }

}  // extern "C"
