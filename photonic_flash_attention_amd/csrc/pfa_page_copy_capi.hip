// pfa_page_copy_capi.hip -- C ABI of the page copy inside a paged KV cache's pools (include/pfa_hip.h, pfa_page_copy*): validation and
// the launch of page_copy_kernel.  No allocation, no synchronisation, no process-wide state, no workspace.
#include "pfa_hip.h"

#include <hip/hip_runtime.h>
#include <stdio.h>

#include "page_copy_kernel.h"
#include "pfa_host.h"

namespace {

// 16-byte work items of one page: page_size tokens of Hkv heads of D / 8 pieces
int64_t items(const pfa_page_copy_args* a) { return (int64_t)a->page_size * a->Hkv * (a->D / 8); }

// workgroups: from host shapes only (page_size, never rows), so a captured graph stays valid while the device data changes
int64_t workgroups(const pfa_page_copy_args* a) {
    return (int64_t)a->n_pairs * ((items(a) + pfa::PAGE_COPY_WG_ITEMS - 1) / pfa::PAGE_COPY_WG_ITEMS);
}

int check(const pfa_page_copy_args* a) {
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_page_copy_args)) return PFA_ERR_STRUCT_SIZE;
    if (a->flags != 0 || a->reserved0 != 0) return PFA_ERR_FLAGS;
    if (!a->k_pool || !a->v_pool || !a->pairs) return PFA_ERR_NULL;
    if (a->n_pairs < 1 || a->Hkv < 1 || a->num_pages < 1 || a->page_size <= 0 || a->page_size % 64 != 0) return PFA_ERR_SHAPE;
    if (a->D < 8 || a->D % 8 != 0 || a->D > 256) return PFA_ERR_HEAD_DIM;
    if (a->dtype != PFA_DTYPE_BF16 && a->dtype != PFA_DTYPE_FP16) return PFA_ERR_DTYPE;
    if (!pfa::multiples_of(8, {a->k_stride_b, a->k_stride_h, a->k_stride_s, a->v_stride_b, a->v_stride_h, a->v_stride_s})) return PFA_ERR_STRIDE;
    if (!pfa::kv_rows_forward(a) || a->pairs_stride < 2) return PFA_ERR_STRIDE;
    if (!pfa::aligned16(a->k_pool) || !pfa::aligned16(a->v_pool) || !pfa::aligned4(a->pairs) || !pfa::aligned4(a->rows)) return PFA_ERR_ALIGN;
    // the grid, and a page's item index inside 32 bits (page_size * Hkv first: the three-way product of any int32 values can leave 64)
    if ((int64_t)a->page_size * a->Hkv > 0x7fffffffLL || items(a) + pfa::PAGE_COPY_WG_ITEMS > 0x7fffffffLL || workgroups(a) > 0x7fffffffLL)
        return PFA_ERR_SHAPE;
    return PFA_OK;
}

}  // namespace

extern "C" {

int pfa_page_copy_check(const pfa_page_copy_args* a) { return check(a); }

int pfa_page_copy_describe(const pfa_page_copy_args* a, char* buf, size_t n) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    if (buf && n) snprintf(buf, n, "page_copy_%s_d%d%s", a->dtype == PFA_DTYPE_BF16 ? "bf16" : "fp16", a->D, a->rows ? "_rows" : "");
    return (int)workgroups(a);
}

int pfa_page_copy(const pfa_page_copy_args* a, void* stream) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    pfa::PageCopyParams p;
    p.k_pool = a->k_pool; p.v_pool = a->v_pool; p.pairs = a->pairs; p.rows = a->rows; p.pairs_stride = a->pairs_stride;
    PFA_FILL_STRIDES(p, a, k); PFA_FILL_STRIDES(p, a, v);
    p.nchunk = (int32_t)(workgroups(a) / a->n_pairs);
    p.dchunks = a->D / 8; p.units = a->Hkv * (a->D / 8);
    p.page_size = a->page_size; p.num_pages = a->num_pages;

    const pfa::KernelFn<pfa::PageCopyParams> fn = a->rows ? &pfa::page_copy_kernel<true> : &pfa::page_copy_kernel<false>;
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    return pfa::launch(fn, dim3((unsigned)workgroups(a)), pfa::PAGE_COPY_THREADS, p, 0, stream);
}

}  // extern "C"
