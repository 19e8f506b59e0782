// pfa_kv_append_capi.hip -- C ABI of the device-side KV-cache append (include/pfa_hip.h, pfa_kv_append*): validation and the launch of
// kv_append_kernel.  No allocation, no synchronisation, no process-wide state, no workspace.
#include <stdio.h>

#include "pfa_append_host.h"

namespace {

constexpr int kPiece = 8;      // a work item is a 16-byte piece of a row

int64_t workgroups(const pfa_kv_append_args* a) { return pfa::append::workgroups(a, a->Hkv, kPiece); }

int check(const pfa_kv_append_args* a) {
    const int st = pfa::append::check_args(a, true);
    if (st != PFA_OK) return st;
    return pfa::append::grid_fits(a, a->Hkv, kPiece) ? PFA_OK : PFA_ERR_SHAPE;
}

}  // namespace

extern "C" {

int pfa_kv_append_check(const pfa_kv_append_args* a) { return check(a); }

int pfa_kv_append_describe(const pfa_kv_append_args* a, char* buf, size_t n) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    if (buf && n)
        snprintf(buf, n, "kv_append_%s_d%d%s%s", a->dtype == PFA_DTYPE_BF16 ? "bf16" : "fp16", a->D, a->cu_seqlens_q ? "_varlen" : "",
                 a->block_table ? "_paged" : "");
    return (int)workgroups(a);
}

int pfa_kv_append(const pfa_kv_append_args* a, void* stream) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    pfa::KvAppendParams p;
    pfa::append::fill_params(p, a, a->Hkv, kPiece);
    p.dchunks = a->D / kPiece;
    const auto fn = pfa::append::kv_kernel<false>(a->cu_seqlens_q != nullptr, a->block_table != nullptr);
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    return pfa::launch(fn, dim3((unsigned)workgroups(a)), pfa::KV_APPEND_THREADS, p, 0, stream);
}

}  // extern "C"
