// pfa_kv_append_fp8_capi.hip -- C ABI of the quantising KV-cache append (include/pfa_hip.h, pfa_kv_append_q8*): the rules of
// pfa_fa3_kv_quant, then everything pfa_kv_append says of the same argument block, and the launch of the QUANT instantiations of
// kv_append_kernel.  Built with -ffp-contract=off (csrc/Makefile), as the rotary object is: the plain-torch model is bit-equal.
// No allocation, no synchronisation, no process-wide state, no workspace.
#include "pfa_append_host.h"
#include "pfa_fp8_host.h"

namespace {

constexpr int kPiece = 16;     // a work item is 16 elements: a 16-byte piece of the cache row; the grid from host shapes only, as pfa_kv_append's

int check(const pfa_kv_append_args* a, const pfa_fa3_kv_quant* quant) {
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_kv_append_args)) return PFA_ERR_STRUCT_SIZE;
    const int st = pfa::check_kv_quant(quant, a);
    if (st != PFA_OK) return st;
    if (a->D % 16 != 0) return PFA_ERR_HEAD_DIM;
    return pfa_kv_append_check(a);       // its grid has twice the items of this one
}

}  // namespace

extern "C" {

int pfa_kv_append_q8_check(const pfa_kv_append_args* a, const pfa_fa3_kv_quant* quant) { return check(a, quant); }

int pfa_kv_append_q8(const pfa_kv_append_args* a, const pfa_fa3_kv_quant* quant, void* stream) {
    const int st = check(a, quant);
    if (st != PFA_OK) return st;
    pfa::KvAppendQ8Params p;
    pfa::append::fill_params(p, a, a->Hkv, kPiece);
    p.dchunks = a->D / kPiece;
    p.k_descale = quant->k_descale; p.v_descale = quant->v_descale; p.ds_sb = quant->descale_stride_b;
    const bool varlen = a->cu_seqlens_q != nullptr, paged = a->block_table != nullptr;
    const auto fn = a->dtype == PFA_DTYPE_BF16 ? pfa::append::kv_kernel<true, __bf16>(varlen, paged) : pfa::append::kv_kernel<true, _Float16>(varlen, paged);
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    return pfa::launch(fn, dim3((unsigned)pfa::append::workgroups(a, a->Hkv, kPiece)), pfa::KV_APPEND_THREADS, p, 0, stream);
}

}  // extern "C"
