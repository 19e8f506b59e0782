// pfa_rotary_capi.hip -- C ABI of the rotary embedding for the training calls (include/pfa_hip_rotary.h, pfa_rotary*): validation and
// the launch of rotary_kernel.  No allocation, no synchronisation, no process-wide state, no workspace.
// Compiled with -ffp-contract=off (csrc/Makefile), as pfa_rope_append_capi is: the kernel's products and sums round separately.
#include "pfa_hip_rotary.h"

#include <stdio.h>

#include "pfa_rows_host.h"
#include "rotary_kernel.h"

namespace {

namespace rows = pfa::rows;
using rows::in_place;

// units of a row: out of place every head's D / 16, in place only the R / 16 that change
int64_t units(const pfa_rotary_args* a) { return rows::units(a, in_place(a) ? a->rot_dim : a->D); }
int64_t workgroups(const pfa_rotary_args* a) { return rows::workgroups(a, units(a), pfa::ROTARY_THREADS); }

int check(const pfa_rotary_args* a) {
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_rotary_args)) return PFA_ERR_STRUCT_SIZE;
    if (a->flags & ~(PFA_ROTARY_INTERLEAVED | PFA_ROTARY_CONJUGATE)) return PFA_ERR_FLAGS;
    if (!rows::positions_exclusive(a) || !rows::in_place_consistent(a)) return PFA_ERR_FLAGS;
    if (!a->x0 || !a->x0_out || !a->cos || !a->sin) return PFA_ERR_NULL;
    if (!rows::null_iff(a->H1 == 0, {a->x1, a->x1_out})) return PFA_ERR_NULL;
    if (!rows::shape_ok(a, false)) return PFA_ERR_SHAPE;
    if (a->D < 16 || a->D % 16 != 0 || a->D > 256) return PFA_ERR_HEAD_DIM;
    if (!rows::rot_dim_ok(a, false)) return PFA_ERR_HEAD_DIM;
    if (a->dtype != PFA_DTYPE_BF16 && a->dtype != PFA_DTYPE_FP16) return PFA_ERR_DTYPE;
    if (!rows::fwd_strides_ok(a) || (in_place(a) && !rows::in_place_strides_equal(a)) || !rows::tables_ok(a)) return PFA_ERR_STRIDE;
    if (!rows::all_aligned16({a->x0, a->x0_out, a->x1, a->x1_out, a->cos, a->sin}) || !rows::ints_aligned(a)) return PFA_ERR_ALIGN;
    // a sequence's item index and the grid inside 32 bits
    if (!rows::items_fit(a, units(a), pfa::ROTARY_THREADS) || workgroups(a) > rows::kLim) return PFA_ERR_SHAPE;
    return PFA_OK;
}

template <typename T>
pfa::KernelFn<pfa::RotaryParams> kernel_of(bool packed, bool interleaved) {
    return pfa::dispatch_bools([](auto pk, auto il) -> pfa::KernelFn<pfa::RotaryParams> { return &pfa::rotary_kernel<T, pk.value, il.value>; },
                               packed, interleaved);
}

}  // namespace

extern "C" {

int pfa_rotary_check(const pfa_rotary_args* a) { return check(a); }

int pfa_rotary_describe(const pfa_rotary_args* a, char* buf, size_t n) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    if (buf && n)
        snprintf(buf, n, "rotary_%s%s%s%s%s", a->dtype == PFA_DTYPE_BF16 ? "bf16" : "fp16", a->cu_seqlens ? "_packed" : "",
                 (a->flags & PFA_ROTARY_INTERLEAVED) ? "_interleaved" : "", (a->flags & PFA_ROTARY_CONJUGATE) ? "_conj" : "",
                 in_place(a) ? "_inplace" : "");
    return (int)workgroups(a);
}

int pfa_rotary(const pfa_rotary_args* a, void* stream) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    const bool packed = a->cu_seqlens != nullptr;
    pfa::RotaryParams p;
    rows::fill_fwd(p, a, units(a), pfa::ROTARY_THREADS);
    p.hunits = in_place(a) ? p.runits : a->D / rows::kPiece;
    p.conjugate = (a->flags & PFA_ROTARY_CONJUGATE) ? 1 : 0;

    const bool il = (a->flags & PFA_ROTARY_INTERLEAVED) != 0;
    const auto fn = a->dtype == PFA_DTYPE_BF16 ? kernel_of<__bf16>(packed, il) : kernel_of<_Float16>(packed, il);
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    return pfa::launch(fn, dim3((unsigned)workgroups(a)), pfa::ROTARY_THREADS, p, 0, stream);
}

}  // extern "C"
