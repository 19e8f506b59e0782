// pfa_rotary_capi.hip -- C ABI of the rotary embedding for the training calls (include/pfa_hip_rotary.h, pfa_rotary*): validation and
// the launch of rotary_kernel.  No allocation, no synchronisation, no process-wide state, no workspace.
// Compiled with -ffp-contract=off (csrc/Makefile), as pfa_rope_append_capi is: the kernel's products and sums round separately.
#include "pfa_hip_rotary.h"

#include <stdio.h>

#include "pfa_host.h"
#include "rotary_kernel.h"

namespace {

constexpr int kPiece = 16;     // a work item is 16 elements of a row: a rotation's pairs lie inside it

bool in_place(const pfa_rotary_args* a) { return a->x0_out == a->x0; }
// units of a row: out of place every head's D / 16, in place only the R / 16 that change
int64_t units(const pfa_rotary_args* a) { return ((int64_t)a->H0 + a->H1) * ((in_place(a) ? a->rot_dim : a->D) / kPiece); }
int64_t items(const pfa_rotary_args* a) { return (int64_t)a->S * units(a); }      // of one sequence, at most
int64_t nchunk(const pfa_rotary_args* a) { return (items(a) + pfa::ROTARY_THREADS - 1) / pfa::ROTARY_THREADS; }
int64_t workgroups(const pfa_rotary_args* a) {     // saturated so that the product cannot wrap
    const int64_t lim = 0x7fffffffLL;
    return nchunk(a) > lim ? lim + 1 : (int64_t)a->B * nchunk(a);
}

int check(const pfa_rotary_args* a) {
    using pfa::aligned16;
    using pfa::aligned4;
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_rotary_args)) return PFA_ERR_STRUCT_SIZE;
    if (a->flags & ~(PFA_ROTARY_INTERLEAVED | PFA_ROTARY_CONJUGATE)) return PFA_ERR_FLAGS;
    if (a->position_ids && a->pos_offsets) return PFA_ERR_FLAGS;
    if (a->x1 && a->x1_out && (a->x1_out == a->x1) != in_place(a)) return PFA_ERR_FLAGS;
    if (!a->x0 || !a->x0_out || !a->cos || !a->sin) return PFA_ERR_NULL;
    if ((a->x1 == nullptr) != (a->H1 == 0) || (a->x1_out == nullptr) != (a->H1 == 0)) return PFA_ERR_NULL;
    const bool packed = a->cu_seqlens != nullptr;
    if (a->B < 1 || a->S < 1 || a->H0 < 1 || a->H1 < 0 || a->max_pos < 1) return PFA_ERR_SHAPE;
    if (packed && (a->total < 1 || a->S > a->total)) return PFA_ERR_SHAPE;
    if (a->D < 16 || a->D % 16 != 0 || a->D > 256) return PFA_ERR_HEAD_DIM;
    if (a->rot_dim < 16 || a->rot_dim % 16 != 0 || a->rot_dim > a->D) return PFA_ERR_HEAD_DIM;
    if (a->dtype != PFA_DTYPE_BF16 && a->dtype != PFA_DTYPE_FP16) return PFA_ERR_DTYPE;
    if (!pfa::multiples_of(8, {a->x0_stride_s, a->x0_stride_h, a->x0o_stride_s, a->x0o_stride_h, a->x1_stride_s, a->x1_stride_h,
                               a->x1o_stride_s, a->x1o_stride_h}))
        return PFA_ERR_STRIDE;
    if (!packed && !pfa::multiples_of(8, {a->x0_stride_b, a->x0o_stride_b, a->x1_stride_b, a->x1o_stride_b})) return PFA_ERR_STRIDE;
    if (in_place(a)) {     // the same tensor: an item reads what it writes and nothing else
        if (a->x0o_stride_s != a->x0_stride_s || a->x0o_stride_h != a->x0_stride_h || a->x1o_stride_s != a->x1_stride_s ||
            a->x1o_stride_h != a->x1_stride_h)
            return PFA_ERR_STRIDE;
        if (!packed && (a->x0o_stride_b != a->x0_stride_b || a->x1o_stride_b != a->x1_stride_b)) return PFA_ERR_STRIDE;
    }
    if (a->cs_stride % 4 != 0 || a->cs_stride < a->rot_dim / 2) return PFA_ERR_STRIDE;
    if (!aligned16(a->x0) || !aligned16(a->x0_out) || !aligned16(a->x1) || !aligned16(a->x1_out) || !aligned16(a->cos) || !aligned16(a->sin))
        return PFA_ERR_ALIGN;
    if (!aligned4(a->cu_seqlens) || !aligned4(a->pos_offsets) || !aligned4(a->position_ids)) return PFA_ERR_ALIGN;
    // a sequence's item index and the grid inside 32 bits
    if (items(a) + pfa::ROTARY_THREADS > 0x7fffffffLL || workgroups(a) > 0x7fffffffLL) return PFA_ERR_SHAPE;
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
    p.x0 = a->x0; p.x0_out = a->x0_out; p.x1 = a->x1; p.x1_out = a->x1_out;
    p.cos = a->cos; p.sin = a->sin;
    p.cu_seqlens = a->cu_seqlens; p.pos_offsets = a->pos_offsets; p.position_ids = a->position_ids;
    PFA_FILL_STRIDES(p, a, x0); PFA_FILL_STRIDES(p, a, x0o); PFA_FILL_STRIDES(p, a, x1); PFA_FILL_STRIDES(p, a, x1o);
    p.pid_sb = a->pid_stride_b; p.pid_ss = a->pid_stride_s; p.cs_stride = a->cs_stride;
    p.nchunk = (int32_t)nchunk(a);
    p.S = a->S; p.total = a->total; p.H0 = a->H0;
    p.runits = a->rot_dim / kPiece;
    p.hunits = in_place(a) ? p.runits : a->D / kPiece;
    p.units = (int32_t)units(a);
    p.max_pos = a->max_pos;
    p.conjugate = (a->flags & PFA_ROTARY_CONJUGATE) ? 1 : 0;

    const bool il = (a->flags & PFA_ROTARY_INTERLEAVED) != 0;
    const auto fn = a->dtype == PFA_DTYPE_BF16 ? kernel_of<__bf16>(packed, il) : kernel_of<_Float16>(packed, il);
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    return pfa::launch(fn, dim3((unsigned)workgroups(a)), pfa::ROTARY_THREADS, p, 0, stream);
}

}  // extern "C"
