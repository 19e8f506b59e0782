// pfa_capi.hip -- the C ABI of libpfa_hip.so (see include/pfa_hip.h for the contract and the
// reference lines each entry point replaces).  Host side only validates, picks a kernel variant
// and enqueues it; no allocation, no synchronisation; the only process-wide state is pfa_p4.hip's per-device module handle.
#include "pfa_hip.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "fa3_fwd_kernel.h"
#include "fa3_weights_kernel.h"
#include "fa3_fwd_f32_kernel.h"
#include "pfa_host.h"
#include "pfa_mask_host.h"
#include "pfa_p4.h"

namespace pfa { KernelFn<FwdParams> w4_kernel(int dtype, bool causal, bool out32); }   // pfa_w4.hip

namespace {

thread_local int g_last_hip_error = 0;

struct Variant {
    pfa::KernelFn<pfa::FwdParams> fn;
    char name[96];
    int lds_bytes;
    bool grid3 = false;    // 4-wave kernel: (head-in-XCD-group, Q block, group) arrive as blockIdx.x/y/z -- no divisions in its prologue
    int nthreads;
    int block_m;
    int xcd_group = 0;
    bool p4 = false;       // the persistent assembly kernel (pfa_p4.hip): launched through its own module, fn unused
    int p4_grid = 0;
};

// The 8-wave kernel's names end in _v8269: the schedule-flag word of the round-1 build, kept because tools and logs match on the names.
constexpr int kFwdNameTag = 8269;

const char* elem_name(const pfa_fa3_args* a) { return a->dtype_in == PFA_DTYPE_BF16 ? "bf16" : "fp16"; }

// The 8-wave kernel for every (dtype, D, causal, split, kmask, out).
Variant w8_variant(const pfa_fa3_args* a, bool causal, bool split, bool kmask, bool out32) {
    Variant v;
    v.fn = pfa::dispatch_elem_dim(a->dtype_in, a->D, [&](auto t) {
        using T = typename decltype(t)::type;
        return pfa::dispatch_bools([](auto c, auto s, auto k, auto o32) -> pfa::KernelFn<pfa::FwdParams> {
            return &pfa::fa3_fwd_kernel<T, decltype(t)::D, c.value, s.value, k.value, pfa::out_t<o32.value, T>>;
        }, causal, split, kmask, out32);
    });
    snprintf(v.name, sizeof(v.name), "fa3_fwd_%s_d%d_%s%s%s_%s_v%d", elem_name(a), a->D, causal ? "causal" : "full", split ? "_splitp" : "",
             kmask ? "_kmask" : "", out32 ? "o32" : "o16", kFwdNameTag);
    v.lds_bytes = 2 * 2 * pfa::BLOCK_N * a->D * 2;      // two buffers of a K and a V tile image
    v.nthreads = pfa::FWD_THREADS;
    v.block_m = pfa::FWD_BLOCK_M;
    return v;
}

// persistent 4 waves x 64 rows in assembly (gen_fa3_fwd_p4.py / pfa_p4.hip)
Variant p4_variant(const pfa_fa3_args* a, bool causal) {
    Variant v;
    v.fn = nullptr;
    snprintf(v.name, sizeof(v.name), "fa3_fwd_p4_%s_d%d_%s%s_%s", elem_name(a), a->D, causal ? "causal" : "full",
             pfa::p4_flavour(a) == 1 ? "_km" : (pfa::p4_flavour(a) == 2 ? "_kl" : ""), a->dtype_out == PFA_DTYPE_FP32 ? "splitp_o32" : "o16");
    v.p4 = true;
    v.p4_grid = pfa::p4_workgroups(a);
    v.lds_bytes = 0;
    v.nthreads = 256;
    v.block_m = 256;
    return v;
}

// 4 waves x 64 rows (fa3_fwd_w4_kernel.h): D = 128, single P, no element mask
Variant w4_variant(const pfa_fa3_args* a, bool causal, bool out32) {
    Variant v;
    v.fn = pfa::w4_kernel(a->dtype_in, causal, out32);
    snprintf(v.name, sizeof(v.name), "fa3_fwd_w4_%s_d128_%s_%s", elem_name(a), causal ? "causal" : "full", out32 ? "o32" : "o16");
    v.grid3 = true;
    v.lds_bytes = 8 * pfa::BLOCK_N * 128 * 2;      // K ring 2 + V ring 2 tiles, then the Q block's 64-KiB landing zone
    v.nthreads = 256;
    v.block_m = 256;
    // block order: an XCD walks its heads in groups of 4 (2 if 4 does not divide them): fewer heads' K/V live in its 4-MiB L2
    // at a time -- FETCH_SIZE -30 % at C3, S = 2048 x 256 heads +5 %, C3 +1 %, C4 / C5 unchanged (variant 49: the old order)
    const int hpx = (a->B * a->H) % 8 == 0 ? (a->B * a->H) / 8 : 0;
    v.xcd_group = (hpx > 0 && hpx % 4 == 0) ? 4 : ((hpx > 0 && hpx % 2 == 0) ? 2 : 0);
    return v;
}

Variant pick(const pfa_fa3_args* a) {
    const bool causal = a->causal != 0, split = (a->flags & PFA_FLAG_SPLIT_P) != 0;
    const bool kmask = a->key_mask != nullptr || a->mask != nullptr;
    const bool out32 = a->dtype_out == PFA_DTYPE_FP32;
    const unsigned var = (a->flags >> 8) & 0xffu;   // 0 = production default
    // The 4-wave x 64-row kernel (D = 128, single P, no element mask) wins once a workgroup streams enough key tiles to
    // amortise its fill and drain (one workgroup per CU: nothing overlaps them): from ~16 tiles per workgroup on
    // (tools/ab_bench.py, one box, against the 8-wave kernel: S1K +2.6 %, S2Kc +0.5 %, C3 +4 %, C4 / C5 / S8Kc +5 %, S2K +8 %;
    // below: S512 +1 %, S1Kc -6 %, S512c -6 %, S256 -5 %).  Variant 43 forces it, 44 forces the 8-wave kernel (A/B).
    const bool w4_ok = a->D == 128 && !split && !kmask && (int64_t)a->B * a->H * a->H < (1ll << 32);   // last: its multiply-high head index
    const int64_t avg_tiles = (causal ? (int64_t)a->Sk / 2 : (int64_t)a->Sk) / pfa::BLOCK_N;
    // Production selectors (A/B and tests): 43 = the 4-wave HIP kernel, 44 = the 8-wave kernel, 45 = the persistent assembly kernel.
    // The persistent kernel takes every aligned problem (pfa::p4_eligible): without a cold fill per Q block it also wins on short
    // sequences (same box, against the better HIP kernel: S256 +26 %, S512 +22 %, S512 causal +18 %, S1024 +12 %, S1024 causal
    // +24 %, S2048 causal +12 %: profiles/r02_p4_experiments.txt); the 4-wave HIP kernel keeps the other long problems.
    if (pfa::p4_eligible(a) && (var == 45 || var == 0)) {
        Variant v = p4_variant(a, causal);
        // D = 64 too since round 3: with the fast loop (no row max) and the mid-phase barrier the persistent kernel beats the 8-wave HIP kernel
        // on every D = 64 shape tried, also with several units per CU (same box, selector 44 -> 45: C2 527 -> 615 TFLOP/s, B16 H16 S2048 922 ->
        // 1000, B4 H12 S2048 causal 599 -> 681, B4 H16 S4096 causal 904 -> 925: profiles/r03_p4_experiments.txt).
        if (v.p4_grid > 0) return v;   // (0: the code object did not load on this device -- fall through to the HIP kernels)
    }
    if (w4_ok && (var == 43 || ((var == 0 || var == 45) && avg_tiles >= 16))) return w4_variant(a, causal, out32);
    return w8_variant(a, causal, split, kmask, out32);
}

int check(const pfa_fa3_args* a) {
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_fa3_args)) return PFA_ERR_STRUCT_SIZE;
    if (a->flags & ~(PFA_FLAG_SPLIT_P | PFA_FLAG_NO_XCD_MAP | PFA_FLAG_VARIANT_MASK)) return PFA_ERR_FLAGS;
    {   // the library knows three kernel selectors (43 / 44 / 45, see pick())
        const unsigned var = (a->flags & PFA_FLAG_VARIANT_MASK) >> 8;
        if (var != 0 && var != 43 && var != 44 && var != 45) return PFA_ERR_FLAGS;
    }
    if (!a->q || !a->k || !a->v || !a->o) return PFA_ERR_NULL;
    if (a->key_mask && a->mask) return PFA_ERR_FLAGS;
    if (a->kv_group < 0 || a->reserve_cus < 0 || a->reserved1 != 0 || (a->kv_group > 1 && a->H % a->kv_group != 0)) return PFA_ERR_SHAPE;
    if (a->drop_mask && (a->dtype_in != PFA_DTYPE_FP32 || !(a->drop_scale >= 1.f) || !isfinite(a->drop_scale))) return PFA_ERR_FLAGS;
    if (a->B <= 0 || a->H <= 0 || a->Sq <= 0 || a->Sk <= 0) return PFA_ERR_SHAPE;
    if (a->D != 64 && a->D != 128) return PFA_ERR_HEAD_DIM;
    if (a->dtype_in != PFA_DTYPE_BF16 && a->dtype_in != PFA_DTYPE_FP16 && a->dtype_in != PFA_DTYPE_FP32) return PFA_ERR_DTYPE;
    if (a->dtype_out != a->dtype_in && a->dtype_out != PFA_DTYPE_FP32) return PFA_ERR_DTYPE;
    using pfa::aligned16; using pfa::aligned4; using pfa::slab_fits32;
    const int32_t Sq = a->Sq, Sk = a->Sk, D = a->D;
    if (a->dtype_in == PFA_DTYPE_FP32) {       // the exact fp32 kernel (fa3_fwd_f32_kernel.h): 16-byte rows, no kernel selector, no split P
        if (a->flags & (PFA_FLAG_SPLIT_P | PFA_FLAG_VARIANT_MASK)) return PFA_ERR_FLAGS;
        if (!pfa::qkv_strides_multiples_of(4, a)) return PFA_ERR_STRIDE;
        if (!aligned16(a->q) || !aligned16(a->k) || !aligned16(a->v) || !aligned4(a->o)) return PFA_ERR_ALIGN;
        if (!pfa::scale_ok(a->softmax_scale)) return PFA_ERR_SHAPE;
        if ((int64_t)((Sq + 63) / 64) * a->B * a->H > 0x7fffffffLL) return PFA_ERR_SHAPE;
        if (!aligned4(a->lse)) return PFA_ERR_ALIGN;
        // rows at least D apart, 32-bit slabs
        if (a->q_stride_s < D || a->k_stride_s < D || a->v_stride_s < D || a->o_stride_s < D) return PFA_ERR_STRIDE;
        if (!slab_fits32(Sq, a->q_stride_s, D, 4) || !slab_fits32(Sk, a->k_stride_s, D, 4) || !slab_fits32(Sk, a->v_stride_s, D, 4) ||
            !slab_fits32(Sq, a->o_stride_s, D, 4))
            return PFA_ERR_SHAPE;
        return PFA_OK;
    }
    if (!pfa::scale_ok(a->softmax_scale)) return PFA_ERR_SHAPE;
    if (!pfa::qkv_strides_multiples_of(8, a) || !pfa::multiples_of(4, {a->o_stride_b, a->o_stride_h, a->o_stride_s})) return PFA_ERR_STRIDE;
    if (!aligned16(a->q) || !aligned16(a->k) || !aligned16(a->v) || !aligned16(a->o) || !aligned4(a->lse)) return PFA_ERR_ALIGN;
    if ((int64_t)((Sq + 127) / 128) * a->B * a->H > 0x7fffffffLL) return PFA_ERR_SHAPE;
    // K/V slabs of one (batch, head) are addressed through 32-bit buffer descriptors; Q too, by the 4-wave kernel's DMA
    if (!slab_fits32(Sk, a->k_stride_s, D, 2) || !slab_fits32(Sk, a->v_stride_s, D, 2) || !slab_fits32(Sq, a->q_stride_s, D, 2)) return PFA_ERR_SHAPE;
    if (!pfa::kv_rows_forward(a) || a->k_stride_s * 64 > 0x3fffffffLL || a->v_stride_s * 64 > 0x3fffffffLL) return PFA_ERR_STRIDE;
    return PFA_OK;
}

// Masks are condensed into one 64-bit word per mask row and 64-key tile before the forward and the weights pass (pfa_mask_host.h)
using pfa::take_mask_words;
pfa::MaskWords mask_words(const pfa_fa3_args* a) { return pfa::fwd_mask_words(a); }
// (named here, in front of the fp32 launch: the compiler emits template kernels in the order the host code first names them)
bool enqueue_mask_words(const pfa::MaskWords& mb, const pfa_fa3_args* a, void* stream) { return pfa::launch_row_words(mb, a->workspace, stream); }

using pfa::fill_common;

int launch_f32(const pfa_fa3_args* a, void* stream) {
    pfa::F32Params p;
    p.q = (const float*)a->q; p.k = (const float*)a->k; p.v = (const float*)a->v; p.o = (float*)a->o;
    p.lse = a->lse;
    fill_common(p, a);
    pfa::fill_qkvo_strides(p, a);
    p.causal = a->causal != 0;
    p.scale = a->softmax_scale;
    p.drop_mask = a->drop_mask;
    p.drop_scale = a->drop_scale;
    const auto fn = pfa::dispatch_dim(a->D, [](auto d) -> pfa::KernelFn<pfa::F32Params> { return &pfa::fa3_fwd_f32_kernel<d.value>; });
    const int lds = pfa::dispatch_dim(a->D, [](auto d) { return pfa::f32_lds_bytes<d.value>(); });
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    return pfa::launch(fn, dim3((unsigned)(((a->Sq + pfa::F32_BM - 1) / pfa::F32_BM) * a->B * a->H)), 256, p, (size_t)lds, stream);
}

}  // namespace

namespace pfa { void set_last_hip_error(int e) { g_last_hip_error = e; } }   // for the other translation units' entry points

extern "C" {

int pfa_abi_version(void) { return PFA_ABI_VERSION; }

const char* pfa_status_string(int status) {
    switch (status) {
        case PFA_OK: return "ok";
        case PFA_ERR_NULL: return "required pointer is NULL";
        case PFA_ERR_STRUCT_SIZE: return "pfa_fa3_args.size does not match this library's struct";
        case PFA_ERR_SHAPE: return "invalid shape or softmax_scale (B,H,Sq,Sk must be > 0, scale finite > 0)";
        case PFA_ERR_HEAD_DIM: return "head dim must be 64 or 128";
        case PFA_ERR_DTYPE: return "dtype_in must be bf16/fp16 and dtype_out the same or fp32";
        case PFA_ERR_STRIDE: return "q/k/v strides must be multiples of 8 elements (o: 4)";
        case PFA_ERR_ALIGN: return "q/k/v/o base pointers must be 16-byte aligned";
        case PFA_ERR_DEVICE: return "device is not a supported gfx950 part";
        case PFA_ERR_LAUNCH: return "HIP kernel launch failed";
        case PFA_ERR_FLAGS: return "unknown flag bits, both key_mask and mask set, or drop_mask without fp32 operands";
        default: return "unknown pfa_status";
    }
}

int pfa_last_hip_error(void) { return g_last_hip_error; }

int pfa_device_supported(int device_id) {
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device_id);
    if (pfa::hip_failed(e)) return PFA_ERR_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return 0;
    int herr = 0;                   // load the assembly kernels' code object now: no later call (or graph capture) has to
    if (pfa::p4_prepare(device_id, &herr) != PFA_OK) g_last_hip_error = herr;     // (the HIP kernels still serve the device)
    return 1;
}

int pfa_fa3_prepare(int device_id) {
    int herr = 0;
    const int st = pfa::p4_prepare(device_id, &herr);
    if (st != PFA_OK) g_last_hip_error = herr;
    return st;
}

size_t pfa_fa3_workspace_bytes(const pfa_fa3_args* a) { return (a && a->dtype_in != PFA_DTYPE_FP32) ? mask_words(a).bytes() : 0; }

int pfa_fa3_check(const pfa_fa3_args* a) { return check(a); }

int pfa_fa3_describe(const pfa_fa3_args* a, char* buf, size_t n) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    if (a->dtype_in == PFA_DTYPE_FP32) {
        if (buf && n) snprintf(buf, n, "fa3_fwd_f32_mfma_d%d_exact", a->D);
        return ((a->Sq + pfa::F32_BM - 1) / pfa::F32_BM) * a->B * a->H;
    }
    const Variant v = pick(a);
    if (buf && n) {
        strncpy(buf, v.name, n - 1);
        buf[n - 1] = 0;
    }
    if (v.p4) return v.p4_grid;
    const int nq = (a->Sq + v.block_m - 1) / v.block_m;
    return nq * a->B * a->H;
}

int pfa_fa3_fwd(const pfa_fa3_args* a, void* stream) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    if (a->dtype_in == PFA_DTYPE_FP32) return launch_f32(a, stream);

    pfa::FwdParams p;
    p.q = a->q; p.k = a->k; p.v = a->v; p.o = a->o;
    p.lse = a->lse;
    fill_common(p, a);
    pfa::fill_qkvo_strides(p, a);
    p.dbg = (unsigned long long*)a->workspace;   // written by diagnostic builds of the 4-wave kernel only (PFA_W4_STAMP)
    const pfa::MaskWords mb = mask_words(a);
    const bool use_mbits = take_mask_words(p, mb, a);
    if (use_mbits) {
        p.mrange = (const int*)((const char*)a->workspace + mb.word_bytes());
        p.mr_sb = mb.range_sb(); p.mr_sh = mb.range_sh(); p.mr_q = mb.range_q();
    }
    const Variant v = pick(a);
    if (v.p4) {
        int herr = 0;
        const int st4 = pfa::p4_launch(a, stream, &herr);
        if (st4 != PFA_OK) g_last_hip_error = herr;
        return st4;
    }
    p.nqblk = (a->Sq + v.block_m - 1) / v.block_m;
    p.xcd_group = v.xcd_group;
    p.scale_log2 = a->softmax_scale * pfa::LOG2E;
    p.magic_h = (uint32_t)((1ull << 32) / (uint64_t)a->H) + 1u;
    p.magic_g = (uint32_t)((1ull << 32) / (uint64_t)p.kv_group) + 1u;

    dim3 grid((unsigned)(p.nqblk * a->B * a->H));
    if (v.grid3) {
        // linear dispatch order is x fastest and workgroup n runs on XCD n % 8: x = XCD + 8 * (head within the XCD's current
        // group of G), y = Q block rank (heaviest first), z = group  ==  the order the kernel used to derive with divisions
        const int BH = a->B * a->H;
        if (p.xcd_group > 0 && (BH % (8 * p.xcd_group) != 0 || BH / (8 * p.xcd_group) > 65535)) p.xcd_group = 0;
        if (p.nqblk > 65535) return PFA_ERR_SHAPE;
        grid = p.xcd_group > 0 ? dim3(8u * p.xcd_group, (unsigned)p.nqblk, (unsigned)(BH / (8 * p.xcd_group)))
                               : dim3((unsigned)BH, (unsigned)p.nqblk, 1u);
    }
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    if (use_mbits && !enqueue_mask_words(mb, a, stream)) return PFA_ERR_LAUNCH;
    return pfa::launch(v.fn, grid, v.nthreads, p, (size_t)v.lds_bytes, stream);
}

int pfa_fa3_weights(const pfa_fa3_args* a, void* w, int32_t w_dtype, int64_t w_stride_b, int64_t w_stride_h,
                    int64_t w_stride_q, void* stream) {
    if (!a || !w) return PFA_ERR_NULL;
    pfa_fa3_args probe = *a;             // same validation as the forward; v/o are not read here
    if (!probe.v) probe.v = probe.k;
    if (!probe.o) {                      // no forward output: q stands in (an operand, so the forward's rules hold for it) -- never W,
        probe.o = const_cast<void*>(probe.q);                     // whose rules are its own, below
        probe.o_stride_b = probe.q_stride_b; probe.o_stride_h = probe.q_stride_h; probe.o_stride_s = probe.q_stride_s;
        probe.dtype_out = probe.dtype_in;
    }
    const int st = check(&probe);
    if (st != PFA_OK) return st;
    if (a->dtype_in == PFA_DTYPE_FP32) return PFA_ERR_DTYPE;      // the weights pass is MFMA only: hand it the 16-bit operands
    if (!a->lse) return PFA_ERR_NULL;
    if (w_dtype != a->dtype_in && w_dtype != PFA_DTYPE_FP32) return PFA_ERR_DTYPE;
    // W: aligned to its element (the kernel stores 16-byte pieces only where base and row stride allow it, else per element); rows
    // forward and at least Sk apart
    if (reinterpret_cast<uintptr_t>(w) % (w_dtype == PFA_DTYPE_FP32 ? 4 : 2) != 0) return PFA_ERR_ALIGN;
    if (w_stride_q < a->Sk || w_stride_b < 0 || w_stride_h < 0) return PFA_ERR_STRIDE;

    pfa::WeightsParams p;
    p.q = a->q; p.k = a->k; p.lse = a->lse; p.w = w;
    fill_common(p, a);
    pfa::fill_qk_strides(p, a);
    p.w_sb = w_stride_b; p.w_sh = w_stride_h; p.w_sq = w_stride_q;
    p.nqblk = (a->Sq + 127) / 128;
    p.scale_log2 = a->softmax_scale * pfa::LOG2E;
    const pfa::MaskWords mb = mask_words(a);          // as in pfa_fa3_fwd: the mask as words when the caller gave workspace
    const bool use_mbits = take_mask_words(p, mb, a);
    const bool causal = a->causal != 0, kmask = p.mask != nullptr, w32 = w_dtype == PFA_DTYPE_FP32;
    const auto fn = pfa::dispatch_elem_dim(a->dtype_in, a->D, [&](auto t) {
        using T = typename decltype(t)::type;
        return pfa::dispatch_bools([](auto c, auto k, auto o32) -> pfa::KernelFn<pfa::WeightsParams> {
            return &pfa::fa3_weights_kernel<T, decltype(t)::D, c.value, k.value, pfa::out_t<o32.value, T>>;
        }, causal, kmask, w32);
    });
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    if (use_mbits && !enqueue_mask_words(mb, a, stream)) return PFA_ERR_LAUNCH;      // (again: the call may come without a forward before it)
    return pfa::launch(fn, dim3((unsigned)(p.nqblk * a->B * a->H)), 256, p, 0, stream);
}

}  // extern "C"
