// pfa_fwd_sink_capi.hip -- C ABI of the dense training forward with attention sinks (include/pfa_hip_train_sinks.h, pfa_fa3_fwd_sink*): the entry
// points and the SINK instantiations of fa3_fwd_kernel, the 8-wave forward -- every (dtype, D, causal, split P, mask, store) set, and only
// that kernel.  The rules of pfa_fa3_sinks come first, then everything pfa_fa3_check says of the argument block, then what the sink
// refuses; a NULL block is pfa_fa3_fwd itself.  A translation unit of its own, built with the flags of pfa_capi.hip (whose instantiations
// of the same body it matches bit for bit at a sink of -inf).  No allocation, no synchronisation, no process-wide state.
#include "pfa_hip_train_sinks.h"

#include <hip/hip_runtime.h>
#include <stdio.h>

#include "fa3_fwd_kernel.h"
#include "pfa_cache_modes.h"
#include "pfa_host.h"
#include "pfa_mask_host.h"

namespace {

using SinkParams = pfa::FwdBlock<true>;

int check(const pfa_fa3_args* a, const pfa_fa3_sinks* sinks) {
    int st = pfa::check_sinks(sinks);
    if (st != PFA_OK) return st;
    st = pfa_fa3_check(a);
    if (st != PFA_OK) return st;
    if (a->dtype_in == PFA_DTYPE_FP32) return PFA_ERR_DTYPE;      // the exact fp32 kernels (and with them dropout) carry no sink
    const unsigned var = (a->flags & PFA_FLAG_VARIANT_MASK) >> 8;
    if (var == 43 || var == 45) return PFA_ERR_FLAGS;             // the 4-wave and the persistent kernel carry none either
    return PFA_OK;
}

bool has_mask(const pfa_fa3_args* a) { return a->key_mask != nullptr || a->mask != nullptr; }

int nqblk(const pfa_fa3_args* a) { return (a->Sq + pfa::FWD_BLOCK_M - 1) / pfa::FWD_BLOCK_M; }

}  // namespace

extern "C" {

int pfa_fa3_fwd_sink_check(const pfa_fa3_args* a, const pfa_fa3_sinks* sinks) { return sinks ? check(a, sinks) : pfa_fa3_check(a); }

int pfa_fa3_fwd_sink_describe(const pfa_fa3_args* a, const pfa_fa3_sinks* sinks, char* buf, size_t n) {
    if (!sinks) return pfa_fa3_describe(a, buf, n);
    const int st = check(a, sinks);
    if (st != PFA_OK) return st;
    if (buf && n)      // pfa_capi.hip's 8-wave name, "_sink" in front of the tag
        snprintf(buf, n, "fa3_fwd_%s_d%d_%s%s%s_%s_sink_v8269", a->dtype_in == PFA_DTYPE_BF16 ? "bf16" : "fp16", a->D, a->causal ? "causal" : "full",
                 (a->flags & PFA_FLAG_SPLIT_P) ? "_splitp" : "", has_mask(a) ? "_kmask" : "", a->dtype_out == PFA_DTYPE_FP32 ? "o32" : "o16");
    return nqblk(a) * a->B * a->H;
}

int pfa_fa3_fwd_sink(const pfa_fa3_args* a, const pfa_fa3_sinks* sinks, void* stream) {
    if (!sinks) return pfa_fa3_fwd(a, stream);
    const int st = check(a, sinks);
    if (st != PFA_OK) return st;

    SinkParams p;      // filled as pfa_fa3_fwd fills its block for the 8-wave kernel
    p.q = a->q; p.k = a->k; p.v = a->v; p.o = a->o;
    p.lse = a->lse;
    pfa::fill_common(p, a);
    pfa::fill_qkvo_strides(p, a);
    p.dbg = nullptr;
    const pfa::MaskWords mb = pfa::fwd_mask_words(a);      // the mask as words when the caller gave workspace
    const bool use_mbits = pfa::take_mask_words(p, mb, a);
    if (use_mbits) {
        p.mrange = (const int*)((const char*)a->workspace + mb.word_bytes());
        p.mr_sb = mb.range_sb(); p.mr_sh = mb.range_sh(); p.mr_q = mb.range_q();
    }
    p.nqblk = nqblk(a);
    p.xcd_group = 0; p.magic_h = p.magic_g = 0;
    p.scale_log2 = a->softmax_scale * pfa::LOG2E;
    p.sinks = sinks->sinks;

    const bool causal = a->causal != 0, split = (a->flags & PFA_FLAG_SPLIT_P) != 0, out32 = a->dtype_out == PFA_DTYPE_FP32;
    const auto fn = pfa::dispatch_elem_dim(a->dtype_in, a->D, [&](auto t) {
        using T = typename decltype(t)::type;
        return pfa::dispatch_bools([](auto c, auto s, auto k, auto o32) -> pfa::KernelFn<SinkParams> {
            return &pfa::fa3_fwd_kernel<T, decltype(t)::D, c.value, s.value, k.value, pfa::out_t<o32.value, T>>;
        }, causal, split, has_mask(a), out32);
    });
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    if (use_mbits && !pfa::launch_row_words(mb, a->workspace, stream)) return PFA_ERR_LAUNCH;
    const size_t lds = 2 * 2 * pfa::BLOCK_N * a->D * 2;      // two buffers of a K and a V tile image
    return pfa::launch(fn, dim3((unsigned)(p.nqblk * a->B * a->H)), pfa::FWD_THREADS, p, lds, stream);
}

}  // extern "C"
