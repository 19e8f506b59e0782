// pfa_host.h -- host-side glue the entry points of libpfa_hip.so share (internal: nothing here is exported).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pfa_hip.h"

namespace pfa {

void set_last_hip_error(int e);   // pfa_capi.hip: what pfa_last_hip_error() reports

// A failed HIP call: keep its code (in *sink if given, else for pfa_last_hip_error) and clear HIP's sticky error.
inline bool hip_failed(hipError_t e, int* sink = nullptr) {
    if (e == hipSuccess) return false;
    if (sink) *sink = (int)e;
    else set_last_hip_error((int)e);
    (void)hipGetLastError();
    return true;
}

// Makes `dev` the current device for the scope and puts the caller's device back on every way out.
class DeviceScope {
    int prev_ = -1;
    bool switched_ = false;
    hipError_t err_;

public:
    explicit DeviceScope(int dev) {
        err_ = hipGetDevice(&prev_);
        if (err_ == hipSuccess && prev_ != dev) {
            err_ = hipSetDevice(dev);
            switched_ = err_ == hipSuccess;
        }
    }
    ~DeviceScope() {
        if (switched_) (void)hipSetDevice(prev_);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
    hipError_t error() const { return err_; }   // of the switch; a launch behind a failed one is PFA_ERR_DEVICE
};

// The mask fields of a kernel parameter block (FwdParams, F32Params, WeightsParams): the element mask with its four byte
// strides, or the [B, Sk] key mask as (stride, 0, 0, 1), or null.
template <typename Params>
inline void fill_mask(Params& p, const pfa_fa3_args* a) {
    if (a->mask) {
        p.mask = a->mask; p.m_sb = a->mask_stride_b; p.m_sh = a->mask_stride_h; p.m_sq = a->mask_stride_q; p.m_sk = a->mask_stride_k;
    } else {
        p.mask = a->key_mask; p.m_sb = a->key_mask_stride_b; p.m_sh = 0; p.m_sq = 0; p.m_sk = 1;
    }
}

}  // namespace pfa
