// fp8_cvt.h -- the one conversion the kernels over an FP8 (OCP e4m3fn) KV cache share (fa3_decode_kernel.h, fa3_prefill_kernel.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pfa {

// 8 e4m3fn bytes (element j in byte j) -> 8 elements of T, exactly
template <typename T, typename V8> __device__ __forceinline__ V8 cvt_e4m3x8(uint32_t w0, uint32_t w1) {
    typedef __attribute__((ext_vector_type(2))) float f32x2;
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, true);
    const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, true);
    return V8{(T)a[0], (T)a[1], (T)b[0], (T)b[1], (T)c[0], (T)c[1], (T)d[0], (T)d[1]};
}

}  // namespace pfa
