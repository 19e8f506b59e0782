// sink_grad_kernel.h -- the gradient of the attention sinks of the training forward (include/pfa_hip_train_sinks.h, pfa_fa3_sink_grad), hand-written HIP
// for MI355X (gfx950).
//
// The sink of head h is one more key of score sinks[h] and a zero value row (fa3_fwd_kernel.h, SINK).  Its softmax weight in row i is
// p_i = exp(sinks[h] - LSE_i), its dP is dO_i . 0 = 0, so dS = p_i (0 - delta_i) and
//     d_sinks[h] = - sum over the rows (b, i) of head h of  exp(sinks[h] - LSE[b,h,i]) * delta[b,h,i]
// with LSE the forward's (the sink inside) and delta = rowsum(dO o O) as the dQ kernel of the backward leaves it.  A memory-bound reduction
// of two fp32 arrays, 8 bytes per row.
//
// Two stages, no atomics, every sum in an order fixed by the shapes alone (bitwise reproducible):
//   1. sink_grad_partial_kernel: workgroup (chunk c, batch b, head h) sums rows [c * SINK_GRAD_CHUNK, (c + 1) * SINK_GRAD_CHUNK) of sequence
//      b -- thread t takes rows t, t + 256, ... of the chunk in that order, a wave folds its 64 lanes by xor-butterfly, thread 0 adds the four
//      wave sums in wave order -- and leaves one fp32 in the workspace, partial[h][b * nchunk + c].  A chunk past the sequence's rows leaves 0.
//   2. sink_grad_final_kernel: one workgroup per head sums the head's B * nchunk partials the same way and OVERWRITES d_sinks[h] with minus
//      the sum.
// One workgroup per head alone would stream the whole head through one CU (tens of GB/s against the chip's TB/s): fine at 16 K rows, not at
// a million.  The grids come from host shapes only (packed: max_seqlen_q), so a captured step replays while sinks, lengths and data change.
//
// Rows: dense [B, H, Sq] by (batch, head) element strides, rows contiguous; or packed [H, total_q] as pfa_fa3_varlen_bwd leaves it, sequence
// b owning the rows packed_seq(cu_seqlens_q, b) says (clamped as the packed kernels clamp them; at most max_seqlen_q rows of a sequence).
// Rows no sequence covers -- the tail behind cu[B], gaps, rows past max_seqlen_q -- are never read.  A row with LSE = -inf (no key and no
// sink: it has no weight on the sink) is SKIPPED, not multiplied by zero: delta there may be anything.  sinks[h] = -inf: every row is
// skipped and d_sinks[h] = 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa3_fwd_kernel.h"

namespace pfa {

constexpr int SINK_GRAD_THREADS = 256;
constexpr int SINK_GRAD_CHUNK = 2048;      // rows per stage-1 workgroup: 8 per thread, 16 KiB of LSE and delta

struct SinkGradParams {
    const float* lse;
    const float* delta;
    const float* sinks;
    float* d_sinks;
    float* partial;            // [H][B * nchunk]
    const int32_t* cu_q;       // packed: int32 [B + 1] on the device; null: dense
    int64_t l_sb, l_sh;        // dense: element strides of lse between batches and heads (rows contiguous)
    int64_t d_sb, d_sh;        // ... and of delta
    int32_t B, H, Sq;          // Sq: rows of a sequence (packed: max_seqlen_q)
    int32_t total_q;           // packed: rows of the [H, total_q] arrays
    int32_t nchunk;            // ceil(Sq / SINK_GRAD_CHUNK)
};

// sum of x over the workgroup's 256 threads, in thread 0: lanes by xor-butterfly, then the four waves in order
__device__ __forceinline__ float sink_grad_block_sum(float x, float* wave_sums) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = x;
    __syncthreads();
    return (wave_sums[0] + wave_sums[1]) + (wave_sums[2] + wave_sums[3]);
}

template <bool PACKED>
__global__ __launch_bounds__(SINK_GRAD_THREADS) void sink_grad_partial_kernel(const SinkGradParams p) {
    __shared__ float wave_sums[SINK_GRAD_THREADS / 64];
    const int n = blockIdx.x;                       // ((h * B) + b) * nchunk + c
    const int c = n % p.nchunk, bh = n / p.nchunk, b = bh % p.B, hh = bh / p.B;
    const float* L;
    const float* Dl;
    int len;
    if constexpr (PACKED) {
        const PackedSeq sq = packed_seq(p.cu_q, b, p.total_q, p.Sq);
        len = sq.len;
        L = p.lse + (int64_t)hh * p.total_q + sq.start;
        Dl = p.delta + (int64_t)hh * p.total_q + sq.start;
    } else {
        len = p.Sq;
        L = p.lse + (int64_t)b * p.l_sb + (int64_t)hh * p.l_sh;
        Dl = p.delta + (int64_t)b * p.d_sb + (int64_t)hh * p.d_sh;
    }
    const float s = p.sinks[hh];
    float acc = 0.f;
    if (s > -INFINITY) {                            // (workgroup-uniform; a -inf sink has no weight anywhere)
        const int i0 = c * SINK_GRAD_CHUNK + (int)threadIdx.x;
        float l[SINK_GRAD_CHUNK / SINK_GRAD_THREADS], d[SINK_GRAD_CHUNK / SINK_GRAD_THREADS];
#pragma unroll
        for (int k = 0; k < SINK_GRAD_CHUNK / SINK_GRAD_THREADS; ++k) {       // all loads first: 16 in flight per thread
            const int i = i0 + k * SINK_GRAD_THREADS;
            const bool in = i < len;
            l[k] = in ? L[i] : -INFINITY;
            d[k] = in ? Dl[i] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < SINK_GRAD_CHUNK / SINK_GRAD_THREADS; ++k)
            if (l[k] > -INFINITY) acc += expf(s - l[k]) * d[k];               // skipped, not multiplied by zero
    }
    const float tot = sink_grad_block_sum(acc, wave_sums);
    if (threadIdx.x == 0) p.partial[n] = tot;
}

template <int UNUSED = 0>
__global__ __launch_bounds__(SINK_GRAD_THREADS) void sink_grad_final_kernel(const SinkGradParams p) {
    __shared__ float wave_sums[SINK_GRAD_THREADS / 64];
    const int hh = blockIdx.x;
    const int64_t P = (int64_t)p.B * p.nchunk;
    const float* part = p.partial + (int64_t)hh * P;
    float acc = 0.f;
    for (int64_t i = threadIdx.x; i < P; i += SINK_GRAD_THREADS) acc += part[i];
    const float tot = sink_grad_block_sum(acc, wave_sums);
    if (threadIdx.x == 0) p.d_sinks[hh] = 0.f - tot;
}

}  // namespace pfa
