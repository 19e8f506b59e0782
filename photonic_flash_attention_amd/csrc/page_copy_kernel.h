// page_copy_kernel.h -- copy-on-write's data movement for a paged KV cache on MI355X (gfx950), hand-written HIP: copies whole or
// partial pages inside the K and V pools from a device pair list, so that a fork's first write needs no host round trip (what vLLM's
// copy_blocks does).
//
// Pair i = (s, d) = (pairs[i][0], pairs[i][1]).  It is EMPTY when s or d lies outside [0, num_pages - 1] (-1 is the documented "no
// copy") or s == d: an empty pair reads nothing and writes nothing.  Otherwise tokens [0, r_i) of K page s go to K page d, the same for
// V, with r_i = page_size (ROWS off) or clamp(rows[i], 0, page_size); tokens >= r_i of page d are not written.  Bad device data loses a
// copy, it never makes an address outside the pools: s and d are range-checked, r_i is clamped, and a token, head and piece inside a
// page come from host shapes alone.
// The caller promises that no page is the destination of two non-empty pairs, that no destination is the source of another, and that
// the pages of a pool do not overlap: then a replay is idempotent.  Without the promise a destination ends up as one of the candidates.
//
// Work item = 8 elements (16 bytes) of one head of one token, K and V both.  A page has page_size * units items, units = Hkv * D / 8,
// laid out [token][head][piece] so that consecutive lanes move consecutive 16-byte pieces of a token row.  A workgroup of 256 threads
// takes PAGE_COPY_ITEMS * 256 consecutive items of ONE pair: lane t the items base + j * 256 + t.  s, d and r_i are uniform per workgroup,
// so they are scalar loads, and the workgroups of an empty pair or past r_i * units return before any vector memory instruction.  A lane
// issues all its K and V loads, then its stores: PAGE_COPY_ITEMS = 4 puts 8 x 16 bytes per lane, 32 KiB per workgroup, in flight -- what
// a CU needs outstanding to stream from HBM is then met by one resident workgroup, at 32 VGPRs of payload, which leaves occupancy alone.
// Grid = n_pairs * ceil(page_size * units / (256 * PAGE_COPY_ITEMS)) from host shapes only: capturable, and valid while pairs, rows and
// the pools change between replays.  No LDS, no atomics, no workspace; the element type does not matter (any 2-byte type moves alike).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pfa {

constexpr int PAGE_COPY_THREADS = 256;
constexpr int PAGE_COPY_ITEMS = 4;                                   // 16-byte pieces of K, and of V, per lane
constexpr int PAGE_COPY_WG_ITEMS = PAGE_COPY_THREADS * PAGE_COPY_ITEMS;

struct PageCopyParams {
    void* k_pool;                // pools [num_pages, page_size, Hkv, D] by element strides
    void* v_pool;
    const int32_t* pairs;        // [n_pairs][2] = (src, dst), rows pairs_stride apart
    const int32_t* rows;         // ROWS: [n_pairs]
    int64_t pairs_stride;
    int64_t k_sb, k_sh, k_ss;    // page, head, token
    int64_t v_sb, v_sh, v_ss;
    int32_t nchunk;              // workgroups per pair: ceil(page_size * units / PAGE_COPY_WG_ITEMS)
    int32_t dchunks;             // D / 8
    int32_t units;               // Hkv * D / 8; page_size * units + PAGE_COPY_WG_ITEMS fits 32 bits (checked by the host)
    int32_t page_size, num_pages;
};

typedef uint32_t page_copy_b128 __attribute__((ext_vector_type(4)));

template <bool ROWS>
__global__ __launch_bounds__(PAGE_COPY_THREADS) void page_copy_kernel(const PageCopyParams p) {
    const int i = blockIdx.x / p.nchunk;
    const int item0 = (blockIdx.x - i * p.nchunk) * PAGE_COPY_WG_ITEMS;     // the workgroup's first item of pair i

    const int s = p.pairs[(int64_t)i * p.pairs_stride];
    const int d = p.pairs[(int64_t)i * p.pairs_stride + 1];
    if ((unsigned)s >= (unsigned)p.num_pages || (unsigned)d >= (unsigned)p.num_pages || s == d) return;      // wave-uniform: empty pair
    int r = p.page_size;
    if constexpr (ROWS) r = min(max(p.rows[i], 0), p.page_size);
    const int n = r * p.units;                                               // the pair's items
    if (item0 >= n) return;                                                  // wave-uniform: nothing of the pair in the workgroup

    const uint16_t* ks = (const uint16_t*)p.k_pool + (int64_t)s * p.k_sb;
    const uint16_t* vs = (const uint16_t*)p.v_pool + (int64_t)s * p.v_sb;
    uint16_t* kd = (uint16_t*)p.k_pool + (int64_t)d * p.k_sb;
    uint16_t* vd = (uint16_t*)p.v_pool + (int64_t)d * p.v_sb;

    // A lane past the pair's last item loads that last item again (an address inside rows [0, r) of the source page) and stores
    // nothing: with no branch around the loads all eight are issued back to back, ahead of the first store.
    int64_t koff[PAGE_COPY_ITEMS], voff[PAGE_COPY_ITEMS];
    bool ok[PAGE_COPY_ITEMS];
    page_copy_b128 kx[PAGE_COPY_ITEMS], vx[PAGE_COPY_ITEMS];
#pragma unroll
    for (int j = 0; j < PAGE_COPY_ITEMS; ++j) {
        const int mine = item0 + j * PAGE_COPY_THREADS + (int)threadIdx.x;
        ok[j] = mine < n;
        const int item = min(mine, n - 1);               // 0 <= item < n = r * units
        const int tok = item / p.units;                  // < r <= page_size
        const int rem = item - tok * p.units;
        const int hk = rem / p.dchunks;
        const int c = rem - hk * p.dchunks;
        koff[j] = (int64_t)tok * p.k_ss + (int64_t)hk * p.k_sh + c * 8;
        voff[j] = (int64_t)tok * p.v_ss + (int64_t)hk * p.v_sh + c * 8;
    }
#pragma unroll
    for (int j = 0; j < PAGE_COPY_ITEMS; ++j) {
        kx[j] = *reinterpret_cast<const page_copy_b128*>(ks + koff[j]);
        vx[j] = *reinterpret_cast<const page_copy_b128*>(vs + voff[j]);
    }
#pragma unroll
    for (int j = 0; j < PAGE_COPY_ITEMS; ++j)
        if (ok[j]) {
            *reinterpret_cast<page_copy_b128*>(kd + koff[j]) = kx[j];
            *reinterpret_cast<page_copy_b128*>(vd + voff[j]) = vx[j];
        }
}

}  // namespace pfa
