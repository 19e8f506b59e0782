/*
 * pfa_hip.h -- C ABI of libpfa_hip.so: the MI355X (gfx950) Flash-Attention forward (and backward) that
 * replaces the body of the reference's electronic attention core.
 * ABI history: v1 forward; v2 general masks + weights; v3 backward; v4 grouped-query heads (kv_group); v5 fp32 operands (exact
 * fp32 kernels, forward and backward) and dense-branch attention dropout; v6 pfa_fa3_prepare, reserve_cus, pfa_probe_mfma;
 * v7 pfa_fa3_bwd_args.kv_group (grouped-query heads in the backward: dK / dV summed over the group in the kernel); v8 split-KV decode
 * over a KV cache (pfa_fa3_decode_args, pfa_fa3_decode*: query rows of a K/V head packed together, keys split over workgroups);
 * v9 paged KV cache for the decode (pfa_fa3_decode_args.block_table / page_size / num_pages appended: a pool of pages and a block table);
 * v9, additive: pfa_fa3_prefill* -- the compute-bound forward over a KV cache (any number of query rows, contiguous or paged, on the
 * unchanged pfa_fa3_decode_args);
 * v9, additive: pfa_fa3_prefill_varlen* -- the same forward for ragged batches (packed query rows, cu_seqlens_q on the device);
 * v9, additive: pfa_fa3_cache_ext and the *_ex entry points of the three calls over a KV cache -- a sliding window (each row sees its
 * last `window` keys), with keys and block-table entries behind the window never read;
 * v9, additive: pfa_kv_append* -- the device-side append of a step's new K / V rows into a contiguous or paged cache.
 * v9, additive: pfa_rope_append* -- rotary embedding fused into that append: Q and the new K rotated by positions derived on the device.
 * v9, additive: pfa_attn_merge* -- the merge of partial attention results (O, LSE) over disjoint key sets into the result over their
 * union: what a shared prefix computed once per batch, a split over keys or keys spread over several GPUs need behind them.
 * v9, additive: pfa_page_copy* -- whole or partial pages copied inside the pools of a paged cache from a device pair list: the data
 * movement of copy-on-write for sequences that share pages.
 * v9, additive: pfa_fa3_tree_mask and pfa_fa3_decode_tree* -- the decode with a 64-bit visibility word per query row over the step's own
 * keys in place of the causal triangle: the verification of a drafted token TREE (speculative decoding) in one pass over the cache.
 * v9, additive: pfa_fa3_varlen_args / pfa_fa3_varlen_bwd_args and pfa_fa3_varlen_* -- packed variable-length attention for training,
 * forward and backward: sequences of different lengths one after the other in [total, H, D] tensors, cu_seqlens_q / cu_seqlens_k on
 * the device (flash-attn's flash_attn_varlen_func), on the dense 16-bit kernels in a packed mode.
 * v9, additive: PFA_DTYPE_FP8_E4M3, pfa_fa3_kv_quant, pfa_fa3_decode_q8* and pfa_kv_append_q8* -- the decode over an FP8 (e4m3fn) KV
 * cache with one fp32 descale per (sequence, K/V head), and the append that quantises a step's 16-bit rows into it.
 * v9, additive: pfa_fa3_prefill_q8* and pfa_fa3_prefill_varlen_q8* -- the forward over an FP8 (e4m3fn) KV cache, uniform and ragged,
 * contiguous and paged: chunked and prefix-cached prefill, speculative steps past 64 rows and mixed batches on one-byte pages.
 * v9, additive: pfa_fa3_sinks and pfa_fa3_decode_sink*, pfa_fa3_prefill_sink*, pfa_fa3_prefill_varlen_sink*, pfa_fa3_prefill_split_sink* --
 * attention sinks over a 16-bit KV cache: one learned fp32 value per query head in every row's softmax denominator, in the decode, the
 * forward (uniform, ragged, windowed) and the split over keys.
 * v9, additive, declared in pfa_hip_train_sinks.h: pfa_fa3_fwd_sink*, pfa_fa3_varlen_fwd_sink* and pfa_fa3_sink_grad* -- attention sinks
 * for training: the dense and the packed forward (8-wave kernel) with a pfa_fa3_sinks block, and the gradient of the sinks behind the
 * unchanged backward.
 *
 * Reference seam (danieleschmidt/Photonic-Flash-Attention, all paths under
 * src/photonic_flash_attention/):
 *
 *   pfa_fa3_fwd             replaces  core/flash_attention_3.py:120-150  _flash_attention_forward
 *                                     = :152-180 _standard_attention + :182-262 _tiled_attention
 *                                     (called from FlashAttention3.forward at :102)
 *   pfa_fa3_args.softmax_scale         the `q = q * self.scaling` pass at :138, folded into the kernel
 *   pfa_fa3_args.causal / seqlens_k /  the `attention_mask` argument (:165-168, :234-236): causal = 4-D
 *     key_mask / mask                  lower-triangular mask, seqlens_k / key_mask = 2-D [B,Sk] key mask,
 *                                      mask = any 4-D mask
 *   pfa_fa3_weights                    the `need_weights=True` outputs (:171,:180,:257-258)
 *   pfa_fa3_args.o strides             the `.transpose(1,2).contiguous()` copy at :107 (the kernel writes
 *                                     [B,S,H,D] directly, so the copy disappears)
 *   pfa_fa3_bwd                        autograd through :152-262 -- the reference's only backward (its modules train
 *                                     through the eager core; tests/unit/test_flash_attention_3.py:137-160)
 *   pfa_fa3_workspace_bytes           the tile-size memory budget of :264-293 (this path needs none; a key mask can use a few bytes)
 *   pfa_device_supported              the `torch.cuda.is_available()` probes at :71,:142
 *
 * The reference has no native code, so nothing binds an FFI today; INTEGRATION.md
 * shows the ctypes stub a maintainer adds at flash_attention_3.py:102.
 *
 * Conventions
 *   - plain C, no C++/torch types; every pointer is a DEVICE pointer owned by the caller;
 *   - the library allocates nothing, frees nothing, keeps no reference after return;
 *   - asynchronous: work is enqueued on `stream` (a hipStream_t passed as void*), no implicit sync;
 *   - re-entrant and thread-safe; the only process-wide state is one code-object handle per device (the assembly kernels'
 *     hipModule_t), loaded once under a mutex by pfa_fa3_prepare / pfa_device_supported (or, failing that, by the first call)
 *     and never changed afterwards;
 *   - returns PFA_OK (0) or a negative pfa_status; never aborts the process.
 */
#ifndef PFA_HIP_H
#define PFA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFA_ABI_VERSION 9

typedef enum pfa_status {
    PFA_OK = 0,
    PFA_ERR_NULL = -1,          /* required pointer is NULL                         */
    PFA_ERR_STRUCT_SIZE = -2,   /* args->size does not match a known struct version */
    PFA_ERR_SHAPE = -3,         /* B,H,Sq,Sk <= 0 or grid limits exceeded           */
    PFA_ERR_HEAD_DIM = -4,      /* D not in {64, 128}                               */
    PFA_ERR_DTYPE = -5,         /* dtype_in / dtype_out unsupported                 */
    PFA_ERR_STRIDE = -6,        /* a stride is not a multiple of 8 elements         */
    PFA_ERR_ALIGN = -7,         /* a base pointer is not 16-byte aligned            */
    PFA_ERR_DEVICE = -8,        /* device is not gfx950 / cannot be selected        */
    PFA_ERR_LAUNCH = -9,        /* hipLaunchKernel failed (see pfa_last_hip_error)  */
    PFA_ERR_FLAGS = -10         /* unknown flag bits                                */
} pfa_status;

typedef enum pfa_dtype {
    PFA_DTYPE_BF16 = 0,
    PFA_DTYPE_FP16 = 1,
    PFA_DTYPE_FP32 = 2,         /* output of the 16-bit kernels; as dtype_in: the EXACT fp32 kernel (fp32 modules, slow) */
    PFA_DTYPE_FP8_E4M3 = 3      /* OCP e4m3fn (max finite 448, 0x7f / 0xff NaN, no infinities; not MI300's fnuz): only as
                                   pfa_fa3_kv_quant.kv_dtype, the element type of a KV cache */
} pfa_dtype;

/* flags */
#define PFA_FLAG_SPLIT_P   0x1u  /* carry P as bf16 hi+lo (two PV MFMA passes): the <=1e-3 parity mode        */
#define PFA_FLAG_NO_XCD_MAP 0x2u /* debugging: identity block->work mapping                                  */
#define PFA_FLAG_VARIANT_MASK 0xff00u /* bits 8..15: kernel selector for tests / A-B runs.  0 = the library chooses; 43 = the 4-wave HIP kernel,
                                         44 = the 8-wave HIP kernel, 45 = the persistent 4-wave assembly kernel (each only where it applies;
                                         otherwise the library's choice).  Anything else is PFA_ERR_FLAGS. */

/*
 * One attention problem: O[b,i,h,:] = softmax_j(scale * <Q[b,i,h,:], K[b,j,h,:]> + mask) V[b,j,h,:]
 *
 * Tensors are addressed as base + b*stride_b + h*stride_h + s*stride_s + d (strides in ELEMENTS of the
 * tensor's dtype, last dimension contiguous).  That covers [B,S,H,D] (what a fused QKV projection yields:
 * q = qkv[..., 0:E] has stride_s = 3E, stride_h = D), [B,H,S,D], and slices of either.
 */
typedef struct pfa_fa3_args {
    uint32_t size;              /* = sizeof(pfa_fa3_args); versions the struct       */
    uint32_t flags;             /* PFA_FLAG_*                                        */

    const void* q;              /* [B, Sq, H, D] by strides, dtype_in                */
    const void* k;              /* [B, Sk, H, D]                                     */
    const void* v;              /* [B, Sk, H, D]                                     */
    void*       o;              /* [B, Sq, H, D], dtype_out                          */
    float*      lse;            /* optional [B, H, Sq] fp32 natural-log LSE, or NULL */
    const int32_t* seqlens_k;   /* optional [B]: keys >= seqlens_k[b] are masked     */
    const uint8_t* key_mask;    /* optional [B, Sk] bytes, 0 = masked (2-D mask)     */

    int64_t q_stride_b, q_stride_h, q_stride_s;
    int64_t k_stride_b, k_stride_h, k_stride_s;
    int64_t v_stride_b, v_stride_h, v_stride_s;
    int64_t o_stride_b, o_stride_h, o_stride_s;
    int64_t key_mask_stride_b;  /* bytes between batches of key_mask                 */

    int32_t B, H, Sq, Sk, D;
    int32_t dtype_in;           /* PFA_DTYPE_BF16 | PFA_DTYPE_FP16 | PFA_DTYPE_FP32 (exact fp32 kernel: strides multiples of 4 elements, dtype_out fp32, no flags) */
    int32_t dtype_out;          /* = dtype_in, or PFA_DTYPE_FP32                     */
    int32_t causal;             /* 1: key j visible to row i iff j <= i (top-left; pfa_fa3_decode_args.causal is bottom-right) */
    float   softmax_scale;      /* usually D^-0.5                                    */
    int32_t device_id;          /* HIP device ordinal the pointers live on           */

    void*   workspace;          /* pfa_fa3_workspace_bytes() bytes, may be NULL if 0 */
    size_t  workspace_bytes;

    /* ABI v2: general mask, the reference's 4-D `attention_mask` (flash_attention_3.py:168,235-236).
     * u8, 0 = masked, element (b,h,i,j) at mask + b*mask_stride_b + h*mask_stride_h + i*mask_stride_q +
     * j*mask_stride_k (BYTE strides; 0 broadcasts a dimension).  At most one of key_mask / mask may be set;
     * `causal` and `seqlens_k` combine with either. */
    const uint8_t* mask;
    int64_t mask_stride_b, mask_stride_h, mask_stride_q, mask_stride_k;

    /* ABI v4: grouped-query attention (not in the reference; what Hugging Face decoder models hand over).  k and v hold
     * H / kv_group heads and query head h reads K/V head h / kv_group, so nothing has to be expanded in memory.
     * 0 or 1 = one K/V head per query head.  H must be a multiple of kv_group.  (The backward takes the same field since ABI v7:
     * pfa_fa3_bwd_args.kv_group.) */
    int32_t kv_group;
    /* ABI v6: CUs to leave free (0 = none).  The persistent forward holds one workgroup on every CU for the whole launch, so a
     * kernel-based collective (RCCL) enqueued beside it only runs when it drains; a caller that overlaps such a collective passes
     * the CUs it needs (the grid shrinks to n_cu - reserve_cus, a multiple of 8).  Copy-engine transfers need none. */
    int32_t reserve_cus;

    /* ABI v5: attention dropout of the reference's dense branch (flash_attention_3.py:174-175: dropout(softmax(scores)) @ v).
     * drop_mask: keep-mask bytes [B][H][Sq][Sk] contiguous (non-zero = keep), drawn by the caller; kept weights are scaled by
     * drop_scale = 1 / (1 - p), the softmax normaliser is the un-dropped row sum.  Only with dtype_in = fp32 (the fp32 kernels);
     * NULL = no dropout. */
    const uint8_t* drop_mask;
    float   drop_scale;
    int32_t reserved1;          /* must be 0 */
} pfa_fa3_args;

/* ABI version of the loaded library (== PFA_ABI_VERSION of the header it was built from). */
int pfa_abi_version(void);

/* Human-readable text for a pfa_status. */
const char* pfa_status_string(int status);

/* 1 if HIP device `device_id` is a gfx950 part this library has code for, 0 if not, <0 on error. */
int pfa_device_supported(int device_id);

/* ABI v6: load the device's code objects NOW (idempotent, thread-safe): afterwards no call on that device loads a module, so a
 * first pfa_fa3_fwd may sit inside a hipStreamBeginCapture region or a timed loop.  pfa_device_supported does the same.
 * PFA_OK, or PFA_ERR_DEVICE (pfa_last_hip_error: why). */
int pfa_fa3_prepare(int device_id);

/* Last hipError_t seen by a failing call on this thread (0 = hipSuccess). */
int pfa_last_hip_error(void);

/* Scratch bytes pfa_fa3_fwd can use for `a`: 0 without a mask; with key_mask or mask, 8 bytes per un-broadcast mask row and
 * 64-key tile (+ 128 bytes per 256 mask rows) -- pfa_fa3_fwd first condenses the mask into one 64-bit word per row and tile
 * there (one word read per tile instead of a mask byte per score: 2-4 x faster) and notes, per 256 rows, the first and last
 * tile that holds a visible key: a Q block then runs only those tiles, so a structured mask (a band, a triangle, padding)
 * skips what it hides.  Optional: with workspace == NULL or too few bytes the mask is read byte-wise, every tile runs, and
 * the result is the same. */
size_t pfa_fa3_workspace_bytes(const pfa_fa3_args* a);

/* Validate `a` without launching: PFA_OK or the error pfa_fa3_fwd would return. */
int pfa_fa3_check(const pfa_fa3_args* a);

/* Enqueue the forward on `stream` (hipStream_t as void*, NULL = default stream). */
int pfa_fa3_fwd(const pfa_fa3_args* a, void* stream);

/*
 * Attention weights on request (the reference's need_weights=True, flash_attention_3.py:171,180,257-258):
 * W[b,h,i,j] = exp(scale*<q_i,k_j> + mask - lse[b,h,i]), the TRUE softmax row (the reference's tiled branch
 * returns un-renormalised tiles; documented divergence).  `a` is the argument block of the forward call that
 * produced a->lse (required; a->v and a->o are ignored).  W is addressed base + b*w_stride_b + h*w_stride_h +
 * i*w_stride_q + j (ELEMENT strides, last dim contiguous), dtype w_dtype = a->dtype_in or PFA_DTYPE_FP32.
 * Every element of W is written exactly once (masked ones as zeros): W may be uninitialised.
 *
 * Field rules: those of pfa_fa3_fwd for `a` (with a->o NULL, q stands in for it: W is never judged by the output's rules), then
 * fp32 operands -> PFA_ERR_DTYPE; a->lse NULL -> PFA_ERR_NULL; w_dtype neither a->dtype_in nor fp32 -> PFA_ERR_DTYPE; W not aligned
 * to its own element size (2 or 4 bytes) -> PFA_ERR_ALIGN; w_stride_q < Sk or a negative W stride -> PFA_ERR_STRIDE.  Nothing more is
 * asked of W: where its base and row stride are multiples of 16 bytes the rows leave in 16-byte pieces, elsewhere element by element.
 */
int pfa_fa3_weights(const pfa_fa3_args* a, void* w, int32_t w_dtype, int64_t w_stride_b, int64_t w_stride_h,
                    int64_t w_stride_q, void* stream);

/*
 * Backward pass (ABI v3).  The reference obtains gradients from autograd through its eager forward
 * (flash_attention_3.py:152-262; its unit tests only require that gradients exist, tests/unit/
 * test_flash_attention_3.py:137-160); this entry point computes dQ, dK, dV from q, k, v, o, dO and the forward's
 * LSE by recomputation (two launches: dQ per query block, which also produces delta = rowsum(dO*O), then dK/dV per key block; no
 * atomics, bitwise reproducible).  Masks: `causal`, `seqlens_k` and the forward's general u8 `mask` (field below; a [B,Sk] key mask
 * is the broadcast form mask_stride_b = Sk, _h = 0, _q = 0, _k = 1).
 * All tensors [B,S,H,D] by element strides, last dim contiguous; gradients in `dtype_grad` (= dtype or fp32).
 * `delta` is caller-provided scratch of pfa_fa3_bwd_workspace_bytes() bytes ([B,H,Sq] fp32).
 */
typedef struct pfa_fa3_bwd_args {
    uint32_t size;              /* = sizeof(pfa_fa3_bwd_args) */
    uint32_t flags;             /* must be 0 */
    const void* q;
    const void* k;
    const void* v;
    const void* o;              /* forward output */
    const void* dout;           /* gradient of the forward output */
    const float* lse;           /* [B,H,Sq] from the forward (pfa_fa3_args.lse) */
    void* dq;
    void* dk;
    void* dv;
    float* delta;               /* scratch [B,H,Sq] */
    const int32_t* seqlens_k;   /* optional [B] */
    int64_t q_stride_b, q_stride_h, q_stride_s;
    int64_t k_stride_b, k_stride_h, k_stride_s;
    int64_t v_stride_b, v_stride_h, v_stride_s;
    int64_t o_stride_b, o_stride_h, o_stride_s;
    int64_t do_stride_b, do_stride_h, do_stride_s;
    int64_t dq_stride_b, dq_stride_h, dq_stride_s;
    int64_t dk_stride_b, dk_stride_h, dk_stride_s;
    int64_t dv_stride_b, dv_stride_h, dv_stride_s;
    int32_t B, H, Sq, Sk, D;
    int32_t dtype;              /* PFA_DTYPE_BF16 | PFA_DTYPE_FP16 | PFA_DTYPE_FP32 (v5): q,k,v,o,dout */
    int32_t dtype_grad;         /* = dtype or PFA_DTYPE_FP32: dq,dk,dv */
    int32_t causal;
    float   softmax_scale;
    int32_t device_id;
    /* optional element mask of the forward, same convention as pfa_fa3_args.mask (u8, 0 = masked, BYTE strides, 0
     * broadcasts a dimension; a [B,Sk] key mask is mask_stride_b = Sk, _h = 0, _q = 0, _k = 1).  Masked scores get no
     * gradient; rows the forward found fully masked (lse = -inf) get dq = 0 and contribute nothing to dk, dv. */
    const uint8_t* mask;
    int64_t mask_stride_b, mask_stride_h, mask_stride_q, mask_stride_k;
    /* ABI v5: dtype = PFA_DTYPE_FP32 (all tensors fp32, strides multiples of 4 elements, `delta` unused) runs the fp32 backward
     * kernels; only they take the forward's dropout keep-mask (see pfa_fa3_args.drop_mask). */
    const uint8_t* drop_mask;
    float   drop_scale;
    int32_t kv_group;           /* ABI v7 (was reserved1, must-be-0): grouped-query heads as in pfa_fa3_args.kv_group -- k, v, dk, dv hold
                                 * H / kv_group heads; dK / dV are summed over each group inside the kernel.  0 or 1 = none.  16-bit operands only. */
    /* ABI v7: optional scratch for an ELEMENT mask (16-bit operands; ignored for key-only masks): pfa_fa3_bwd_mask_workspace_bytes()
     * bytes.  pfa_fa3_bwd condenses the mask there into a word per row and 64-key tile, the same transposed (a word per key and 64-row
     * tile) and the tile ranges that hold visible entries: the kernels then read one word per tile instead of a mask byte per score and
     * run only the tiles a structured mask (a band, a triangle, documents) leaves visible.  NULL / too small: the byte paths, same result. */
    void*   mask_workspace;
    size_t  mask_workspace_bytes;
} pfa_fa3_bwd_args;

size_t pfa_fa3_bwd_workspace_bytes(const pfa_fa3_bwd_args* a);
size_t pfa_fa3_bwd_mask_workspace_bytes(const pfa_fa3_bwd_args* a);
int pfa_fa3_bwd(const pfa_fa3_bwd_args* a, void* stream);

/*
 * Kernel-selection introspection for tests/bench: writes the name of the kernel variant pfa_fa3_fwd
 * would launch for `a` into buf (NUL terminated, truncated to n) and returns the number of workgroups.
 */
int pfa_fa3_describe(const pfa_fa3_args* a, char* buf, size_t n);

/*
 * Decode over a KV cache (ABI v8), in the style of flash_attn_with_kvcache: a few new query rows per batch against the keys a cache
 * holds.  O[b,i,h,:] = softmax_j(scale * <Q[b,i,h,:], K[b,j,h/g,:]> + mask) V[b,j,h/g,:], g = H / Hkv.
 *
 *   q, o            [B, Sq, H, D] by element strides (last dim contiguous); 1 <= Sq <= 64; o in dtype_in or fp32
 *   k_cache/v_cache [B, Smax, Hkv, D] by element strides: HF's [B, Hkv, S, D] cache and a slice of a larger preallocated cache are other
 *                   strides.  Query head h reads K/V head h / (H / Hkv).
 *   cache_seqlens   optional int32 [B] on the device: valid keys of each batch (<= Smax; keys at and past it are never read).  NULL = Smax.
 *   key_mask        optional [B, Smax] bytes, 0 = masked (left padding, holes of a static cache); key_mask_stride_b bytes between batches.
 *   causal          1: BOTTOM-RIGHT aligned per batch -- row i sees key j iff j <= cache_seqlens[b] - Sq + i (chunked prefill, speculative
 *                   verification).  pfa_fa3_args.causal is top-left (j <= i).
 *   lse             optional fp32 [B, H, Sq] natural-log LSE.  A row with no visible key gets O = 0 and LSE = -inf.
 *
 * bf16 / fp16 operands, D in {64, 128}; q/k/v strides multiples of 8 elements, o strides of 4; base pointers 16-byte aligned.
 * Work is split over keys: each split writes fp32 partials (O, m, l) into `workspace` and a second launch combines them (no atomics:
 * bitwise reproducible).  pfa_fa3_decode_workspace_bytes() depends on the shapes (B, H, Hkv, Sq, Smax, D) only, never on the
 * device-side lengths, so a captured graph stays valid while cache_seqlens and the cache change between replays.  The workspace is
 * required when that size is non-zero (missing or too small: PFA_ERR_NULL).
 *
 * Paged cache (ABI v9), block_table != NULL: k_cache / v_cache point at pools [num_pages, page_size, Hkv, D] by element strides, where
 * k_stride_b / v_stride_b are the PAGE strides, *_stride_s the token stride inside a page and *_stride_h the head stride.  block_table is a
 * device int32 [B][max_pages] (block_table_stride_b entries between batches, >= max_pages): logical key j of batch b lives in page
 * block_table[b][j / page_size] at token j % page_size.  Smax is the LOGICAL capacity and must equal max_pages * page_size; cache_seqlens,
 * key_mask and causal keep their meaning over logical keys.  page_size must be a multiple of 64, so that a key tile never straddles a
 * page (pages of 16 or 32 keys are not supported).  Page ids are clamped to [0, num_pages - 1] in the kernel -- a bad table gives wrong
 * numbers, never an out-of-range address -- and entries at and past ceil(cache_seqlens[b] / page_size) are never read.  The workspace size
 * and the split count equal those of the contiguous call of the same (B, H, Hkv, Sq, Smax, D), and the result is bit for bit that of
 * the contiguous call on the gathered cache.  block_table == NULL is the contiguous call; page_size, num_pages and
 * block_table_stride_b must then be 0 (PFA_ERR_FLAGS).
 */
typedef struct pfa_fa3_decode_args {
    uint32_t size;              /* = sizeof(pfa_fa3_decode_args) */
    uint32_t flags;             /* must be 0 */
    const void* q;
    const void* k_cache;
    const void* v_cache;
    void*       o;
    float*      lse;
    const int32_t* cache_seqlens;
    const uint8_t* key_mask;
    int64_t q_stride_b, q_stride_h, q_stride_s;
    int64_t k_stride_b, k_stride_h, k_stride_s;
    int64_t v_stride_b, v_stride_h, v_stride_s;
    int64_t o_stride_b, o_stride_h, o_stride_s;
    int64_t key_mask_stride_b;
    int32_t B, H, Hkv, Sq, Smax, D;
    int32_t dtype_in;           /* PFA_DTYPE_BF16 | PFA_DTYPE_FP16 */
    int32_t dtype_out;          /* = dtype_in, or PFA_DTYPE_FP32 */
    int32_t causal;             /* bottom-right, see above */
    float   softmax_scale;
    int32_t device_id;
    int32_t reserved0;          /* must be 0 */
    void*   workspace;          /* pfa_fa3_decode_workspace_bytes() bytes */
    size_t  workspace_bytes;
    /* ABI v9: paged cache, see above.  NULL / 0: the contiguous cache. */
    const int32_t* block_table;
    int64_t block_table_stride_b;
    int32_t page_size;          /* keys per page, a multiple of 64 */
    int32_t num_pages;          /* pages in the pools */
} pfa_fa3_decode_args;

/* Scratch bytes pfa_fa3_decode needs for `a` (0: none); from shapes only.  0 also for arguments pfa_fa3_decode_check refuses. */
size_t pfa_fa3_decode_workspace_bytes(const pfa_fa3_decode_args* a);
/* Validate `a` without launching: PFA_OK or the error pfa_fa3_decode would return. */
int pfa_fa3_decode_check(const pfa_fa3_decode_args* a);
/* Enqueue the decode (one launch, plus the combine launch when the keys are split) on `stream`. */
int pfa_fa3_decode(const pfa_fa3_decode_args* a, void* stream);
/* Introspection for tests / tools: the kernel name ("_paged" appended with a block table) into buf (NUL terminated, truncated to n), the number of key splits into *nsplit
 * (may be NULL); returns the workgroups of the main launch, or a pfa_status. */
int pfa_fa3_decode_describe(const pfa_fa3_decode_args* a, char* buf, size_t n, int32_t* nsplit);

/*
 * Forward over a KV cache (ABI v9, additive): chunked prefill, the suffix of a prefix-cached prompt, speculative verification -- ANY number
 * of query rows against the keys a cache holds, on the 8-wave MFMA forward's schedule (256 rows per workgroup) instead of the decode's
 * bandwidth kernel.  Takes pfa_fa3_decode_args as pfa_fa3_decode does, contiguous or paged, with the same conventions (bottom-right
 * causal per batch, cache_seqlens on the device, grouped-query heads, page ids clamped, table entries at and past
 * ceil(cache_seqlens[b] / page_size) never read, a row with no visible key -> O = 0 and LSE = -inf) and the same field rules, except:
 *   - Sq is any value >= 1 (B * H * ceil(Sq / 256) workgroups, up to the grid limit);
 *   - key_mask must be NULL (PFA_ERR_FLAGS): key masks over the cache are out of scope here, pfa_fa3_decode takes them;
 *   - workspace / workspace_bytes are ignored: this call does not split the keys (pfa_fa3_prefill_split below does), one launch, no
 *     atomics (bitwise reproducible).
 * Keys at and past cache_seqlens[b] are never read (a cache's unfilled tail may hold anything, NaN included).  The grid depends on
 * shapes only, so a captured graph stays valid while lengths, table and cache change between replays.  A paged call returns the bits of
 * the contiguous call on the gathered cache.
 */
int pfa_fa3_prefill_check(const pfa_fa3_decode_args* a);
int pfa_fa3_prefill(const pfa_fa3_decode_args* a, void* stream);
/* Introspection: the kernel name ("_paged" appended with a block table) into buf (NUL terminated, truncated to n); returns the workgroups, or a pfa_status. */
int pfa_fa3_prefill_describe(const pfa_fa3_decode_args* a, char* buf, size_t n);

/*
 * Ragged forward over a KV cache (ABI v9, additive): pfa_fa3_prefill for batches whose sequences bring DIFFERENT numbers of query rows --
 * one step of continuous batching (a prompt chunk, a suffix behind shared prefix pages, a speculative verification and one-token decode
 * rows) in one launch.  The packed "varlen" form of flash-attn: the query rows of all sequences lie one after the other in one tensor and
 * cu_seqlens_q says where each sequence starts.  Same kernel schedule, cache conventions and field rules as pfa_fa3_prefill.
 *
 *   q, o            [total_q, H, D] by element strides *_stride_s (between packed rows) and *_stride_h (last dim contiguous); there is no
 *                   batch stride.  o in dtype_in or fp32.
 *   cu_seqlens_q    required int32 [B + 1] on the device, non-decreasing, cu[0] >= 0, cu[B] <= total_q: sequence b owns the packed rows
 *                   cu[b] .. cu[b + 1] - 1 (none if the two are equal).  Read by the kernel as s_b = clamp(cu[b], 0, total_q),
 *                   e_b = clamp(cu[b + 1], s_b, total_q), Sq_b = min(e_b - s_b, max_seqlen_q): bad values give wrong numbers, never an
 *                   address outside the packed tensors (the rule for page ids).
 *   max_seqlen_q    host bound on the rows of one sequence, 1 <= max_seqlen_q <= total_q.  It sizes the grid, B * H * ceil(max_seqlen_q /
 *                   256) workgroups from host shapes only, so a captured graph stays valid while cu_seqlens_q, cache_seqlens, the block
 *                   table and the cache change between replays.  Of a sequence with more rows only the first max_seqlen_q are computed
 *                   (as a sequence of max_seqlen_q rows); the others are left unwritten.
 *   k_cache/v_cache [B, Smax, Hkv, D] by element strides, or with block_table pools [num_pages, page_size, Hkv, D] where *_stride_b are
 *                   the PAGE strides, exactly as in pfa_fa3_decode_args.  Smax is then max_pages * page_size.
 *   cache_seqlens   optional int32 [B] on the device: valid keys of each sequence, its Sq_b new rows' own keys INCLUDED (append the
 *                   step's K / V first, then call).  NULL = Smax.  Keys at and past len_b = clamp(cache_seqlens[b], 0, Smax) and table
 *                   entries at and past ceil(len_b / page_size) are never read (an unfilled tail may hold anything, NaN included).
 *   causal          1: bottom-right aligned per sequence -- row i of sequence b sees key j iff j < len_b and j <= len_b - Sq_b + i.
 *                   0: every row sees the len_b keys.
 *   lse             optional fp32 [H, total_q] natural-log LSE: entry h * total_q + (cu[b] + i).
 * A row with no visible key (len_b = 0, or under causal the first Sq_b - len_b rows when len_b < Sq_b) gets O = 0 and LSE = -inf.
 * Packed rows no sequence covers -- gaps between sequences, the tail behind cu[B], rows of a sequence past max_seqlen_q -- are never
 * written, in O or in LSE.  A sequence with no rows costs its workgroups an immediate return.
 *
 * The result is bit for bit that of pfa_fa3_prefill called per sequence (B = 1, Sq = Sq_b) on that sequence's rows, cache and length; one
 * launch, no workspace, no atomics (bitwise reproducible).  A paged call returns the bits of the contiguous call on the gathered cache.
 *
 * Field rules: those of pfa_fa3_prefill where the fields coincide (D in {64, 128}, bf16 / fp16 operands, q / k / v strides multiples of 8
 * elements and o strides of 4, base pointers 16-byte aligned, paging fields all set or all zero), and: cu_seqlens_q NULL -> PFA_ERR_NULL,
 * not 4-byte aligned -> PFA_ERR_ALIGN; total_q < 1, max_seqlen_q < 1, max_seqlen_q > total_q or more workgroups than a grid holds ->
 * PFA_ERR_SHAPE.  There is no key mask.
 */
typedef struct pfa_fa3_prefill_varlen_args {
    uint32_t size;              /* = sizeof(pfa_fa3_prefill_varlen_args) */
    uint32_t flags;             /* must be 0 */
    const void* q;
    const void* k_cache;
    const void* v_cache;
    void*       o;
    float*      lse;
    const int32_t* cu_seqlens_q;
    const int32_t* cache_seqlens;
    int64_t q_stride_s, q_stride_h;
    int64_t o_stride_s, o_stride_h;
    int64_t k_stride_b, k_stride_h, k_stride_s;
    int64_t v_stride_b, v_stride_h, v_stride_s;
    int32_t B, H, Hkv, total_q, max_seqlen_q, Smax, D;
    int32_t dtype_in;           /* PFA_DTYPE_BF16 | PFA_DTYPE_FP16 */
    int32_t dtype_out;          /* = dtype_in, or PFA_DTYPE_FP32 */
    int32_t causal;             /* bottom-right per sequence, see above */
    float   softmax_scale;
    int32_t device_id;
    int32_t reserved0;          /* must be 0 */
    /* paged cache, as in pfa_fa3_decode_args.  NULL / 0: the contiguous cache. */
    const int32_t* block_table;
    int64_t block_table_stride_b;
    int32_t page_size;          /* keys per page, a multiple of 64 */
    int32_t num_pages;          /* pages in the pools */
} pfa_fa3_prefill_varlen_args;

/* Validate `a` without launching: PFA_OK or the error pfa_fa3_prefill_varlen would return. */
int pfa_fa3_prefill_varlen_check(const pfa_fa3_prefill_varlen_args* a);
/* Enqueue the ragged forward (one launch) on `stream`. */
int pfa_fa3_prefill_varlen(const pfa_fa3_prefill_varlen_args* a, void* stream);
/* Introspection: the kernel name (pfa_fa3_prefill_describe's with "_varlen" in front of any "_paged") into buf (NUL terminated, truncated
 * to n); returns the workgroups, or a pfa_status. */
int pfa_fa3_prefill_varlen_describe(const pfa_fa3_prefill_varlen_args* a, char* buf, size_t n);

/*
 * Per-call options of the three calls over a KV cache (ABI v9, additive): pfa_fa3_decode, pfa_fa3_prefill and pfa_fa3_prefill_varlen each
 * have *_ex twins that take their unchanged argument block plus this extension.  ext == NULL, or an extension whose window is 0, is
 * exactly the call without the extension: the same kernel function, grid and workspace size, the same bits.  The old entry points are
 * the new ones with ext = NULL.
 *
 * Sliding window.  window = W >= 1 (a host integer): a row sees at most W keys, its own diagonal key included -- Hugging Face's
 * sliding_window, flash-attn's window_size = (W - 1, 0).  With len_b the sequence's valid keys, Sq_b its query rows (Sq; the ragged
 * call: its own count) and off_b = len_b - Sq_b, row i of sequence b sees key j iff
 *       j < len_b   and   j <= i + off_b   and   j > i + off_b - W.
 * The window needs causal = 1 (causal = 0 with window > 0: PFA_ERR_FLAGS).  Rows with no visible key are the rows of len_b < Sq_b that
 * have none without a window either (O = 0, LSE = -inf); the window adds no others.  pfa_fa3_decode's key_mask combines with the window
 * by logical AND.  A window >= Smax hides nothing and returns the bits of the call without a window.
 *
 * What is never read, next to "keys at and past len_b and table entries at and past ceil(len_b / page_size)": let
 * lo_b = max(0, off_b - W + 1), the lowest key row 0 of the call can see.  Keys below floor64(lo_b) = lo_b rounded down to a multiple of
 * 64 are never read, and with a block table the entries below lo_b / page_size are never read (page_size is a multiple of 64: the same
 * boundary at page granularity) -- a server may hand the pages behind the window to other sequences and leave anything in those table
 * entries.  Keys in [floor64(lo_b), lo_b), and keys that lie inside a 64-key tile but below an individual row's bound, ARE read and
 * hidden by the score mask: they are live cache contents and must be finite.
 *
 * pfa_fa3_decode_ex splits [floor64(lo_b), len_b) over the key splits instead of [0, len_b), and picks the number of splits and the
 * workspace from the shapes and the host `window` alone (min(Smax, window + Sq - 1 rounded up to 64) stands where Smax does), so a
 * captured graph stays valid while lengths, table and cache change: ask pfa_fa3_decode_workspace_bytes_ex with the same ext.
 *
 * Field rules, after those of the argument block: size wrong -> PFA_ERR_STRUCT_SIZE; flags or reserved non-zero -> PFA_ERR_FLAGS;
 * window < 0 -> PFA_ERR_SHAPE; window > 0 with causal == 0 -> PFA_ERR_FLAGS.  *_describe_ex appends "_win" to the kernel's name (in
 * front of any "+combine", "_varlen" or "_paged") when a window is set.
 */
typedef struct pfa_fa3_cache_ext {
    uint32_t size;              /* = sizeof(pfa_fa3_cache_ext) */
    uint32_t flags;             /* must be 0 */
    int32_t  window;            /* 0: none; W >= 1: each row sees its last W keys, see above */
    int32_t  reserved;          /* must be 0 */
} pfa_fa3_cache_ext;

size_t pfa_fa3_decode_workspace_bytes_ex(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext);
int pfa_fa3_decode_check_ex(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext);
int pfa_fa3_decode_ex(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, void* stream);
int pfa_fa3_decode_describe_ex(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, char* buf, size_t n, int32_t* nsplit);
int pfa_fa3_prefill_check_ex(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext);
int pfa_fa3_prefill_ex(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, void* stream);
int pfa_fa3_prefill_describe_ex(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, char* buf, size_t n);
int pfa_fa3_prefill_varlen_check_ex(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext);
int pfa_fa3_prefill_varlen_ex(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, void* stream);
int pfa_fa3_prefill_varlen_describe_ex(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, char* buf, size_t n);

/*
 * Tree attention masks in the decode (ABI v9, additive): the verification step of speculative decoders that draft a TREE of tokens
 * (Medusa, EAGLE, SpecInfer).  The step's Sq <= 64 rows are the tree's nodes, appended to the cache like any step's rows; a node must
 * see the cached prefix and its own ancestors, but not its siblings.  pfa_fa3_cache_ext is full, so the mask comes in a block of its
 * own and through entry points of its own, pfa_fa3_decode_ex with one more argument.  tree == NULL is pfa_fa3_decode_ex in every
 * respect: status, workspace, kernel function, grid and bits.
 *
 * The rule.  With len_b the sequence's valid keys AFTER the step's Sq rows were appended and off_b = len_b - Sq, row i of sequence b
 * sees key j iff
 *       j < len_b   and   ( j < off_b   or   bit (j - off_b) of words[b * stride_b + i] is set ),
 * and, where a key_mask is given, the key mask allows j (logical AND).  Bits at and above Sq are ignored.  Nothing is required of the
 * pattern: no self bit, no ancestor order, bits above the diagonal are allowed.  The chain (word i = bits 0 .. i) is exactly the causal
 * rule and returns the bits of the causal call; all-ones is exactly causal = 0.  For len_b < Sq new row r has no key when
 * off_b + r < 0, and its bit selects nothing.  A row with no visible key (an empty word and no prefix) gets O = 0 and LSE = -inf, as
 * everywhere.
 *
 * What is never read is what the call without a tree never reads: keys at and past len_b, and table entries at and past
 * ceil(len_b / page_size).  Keys inside [off_b, len_b) that a word hides ARE read and hidden by the score mask: they are live cache
 * contents and must be finite (the statement the window makes about its boundary keys).  `words` is read once per workgroup lane,
 * Sq words per sequence.
 *
 * The number of key splits and the workspace are those of the call without a tree, a function of (B, H, Hkv, Sq, Smax, D) alone:
 * a captured graph replays while words, lengths, table and cache change.  Rotary positions: the fused rotary append rotates by row
 * index; a node's position is off_b + its depth, so the caller of a tree step rotates Q and K itself.
 *
 * Field rules, after those of the argument block and of ext, in this order: size wrong -> PFA_ERR_STRUCT_SIZE; flags non-zero ->
 * PFA_ERR_FLAGS; words NULL -> PFA_ERR_NULL; words not 8-byte aligned -> PFA_ERR_ALIGN; stride_b < Sq -> PFA_ERR_SHAPE; causal == 0 ->
 * PFA_ERR_FLAGS (the words replace the triangle and have no meaning without one); a window > 0 together with a tree -> PFA_ERR_FLAGS
 * (a node's window would be by depth, not by row index).  pfa_fa3_decode_tree_workspace_bytes takes no pointers and returns 0 for
 * what the other rules refuse.  *_describe appends "_tree" to the kernel's name where "_win" would stand.
 */
typedef struct pfa_fa3_tree_mask {
    uint32_t size;              /* = sizeof(pfa_fa3_tree_mask) */
    uint32_t flags;             /* must be 0 */
    const uint64_t* words;      /* device [B][stride_b], words[b * stride_b + i] for row i; 8-byte aligned */
    int64_t  stride_b;          /* words between sequences, >= Sq */
} pfa_fa3_tree_mask;

size_t pfa_fa3_decode_tree_workspace_bytes(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_tree_mask* tree);
int pfa_fa3_decode_tree_check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_tree_mask* tree);
int pfa_fa3_decode_tree(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_tree_mask* tree, void* stream);
int pfa_fa3_decode_tree_describe(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_tree_mask* tree, char* buf, size_t n,
                                 int32_t* nsplit);

/*
 * Forward over a KV cache with the keys split over workgroups (ABI v9, additive).  pfa_fa3_prefill launches B * H * ceil(Sq / 256)
 * workgroups and each walks every key its rows see: a short chunk of few sequences against a long cache (chunked prefill at B = 1, the
 * prefix pass of a shared-prefix step) leaves most of the chip idle.  These entry points take the unchanged pfa_fa3_decode_args plus a host
 * integer (pfa_fa3_cache_ext is full), cut every q block's keys into N ranges, run one workgroup per range and join the N fp32 partial
 * results with pfa_attn_merge.  Same conventions and field rules as pfa_fa3_prefill; there is no window and no ragged form.
 *
 *   key_splits      1 .. PFA_PREFILL_MAX_SPLITS: exactly that many splits.  0: the library's plan.  Anything else: PFA_ERR_SHAPE.
 *   the plan        pfa_fa3_prefill_split_plan returns the resolved count N in 1 .. 8 (or a negative pfa_status): key_splits itself, or for
 *                   0 the largest N that keeps B * H * ceil(Sq / 256) * N within 256 workgroups (one round of one D = 128 workgroup per
 *                   CU), capped by Smax / 1024 (a split holds at least 1024 keys of capacity) and by 8, and at least 1.  It is 1 when
 *                   B * H * ceil(Sq / 256) > 128 and when Smax is below 2048.  A function of (B, H, Sq, Smax, D) only -- never of
 *                   pointers, cache_seqlens, the block table or the page size -- so a captured graph stays valid while they change
 *                   and a paged call plans like the contiguous one.
 *   N = 1           the call IS pfa_fa3_prefill: the same kernel function, grid, field rules and bits.  No workspace (0 bytes; the
 *                   workspace fields are ignored).
 *   N > 1           one launch of B * H * ceil(Sq / 256) * N workgroups into `workspace`, then pfa_attn_merge of the N parts, in split
 *                   order, into o (dtype_out) and the optional lse.  Two launches, fixed order, no atomics (bitwise reproducible), no
 *                   host synchronisation, no allocation; both grids come from host shapes, so the pair is capturable.
 *   the split rule  a q block (256 rows) that would run n 64-key tiles unsplit -- n = ceil(len_b / 64), under causal
 *                   ceil(min(len_b, q0 + 256 + len_b - Sq) / 64) for the block whose first row is q0 -- gives split s the tiles
 *                   [s * per, min(n, (s + 1) * per)), per = ceil(n / N).  An empty range fetches nothing and contributes a part whose
 *                   LSE is -inf, which the merge skips.  The partial result of split s is bit for bit the fp32 result (and LSE) of
 *                   pfa_fa3_prefill over those keys alone, so the whole call equals pfa_attn_merge of N such calls.
 *   workspace       N * B * Sq * H * (D + 1) * 4 bytes (pfa_fa3_prefill_split_workspace_bytes; 0 for N = 1 and for refused shapes), 16-byte
 *                   aligned: partial O fp32 [N][B][Sq][H][D], then partial LSE fp32 [N][B][H][Sq].  Every byte of it is written.
 *   never read      keys at and past len_b; table entries at and past ceil(len_b / page_size); by a given workgroup, table entries
 *                   outside its own tiles (a split may begin in the middle of a page; page ids are clamped as always).
 * A paged call returns the bits of the contiguous call with the same N on the gathered cache.
 *
 * Field rules, in the order their errors are reported: those of pfa_fa3_prefill's argument block (pfa_fa3_decode_args above); key_mask set
 * -> PFA_ERR_FLAGS; key_splits outside 0 .. 8 -> PFA_ERR_SHAPE; B * H * ceil(Sq / 256) * N past 2^31 - 1 -> PFA_ERR_SHAPE; and for N > 1:
 * a 16-bit o whose strides are not multiples of 8 elements (the merge's rule, on top of the prefill's 4) -> PFA_ERR_STRIDE; workspace NULL or
 * smaller than the size above -> PFA_ERR_NULL; workspace not 16-byte aligned -> PFA_ERR_ALIGN; then what pfa_attn_merge_check says of the
 * merge (its grid: B * Sq * H * (D / 8) + 256 past 2^31 - 1 -> PFA_ERR_SHAPE).
 */
#define PFA_PREFILL_MAX_SPLITS 8      /* = PFA_MERGE_MAX_PARTS */
/* The resolved number of key splits, 1 .. 8, from shapes only; or a negative pfa_status (NULL, size, shape, head dim, key_splits). */
int pfa_fa3_prefill_split_plan(const pfa_fa3_decode_args* a, int32_t key_splits);
/* Scratch bytes pfa_fa3_prefill_split needs for (`a`, key_splits); from shapes only.  0 for one split and for what _plan refuses. */
size_t pfa_fa3_prefill_split_workspace_bytes(const pfa_fa3_decode_args* a, int32_t key_splits);
/* Validate without launching: PFA_OK or the error pfa_fa3_prefill_split would return. */
int pfa_fa3_prefill_split_check(const pfa_fa3_decode_args* a, int32_t key_splits);
/* Enqueue the forward (one split: pfa_fa3_prefill; else the split launch and the merge launch) on `stream`. */
int pfa_fa3_prefill_split(const pfa_fa3_decode_args* a, int32_t key_splits, void* stream);
/* Introspection: pfa_fa3_prefill_describe's name with "_split{N}+merge" in front of any "_paged" when N > 1, the resolved N into *nsplit
 * (may be NULL); returns the workgroups of the main launch, B * H * ceil(Sq / 256) * N, or a pfa_status. */
int pfa_fa3_prefill_split_describe(const pfa_fa3_decode_args* a, int32_t key_splits, char* buf, size_t n, int32_t* nsplit);

/*
 * Device-side KV-cache append (ABI v9, additive): the write side of a step over a KV cache.  Places the step's new K / V rows into a
 * contiguous or paged cache from device data alone, so that append + attention is two launches with no host round trip, capturable as
 * a whole -- what flash_attn_with_kvcache(k=, v=) does in front of its attention.
 *
 * Lengths are those AFTER the step, the convention of the three calls over a KV cache: one device cache_seqlens serves this call and
 * the attention call behind it.  The kernel never writes lengths, and a replay is idempotent.  For sequence b:
 *       len_b = clamp(cache_seqlens[b], 0, Smax)
 *       ragged  (cu_seqlens_q != NULL): s_b = clamp(cu[b], 0, total_new), e_b = clamp(cu[b + 1], s_b, total_new),
 *               Sq_b = min(e_b - s_b, max_seqlen_q) -- exactly pfa_fa3_prefill_varlen's clamps; row i is packed row s_b + i
 *       uniform (cu_seqlens_q == NULL): Sq_b = max_seqlen_q; row i is at b * *n_stride_b + i * *n_stride_s
 *       new row i (0 <= i < Sq_b) goes to logical key pos = len_b - Sq_b + i.
 *
 *   k_new, v_new    [total_new, Hkv, D] packed rows by *n_stride_s / *n_stride_h (last dim contiguous), or uniform [B, Sq, Hkv, D] with
 *                   *n_stride_b as well; total_new is the rows the tensors hold (ragged: >= max_seqlen_q; uniform: >= B * max_seqlen_q).
 *   k_cache/v_cache [B, Smax, Hkv, D] by element strides: dst = cache + b * stride_b + pos * stride_s + hk * stride_h.  With block_table,
 *                   pools [num_pages, page_size, Hkv, D] where *_stride_b are the PAGE strides, exactly as in pfa_fa3_decode_args: the row
 *                   goes to page block_table[b][pos / page_size] at token pos % page_size, and Smax is max_pages * page_size.
 *   cache_seqlens   REQUIRED int32 [B] on the device: valid keys of each sequence after the step, its new rows included.
 *   max_seqlen_q    host bound on the rows of one sequence.  It sizes the grid, B * ceil(max_seqlen_q * Hkv * (D / 8) / 256) workgroups
 *                   from host shapes only, so a captured graph stays valid while cu_seqlens_q, cache_seqlens, the block table and the
 *                   tensors change between replays.  Of a sequence with more rows only the first max_seqlen_q are written (at
 *                   len_b - max_seqlen_q + i: where the attention call, which computes only those rows, looks for them).
 *
 * Dropped, not written anywhere: rows with pos < 0 (a sequence with len_b < Sq_b: the rows the attention call gives O = 0), and on a
 * paged cache rows whose page id lies outside [0, num_pages - 1].  A write is NOT clamped into the pool as the reads are: a clamped read
 * gives wrong numbers, a clamped write would overwrite a live page of another sequence.  Bad device data loses rows; it never yields an
 * address outside the cache, the pools or the packed tensors.
 * Never read: packed rows no sequence covers -- gaps between sequences, the tail behind cu[B], rows of a sequence past max_seqlen_q --
 * and table entries other than those of the destination rows.  Never written: anything but the destination rows, in cache or pool
 * (lengths and table included).
 * If two sequences are given the same destination (a shared prefix page handed to two writers) the row ends up as one of the two.
 * Copy-on-write of shared pages is pfa_page_copy (below) in front of this call; PagedKVCache(copy_on_write=True) drives it.
 *
 * One launch; no workspace, no atomics, no LDS.  bf16 / fp16 (any 2-byte type moves the same way), D a multiple of 8 up to 256, strides
 * multiples of 8 elements, base pointers 16-byte aligned: K and V move as 16-byte loads and stores.
 *
 * Field rules, in the order their errors are reported: size wrong -> PFA_ERR_STRUCT_SIZE; flags / reserved0 / reserved1 non-zero ->
 * PFA_ERR_FLAGS; k_new, v_new, k_cache, v_cache or cache_seqlens NULL -> PFA_ERR_NULL; B, Hkv, Smax, total_new or max_seqlen_q < 1 ->
 * PFA_ERR_SHAPE; D not a multiple of 8 in [8, 256] -> PFA_ERR_HEAD_DIM; dtype not bf16 / fp16 -> PFA_ERR_DTYPE; a stride not a multiple
 * of 8, or a negative cache token stride -> PFA_ERR_STRIDE; a base not 16-byte aligned, cache_seqlens / cu_seqlens_q / block_table not
 * 4-byte aligned -> PFA_ERR_ALIGN; the paging fields as in pfa_fa3_decode_args (all zero without a table: PFA_ERR_FLAGS; page_size not a
 * multiple of 64, num_pages < 1, Smax not a multiple of page_size or block_table_stride_b < Smax / page_size: PFA_ERR_SHAPE); ragged
 * with a non-zero kn_stride_b / vn_stride_b -> PFA_ERR_FLAGS; ragged with max_seqlen_q > total_new, uniform with B * max_seqlen_q >
 * total_new, more workgroups than a grid holds or max_seqlen_q * Hkv * (D / 8) + 256 past 2^31 - 1 -> PFA_ERR_SHAPE.
 */
typedef struct pfa_kv_append_args {
    uint32_t size;              /* = sizeof(pfa_kv_append_args) */
    uint32_t flags;             /* must be 0 */
    const void* k_new;
    const void* v_new;
    void*       k_cache;
    void*       v_cache;
    const int32_t* cu_seqlens_q;   /* device [B + 1], or NULL = uniform */
    const int32_t* cache_seqlens;  /* device [B], required: lengths after the step */
    int64_t kn_stride_b, kn_stride_s, kn_stride_h;   /* *_b: uniform only, else 0 */
    int64_t vn_stride_b, vn_stride_s, vn_stride_h;
    int64_t k_stride_b, k_stride_h, k_stride_s;
    int64_t v_stride_b, v_stride_h, v_stride_s;
    int32_t B, Hkv, total_new, max_seqlen_q, Smax, D;
    int32_t dtype;              /* PFA_DTYPE_BF16 | PFA_DTYPE_FP16 */
    int32_t device_id;
    /* paged cache, as in pfa_fa3_decode_args.  NULL / 0: the contiguous cache. */
    const int32_t* block_table;
    int64_t block_table_stride_b;
    int32_t page_size;          /* keys per page, a multiple of 64 */
    int32_t num_pages;          /* pages in the pools */
    int32_t reserved0, reserved1;   /* must be 0 */
} pfa_kv_append_args;

/* Validate `a` without launching: PFA_OK or the error pfa_kv_append would return. */
int pfa_kv_append_check(const pfa_kv_append_args* a);
/* Enqueue the append (one launch) on `stream`. */
int pfa_kv_append(const pfa_kv_append_args* a, void* stream);
/* Introspection: the kernel name ("_varlen" appended with cu_seqlens_q, then "_paged" with a block table) into buf (NUL terminated,
 * truncated to n); returns the workgroups, or a pfa_status. */
int pfa_kv_append_describe(const pfa_kv_append_args* a, char* buf, size_t n);

/*
 * Rotary embedding fused into the KV-cache append (ABI v9, additive): pfa_kv_append that also rotates the step's Q and new K rows by
 * each row's position -- flash-attn's flash_attn_with_kvcache(k=, v=, rotary_cos=, rotary_sin=, rotary_interleaved=).  The position is
 * derived on the device from the data the append already reads, so rotary + append + attention is two launches with no host round
 * trip and replays as one graph.
 *
 * Sequences, lengths, clamps, drops and paging are exactly pfa_kv_append's (above): len_b, s_b, e_b, Sq_b, and new row i of sequence b
 * belongs to logical key pos = len_b - Sq_b + i.
 *
 *   position        p = clamp(pos + pos_offsets[b], 0, max_pos - 1), computed in 64 bits.  pos_offsets: optional device int32 [B], NULL =
 *                   all 0 (a cache whose leading tokens were evicted or left-padded).  An out-of-range position gives wrong numbers,
 *                   never an address outside the tables: the rule for page ids.
 *   rot_dim         R, a multiple of 16 with 16 <= R <= D; D a multiple of 16 with 16 <= D <= 256.  half = R / 2.  Elements at and past R
 *                   of every head are copied unchanged.
 *   cos, sin        fp32 [max_pos, half] device tables, row stride cs_stride elements (>= half, a multiple of 4), bases 16-byte aligned.
 *   pairing         default (half-rotated: Hugging Face rotate_half, NeoX, Llama): (x1, x2) = (x[j], x[j + half]), j < half;
 *                   PFA_ROPE_INTERLEAVED (GPT-J): (x1, x2) = (x[2j], x[2j + 1]).  With c = cos[p][j], s = sin[p][j]:
 *                       y1 = x1 * c - x2 * s        y2 = x2 * c + x1 * s
 *   arithmetic      operands widened to fp32; each product and the one add / subtract rounded to fp32 separately (no fused multiply-
 *                   add); the result converted round-to-nearest-even to the operand dtype.  Reproducible, and a plain-torch model
 *                   written as separate fp32 ops matches bit for bit.  (A NaN result is a NaN; its payload is not specified.)
 *   K               row i rotated and written where pfa_kv_append would write it, with the same drops: pos < 0, and on a paged cache a
 *                   page id outside [0, num_pages - 1].
 *   V               copied there unrotated.
 *   q, q_out        optional (both NULL, with H = 0: K / V only).  H heads, laid out as the step's rows: packed [total_new, H, D] by
 *                   *_stride_s / *_stride_h, or uniform [B, Sq, H, D] with *_stride_b as well.  Every one of the sequence's Sq_b rows is
 *                   rotated at its clamped p and written to q_out, rows with pos < 0 included (the attention call gives those O = 0
 *                   whatever Q holds).  q_out may be q itself (same pointer and strides: in place) or disjoint storage; partial overlap
 *                   is undefined.
 *   max_seqlen_q    sizes the grid as in pfa_kv_append: B * ceil(max_seqlen_q * (H + 2 * Hkv) * (D / 16) / 256) workgroups from host
 *                   shapes only, valid while cu_seqlens_q, cache_seqlens, pos_offsets, the block table, the tables' contents and the
 *                   tensors change between replays.
 *
 * Never read: packed rows no sequence covers, and table rows other than the p of a row that is processed.  Never written: anything but
 * the destination rows of the cache or pool and the covered rows of q_out (lengths, offsets and block table included), so a replay is
 * idempotent unless it runs in place on Q.
 *
 * One launch; no workspace, no atomics, no LDS.  Q, K and V move as 16-byte loads and stores; every source element is read by one
 * work item and every destination written by one, and an item reads all it needs before it writes.
 *
 * Field rules, in the order their errors are reported.  First pfa_kv_append's, in its order, where the fields coincide: size wrong ->
 * PFA_ERR_STRUCT_SIZE; reserved0 / reserved1 non-zero -> PFA_ERR_FLAGS; k_new, v_new, k_cache, v_cache or cache_seqlens NULL ->
 * PFA_ERR_NULL; B, Hkv, Smax, total_new or max_seqlen_q < 1 -> PFA_ERR_SHAPE; D not a multiple of 8 in [8, 256] -> PFA_ERR_HEAD_DIM; dtype
 * not bf16 / fp16 -> PFA_ERR_DTYPE; a kn / vn / k / v stride not a multiple of 8, or a negative cache token stride -> PFA_ERR_STRIDE;
 * k_new, v_new, k_cache or v_cache not 16-byte aligned, cache_seqlens / cu_seqlens_q / block_table not 4-byte aligned -> PFA_ERR_ALIGN;
 * the paging fields as in pfa_fa3_decode_args; ragged with a non-zero kn_stride_b / vn_stride_b -> PFA_ERR_FLAGS; ragged with max_seqlen_q
 * > total_new, uniform with B * max_seqlen_q > total_new -> PFA_ERR_SHAPE.  Then: flag bits other than PFA_ROPE_INTERLEAVED ->
 * PFA_ERR_FLAGS; cos or sin NULL -> PFA_ERR_NULL; exactly one of q / q_out NULL -> PFA_ERR_NULL; H < 1 with q -> PFA_ERR_SHAPE; H != 0
 * without q -> PFA_ERR_FLAGS; max_pos < 1 -> PFA_ERR_SHAPE; D not a multiple of 16 in [16, 256] or rot_dim not a multiple of 16 in
 * [16, D] -> PFA_ERR_HEAD_DIM; a q / qo stride not a multiple of 8, cs_stride not a multiple of 4 or < rot_dim / 2 -> PFA_ERR_STRIDE; q,
 * q_out, cos or sin not 16-byte aligned, pos_offsets not 4-byte aligned -> PFA_ERR_ALIGN; ragged with a non-zero q_stride_b /
 * qo_stride_b -> PFA_ERR_FLAGS; more workgroups than a grid holds or max_seqlen_q * (H + 2 * Hkv) * (D / 16) + 256 past 2^31 - 1 ->
 * PFA_ERR_SHAPE.
 */
#define PFA_ROPE_INTERLEAVED 0x1u   /* pfa_rope_append_args.flags: pair (x[2j], x[2j + 1]) instead of (x[j], x[j + rot_dim / 2]) */

typedef struct pfa_rope_append_args {
    uint32_t size;              /* = sizeof(pfa_rope_append_args) */
    uint32_t flags;             /* 0 | PFA_ROPE_INTERLEAVED */
    const void* q;              /* NULL with q_out NULL and H = 0: K / V only */
    void*       q_out;          /* may be q (in place) */
    const void* k_new;
    const void* v_new;
    void*       k_cache;
    void*       v_cache;
    const float* cos;           /* device fp32 [max_pos, rot_dim / 2] by cs_stride */
    const float* sin;
    const int32_t* cu_seqlens_q;   /* device [B + 1], or NULL = uniform */
    const int32_t* cache_seqlens;  /* device [B], required: lengths after the step */
    const int32_t* pos_offsets;    /* device [B], or NULL = 0 */
    int64_t q_stride_b, q_stride_s, q_stride_h;      /* *_b: uniform only, else 0 */
    int64_t qo_stride_b, qo_stride_s, qo_stride_h;   /* of q_out */
    int64_t kn_stride_b, kn_stride_s, kn_stride_h;
    int64_t vn_stride_b, vn_stride_s, vn_stride_h;
    int64_t k_stride_b, k_stride_h, k_stride_s;
    int64_t v_stride_b, v_stride_h, v_stride_s;
    int64_t cs_stride;          /* row stride of cos and of sin, in elements */
    int32_t B, H, Hkv, total_new, max_seqlen_q, Smax, D, rot_dim, max_pos;
    int32_t dtype;              /* PFA_DTYPE_BF16 | PFA_DTYPE_FP16 */
    int32_t device_id;
    int32_t reserved0;          /* must be 0 */
    /* paged cache, as in pfa_fa3_decode_args.  NULL / 0: the contiguous cache. */
    const int32_t* block_table;
    int64_t block_table_stride_b;
    int32_t page_size;          /* keys per page, a multiple of 64 */
    int32_t num_pages;          /* pages in the pools */
    int32_t reserved1;          /* must be 0 */
} pfa_rope_append_args;

/* Validate `a` without launching: PFA_OK or the error pfa_rope_append would return. */
int pfa_rope_append_check(const pfa_rope_append_args* a);
/* Enqueue the rotation and the append (one launch) on `stream`. */
int pfa_rope_append(const pfa_rope_append_args* a, void* stream);
/* Introspection: the kernel name rope_append_{bf16|fp16}_d{D}_r{rot_dim} ("_il" appended with PFA_ROPE_INTERLEAVED, then "_varlen" with
 * cu_seqlens_q, then "_paged" with a block table) into buf (NUL terminated, truncated to n); returns the workgroups, or a pfa_status. */
int pfa_rope_append_describe(const pfa_rope_append_args* a, char* buf, size_t n);

/*
 * Merge of partial attention results (ABI v9, additive).  N attention results over DISJOINT key sets -- each an O and the natural-log LSE
 * the calls over a KV cache return -- become the result over the union of the keys: FlashInfer's merge_state, vLLM's
 * merge_attn_states.  For every row (b, i, h), in fp32 and in part order n = 0 .. N - 1:
 *       m    = max_n lse_n                    over the parts whose lse_n > -inf
 *       w_n  = exp(lse_n - m),   s = sum_n w_n
 *       O[d] = (sum_n w_n * O_n[d]) / s,      LSE = m + log(s)
 *   -inf            a part whose LSE is -inf (a row with no visible key there) is SKIPPED, not multiplied by zero: its O may hold
 *                   anything, NaN included, and does not reach the result.  If every part is -inf: O = 0 and LSE = -inf, the library's
 *                   row with no visible key.
 *   NaN             a NaN LSE gives a NaN row (O and LSE).
 *   rows            are independent: garbage in one input row stays in that row.
 *   reproducible    no atomics, fixed order: two runs give the same bits.
 *   exact           merging one finite part with parts that are all -inf returns that part's LSE bit for bit and its O bit for bit
 *                   (fp32 output) or rounded once (16-bit output): exp(0) = 1 and log(1) = 0 are exact in the hardware
 *                   transcendentals the kernel uses, and it divides by s itself (no epsilon, no reciprocal).
 *
 *   n_parts         N, 2 <= N <= PFA_MERGE_MAX_PARTS.  Array entries at and past N are ignored.
 *   o_part[n]       [B, Sq, H, D] by element strides op_stride_b / _h / _s[n] (last dim contiguous), dtype_part (one for all parts:
 *                   bf16, fp16 or fp32).
 *   lse_part[n]     fp32, entry (b, h, i) at lp_stride_b[n] * b + lp_stride_h[n] * h + lp_stride_s[n] * i.  Any strides: the parts of
 *                   one merge come from calls with different layouts -- [B, H, Sq]; one call over all B * Sq rows as one sequence,
 *                   [1, H, B * Sq] (strides Sq, B * Sq, 1); the ragged call's [H, total_q] (B = 1, Sq = total_q).
 *   o               [B, Sq, H, D] by element strides, dtype_out: bf16, fp16 or fp32; with 16-bit parts dtype_part or fp32.  16-bit
 *                   output is converted round-to-nearest-even.  o must not overlap a part (undefined).
 *   lse_out         optional fp32 by lo_stride_b / _h / _s, as lse_part; NULL: not written.
 * Nothing but the B * Sq * H rows of o and lse_out is written.
 *
 * One launch of a memory-bound kernel: ceil(B * Sq * H * (D / 8) / 256) workgroups from host shapes only, so a captured graph stays
 * valid while the tensors' contents change.  No workspace, no LDS.
 *
 * Field rules, in the order their errors are reported: size wrong -> PFA_ERR_STRUCT_SIZE; flags / reserved0 / reserved1 non-zero ->
 * PFA_ERR_FLAGS; o, or o_part[n] / lse_part[n] of a part n < min(n_parts, PFA_MERGE_MAX_PARTS), NULL -> PFA_ERR_NULL; n_parts outside
 * [2, PFA_MERGE_MAX_PARTS], B, H or Sq < 1 -> PFA_ERR_SHAPE; D not a multiple of 8 in [8, 256] -> PFA_ERR_HEAD_DIM; dtype_part or
 * dtype_out not bf16 / fp16 / fp32, or 16-bit parts with a dtype_out that is neither dtype_part nor fp32 -> PFA_ERR_DTYPE; an op_stride
 * or o_stride not a multiple of 8 elements (16-bit tensor) or of 4 (fp32 tensor) -> PFA_ERR_STRIDE; o or an o_part not 16-byte aligned,
 * lse_out or an lse_part not 4-byte aligned -> PFA_ERR_ALIGN; B * Sq * H * (D / 8) + 256 past 2^31 - 1 (the grid and the item index) ->
 * PFA_ERR_SHAPE.
 */
#define PFA_MERGE_MAX_PARTS 8

typedef struct pfa_attn_merge_args {
    uint32_t size;              /* = sizeof(pfa_attn_merge_args) */
    uint32_t flags;             /* must be 0 */
    const void*  o_part[PFA_MERGE_MAX_PARTS];
    const float* lse_part[PFA_MERGE_MAX_PARTS];
    void*        o;
    float*       lse_out;       /* optional */
    int64_t op_stride_b[PFA_MERGE_MAX_PARTS], op_stride_h[PFA_MERGE_MAX_PARTS], op_stride_s[PFA_MERGE_MAX_PARTS];
    int64_t lp_stride_b[PFA_MERGE_MAX_PARTS], lp_stride_h[PFA_MERGE_MAX_PARTS], lp_stride_s[PFA_MERGE_MAX_PARTS];
    int64_t o_stride_b, o_stride_h, o_stride_s;
    int64_t lo_stride_b, lo_stride_h, lo_stride_s;
    int32_t n_parts, B, H, Sq, D;
    int32_t dtype_part;         /* PFA_DTYPE_BF16 | PFA_DTYPE_FP16 | PFA_DTYPE_FP32, of every o_part */
    int32_t dtype_out;          /* any of the three; with 16-bit parts: = dtype_part, or PFA_DTYPE_FP32 */
    int32_t device_id;
    int32_t reserved0, reserved1;   /* must be 0 */
} pfa_attn_merge_args;

/* Validate `a` without launching: PFA_OK or the error pfa_attn_merge would return. */
int pfa_attn_merge_check(const pfa_attn_merge_args* a);
/* Enqueue the merge (one launch) on `stream`. */
int pfa_attn_merge(const pfa_attn_merge_args* a, void* stream);
/* Introspection: the kernel name attn_merge_{bf16|fp16|fp32}_{bf16|fp16|fp32}_d{D}_n{N} (part dtype, then output dtype) into buf (NUL
 * terminated, truncated to n); returns the workgroups, or a pfa_status. */
int pfa_attn_merge_describe(const pfa_attn_merge_args* a, char* buf, size_t n);

/*
 * Page copy inside a paged KV cache's pools (ABI v9, additive): the data movement of copy-on-write.  Copies whole or partial pages of
 * the K pool and of the V pool from a device pair list -- what vLLM's copy_blocks does -- so that the first write of a sequence forked
 * from another (parallel sampling, beam search, a cached prefix) costs one launch and no host round trip, capturable with the step.
 *
 * Pair i is (s, d) = (pairs[i * pairs_stride], pairs[i * pairs_stride + 1]).
 *   - The pair is EMPTY when s or d lies outside [0, num_pages - 1], or when s == d; -1 is the documented "no copy" marker.  An empty
 *     pair reads nothing and writes nothing.
 *   - Otherwise tokens [0, r_i) of K page s go to K page d, and the same for V: r_i = page_size when rows is NULL, else
 *     r_i = clamp(rows[i], 0, page_size).  Tokens >= r_i of page d are not written.
 * Bad device data can lose a copy; it never yields an address outside the pools (s and d are range-checked, r_i is clamped).
 * The caller promises: no page is the destination of two non-empty pairs, no destination is the source of another non-empty pair, and
 * the pages of a pool do not overlap.  Under that promise a replay is idempotent.  Breaking it leaves a destination as one of the
 * candidate values, with every address still inside the pools.
 *
 *   k_pool, v_pool  pools [num_pages, page_size, Hkv, D] by element strides (last dim contiguous), *_stride_b the PAGE strides exactly
 *                   as pfa_kv_append_args gives them: token t of head hk of page g is at pool + g * stride_b + t * stride_s + hk * stride_h.
 *                   Head-major and token-major (flash-attn) pools both work.
 *   pairs           int32 device [n_pairs][2], rows pairs_stride (>= 2) elements apart.
 *   rows            int32 device [n_pairs], or NULL = whole pages.
 *
 * One launch of n_pairs * ceil(page_size * Hkv * (D / 8) / 1024) workgroups, from host shapes only: a captured graph stays valid while
 * pairs, rows and the pools change between replays, and the workgroups of an empty pair return before any vector memory instruction.
 * No workspace, no atomics, no LDS.  bf16 / fp16 (any 2-byte type moves the same way): K and V move as 16-byte loads and stores.
 *
 * Field rules, in the order their errors are reported: size wrong -> PFA_ERR_STRUCT_SIZE; flags / reserved0 non-zero -> PFA_ERR_FLAGS;
 * k_pool, v_pool or pairs NULL -> PFA_ERR_NULL; n_pairs, Hkv or num_pages < 1, or page_size not a positive multiple of 64 ->
 * PFA_ERR_SHAPE; D not a multiple of 8 in [8, 256] -> PFA_ERR_HEAD_DIM; dtype not bf16 / fp16 -> PFA_ERR_DTYPE; a pool stride not a
 * multiple of 8, a negative token stride, or pairs_stride < 2 -> PFA_ERR_STRIDE; a pool base not 16-byte aligned, pairs / rows not
 * 4-byte aligned -> PFA_ERR_ALIGN; more workgroups than a grid holds, or page_size * Hkv * (D / 8) + 1024 past 2^31 - 1 -> PFA_ERR_SHAPE.
 */
typedef struct pfa_page_copy_args {
    uint32_t size;              /* = sizeof(pfa_page_copy_args) */
    uint32_t flags;             /* must be 0 */
    void* k_pool;
    void* v_pool;
    const int32_t* pairs;       /* device [n_pairs][2] = (src, dst), row stride pairs_stride (>= 2) */
    const int32_t* rows;        /* device [n_pairs], or NULL = whole pages */
    int64_t pairs_stride;
    int64_t k_stride_b, k_stride_h, k_stride_s;   /* page, head, token */
    int64_t v_stride_b, v_stride_h, v_stride_s;
    int32_t n_pairs, Hkv, D, page_size, num_pages;
    int32_t dtype;              /* PFA_DTYPE_BF16 | PFA_DTYPE_FP16 */
    int32_t device_id;
    int32_t reserved0;          /* must be 0 */
} pfa_page_copy_args;

/* Validate `a` without launching: PFA_OK or the error pfa_page_copy would return. */
int pfa_page_copy_check(const pfa_page_copy_args* a);
/* Enqueue the copy (one launch) on `stream`. */
int pfa_page_copy(const pfa_page_copy_args* a, void* stream);
/* Introspection: the kernel name page_copy_{bf16|fp16}_d{D} ("_rows" appended with rows) into buf (NUL terminated, truncated to n);
 * returns the workgroups, or a pfa_status. */
int pfa_page_copy_describe(const pfa_page_copy_args* a, char* buf, size_t n);

/*
 * Packed variable-length attention for training, forward and backward (ABI v9, additive): pfa_fa3_fwd / pfa_fa3_bwd for a batch of
 * sequences of DIFFERENT lengths that is not padded -- flash-attn's flash_attn_varlen_func.  The rows of all sequences lie one after the
 * other in one tensor per operand and two cu_seqlens arrays say where each sequence's query rows and keys start.  The kernels are the
 * dense 16-bit ones (the 8-wave forward, the dQ and the dK/dV kernel) in their packed mode: same tiles, same arithmetic.
 *
 *   q, o, dout, dq  [total_q, H, D] by element strides *_stride_s (between packed rows) and *_stride_h (last dim contiguous); there is
 *                   no batch stride.  o in dtype_in or fp32; dq / dk / dv in dtype or fp32.
 *   k, v, dk, dv    [total_k, Hkv, D] likewise.  Grouped-query heads: H % Hkv == 0, query head h reads K/V head h / (H / Hkv); dK / dV
 *                   are summed over each group inside the kernel.
 *   cu_seqlens_q    required int32 [B + 1] on the device, non-decreasing, cu[0] >= 0, cu[B] <= total_q: sequence b owns the packed rows
 *   cu_seqlens_k    cu[b] .. cu[b + 1] - 1 (none if the two are equal); cu_seqlens_k likewise for the keys, against total_k.  Read by
 *                   the kernels as s_b = clamp(cu[b], 0, total), e_b = clamp(cu[b + 1], s_b, total), S_b = min(e_b - s_b, max_seqlen):
 *                   bad values give wrong numbers, never an address outside the packed tensors (the rule of
 *                   pfa_fa3_prefill_varlen_args).  The sequence's offset s_b * stride_s is added to the 64-bit base pointers; buffer
 *                   descriptors end at the sequence's own last row, so a neighbouring sequence is never loaded and never written.
 *   max_seqlen_q    host bounds on the rows / keys of one sequence, 1 <= max_seqlen_* <= total_*.  They size the grids from host shapes
 *   max_seqlen_k    only -- forward and dQ: B * H * ceil(max_seqlen_q / 256) workgroups, dK/dV: B * Hkv * ceil(max_seqlen_k / 128) -- so
 *                   a captured graph stays valid while the contents of the cu_seqlens arrays change between replays.  Of a longer
 *                   sequence only the first max_seqlen rows / keys take part; the others are neither read nor written.
 *   causal          1: the DENSE rule, top-left aligned per sequence -- row i of sequence b sees key j iff j <= i.  This is not the
 *                   bottom-right rule of the calls over a KV cache; for packed self-attention (cu_seqlens_k is cu_seqlens_q) the two
 *                   coincide.  0: every row sees its sequence's Sk_b keys.
 *   lse, delta      fp32 [H, total_q], entry h * total_q + (s_b + i): the layout of pfa_fa3_prefill_varlen and of flash-attn.  lse is
 *                   optional in the forward and required in the backward; delta is the backward's scratch of
 *                   pfa_fa3_varlen_bwd_workspace_bytes() bytes.
 * A row with no visible key (Sk_b = 0) gets O = 0, LSE = -inf and dQ = 0.  Keys no row sees (Sq_b = 0, or under causal the keys
 * j >= Sq_b) get dK = dV = exactly 0.  Every row of dQ in [s_b, s_b + Sq_b) and every row of dK / dV in [s_b, s_b + Sk_b) is written
 * exactly once, so the gradient buffers may be uninitialised.  Packed rows no sequence covers -- gaps between sequences, the tail behind
 * cu[B], rows past max_seqlen -- are never read or written.  A workgroup without rows (keys) of its sequence returns at once.
 *
 * The results are bit for bit those of pfa_fa3_fwd (8-wave kernel, selector 44) and pfa_fa3_bwd called per sequence on that sequence's
 * rows alone; no atomics, bitwise reproducible.  dtype_out = fp32 selects split P (P carried as hi + lo), as ops.fa3_forward does.
 *
 * Out of scope (use the dense calls): key and element masks, seqlens_k, dropout, the exact-fp32 kernels, split-P selection other than
 * through dtype_out, the persistent assembly forward and the 4-wave forward -- the packed forward runs on the 8-wave schedule only.
 *
 * Field rules: those of pfa_fa3_fwd / pfa_fa3_bwd where the fields coincide (D in {64, 128}, bf16 / fp16 operands, output and gradients
 * in the operand dtype or fp32, strides multiples of 8 elements -- 4 for fp32 outputs --, base pointers 16-byte aligned, int32 / fp32
 * arrays 4-byte aligned, one sequence's slab of max_seqlen rows at the row stride inside the 32-bit descriptor, k / v rows forward), and:
 * a NULL cu_seqlens pointer -> PFA_ERR_NULL; total_* < 1, max_seqlen_* < 1, max_seqlen_* > total_*, H % Hkv != 0 or more workgroups than
 * a grid holds -> PFA_ERR_SHAPE; flags or reserved0 not 0 -> PFA_ERR_FLAGS.
 */
typedef struct pfa_fa3_varlen_args {
    uint32_t size;              /* = sizeof(pfa_fa3_varlen_args) */
    uint32_t flags;             /* must be 0 */
    const void* q;
    const void* k;
    const void* v;
    void*       o;
    float*      lse;            /* optional [H, total_q] */
    const int32_t* cu_seqlens_q;
    const int32_t* cu_seqlens_k;
    int64_t q_stride_s, q_stride_h;
    int64_t k_stride_s, k_stride_h;
    int64_t v_stride_s, v_stride_h;
    int64_t o_stride_s, o_stride_h;
    int32_t B, H, Hkv, total_q, total_k, max_seqlen_q, max_seqlen_k, D;
    int32_t dtype_in;           /* PFA_DTYPE_BF16 | PFA_DTYPE_FP16 */
    int32_t dtype_out;          /* = dtype_in, or PFA_DTYPE_FP32 (split P) */
    int32_t causal;             /* top-left per sequence, see above */
    float   softmax_scale;
    int32_t device_id;
    int32_t reserved0;          /* must be 0 */
} pfa_fa3_varlen_args;

/* Validate `a` without launching: PFA_OK or the error pfa_fa3_varlen_fwd would return. */
int pfa_fa3_varlen_check(const pfa_fa3_varlen_args* a);
/* Enqueue the packed forward (one launch) on `stream`. */
int pfa_fa3_varlen_fwd(const pfa_fa3_varlen_args* a, void* stream);
/* Introspection: the kernel name fa3_fwd_varlen_{bf16|fp16}_d{D}_{causal|full}[_splitp]_{o16|o32} into buf (NUL terminated, truncated
 * to n); returns the workgroups, or a pfa_status. */
int pfa_fa3_varlen_describe(const pfa_fa3_varlen_args* a, char* buf, size_t n);

typedef struct pfa_fa3_varlen_bwd_args {
    uint32_t size;              /* = sizeof(pfa_fa3_varlen_bwd_args) */
    uint32_t flags;             /* must be 0 */
    const void* q;
    const void* k;
    const void* v;
    const void* o;              /* forward output, in `dtype` */
    const void* dout;           /* gradient of the forward output, in `dtype` */
    const float* lse;           /* [H, total_q] from the forward */
    void* dq;
    void* dk;
    void* dv;
    float* delta;               /* scratch [H, total_q] */
    const int32_t* cu_seqlens_q;
    const int32_t* cu_seqlens_k;
    int64_t q_stride_s, q_stride_h;
    int64_t k_stride_s, k_stride_h;
    int64_t v_stride_s, v_stride_h;
    int64_t o_stride_s, o_stride_h;
    int64_t do_stride_s, do_stride_h;
    int64_t dq_stride_s, dq_stride_h;
    int64_t dk_stride_s, dk_stride_h;
    int64_t dv_stride_s, dv_stride_h;
    int32_t B, H, Hkv, total_q, total_k, max_seqlen_q, max_seqlen_k, D;
    int32_t dtype;              /* PFA_DTYPE_BF16 | PFA_DTYPE_FP16: q, k, v, o, dout */
    int32_t dtype_grad;         /* = dtype, or PFA_DTYPE_FP32: dq, dk, dv */
    int32_t causal;
    float   softmax_scale;
    int32_t device_id;
    int32_t reserved0;          /* must be 0 */
} pfa_fa3_varlen_bwd_args;

/* Bytes of `delta`: H * total_q fp32 (0 for a NULL or shapeless block). */
size_t pfa_fa3_varlen_bwd_workspace_bytes(const pfa_fa3_varlen_bwd_args* a);
/* Validate `a` without launching: PFA_OK or the error pfa_fa3_varlen_bwd would return. */
int pfa_fa3_varlen_bwd_check(const pfa_fa3_varlen_bwd_args* a);
/* Enqueue the packed backward (two launches: dQ, which also leaves delta, then dK/dV) on `stream`. */
int pfa_fa3_varlen_bwd(const pfa_fa3_varlen_bwd_args* a, void* stream);
/* Introspection: "fa3_bwd_dq_varlen_<tag>+fa3_bwd_dkdv_varlen_<tag>", <tag> = {bf16|fp16}_d{D}_{causal|full}_{g16|g32}, into buf (NUL
 * terminated, truncated to n); returns the dQ launch's workgroups and, in *dkdv_workgroups (may be NULL), the dK/dV launch's; or a
 * pfa_status. */
int pfa_fa3_varlen_bwd_describe(const pfa_fa3_varlen_bwd_args* a, char* buf, size_t n, int32_t* dkdv_workgroups);

/*
 * FP8 (e4m3fn) KV cache (ABI v9, additive): pfa_fa3_decode over a cache of one-byte elements, and the append that quantises a step's
 * 16-bit rows into it.  An 8-bit cache halves the bytes a decode step streams and doubles the keys a page pool holds.
 *
 * The cache tensors of the argument block (k_cache / v_cache, contiguous or the paged pools) hold OCP e4m3fn bytes; their strides are in
 * elements, which are bytes.  Everything else in the block keeps its meaning: dtype_in (dtype of pfa_kv_append_args) stays the 16-bit
 * type of q (of k_new / v_new).  Value of a cache element: e4m3(byte) * descale, with one fp32 descale per (sequence, K/V head),
 *       k_descale[b * descale_stride_b + hk],   v_descale[b * descale_stride_b + hk]
 * on the device; descale_stride_b = 0 gives every sequence the same row of Hkv values (what a paged cache with shared pages needs).
 *
 * pfa_fa3_decode_q8: pfa_fa3_decode_ex of the dequantised cache.  K and V bytes are converted to q's type in registers (exact: every e4m3
 * value is a bf16 and an fp16 value) in front of the same 16-bit MFMA; k_descale multiplies softmax_scale, v_descale the output once.
 * Split rule, key mask, bottom-right causal, paging, partials and the O = 0 / LSE = -inf rule of rows with no visible key are those of
 * pfa_fa3_decode; with all descales 1 the result has the bits of pfa_fa3_decode on the converted cache.  The number of key splits and
 * the workspace are those of pfa_fa3_decode for the same shapes, so a captured graph stays valid while lengths, table, cache and the
 * descales' CONTENTS change.  `ext` may be NULL or carry window = 0: a window does not combine with the FP8 cache here, nor does a tree.
 * Bytes at and past a sequence's length are never converted into a result (0x7f there is harmless); NaN bytes below it give NaN.
 *
 * pfa_kv_append_q8: pfa_kv_append's placement (position len_b - Sq_b + i; rows in front of key 0 and rows whose page id lies outside
 * the pool are dropped; the grid comes from host shapes; lengths are never written), each 16-bit source element x stored as
 *       e4m3fn( clamp( float(x) / descale[b, hk], -448, 448 ) )
 * with an IEEE fp32 division and round-to-nearest-even; NaN stays NaN (0x7f or 0xff).  A work item is 16 elements: 32 bytes loaded, 16
 * stored.  D a multiple of 16 up to 256.
 *
 * Field rules of both calls, in the order their errors are reported: `a` NULL -> PFA_ERR_NULL, a->size wrong -> PFA_ERR_STRUCT_SIZE (the
 * rules below read the block); quant NULL -> PFA_ERR_NULL; quant->size wrong -> PFA_ERR_STRUCT_SIZE; quant->flags or reserved non-zero ->
 * PFA_ERR_FLAGS; kv_dtype other than PFA_DTYPE_FP8_E4M3 -> PFA_ERR_DTYPE; k_descale or v_descale NULL -> PFA_ERR_NULL; either not 4-byte
 * aligned -> PFA_ERR_ALIGN; descale_stride_b neither 0 nor >= Hkv -> PFA_ERR_STRIDE; a cache stride not a multiple of 16 elements, or a
 * negative cache token stride -> PFA_ERR_STRIDE; k_cache or v_cache not 16-byte aligned -> PFA_ERR_ALIGN; (decode) ext->window > 0 ->
 * PFA_ERR_FLAGS, (append) D not a multiple of 16 -> PFA_ERR_HEAD_DIM; then the unchanged rules of pfa_fa3_decode_ex / pfa_kv_append.
 * The workspace query takes no pointers and skips the pointer and stride rules.
 */
typedef struct pfa_fa3_kv_quant {
    uint32_t size;              /* = sizeof(pfa_fa3_kv_quant) */
    uint32_t flags;             /* must be 0 */
    int32_t kv_dtype;           /* PFA_DTYPE_FP8_E4M3 */
    int32_t reserved;           /* must be 0 */
    const float* k_descale;     /* device fp32 [B or 1][Hkv] */
    const float* v_descale;
    int64_t descale_stride_b;   /* elements between sequences; 0: one row for all */
} pfa_fa3_kv_quant;

size_t pfa_fa3_decode_q8_workspace_bytes(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant);
int pfa_fa3_decode_q8_check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant);
int pfa_fa3_decode_q8(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant, void* stream);
/* As pfa_fa3_decode_describe_ex; "_kv8" is appended to the kernel's name (in front of "+combine" and "_paged"). */
int pfa_fa3_decode_q8_describe(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant, char* buf, size_t n,
                               int32_t* nsplit);
int pfa_kv_append_q8_check(const pfa_kv_append_args* a, const pfa_fa3_kv_quant* quant);
int pfa_kv_append_q8(const pfa_kv_append_args* a, const pfa_fa3_kv_quant* quant, void* stream);

/*
 * The forward over an FP8 (e4m3fn) KV cache (ABI v9, additive): pfa_fa3_prefill_ex and pfa_fa3_prefill_varlen_ex of the dequantised
 * cache -- any number of query rows per sequence, uniform or ragged, contiguous or paged.  The argument blocks, the cache layout (one
 * byte per element, strides in elements = bytes) and pfa_fa3_kv_quant are those of pfa_fa3_decode_q8 above.
 *
 * K and V tiles are loaded as bytes, converted to q's type in registers (exact) and written into the LDS tile images the 16-bit kernel
 * builds by LDS-DMA; everything behind the images is the 16-bit kernel's one code path.  k_descale multiplies softmax_scale, v_descale
 * the output once: with all descales 1 the result has the bits of pfa_fa3_prefill_ex (pfa_fa3_prefill_varlen_ex) on the converted
 * cache.  Length and causal rules, paging, the O = 0 / LSE = -inf rule and the workgroups (from host shapes only: B * H *
 * ceil(Sq / 256)) are the 16-bit call's: a captured graph stays valid while lengths, cu_seqlens_q, table, cache and the descales'
 * CONTENTS change.  No workspace, no atomics.  `ext` may be NULL or carry window = 0: a window does not combine with the FP8 cache
 * here, nor does the split over keys (pfa_fa3_prefill_split).  Rows at and past a sequence's length read as +0 and table entries at
 * and past ceil(len_b / page_size) are never read (0x7f bytes there are harmless); NaN bytes below a length give NaN.
 *
 * Field rules, in the order their errors are reported: `a` NULL -> PFA_ERR_NULL, a->size wrong -> PFA_ERR_STRUCT_SIZE; the rules of
 * pfa_fa3_kv_quant as listed above (through the cache alignment); ext->window > 0 -> PFA_ERR_FLAGS; then the unchanged rules of
 * pfa_fa3_prefill_check_ex / pfa_fa3_prefill_varlen_check_ex, which these calls ask (a key mask -> PFA_ERR_FLAGS, as there).
 */
int pfa_fa3_prefill_q8_check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant);
int pfa_fa3_prefill_q8(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant, void* stream);
/* As pfa_fa3_prefill_describe_ex: "fa3_prefill_..._kv8[_varlen][_paged]" into buf -> the 16-bit call's workgroups, or a pfa_status. */
int pfa_fa3_prefill_q8_describe(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant, char* buf, size_t n);
int pfa_fa3_prefill_varlen_q8_check(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant);
int pfa_fa3_prefill_varlen_q8(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant, void* stream);
int pfa_fa3_prefill_varlen_q8_describe(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant,
                                       char* buf, size_t n);

/*
 * Attention sinks over a 16-bit KV cache (ABI v9, additive): pfa_fa3_decode_ex, pfa_fa3_prefill_ex, pfa_fa3_prefill_varlen_ex and
 * pfa_fa3_prefill_split with one learned value per QUERY head in every row's softmax denominator (the GPT-OSS-style layer: grouped
 * heads, D = 64, full and sliding-window layers, a sink per head).  pfa_fa3_cache_ext is full, so the sink has a block of its own.
 *
 * sinks[h] is in the units of the scaled scores x_ij = softmax_scale * <q_i, k_j> (natural log); it is NOT multiplied by
 * softmax_scale.  With V_i the keys row i of head h sees after lengths, causal rule, window and key mask:
 *     den_i = sum_{j in V_i} exp(x_ij) + exp(sinks[h]),   O_i = sum_{j in V_i} exp(x_ij) v_j / den_i,   LSE_i = log(den_i)
 * -- one extra key with score sinks[h] and a zero value row; the sink is inside the LSE.  A row with no visible key (length 0, rows in
 * front of key 0, everything masked) gets O = 0 exactly and LSE = sinks[h], not -inf.  sinks[h] = -inf: head h has the O bits of the
 * sink-less call and -inf in the LSE where that call has it.  +inf or NaN in `sinks` is the caller's error: device data, not validated;
 * that head's rows are unspecified, other heads are unaffected, and the call does only arithmetic with it.
 *
 * Merging: because the LSE contains the sink, pfa_attn_merge of a sink-carrying part with sink-less parts over disjoint keys is the
 * sink-carrying result over the union.  Inside these calls exactly ONE part carries it: of the decode's key splits the partial of split 0
 * of each item, of pfa_fa3_prefill_split_sink the partial of split 0 of each q block.  That part writes O = 0, LSE = sinks[h] when it has
 * no key of its own; the others write -inf as before.  fa3_decode_combine_kernel and pfa_attn_merge are reused unchanged.  (A caller that
 * cuts a shared prefix off gives the sinks to ONE of its passes.)
 *
 * The sink is read by ordinary loads and written nowhere: no atomics, no workspace beyond the sink-less call's.  Workgroups, split
 * count and workspace bytes are the sink-less call's, from host shapes alone; the pointer is a launch argument and its contents are
 * read on the device, so a captured graph replays while the sink values change.  A tree mask (pfa_fa3_decode_tree) and an FP8 cache
 * (the *_q8 calls) take no sinks.
 *
 * `sinks` NULL: the call IS its sink-less sibling (pfa_fa3_decode_ex, pfa_fa3_prefill_ex, pfa_fa3_prefill_varlen_ex,
 * pfa_fa3_prefill_split) in every respect -- status, workspace, kernel function, grid, bits.  With a block, field rules in the order
 * their errors are reported: sinks->size wrong -> PFA_ERR_STRUCT_SIZE; sinks->flags != 0 -> PFA_ERR_FLAGS; sinks->sinks NULL ->
 * PFA_ERR_NULL; not 4-byte aligned -> PFA_ERR_ALIGN; then the unchanged rules of the sibling's _check, which these calls ask.  The
 * workspace queries leave out the two rules about the pointer and answer 0 where a rule fails.
 */
typedef struct pfa_fa3_sinks {
    uint32_t size;      /* = sizeof(pfa_fa3_sinks) */
    uint32_t flags;     /* must be 0 */
    const float* sinks; /* [H] fp32, device, 4-byte aligned; units of the scaled scores */
} pfa_fa3_sinks;

size_t pfa_fa3_decode_sink_workspace_bytes(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks);
int pfa_fa3_decode_sink_check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks);
int pfa_fa3_decode_sink(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks, void* stream);
/* As the sibling's describe, with "_sink" in the name behind "_win" and in front of "+combine", "_varlen", "_split{N}+merge" and "_paged":
 * "fa3_decode_..._o16[_win]_sink[+combine][_paged]", "fa3_prefill_..._causal[_win]_sink[_varlen][_split{N}+merge][_paged]".  -> the
 * sibling's workgroups (and split count in *nsplit), or a pfa_status. */
int pfa_fa3_decode_sink_describe(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks, char* buf, size_t n,
                                 int32_t* nsplit);
int pfa_fa3_prefill_sink_check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks);
int pfa_fa3_prefill_sink(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks, void* stream);
int pfa_fa3_prefill_sink_describe(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks, char* buf, size_t n);
int pfa_fa3_prefill_varlen_sink_check(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks);
int pfa_fa3_prefill_varlen_sink(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks, void* stream);
int pfa_fa3_prefill_varlen_sink_describe(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_sinks* sinks, char* buf,
                                         size_t n);
/* key_splits as in pfa_fa3_prefill_split; a count that resolves to 1 is pfa_fa3_prefill_sink without an extension block */
size_t pfa_fa3_prefill_split_sink_workspace_bytes(const pfa_fa3_decode_args* a, int32_t key_splits, const pfa_fa3_sinks* sinks);
int pfa_fa3_prefill_split_sink_check(const pfa_fa3_decode_args* a, int32_t key_splits, const pfa_fa3_sinks* sinks);
int pfa_fa3_prefill_split_sink(const pfa_fa3_decode_args* a, int32_t key_splits, const pfa_fa3_sinks* sinks, void* stream);
int pfa_fa3_prefill_split_sink_describe(const pfa_fa3_decode_args* a, int32_t key_splits, const pfa_fa3_sinks* sinks, char* buf, size_t n,
                                        int32_t* nsplit);

/*
 * Measurement aid (bench.py, roofline.probe_tflops; not on the hot path): enqueue a bare v_mfma_f32_32x32x16_bf16 stream -- one wave
 * per SIMD on every CU, A operands re-read from LDS as the forward's tile loop reads its K / V^T fragments, random operands taken from
 * `random_64k` (64 KiB of device memory holding bf16 values) -- of `iters` x 64 MFMAs per wave.  `sink`: device scratch of
 * 4 B x 256 x the number of CUs.  Returns the number of workgroups launched (> 0) or a pfa_status; *flops = the launch's flops.
 */
int pfa_probe_mfma(const void* random_64k, float* sink, int iters, int device_id, void* stream, double* flops);

#ifdef __cplusplus
}
#endif
#endif /* PFA_HIP_H */
