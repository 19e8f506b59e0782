// page_copy_check_main.cpp -- pfa_page_copy_check over its rule table from a stand-alone program (host code only, no GPU): built with
// the host half of pfa_page_copy_capi.hip under AddressSanitizer and UBSan, it shows that the validation reads nothing but the
// argument block and overflows nothing on the extreme shapes.
//
//   hipcc -std=c++17 --offload-arch=gfx950 -Iinclude -Iphotonic_flash_attention_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -x hip tools/page_copy_check_main.cpp photonic_flash_attention_amd/csrc/pfa_page_copy_capi.hip -o page_copy_check && ./page_copy_check
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include "pfa_hip.h"

namespace pfa {
void set_last_hip_error(int) {}      // pfa_capi.hip's, which this program leaves out
}

static pfa_page_copy_args good() {
    pfa_page_copy_args a;
    memset(&a, 0, sizeof a);
    a.size = sizeof a;
    a.k_pool = (void*)0x1000000; a.v_pool = (void*)0x2000000; a.pairs = (const int32_t*)0x9000; a.rows = (const int32_t*)0x5000;
    a.pairs_stride = 2;
    a.k_stride_b = a.v_stride_b = 128 * 2 * 128; a.k_stride_h = a.v_stride_h = 128; a.k_stride_s = a.v_stride_s = 2 * 128;
    a.n_pairs = 8; a.Hkv = 2; a.D = 128; a.page_size = 128; a.num_pages = 100; a.dtype = PFA_DTYPE_BF16;
    return a;
}

static int failures = 0;
static void expect(const char* what, const pfa_page_copy_args* a, int want) {
    const int got = pfa_page_copy_check(a);
    if (got != want) {
        printf("FAIL %s: got %d, want %d\n", what, got, want);
        ++failures;
    }
}
#define CASE(want, ...)            \
    do {                           \
        pfa_page_copy_args a = good(); \
        __VA_ARGS__;               \
        expect(#__VA_ARGS__, &a, want); \
    } while (0)

int main() {
    expect("NULL block", nullptr, PFA_ERR_NULL);
    CASE(PFA_OK, (void)a);
    CASE(PFA_OK, a.rows = nullptr);
    CASE(PFA_ERR_STRUCT_SIZE, a.size = 16);
    CASE(PFA_ERR_STRUCT_SIZE, a.size = 0; a.flags = 1);
    CASE(PFA_ERR_FLAGS, a.flags = 1; a.k_pool = nullptr);
    CASE(PFA_ERR_FLAGS, a.reserved0 = INT_MIN);
    CASE(PFA_ERR_NULL, a.k_pool = nullptr; a.n_pairs = 0);
    CASE(PFA_ERR_NULL, a.v_pool = nullptr);
    CASE(PFA_ERR_NULL, a.pairs = nullptr; a.page_size = 96);
    CASE(PFA_ERR_SHAPE, a.n_pairs = 0; a.D = 100);
    CASE(PFA_ERR_SHAPE, a.n_pairs = INT_MIN);
    CASE(PFA_ERR_SHAPE, a.Hkv = 0);
    CASE(PFA_ERR_SHAPE, a.num_pages = -1);
    CASE(PFA_ERR_SHAPE, a.page_size = 0);
    CASE(PFA_ERR_SHAPE, a.page_size = INT_MIN);
    CASE(PFA_ERR_SHAPE, a.page_size = 96);
    CASE(PFA_ERR_HEAD_DIM, a.D = 0; a.dtype = 7);
    CASE(PFA_ERR_HEAD_DIM, a.D = 100);
    CASE(PFA_ERR_HEAD_DIM, a.D = 264);
    CASE(PFA_ERR_HEAD_DIM, a.D = INT_MAX);
    CASE(PFA_ERR_DTYPE, a.dtype = PFA_DTYPE_FP32; a.pairs_stride = 1);
    CASE(PFA_ERR_STRIDE, a.k_stride_b = 7; a.k_pool = (void*)0x1000008);
    CASE(PFA_ERR_STRIDE, a.v_stride_h = 132);
    CASE(PFA_ERR_STRIDE, a.k_stride_s = -256);
    CASE(PFA_ERR_STRIDE, a.v_stride_s = LLONG_MIN);
    CASE(PFA_ERR_STRIDE, a.pairs_stride = 1);
    CASE(PFA_ERR_STRIDE, a.pairs_stride = LLONG_MIN);
    CASE(PFA_ERR_ALIGN, a.k_pool = (void*)0x1000008; a.n_pairs = INT_MAX);
    CASE(PFA_ERR_ALIGN, a.v_pool = (void*)0x2000002);
    CASE(PFA_ERR_ALIGN, a.pairs = (const int32_t*)0x9002);
    CASE(PFA_ERR_ALIGN, a.rows = (const int32_t*)0x5001);
    CASE(PFA_ERR_SHAPE, a.n_pairs = 1 << 24; a.page_size = 1 << 12);
    CASE(PFA_ERR_SHAPE, a.n_pairs = INT_MAX; a.Hkv = INT_MAX; a.D = 256; a.page_size = 1 << 30);      // products past 32 bits, not past 64
    CASE(PFA_ERR_SHAPE, a.n_pairs = 1; a.Hkv = 1 << 10; a.page_size = 1 << 20; a.D = 256);
    CASE(PFA_OK, a.k_stride_b = a.v_stride_b = LLONG_MAX - 7; a.pairs_stride = LLONG_MAX);
    CASE(PFA_OK, a.n_pairs = 1; a.Hkv = 1; a.D = 8; a.page_size = 64; a.num_pages = 1);
    char buf[4];
    pfa_page_copy_args a = good();
    if (pfa_page_copy_describe(&a, buf, sizeof buf) != 8 * 4 || strcmp(buf, "pag") != 0) {
        printf("FAIL describe: %s\n", buf);
        ++failures;
    }
    a.D = 100;
    if (pfa_page_copy(&a, nullptr) != PFA_ERR_HEAD_DIM) ++failures;      // refused before any device call
    printf("%s: %d failures\n", failures ? "FAILED" : "ok", failures);
    return failures != 0;
}
