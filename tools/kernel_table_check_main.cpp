// kernel_table_check_main.cpp -- does every kernel table of the calls over a KV cache hand out the instantiation its arguments name?
// A stand-alone program (host code only, no GPU; it launches nothing): for every table of csrc/pfa_decode_host.h, pfa_prefill_host.h and
// pfa_append_host.h and every run-time combination of the table's arguments, the pointer the table returns against the address of the
// instantiation spelled with the same values as compile-time arguments -- the host stubs' addresses, which is what a launch is given.
// The expected side walks the values by static recursion (each_elem_dim, each_bools below), never through the tables or the dispatch
// helpers they are built from.  It also counts the distinct kernels of each table against the counts of DESIGN 4.15 / 4.16.
//
//   hipcc -std=c++17 --offload-arch=gfx950 -Iinclude -Iphotonic_flash_attention_amd/csrc \
//         -x hip tools/kernel_table_check_main.cpp -o kernel_table_check && ./kernel_table_check
//
// (A few minutes: the device side of all 418 kernels is compiled into the one program, whose link wants it.)
#include <stdio.h>

#include <set>
#include <type_traits>

#include "pfa_append_host.h"
#include "pfa_decode_host.h"
#include "pfa_prefill_host.h"

namespace pfa {
void set_last_hip_error(int) {}      // pfa_capi.hip's, which this program leaves out
}

namespace {

template <typename T, int HEAD_DIM, int DTYPE>
struct Elem {
    using type = T;
    static constexpr int D = HEAD_DIM, dtype = DTYPE;
};
template <typename F>
void each_elem_dim(F f) {
    f(Elem<__bf16, 64, PFA_DTYPE_BF16>{}); f(Elem<__bf16, 128, PFA_DTYPE_BF16>{});
    f(Elem<_Float16, 64, PFA_DTYPE_FP16>{}); f(Elem<_Float16, 128, PFA_DTYPE_FP16>{});
}
// f(std::bool_constant...) for all 2^N values of N flags
template <int N, bool... Bs, typename F>
void each_bools(F f) {
    if constexpr (N == 0) {
        f(std::bool_constant<Bs>{}...);
    } else {
        each_bools<N - 1, Bs..., false>(f);
        each_bools<N - 1, Bs..., true>(f);
    }
}
template <bool FP32, typename T>
using Out = std::conditional_t<FP32, float, T>;

int failures = 0;

struct Table {
    const char* name;
    std::set<const void*> kernels;
    int combos = 0, wrong = 0;
    template <typename Fn>
    void add(Fn got, Fn want) {       // one type: a table that hands out another kernel's block does not compile here
        ++combos;
        if (got != want) ++wrong;
        if (got) kernels.insert(reinterpret_cast<const void*>(got));
    }
    void merge(const Table& t) {
        kernels.insert(t.kernels.begin(), t.kernels.end());
        combos += t.combos; wrong += t.wrong;
    }
    void report(size_t want_distinct) {
        const bool ok = wrong == 0 && kernels.size() == want_distinct;
        printf("%-22s %3d combinations, %d wrong, %3zu distinct kernels (want %zu): %s\n", name, combos, wrong, kernels.size(), want_distinct,
               ok ? "ok" : "FAILED");
        if (!ok) ++failures;
    }
};

template <bool WINDOW, bool TREE, bool KV8, bool SINK = false>
Table decode_table(const char* name) {
    Table tb{name};
    each_elem_dim([&](auto e) {
        using T = typename decltype(e)::type;
        constexpr int D = decltype(e)::D;
        each_bools<2>([&](auto o32, auto pg) {
            tb.add(pfa::decode::kernel<WINDOW, TREE, KV8, SINK>(e.dtype, D, o32.value, pg.value),
                   &pfa::dec::fa3_decode_kernel<T, D, Out<o32.value, T>, pg.value, WINDOW, TREE, KV8, SINK>);
        });
    });
    return tb;
}

Table combine_table() {
    Table tb{"combine"};
    each_elem_dim([&](auto e) {
        using T = typename decltype(e)::type;
        constexpr int D = decltype(e)::D;
        each_bools<1>([&](auto o32) { tb.add(pfa::decode::combine(e.dtype, D, o32.value), &pfa::dec::fa3_decode_combine_kernel<D, Out<o32.value, T>>); });
    });
    return tb;
}

// nullptr where the kernel allows no instantiation: a window without the causal flag, split parts that are not fp32 (spelled out here, not
// asked of prefill_kernel_exists, which the table under test asks)
template <bool VARLEN, bool WINDOW, bool SPLIT, bool KV8, bool SINK = false>
Table prefill_table(const char* name) {
    using Fn = pfa::KernelFn<pfa::prefill::Params<VARLEN, WINDOW, SPLIT, KV8, SINK>>;
    Table tb{name};
    each_elem_dim([&](auto e) {
        using T = typename decltype(e)::type;
        constexpr int D = decltype(e)::D;
        each_bools<3>([&](auto c, auto pg, auto o32) {
            Fn want = nullptr;
            if constexpr (!(WINDOW && !c.value) && !(SPLIT && !o32.value))
                want = &pfa::fa3_prefill_kernel<T, D, c.value, o32.value, pg.value, Out<o32.value, T>, VARLEN, WINDOW, SPLIT, KV8, SINK>;
            tb.add(pfa::prefill::kernel<VARLEN, WINDOW, SPLIT, KV8, SINK>(e.dtype, D, c.value, pg.value, o32.value), want);
        });
    });
    return tb;
}
template <bool VARLEN, bool SINK = false>
Table prefill16_table(const char* name) {
    Table tb{name};
    tb.merge(prefill_table<VARLEN, false, false, false, SINK>(""));
    tb.merge(prefill_table<VARLEN, true, false, false, SINK>(""));
    return tb;
}

template <bool QUANT, typename T>
void kv_append_rows(Table& tb) {
    using Fn = pfa::KernelFn<typename pfa::KvAppendParamsOf<QUANT>::type>;
    each_bools<2>([&](auto v, auto pg) {
        const Fn want = &pfa::kv_append_kernel<v.value, pg.value, QUANT, T>;
        tb.add(pfa::append::kv_kernel<QUANT, T>(v.value, pg.value), want);
    });
}
template <typename T>
void rope_append_rows(Table& tb) {
    each_bools<3>([&](auto v, auto pg, auto il) {
        const pfa::KernelFn<pfa::RopeAppendParams> want = &pfa::rope_append_kernel<T, v.value, pg.value, il.value>;
        tb.add(pfa::append::rope_kernel<T>(v.value, pg.value, il.value), want);
    });
}

}  // namespace

int main() {
    Table none = decode_table<false, false, false>("decode 16-bit: none"), win = decode_table<true, false, false>("decode 16-bit: window"),
          tree = decode_table<false, true, false>("decode 16-bit: tree"), dec16{"decode 16-bit"};
    none.report(16); win.report(16); tree.report(16);
    dec16.merge(none); dec16.merge(win); dec16.merge(tree);
    dec16.report(48);
    decode_table<false, false, true>("decode FP8").report(16);
    Table sink = decode_table<false, false, false, true>("decode sink: none"), wsink = decode_table<true, false, false, true>("decode sink: window");
    sink.report(16); wsink.report(16);
    sink.merge(wsink); sink.name = "decode sink";
    sink.report(32);
    combine_table().report(6);
    prefill16_table<false>("prefill uniform").report(48);
    prefill16_table<true>("prefill ragged").report(48);
    prefill_table<false, false, true, false>("prefill split").report(16);
    prefill_table<false, false, false, true>("prefill FP8 uniform").report(32);
    prefill_table<true, false, false, true>("prefill FP8 ragged").report(32);
    prefill16_table<false, true>("prefill sink uniform").report(48);
    prefill16_table<true, true>("prefill sink ragged").report(48);
    prefill_table<false, false, true, false, true>("prefill sink split").report(16);
    Table kv{"kv_append"}, kv8{"kv_append_q8"}, rope{"rope_append"};
    kv_append_rows<false, void>(kv);
    kv_append_rows<true, __bf16>(kv8); kv_append_rows<true, _Float16>(kv8);
    rope_append_rows<__bf16>(rope); rope_append_rows<_Float16>(rope);
    kv.report(4); kv8.report(8); rope.report(16);
    printf("%s: %d failures\n", failures ? "FAILED" : "ok", failures);
    return failures != 0;
}
