// launch.h - the launch helpers every unit may use: dynamic-LDS launches, and run-time values -> template arguments through generic lambdas
// (one instantiation of the lambda per admitted value; a combination that is never named is never instantiated).
#pragma once
#include "t4k_common.h"
#include <type_traits>

namespace {

// Launch of a kernel with dynamic LDS: the kernel's limit is raised the first time it is launched, and again only when a later launch
// asks for more (k_head_bwd_l32's request depends on the shapes).  Counted like every launch (T4K_LAUNCH).
template <auto Kern> size_t &lds_granted() { static size_t bytes = 0; return bytes; }      // one per kernel, whatever the call site passes
template <auto Kern, typename... Args>
void launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args &...args) {
    size_t &granted = lds_granted<Kern>();
    if (lds > granted) { (void)hipFuncSetAttribute(reinterpret_cast<const void *>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); granted = lds; }
    T4K_LAUNCH(Kern, grid, block, lds, s, args...);
}
// run-time flags -> template arguments: f(std::bool_constant<flag>{}...), one instantiation of f per combination
template <typename F> void with_flags(F &&f) { f(); }
template <typename F, typename... Bs>
void with_flags(F &&f, bool b, Bs... more) {
    if (b) with_flags([&](auto... cs) { f(std::true_type{}, cs...); }, more...);
    else   with_flags([&](auto... cs) { f(std::false_type{}, cs...); }, more...);
}
// a run-time int -> one of a short compile-time list: pick<32, 64>(bkp, [&](auto bk) { ... decltype(bk)::value ... }); false when v is not in the list
template <int V> using int_c = std::integral_constant<int, V>;
template <int... Vs, typename F>
bool pick(int v, F &&f) { return ((v == Vs ? (f(int_c<Vs>{}), true) : false) || ...); }

// the four convolution geometries the library admits (kernel size, stride, padding): f(Geo<K, S, P>{}); false for any other
template <int K_, int S_, int P_> struct Geo { static constexpr int K = K_, S = S_, P = P_; };
template <typename F>
bool with_geometry(int K, int S, int P, F &&f) {
    if (K == 1 && S == 1 && P == 0) { f(Geo<1, 1, 0>{}); return true; }
    if (K == 3 && S == 1 && P == 1) { f(Geo<3, 1, 1>{}); return true; }
    if (K == 4 && S == 2 && P == 1) { f(Geo<4, 2, 1>{}); return true; }
    if (K == 5 && S == 1 && P == 2) { f(Geo<5, 1, 2>{}); return true; }
    return false;
}
inline bool conv_supported(int K, int S, int P) { return with_geometry(K, S, P, [](auto) {}); }

}
