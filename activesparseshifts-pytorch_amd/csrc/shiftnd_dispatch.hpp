// shiftnd_dispatch.hpp -- run-time values to template arguments, once for every launcher (internal, host side).
//
// Each helper calls a generic lambda with a compile-time tag:
//     with_pad_mirror(g.pad, [&](auto pad) { launch((kernel<T, decltype(pad)::value>), ...); });
// A kernel exists because a launcher names it: which (type, ACTIVE, PAD) combinations the library holds is decided by the helper a
// launcher picks plus the `if constexpr` holes written out in its lambda, next to the comment that justifies them.
#pragma once

#include <type_traits>

#include "shiftnd_launch.hpp"

namespace shiftnd {

// PAD as a template parameter of the step / span / walk kernels takes the values 0 .. 3, and 3 stands for BOTH mirroring modes, reflect
// (3) and symmetric (4): see shiftnd_step.hpp (fold_mirror).  (The flat-stream kernels take 0, 1 and kPadRT: shiftnd_flat.hip.)
constexpr int kPadMirror = 3;
constexpr int pad_template(int pad) { return pad >= kPadMirror ? kPadMirror : pad; }

template <typename T> struct type_tag { using type = T; };
template <typename Tag> using tag_type = typename Tag::type;

// f(integral_constant<int, P>) for the listed template padding that serves `pad`; the last one listed is the catch-all
template <int P0, int... Ps, typename F> inline void with_pad(int pad, F &&f) {
    if constexpr (sizeof...(Ps) == 0) f(std::integral_constant<int, P0>{});
    else if (pad == P0) f(std::integral_constant<int, P0>{});
    else with_pad<Ps...>(pad, f);
}
template <typename F> inline void with_pad_mirror(int pad, F &&f) { with_pad<0, 1, 2, kPadMirror>(pad, f); }   // zeros, border, periodic, reflect / symmetric

template <typename F> inline void with_bool(bool b, F &&f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// f(type_tag<T>) for the listed element type whose kDtype is `dtype`; the last one listed is the catch-all
template <typename T0, typename... Ts, typename F> inline void with_type(int dtype, F &&f) {
    if constexpr (sizeof...(Ts) == 0) f(type_tag<T0>{});
    else if (dtype == T0::kDtype) f(type_tag<T0>{});
    else with_type<Ts...>(dtype, f);
}
template <typename F> inline void with_float_type(int dtype, F &&f) { with_type<f32_t, f64_t, f16_t, bf16_t>(dtype, f); }

// the sparse shift is a raw copy (the weights are widened by their own dtype): one instantiation per element size
template <typename F> inline void with_raw_type(int es, F &&f) {
    if (es == 2) f(type_tag<f16_t>{});
    else if (es == 4) f(type_tag<f32_t>{});
    else f(type_tag<f64_t>{});
}

// the forwards of both shifts: f(type_tag<T>, bool_constant<ACTIVE>) -- per dtype for the interpolating shift, per element size for the
// sparse one
template <typename F> inline void with_shift_type(bool active, int dtype, F &&f) {
    if (active) with_float_type(dtype, [&](auto t) { f(t, std::true_type{}); });
    else with_raw_type(dtype_size(dtype), [&](auto t) { f(t, std::false_type{}); });
}

}  // namespace shiftnd
