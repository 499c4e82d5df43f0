// torch_binding.cpp -- the `torchshifts` operator library for PyTorch-ROCm (host C++): every schema, the composite entries, the
// Autograd key and the CUDA / QuantizedCUDA keys (= HIP tensors on PyTorch-ROCm).  No compute happens here: an adapter pulls
// pointers and strides out of at::Tensor and calls the C ABI of libshiftnd_hip.so (include/shiftnd_hip.h), and there is no CPU
// fallback -- a HIP tensor either runs the HIP kernels or raises.
//
// The op families, in the order every registration block at the end of the file lists them:
//   shift         shift{N}d = check_borders + _shift{N}d_forward, _shift{N}d_backward: the reference's dispatcher surface
//                 (csrc/ops/shifts.cpp, csrc/ops/autograd/shifts_autograd.cpp), so that torchshifts/_C.so is a drop-in
//   pool          shift{N}d_pool / _shift{N}d_pool_forward / _backward: the shift and the average pool the reference's modules
//                 attach (modules/shifts.py:81-89, 150-153) as ONE op; fused on HIP tensors, the two-step sequence elsewhere
//   fixed         shift{N}d_fixed / _shift{N}d_fixed_backward: integer shifts that nobody learns, an input-free backward
//   fixed pool    shift{N}d_fixed_pool / _shift{N}d_fixed_pool_backward: ... followed by the average pool
//   temporal      temporal_shift / _temporal_shift_backward / temporal_shift_quantized: fixed shifts across the frames of [N*T, C, ...]
//   temporal cl   temporal_shift_cl / _temporal_shift_cl_backward / temporal_shift_quantized_cl: ... keeping a channels-last layout
//   learnable     temporal_shift_learnable / _temporal_shift_learnable_forward / _backward: a trained shift across the frames
//   learnable cl  temporal_shift_learnable_cl / _temporal_shift_learnable_cl_forward / _backward: ... keeping a channels-last layout
// ... and, in namespaces of their own (registered last), the families that came after the op set of torchshifts:: was pinned:
//   per clip      torchshifts_per_clip::temporal_shift_learnable_per_clip / _forward / _backward, temporal_shift_per_clip /
//                 _temporal_shift_per_clip_backward: the temporal shifts under a [N, C] table, one row per clip
//   per clip, channels-last  torchshifts_per_clip_cl::temporal_shift_learnable_per_clip_cl / _forward / _backward,
//                 temporal_shift_per_clip_cl / _temporal_shift_per_clip_cl_backward: the same with the argument's layout kept
//   interlace     torchshifts_interlace::temporal_interlace / _temporal_interlace_forward / _backward: the per-clip shift times a scale
//                 per clip, frame and channel (TIN), two tables
//   in place      torchshifts_inplace::temporal_shift_ / temporal_shift_quantized_: the temporal shift written into the input (composes
//                 on CPU tensors), a family that writes its argument
//   online        torchshifts_online::temporal_shift_online_ / temporal_shift_online_quantized_: one frame per call against a cached
//                 state of the previous frames, both written (composes on CPU tensors); inference only, no Autograd key
//   quantized learnable  torchshifts_quantized_learnable::temporal_shift_learnable_quantized: the interpolating temporal shift of a
//                 per-tensor quantized tensor in the integer domain, an fp32 table; inference only, no Autograd key
//   quantized interlace  torchshifts_quantized_interlace::temporal_interlace_quantized: temporal interlacing (scales None: the
//                 per-clip temporal shift) of a per-tensor quantized tensor in the integer domain; inference only, no Autograd key
//   quantized learnable cl  torchshifts_quantized_learnable_cl::temporal_shift_learnable_quantized_cl: ... keeping a channels-last layout
//
// Keys: the Autograd, CUDA and QuantizedCUDA kernels of every family are registered here.  The CPU / QuantizedCPU kernels that
// compute (shift, fixed, fixed pool, temporal, temporal_shift_quantized, quantized learnable, quantized interlace) live in torch_cpu_backend.cpp; the ones that compose other
// ops (pool, temporal cl, learnable, learnable cl) are registered here.
//
// Helpers every family uses: typed_op + one *Ops struct per family (cached dispatcher handles),
// GuardedBackward (the double-backward guard), fill_problem / segment_problem (the only writers of a shiftnd_problem),
// segment_check, PoolArgs, check_status, workspace_like.
#include <ATen/ATen.h>
#include <ATen/core/dispatch/Dispatcher.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_version.h>
#include <torch/autograd.h>
#include <torch/library.h>

#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "shiftnd_hip.h"

namespace torchshifts_amd {

using at::Tensor;
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

// ---- dispatcher re-entry (ops/shifts.cpp:10-88) ------------------------------------------------------
// One *Ops struct per family: the name its double-backward guard raises under, and the typed handles of the ops its nodes and
// kernels call back into the dispatcher.  Every handle is looked up once (a function-local static), here and nowhere else.
using forward_sig = Tensor(const Tensor &, const Tensor &, const Tensor &, at::IntArrayRef, int64_t, bool);
using backward_sig = std::tuple<Tensor, Tensor>(const Tensor &, const Tensor &, const Tensor &, const Tensor &, int64_t,
                                                bool);
using pool_forward_sig = Tensor(const Tensor &, const Tensor &, const Tensor &, at::IntArrayRef, at::IntArrayRef, int64_t, bool);
using pool_backward_sig = std::tuple<Tensor, Tensor>(const Tensor &, const Tensor &, const Tensor &, const Tensor &,
                                                     at::IntArrayRef, int64_t, bool);
using fixed_backward_sig = Tensor(const Tensor &, const Tensor &, const Tensor &, at::IntArrayRef, int64_t);
using fixed_pool_backward_sig = Tensor(const Tensor &, const Tensor &, const Tensor &, at::IntArrayRef, at::IntArrayRef, int64_t);
using temporal_sig = Tensor(const Tensor &, const Tensor &, int64_t, int64_t);
using tsl_forward_sig = Tensor(const Tensor &, const Tensor &, int64_t, int64_t, bool);
using tsl_backward_sig = std::tuple<Tensor, Tensor>(const Tensor &, const Tensor &, const Tensor &, int64_t, int64_t, bool);

template <class Sig> c10::TypedOperatorHandle<Sig> typed_op(const std::string &name, const char *library = "torchshifts") {
    return c10::Dispatcher::singleton().findSchemaOrThrow((library + ("::" + name)).c_str(), "").typed<Sig>();
}

inline std::string nd_name(int nd, const char *suffix = "") { return "shift" + std::to_string(nd) + "d" + suffix; }

template <int ND> struct ShiftOps {
    static std::string name() { return nd_name(ND); }
    static auto &forward() { static auto op = typed_op<forward_sig>("_" + nd_name(ND, "_forward")); return op; }
    static auto &backward() { static auto op = typed_op<backward_sig>("_" + nd_name(ND, "_backward")); return op; }
};
template <int ND> struct PoolOps {
    static std::string name() { return nd_name(ND); }   // (the pooled ops raise under the plain op's name)
    static auto &forward() { static auto op = typed_op<pool_forward_sig>("_" + nd_name(ND, "_pool_forward")); return op; }
    static auto &backward() { static auto op = typed_op<pool_backward_sig>("_" + nd_name(ND, "_pool_backward")); return op; }
};
template <int ND> struct FixedOps {   // (forward: ShiftOps<ND>::forward under the converted table)
    static std::string name() { return nd_name(ND, "_fixed"); }
    static auto &backward() { static auto op = typed_op<fixed_backward_sig>("_" + nd_name(ND, "_fixed_backward")); return op; }
};
template <int ND> struct FixedPoolOps {   // (forward: PoolOps<ND>::forward under the converted table)
    static std::string name() { return nd_name(ND, "_fixed_pool"); }
    static auto &backward() { static auto op = typed_op<fixed_pool_backward_sig>("_" + nd_name(ND, "_fixed_pool_backward")); return op; }
};
struct TemporalOps {
    static const char *name() { return "temporal_shift"; }
    static auto &forward() { static auto op = typed_op<temporal_sig>("temporal_shift"); return op; }
    static auto &backward() { static auto op = typed_op<temporal_sig>("_temporal_shift_backward"); return op; }
};
struct TemporalClOps {
    static const char *name() { return "temporal_shift_cl"; }
    static auto &forward() { static auto op = typed_op<temporal_sig>("temporal_shift_cl"); return op; }
    static auto &backward() { static auto op = typed_op<temporal_sig>("_temporal_shift_cl_backward"); return op; }
};
// The four learnable families also carry what their HIP adapters (tsl_forward_hip / tsl_backward_hip) differ in: the names
// check_same's messages speak under, the argument check, the flag bits of the C-ABI call, the name segment_problem's refusal speaks
// under, and whether the route takes a dense channels-last tensor as it lies (kAsItLies).  A family with kAsItLies MUST also name
// `Plain`, the family every other tensor goes to; the adapters name Ops::Plain only inside `if constexpr (Ops::kAsItLies)`, so a
// family without kAsItLies needs none and has none.
void tsl_check(const Tensor &input, const Tensor &weights, int64_t n_segment, int64_t padding_mode);
void tslpc_check(const Tensor &input, const Tensor &weights, int64_t n_segment, int64_t padding_mode);
struct LearnableOps {
    static const char *name() { return "temporal_shift_learnable"; }
    static auto &forward() { static auto op = typed_op<tsl_forward_sig>("_temporal_shift_learnable_forward"); return op; }
    static auto &backward() { static auto op = typed_op<tsl_backward_sig>("_temporal_shift_learnable_backward"); return op; }
    static constexpr const char *kCuda = "temporal_shift_learnable_cuda", *kBackwardCuda = "temporal_shift_learnable_backward_cuda";
    static constexpr auto check = tsl_check;
    static constexpr int kFlags = SHIFTND_SHIFT_DIM0;
    static constexpr const char *kProblemName = "temporal_shift_learnable";
    static constexpr bool kAsItLies = false;
};
struct LearnableClOps {
    static const char *name() { return "temporal_shift_learnable_cl"; }
    static auto &forward() { static auto op = typed_op<tsl_forward_sig>("_temporal_shift_learnable_cl_forward"); return op; }
    static auto &backward() { static auto op = typed_op<tsl_backward_sig>("_temporal_shift_learnable_cl_backward"); return op; }
    static constexpr const char *kCuda = "temporal_shift_learnable_cl_cuda", *kBackwardCuda = "temporal_shift_learnable_cl_backward_cuda";
    static constexpr auto check = tsl_check;
    static constexpr int kFlags = SHIFTND_SHIFT_DIM0 | SHIFTND_FRAMES;
    static constexpr const char *kProblemName = "temporal_shift";   // (a known slip)
    static constexpr bool kAsItLies = true;
    using Plain = LearnableOps;   // where a tensor that is not dense channels-last goes
};
struct PerClipLearnableOps {
    static const char *name() { return "temporal_shift_learnable_per_clip"; }
    static auto &forward() { static auto op = typed_op<tsl_forward_sig>("_temporal_shift_learnable_per_clip_forward", "torchshifts_per_clip"); return op; }
    static auto &backward() { static auto op = typed_op<tsl_backward_sig>("_temporal_shift_learnable_per_clip_backward", "torchshifts_per_clip"); return op; }
    static constexpr const char *kCuda = "temporal_shift_learnable_per_clip_cuda", *kBackwardCuda = "temporal_shift_learnable_per_clip_backward_cuda";
    static constexpr auto check = tslpc_check;
    static constexpr int kFlags = SHIFTND_SHIFT_DIM0 | SHIFTND_PER_CLIP;
    static constexpr const char *kProblemName = "temporal_shift_learnable_per_clip";
    static constexpr bool kAsItLies = false;
};
struct PerClipLearnableClOps {
    static const char *name() { return "temporal_shift_learnable_per_clip_cl"; }
    static auto &forward() { static auto op = typed_op<tsl_forward_sig>("_temporal_shift_learnable_per_clip_cl_forward", "torchshifts_per_clip_cl"); return op; }
    static auto &backward() { static auto op = typed_op<tsl_backward_sig>("_temporal_shift_learnable_per_clip_cl_backward", "torchshifts_per_clip_cl"); return op; }
    static constexpr const char *kCuda = "temporal_shift_learnable_per_clip_cl_cuda", *kBackwardCuda = "temporal_shift_learnable_per_clip_cl_backward_cuda";
    static constexpr auto check = tslpc_check;
    static constexpr int kFlags = SHIFTND_SHIFT_DIM0 | SHIFTND_CLIP_FRAMES;
    static constexpr const char *kProblemName = "temporal_shift_learnable_per_clip_cl";
    static constexpr bool kAsItLies = true;
    using Plain = PerClipLearnableOps;   // (as LearnableClOps::Plain)
};
// temporal interlacing: two tables (offsets [N, C], scales [N, T, C]), so signatures and adapters of its own (further down)
using tin_forward_sig = Tensor(const Tensor &, const Tensor &, const Tensor &, int64_t, int64_t, bool);
using tin_backward_sig = std::tuple<Tensor, Tensor, Tensor>(const Tensor &, const Tensor &, const Tensor &, const Tensor &, int64_t, int64_t, bool);
// (what the HIP adapters tin_forward_hip / tin_backward_hip differ in travels with the family, as for the learnable families above)
struct InterlaceOps {
    static const char *name() { return "temporal_interlace"; }
    static auto &forward() { static auto op = typed_op<tin_forward_sig>("_temporal_interlace_forward", "torchshifts_interlace"); return op; }
    static auto &backward() { static auto op = typed_op<tin_backward_sig>("_temporal_interlace_backward", "torchshifts_interlace"); return op; }
    static constexpr const char *kCuda = "temporal_interlace_cuda", *kBackwardCuda = "temporal_interlace_backward_cuda";
    static constexpr int kFlags = SHIFTND_SHIFT_DIM0 | SHIFTND_INTERLACE;
    static constexpr bool kAsItLies = false;
};
struct InterlaceClOps {
    static const char *name() { return "temporal_interlace_cl"; }
    static auto &forward() { static auto op = typed_op<tin_forward_sig>("_temporal_interlace_cl_forward", "torchshifts_interlace_cl"); return op; }
    static auto &backward() { static auto op = typed_op<tin_backward_sig>("_temporal_interlace_cl_backward", "torchshifts_interlace_cl"); return op; }
    static constexpr const char *kCuda = "temporal_interlace_cl_cuda", *kBackwardCuda = "temporal_interlace_cl_backward_cuda";
    static constexpr int kFlags = SHIFTND_SHIFT_DIM0 | SHIFTND_INTERLACE_FRAMES;
    static constexpr bool kAsItLies = true;
    using Plain = InterlaceOps;   // (as LearnableClOps::Plain)
};

// ---- the double-backward guard ------------------------------------------------------------------------
// A backward op is itself differentiable only to the extent of raising on a second backward.  GuardedBackward<Ops>::kernel is the
// Autograd-key kernel of the family's backward op, with the signature of Ops::backward(): it calls that op below autograd and
// hangs a node on the results whose backward raises under Ops::name().
inline variable_list as_list(const Tensor &t) { return {t}; }
inline variable_list as_list(const std::tuple<Tensor, Tensor> &t) { return {std::get<0>(t), std::get<1>(t)}; }
inline variable_list as_list(const std::tuple<Tensor, Tensor, Tensor> &t) { return {std::get<0>(t), std::get<1>(t), std::get<2>(t)}; }

template <class Ops, class Handle = std::remove_reference_t<decltype(Ops::backward())>> struct GuardedBackward;
template <class Ops, class R, class... A>
struct GuardedBackward<Ops, c10::TypedOperatorHandle<R(A...)>> : public torch::autograd::Function<GuardedBackward<Ops>> {
    static variable_list forward(AutogradContext *, A... args) {
        at::AutoDispatchBelowADInplaceOrView guard;
        return as_list(Ops::backward().call(args...));
    }
    static variable_list backward(AutogradContext *, const variable_list &) {
        TORCH_CHECK(0, "double backwards on ", Ops::name(), " not supported");
    }
    static R kernel(A... args) {
        auto result = GuardedBackward::apply(args...);
        if constexpr (std::is_same_v<R, Tensor>) return result[0];
        else if constexpr (std::tuple_size_v<R> == 3) return std::make_tuple(result[0], result[1], result[2]);
        else return std::make_tuple(result[0], result[1]);
    }
};

// ---- small things every adapter repeats -----------------------------------------------------------------
inline void check_status(int rc, const char *what) { TORCH_CHECK(rc == SHIFTND_OK, what, ": ", shiftnd_status_string(rc)); }

// `bytes` of workspace on t's device
inline Tensor workspace_like(const Tensor &t, size_t bytes) {
    return at::empty({static_cast<int64_t>(bytes)}, t.options().dtype(at::kByte));
}

// ---- borders -------------------------------------------------------------------------------------------
// check_borders (ops/shifts.cpp:93-135).  Unlike the reference the 6-int result stays on the HOST:
// it is host-known, and the kernels take it as launch arguments (no 24-byte H2D copy per call).
std::tuple<Tensor, std::vector<int64_t>> check_borders(const Tensor &input, const Tensor &borders, int64_t dim) {
    const auto sizes = input.sizes();
    TORCH_CHECK(static_cast<int64_t>(sizes.size()) >= dim + 1, "shift", dim, "d: input has too few dimensions");
    std::vector<int32_t> user;
    if (borders.numel() != 0) {
        Tensor b = borders.to(at::kInt).to(at::kCPU).contiguous();
        TORCH_CHECK(b.numel() >= 2 * std::min<int64_t>(dim, 3), "borders must hold (left, right) per spatial dim");
        user.assign(b.data_ptr<int32_t>(), b.data_ptr<int32_t>() + b.numel());
    }
    Tensor std_borders = at::empty({6}, at::TensorOptions().dtype(at::kInt).device(at::kCPU));
    std::vector<int64_t> new_sizes(sizes.size());
    check_status(shiftnd_check_borders(sizes.data(), static_cast<int>(sizes.size()), user.empty() ? nullptr : user.data(),
                                       static_cast<int>(dim), std_borders.data_ptr<int32_t>(), new_sizes.data()),
                 "check_borders");
    new_sizes.resize(((dim + 1) == static_cast<int64_t>(sizes.size()) ? 1 : 2) + std::min<int64_t>(dim, 3));
    return std::make_tuple(std_borders, new_sizes);
}

// 6 host ints from a borders tensor that may live anywhere (a device tensor costs one D2H sync;
// the composite ops above never produce one)
void read_borders(const Tensor &borders, int32_t out[6]) {
    TORCH_CHECK(borders.numel() == 6, "borders must hold 6 integers [l_i, r_i, l_j, r_j, l_k, r_k]");
    Tensor b = borders.to(at::kCPU).to(at::kInt).contiguous();
    for (int i = 0; i < 6; ++i) out[i] = b.data_ptr<int32_t>()[i];
}

// The reference hands the private ops a 6-int DEVICE tensor that its kernels read (cuda/shifts_cuda.cu:61-67, ops/shifts.cpp:134).
// When the window has the input's own spatial sizes the borders are implied -- 0 <= l < r <= size and r - l == size leave
// l = 0, r = size -- so a reference-style caller stays free of the D2H sync and graph-capturable; a cropped window with
// device-resident borders still costs the one read (the kernels take the window as launch arguments).
// (Which adapter calls read_borders_for and which read_borders is part of its route: the plain shift adapters take this one, the
// pooled and the fixed-backward adapters always read.)
void read_borders_for(const Tensor &borders, const Tensor &input, at::IntArrayRef window, int nd, int32_t out[6]) {
    TORCH_CHECK(borders.numel() == 6, "borders must hold 6 integers [l_i, r_i, l_j, r_j, l_k, r_k]");
    bool whole = !borders.is_cpu() && static_cast<int>(window.size()) == nd && input.dim() == nd + 2;
    for (int r = 0; whole && r < nd; ++r) whole = window[r] == input.size(2 + r);
    if (!whole) return read_borders(borders, out);
    for (int r = 0; r < 3; ++r) {
        out[2 * r] = 0;
        out[2 * r + 1] = r < nd ? static_cast<int32_t>(input.size(2 + r)) : 1;
    }
}

template <int ND> Tensor shift_public(const Tensor &input, const Tensor &weights, const Tensor &borders,
                                      int64_t padding_mode, bool active_flag) {
    auto bands = check_borders(input, borders, ND);
    return ShiftOps<ND>::forward().call(input, weights, std::get<0>(bands), std::get<1>(bands), padding_mode, active_flag);
}

std::tuple<Tensor, std::vector<int64_t>> check_borders_op(const Tensor &input, const Tensor &borders, int64_t dim) {
    return check_borders(input, borders, dim);
}

// ---- Autograd key (ops/autograd/shifts_autograd.cpp) -------------------------------------------------
// ShiftFunction and ShiftPoolFunction (and the fixed pair further down) stay two structs each: they differ in the arity of forward
// and backward and in the NDHWC branch below; one struct would carry an optional pool through both signatures and past that branch.
bool is_channels_last_dense(const Tensor &t);
Tensor channels_last_to_contiguous(const Tensor &t);

template <int ND> struct ShiftFunction : public torch::autograd::Function<ShiftFunction<ND>> {
    static variable_list forward(AutogradContext *ctx, const Tensor &input, const Tensor &weight, const Tensor &borders,
                                 at::IntArrayRef new_size, int64_t padding_mode, bool active_flag) {
        at::AutoDispatchBelowADInplaceOrView guard;
        // (round 6) a dense NDHWC input on the GPU: the backward runs the contiguous kernels behind a layout change (the direct NDHWC
        // backward is slower), and the forward through the layout change costs what the direct forward costs
        // (N8 C128 16x112x112 fp32: 0.29 + 0.26 ms against 0.56; interpolating 0.57 against 0.71).  So the layout changes ONCE, here,
        // and the node keeps the contiguous copy instead of the input -- the backward's 0.29 ms transpose of x is gone (1.04 -> 0.73
        // ms with an NDHWC gradient, 0.74 -> 0.44 with the NCDHW gradient this forward's output produces); the values are the same,
        // the original input can be freed as soon as nobody else holds it.
        Tensor kept = input;
        if constexpr (ND == 3) {
            // (only when a backward can follow: an inference call keeps the direct NDHWC forward)
            if ((input.requires_grad() || weight.requires_grad()) && input.is_cuda() && !input.is_quantized() && input.dim() == 5 &&
                at::isFloatingType(input.scalar_type()) && is_channels_last_dense(input)) {
                c10::DeviceGuard device_guard(input.device());
                kept = channels_last_to_contiguous(input);
            }
        }
        auto output = ShiftOps<ND>::forward().call(kept, weight, borders, new_size, padding_mode, active_flag);
        ctx->saved_data["padding_mode"] = padding_mode;
        ctx->saved_data["active_flag"] = active_flag;
        ctx->save_for_backward({kept, weight, borders});
        return {output};
    }
    static variable_list backward(AutogradContext *ctx, const variable_list &grad_output) {
        auto saved = ctx->get_saved_variables();
        const auto padding_mode = ctx->saved_data["padding_mode"].toInt();
        const auto active_flag = ctx->saved_data["active_flag"].toBool();
        auto result = ShiftOps<ND>::backward().call(grad_output[0], saved[1], saved[0], saved[2], padding_mode, active_flag);
        return {std::get<0>(result), std::get<1>(result), Tensor(), Tensor(), Tensor(), Tensor()};
    }
};

template <int ND> Tensor shift_autograd(const Tensor &input, const Tensor &weights, const Tensor &borders,
                                        at::IntArrayRef new_size, int64_t padding_mode, bool active_flag) {
    return ShiftFunction<ND>::apply(input, weights, borders, new_size, padding_mode, active_flag)[0];
}

// ---- HIP backend adapters (CUDA dispatch key on PyTorch-ROCm) ----------------------------------------
int to_shiftnd_dtype(at::ScalarType t, const char *what) {
    switch (t) {
    case at::kFloat: return SHIFTND_F32;
    case at::kDouble: return SHIFTND_F64;
    case at::kHalf: return SHIFTND_F16;
    case at::kBFloat16: return SHIFTND_BF16;
    default: TORCH_CHECK(false, "\"", what, "\" not implemented for '", c10::toString(t), "'");
    }
    return -1;
}

void fill_strides(const Tensor &t, int nd, int64_t out[5]) {
    for (int i = 0; i < 5; ++i) out[i] = 0;
    for (int i = 0; i < 2 + nd; ++i) out[i] = t.stride(i);
}

// the writer of the spatial families' problem: the sizes of `input`, the window `borders`
void fill_problem(shiftnd_problem &p, int nd, const Tensor &input, const int32_t borders[6], int64_t padding_mode,
                  bool active, int dtype) {
    p.ndim = nd;
    p.dtype = dtype;
    p.padding_mode = static_cast<int32_t>(padding_mode);
    p.active = active ? 1 : 0;
    for (int i = 0; i < 5; ++i) p.sizes[i] = 1;
    for (int i = 0; i < 2 + nd; ++i) p.sizes[i] = input.size(i);
    for (int i = 0; i < 6; ++i) p.borders[i] = borders[i];
}

// the writer of the temporal families' problem: the segment-major view [N, C, T, M] of a [N*T, C, ...] tensor `t` with numel() > 0,
// shifted along T over the whole window, and in `st` its strides -- {T*C*M, M, C*M, 1} for a contiguous tensor, {T*M*C, 1, M*C, C}
// for a dense channels-last one.  `dtype_bits`: the element type with the route's flag bits (SHIFTND_WEIGHTS_F32, SHIFTND_SHIFT_DIM0,
// SHIFTND_FRAMES) or-ed in by the caller; `who`: the op name the 32-bit refusal speaks under.
void segment_problem(shiftnd_problem &p, int64_t st[5], const Tensor &t, int64_t T, int64_t padding_mode, bool active, int dtype_bits,
                     bool channels_last, const char *who) {
    const int64_t C = t.size(1), N = t.size(0) / T, M = t.numel() / (t.size(0) * C);
    TORCH_CHECK(T <= INT32_MAX && M <= INT32_MAX, who, ": n_segment and the frame size must fit 32 bits");
    p.ndim = 2;
    p.dtype = dtype_bits;
    p.padding_mode = static_cast<int32_t>(padding_mode);
    p.active = active ? 1 : 0;
    const int64_t sizes[5] = {N, C, T, M, 1};
    const int64_t contiguous[5] = {T * C * M, M, C * M, 1, 0}, nhwc[5] = {T * M * C, 1, M * C, C, 0};
    const int32_t borders[6] = {0, static_cast<int32_t>(T), 0, static_cast<int32_t>(M), 0, 1};
    for (int i = 0; i < 5; ++i) p.sizes[i] = sizes[i], st[i] = channels_last ? nhwc[i] : contiguous[i];
    for (int i = 0; i < 6; ++i) p.borders[i] = borders[i];
}

// what the temporal families' argument checks share; `kind`: what the family calls its per-channel table ("shifts" / "weights"),
// `table_type_ok` / `table_types`: the family's own test of the table's element type and how the message names the types it takes,
// `per_clip`: the table is [N, C], one row per clip, not [C]
void segment_check(const char *op_name, const Tensor &input, const Tensor &table, int64_t n_segment, int64_t padding_mode,
                   const char *kind, bool table_type_ok, const char *table_types, bool per_clip = false) {
    TORCH_CHECK(input.dim() >= 2 && input.dim() <= 5, op_name, ": expected a [N*T, C, ...] tensor of 2 to 5 dims");
    TORCH_CHECK(n_segment >= 1 && input.size(0) % n_segment == 0, op_name, ": dim 0 (", input.size(0),
                ") must be a multiple of n_segment (", n_segment, ")");
    if (per_clip) {
        TORCH_CHECK(table.dim() == 2 && table.size(0) == input.size(0) / n_segment && table.size(1) == input.size(1), op_name, ": ", kind,
                    " must have shape [N, C] = [", input.size(0) / n_segment, ", ", input.size(1), "]");
    } else {
        TORCH_CHECK((table.dim() == 1 || (table.dim() == 2 && table.size(1) == 1)) && table.size(0) == input.size(1), op_name, ": ", kind,
                    " must have shape [C] or [C, 1]");
    }
    TORCH_CHECK(table.device() == input.device(), op_name, ": ", kind, " must be on the input's device");
    TORCH_CHECK(table_type_ok, op_name, ": ", kind, " must be ", table_types);
    TORCH_CHECK(padding_mode >= 0 && padding_mode <= 4, op_name, ": padding_mode must be 0..4");
}

inline bool is_integer_or_float(const Tensor &t) {
    return at::isFloatingType(t.scalar_type()) || at::isIntegralType(t.scalar_type(), false);
}

hipStream_t current_stream(const Tensor &t) { return c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

void check_same(const char *fn, const Tensor &a, const char *an, const Tensor &b, const char *bn) {
    TORCH_CHECK(a.get_device() == b.get_device(), "Expected tensor for ", an, " to be on the same device as tensor for ", bn,
                "; but ", an, " is on device ", a.get_device(), " and ", bn, " is on device ", b.get_device(),
                " (while checking arguments for ", fn, ")");
    TORCH_CHECK(a.scalar_type() == b.scalar_type(), "Expected tensor for ", an, " to have the same type as tensor for ", bn,
                "; but type ", c10::toString(a.scalar_type()), " does not equal ", c10::toString(b.scalar_type()),
                " (while checking arguments for ", fn, ")");
}

// Mixed precision: fp16 / bf16 tensors with fp32 weights, what torch.autocast hands these ops -- activations in the autocast type,
// parameters as they are.  (No Autocast-key registration is needed for that: an op without one falls through the key, and input and
// weight arrive as the caller holds them.)  Returns SHIFTND_WEIGHTS_F32 for that one combination and 0 for tensors of the same
// type; every other pair raises check_same's error.  grad_weights is allocated like the weights, so it comes back fp32.
int weights_flag(const char *fn, const Tensor &t, const char *tn, const Tensor &weights) {
    const bool half = t.scalar_type() == at::kHalf || t.scalar_type() == at::kBFloat16;
    if (!(half && weights.scalar_type() == at::kFloat && t.get_device() == weights.get_device())) {
        check_same(fn, t, tn, weights, "weights");
        return 0;
    }
    return SHIFTND_WEIGHTS_F32;
}

// ---- channels-last inputs ---------------------------------------------------------------------------------------
// The reference's CUDA backend walks a channels-last input through its strides (cuda/shifts_cuda.cu:217-262:
// uncoalesced) and returns an NCHW-contiguous result.  Here a dense channels-last tensor is first brought to the
// contiguous layout by shiftnd_transpose (a tile transpose at copy bandwidth, several times faster than ATen's layout
// copy), then the contiguous kernels run: for N16 C256 224x224 fp32 0.30 + 0.29 ms instead of 3.4 ms through strides.
bool is_channels_last_dense(const Tensor &t) {
    if (t.dim() < 3 || t.numel() == 0 || t.size(1) < 2 || t.is_contiguous()) return false;
    if (t.stride(1) != 1) return false;
    int64_t expect = t.size(1);
    for (int64_t d = t.dim() - 1; d >= 2; --d) {
        if (t.size(d) != 1 && t.stride(d) != expect) return false;
        expect *= t.size(d);
    }
    return t.size(0) == 1 || t.stride(0) == expect;
}

int64_t spatial_volume(const Tensor &t) {
    int64_t p = 1;
    for (int64_t d = 2; d < t.dim(); ++d) p *= t.size(d);
    return p;
}

// channels-last dense -> new contiguous tensor with the same values (works on int_repr bytes for quantized tensors)
Tensor channels_last_to_contiguous(const Tensor &t) {
    Tensor out = t.is_quantized()
                     ? at::_empty_affine_quantized(t.sizes(), t.options().memory_format(at::MemoryFormat::Contiguous), t.q_scale(),
                                                   t.q_zero_point(), c10::nullopt)
                     : at::empty(t.sizes(), t.options(), at::MemoryFormat::Contiguous);
    check_status(shiftnd_transpose(t.data_ptr(), out.data_ptr(), t.size(0), spatial_volume(t), t.size(1),
                                   static_cast<int32_t>(t.element_size()), current_stream(t)),
                 "shiftnd_transpose (HIP)");
    return out;
}

// contiguous `src` -> the channels-last dense tensor `dst` (same sizes)
void contiguous_to_channels_last(const Tensor &src, Tensor &dst) {
    check_status(shiftnd_transpose(src.data_ptr(), dst.data_ptr(), src.size(0), src.size(1), spatial_volume(src),
                                   static_cast<int32_t>(src.element_size()), current_stream(src)),
                 "shiftnd_transpose (HIP)");
}

template <int ND> Tensor shift_forward_hip(const Tensor &input_, const Tensor &weights, const Tensor &borders,
                                           at::IntArrayRef new_size, int64_t padding_mode, bool active_flag) {
    TORCH_CHECK(input_.is_cuda(), "input must be a CUDA tensor");
    TORCH_CHECK(weights.is_cuda(), "weights must be a CUDA tensor");
    const int mixed = weights_flag("shiftnd_forward_cuda", input_, "input", weights);
    TORCH_CHECK(input_.dim() == ND + 2, "shift", ND, "d: expected a ", ND + 2, "-D input");
    TORCH_CHECK(weights.dim() == 2 && weights.size(0) == input_.size(1) && weights.size(1) == ND,
                "shift", ND, "d: weights must have shape [C, ", ND, "]");
    if (padding_mode < 0 || padding_mode > 4) return Tensor();  // the reference's switch has no default
    c10::DeviceGuard device_guard(input_.device());
    const int dtype = to_shiftnd_dtype(input_.scalar_type(), "shiftnd_forward_cuda") | mixed;
    int32_t b[6];
    if (static_cast<int>(new_size.size()) == ND + 2) read_borders_for(borders, input_, new_size.slice(2), ND, b);
    else read_borders(borders, b);
    Tensor w = weights.contiguous();
    Tensor output = at::empty(new_size, input_.options(), at::MemoryFormat::Contiguous);
    shiftnd_problem p;
    fill_problem(p, ND, input_, b, padding_mode, active_flag, dtype);
    int64_t xs[5], os[5];
    fill_strides(output, ND, os);
    // a dense channels-last input: the library may have a kernel that reads it as it lies and writes the NCHW result
    // (shiftnd_cl_tiled.hip); otherwise one tile transpose, then the contiguous kernels
    bool direct = false;
    if (is_channels_last_dense(input_)) {
        fill_strides(input_, ND, xs);
        direct = shiftnd_forward_serves_channels_last(&p, input_.data_ptr(), xs, output.data_ptr(), os) != 0;
    }
    const Tensor input = (is_channels_last_dense(input_) && !direct) ? channels_last_to_contiguous(input_) : input_;
    fill_strides(input, ND, xs);
    check_status(shiftnd_forward(&p, input.data_ptr(), xs, w.data_ptr(), output.data_ptr(), os, current_stream(input)),
                 "shiftnd_forward (HIP)");
    return output;
}

template <int ND>
std::tuple<Tensor, Tensor> shift_backward_hip(const Tensor &grad_, const Tensor &weights, const Tensor &input_,
                                              const Tensor &borders, int64_t padding_mode, bool active_flag) {
    TORCH_CHECK(grad_.is_cuda(), "grad must be a CUDA tensor");
    TORCH_CHECK(input_.is_cuda(), "input must be a CUDA tensor");
    TORCH_CHECK(weights.is_cuda(), "weights must be a CUDA tensor");
    check_same("shiftnd_backward_cuda", grad_, "grad", input_, "input");
    const int mixed = weights_flag("shiftnd_backward_cuda", grad_, "grad", weights);
    TORCH_CHECK(input_.dim() == ND + 2 && grad_.dim() == ND + 2, "shift", ND, "d backward: expected ", ND + 2, "-D tensors");
    if (padding_mode < 0 || padding_mode > 4) return std::make_tuple(Tensor(), Tensor());
    c10::DeviceGuard device_guard(grad_.device());
    int32_t b[6];
    read_borders_for(borders, input_, grad_.sizes().slice(2), ND, b);
    for (int r = 0; r < ND; ++r)
        TORCH_CHECK(grad_.size(2 + r) == b[2 * r + 1] - b[2 * r], "shift", ND, "d backward: grad does not match borders");
    const int dtype = to_shiftnd_dtype(grad_.scalar_type(), "shiftnd_backward_cuda") | mixed;
    Tensor w = weights.contiguous();
    Tensor grad_weights = at::empty_like(w, at::MemoryFormat::Contiguous);   // (the weights' dtype: fp32 for a mixed call)
    // saved input dense channels-last, incoming gradient channels-last too or NCHW-contiguous (what follows the reference's
    // float forward, which returns NCHW for a channels-last input): the library may have a kernel for that layout
    // (shiftnd_cl_tiled.hip; grad_x comes out in the input's layout); otherwise change the layout once, then the
    // contiguous kernels
    bool direct = false;
    Tensor grad_input;
    if (is_channels_last_dense(input_) && (is_channels_last_dense(grad_) || grad_.is_contiguous())) {
        grad_input = at::empty_like(input_, input_.suggest_memory_format());
        shiftnd_problem pd;
        fill_problem(pd, ND, input_, b, padding_mode, active_flag, dtype);
        int64_t gd[5], xd[5], gxd[5];
        fill_strides(grad_, ND, gd);
        fill_strides(input_, ND, xd);
        fill_strides(grad_input, ND, gxd);
        direct = shiftnd_backward_serves_channels_last(&pd, grad_.data_ptr(), gd, input_.data_ptr(), xd, grad_input.data_ptr(), gxd) != 0;
    }
    const Tensor input = (is_channels_last_dense(input_) && !direct) ? channels_last_to_contiguous(input_) : input_;
    const Tensor grad = (is_channels_last_dense(grad_) && !direct) ? channels_last_to_contiguous(grad_) : grad_;
    if (!direct) grad_input = at::empty_like(input, at::MemoryFormat::Contiguous);
    shiftnd_problem p;
    fill_problem(p, ND, input, b, padding_mode, active_flag, dtype);
    const size_t ws_bytes = shiftnd_backward_workspace_bytes(&p);
    Tensor workspace = workspace_like(input, ws_bytes);
    int64_t gs[5], xs[5], gxs[5];
    fill_strides(grad, ND, gs);
    fill_strides(input, ND, xs);
    fill_strides(grad_input, ND, gxs);
    check_status(shiftnd_backward(&p, grad.data_ptr(), gs, input.data_ptr(), xs, w.data_ptr(), grad_input.data_ptr(), gxs,
                                  grad_weights.data_ptr(), workspace.data_ptr(), ws_bytes, current_stream(grad)),
                 "shiftnd_backward (HIP)");
    return std::make_tuple(grad_input, grad_weights);
}

// ---- shift + average pool as one op ------------------------------------------------------------------------
template <int ND> void check_pool(at::IntArrayRef pool) {
    TORCH_CHECK(static_cast<int>(pool.size()) == ND, "shift", ND, "d_pool: pool must hold ", ND, " window sizes");
    for (auto k : pool) TORCH_CHECK(k >= 1, "shift", ND, "d_pool: window sizes must be >= 1");
}

// what the pooled adapters prepare once `pool` has passed check_pool: the windows as the C ABI takes them (k) and the pooled
// spatial sizes of problem p (ps)
template <int ND> struct PoolArgs {
    int32_t k[3] = {1, 1, 1};
    int64_t ps[3];
    PoolArgs(const shiftnd_problem &p, at::IntArrayRef pool) {
        for (int r = 0; r < ND; ++r) k[r] = static_cast<int32_t>(pool[r]);
        check_status(shiftnd_pooled_sizes(&p, k, ps), "shiftnd_pooled_sizes");
    }
    std::vector<int64_t> output_size(const Tensor &input) const {
        std::vector<int64_t> osize = {input.size(0), input.size(1)};
        for (int r = 0; r < ND; ++r) osize.push_back(ps[r]);
        return osize;
    }
    void check_grad(const Tensor &grad, const char *op_suffix) const {   // op_suffix: "d_pool" / "d_fixed_pool"
        for (int r = 0; r < ND; ++r)
            TORCH_CHECK(grad.size(2 + r) == ps[r], "shift", ND, op_suffix, " backward: grad does not match the pooled size");
    }
};

// the reference's sequence: _reduction_fn(shift(x)) with avg_pool{N}d(kernel = stride = pool, ceil_mode=True)
// (modules/shifts.py:81-89, 150-153).  pool_forward_composed / pool_backward_composed are reached two ways, and both stay: as the
// CPU-key kernels of the pooled ops, and from the HIP adapters for a layout the fused kernels do not take or when the library
// answers SHIFTND_ERR_NOT_FUSED.
template <int ND> Tensor pool_forward_composed(const Tensor &input, const Tensor &weights, const Tensor &borders,
                                               at::IntArrayRef new_size, at::IntArrayRef pool, int64_t padding_mode,
                                               bool active_flag) {
    check_pool<ND>(pool);
    Tensor y = ShiftOps<ND>::forward().call(input, weights, borders, new_size, padding_mode, active_flag);
    if (!y.defined()) return y;
    if constexpr (ND == 1) return at::avg_pool1d(y, pool, pool, {0}, /*ceil_mode=*/true, /*count_include_pad=*/true);
    else if constexpr (ND == 2) return at::avg_pool2d(y, pool, pool, {0, 0}, true, true, c10::nullopt);
    else return at::avg_pool3d(y, pool, pool, {0, 0, 0}, true, true, c10::nullopt);
}

template <int ND>
std::tuple<Tensor, Tensor> pool_backward_composed(const Tensor &grad, const Tensor &weights, const Tensor &input,
                                                  const Tensor &borders, at::IntArrayRef pool, int64_t padding_mode,
                                                  bool active_flag) {
    check_pool<ND>(pool);
    int32_t b[6];
    read_borders(borders, b);
    std::vector<int64_t> ysize = {input.size(0), input.size(1)};
    for (int r = 0; r < ND; ++r) ysize.push_back(b[2 * r + 1] - b[2 * r]);
    Tensor y_like = at::empty(ysize, grad.options());  // avg_pool's backward only looks at its shape
    Tensor g;
    if constexpr (ND == 1) {
        g = at::avg_pool2d_backward(grad.unsqueeze(2), y_like.unsqueeze(2), {1, pool[0]}, {1, pool[0]}, {0, 0}, true, true,
                                    c10::nullopt).squeeze(2);
    } else if constexpr (ND == 2) {
        g = at::avg_pool2d_backward(grad, y_like, pool, pool, {0, 0}, true, true, c10::nullopt);
    } else {
        g = at::avg_pool3d_backward(grad, y_like, pool, pool, {0, 0, 0}, true, true, c10::nullopt);
    }
    return ShiftOps<ND>::backward().call(g, weights, input, borders, padding_mode, active_flag);
}

template <int ND> Tensor pool_forward_hip(const Tensor &input_, const Tensor &weights, const Tensor &borders,
                                          at::IntArrayRef new_size, at::IntArrayRef pool, int64_t padding_mode,
                                          bool active_flag) {
    check_pool<ND>(pool);
    TORCH_CHECK(input_.is_cuda(), "input must be a CUDA tensor");
    TORCH_CHECK(weights.is_cuda(), "weights must be a CUDA tensor");
    const int mixed = weights_flag("shiftnd_pool_forward_cuda", input_, "input", weights);
    TORCH_CHECK(input_.dim() == ND + 2, "shift", ND, "d_pool: expected a ", ND + 2, "-D input");
    TORCH_CHECK(weights.dim() == 2 && weights.size(0) == input_.size(1) && weights.size(1) == ND,
                "shift", ND, "d_pool: weights must have shape [C, ", ND, "]");
    if (padding_mode < 0 || padding_mode > 4) return Tensor();
    c10::DeviceGuard device_guard(input_.device());
    const Tensor input = is_channels_last_dense(input_) ? channels_last_to_contiguous(input_) : input_;
    if (!input.is_contiguous()) return pool_forward_composed<ND>(input, weights, borders, new_size, pool, padding_mode, active_flag);
    const int dtype = to_shiftnd_dtype(input.scalar_type(), "shiftnd_pool_forward_cuda") | mixed;
    int32_t b[6];
    read_borders(borders, b);
    shiftnd_problem p;
    fill_problem(p, ND, input, b, padding_mode, active_flag, dtype);
    const PoolArgs<ND> pa(p, pool);
    Tensor w = weights.contiguous();
    Tensor output = at::empty(pa.output_size(input), input.options(), at::MemoryFormat::Contiguous);
    const int rc = shiftnd_forward_pooled(&p, pa.k, input.data_ptr(), w.data_ptr(), output.data_ptr(), current_stream(input));
    if (rc == SHIFTND_ERR_NOT_FUSED)
        return pool_forward_composed<ND>(input, weights, borders, new_size, pool, padding_mode, active_flag);
    check_status(rc, "shiftnd_forward_pooled (HIP)");
    return output;
}

template <int ND>
std::tuple<Tensor, Tensor> pool_backward_hip(const Tensor &grad, const Tensor &weights, const Tensor &input_,
                                             const Tensor &borders, at::IntArrayRef pool, int64_t padding_mode,
                                             bool active_flag) {
    check_pool<ND>(pool);
    TORCH_CHECK(grad.is_cuda(), "grad must be a CUDA tensor");
    TORCH_CHECK(input_.is_cuda(), "input must be a CUDA tensor");
    TORCH_CHECK(weights.is_cuda(), "weights must be a CUDA tensor");
    check_same("shiftnd_pool_backward_cuda", grad, "grad", input_, "input");
    const int mixed = weights_flag("shiftnd_pool_backward_cuda", grad, "grad", weights);
    TORCH_CHECK(input_.dim() == ND + 2 && grad.dim() == ND + 2, "shift", ND, "d_pool backward: expected ", ND + 2, "-D tensors");
    if (padding_mode < 0 || padding_mode > 4) return std::make_tuple(Tensor(), Tensor());
    c10::DeviceGuard device_guard(grad.device());
    const Tensor input = is_channels_last_dense(input_) ? channels_last_to_contiguous(input_) : input_;
    if (!input.is_contiguous())
        return pool_backward_composed<ND>(grad, weights, input, borders, pool, padding_mode, active_flag);
    const int dtype = to_shiftnd_dtype(grad.scalar_type(), "shiftnd_pool_backward_cuda") | mixed;
    int32_t b[6];
    read_borders(borders, b);
    shiftnd_problem p;
    fill_problem(p, ND, input, b, padding_mode, active_flag, dtype);
    const PoolArgs<ND> pa(p, pool);
    pa.check_grad(grad, "d_pool");
    Tensor g = grad.contiguous();
    Tensor w = weights.contiguous();
    Tensor grad_input = at::empty_like(input, at::MemoryFormat::Contiguous);
    Tensor grad_weights = at::empty_like(w, at::MemoryFormat::Contiguous);   // (the weights' dtype)
    const size_t ws_bytes = shiftnd_backward_pooled_workspace_bytes(&p, pa.k);  // (the pooled plan, not the plain one)
    Tensor workspace = workspace_like(input, ws_bytes);
    const int rc = shiftnd_backward_pooled(&p, pa.k, g.data_ptr(), input.data_ptr(), w.data_ptr(), grad_input.data_ptr(),
                                           grad_weights.data_ptr(), workspace.data_ptr(), ws_bytes, current_stream(grad));
    if (rc == SHIFTND_ERR_NOT_FUSED)
        return pool_backward_composed<ND>(grad, weights, input, borders, pool, padding_mode, active_flag);
    check_status(rc, "shiftnd_backward_pooled (HIP)");
    return std::make_tuple(grad_input, grad_weights);
}

template <int ND> struct ShiftPoolFunction : public torch::autograd::Function<ShiftPoolFunction<ND>> {
    static variable_list forward(AutogradContext *ctx, const Tensor &input, const Tensor &weight, const Tensor &borders,
                                 at::IntArrayRef new_size, at::IntArrayRef pool, int64_t padding_mode, bool active_flag) {
        at::AutoDispatchBelowADInplaceOrView guard;
        auto output = PoolOps<ND>::forward().call(input, weight, borders, new_size, pool, padding_mode, active_flag);
        ctx->saved_data["padding_mode"] = padding_mode;
        ctx->saved_data["active_flag"] = active_flag;
        ctx->saved_data["pool"] = pool.vec();
        ctx->save_for_backward({input, weight, borders});
        return {output};
    }
    static variable_list backward(AutogradContext *ctx, const variable_list &grad_output) {
        auto saved = ctx->get_saved_variables();
        const auto padding_mode = ctx->saved_data["padding_mode"].toInt();
        const auto active_flag = ctx->saved_data["active_flag"].toBool();
        const auto pool = ctx->saved_data["pool"].toIntVector();
        auto result = PoolOps<ND>::backward().call(grad_output[0], saved[1], saved[0], saved[2], pool, padding_mode, active_flag);
        return {std::get<0>(result), std::get<1>(result), Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
    }
};
template <int ND> Tensor pool_autograd(const Tensor &input, const Tensor &weights, const Tensor &borders,
                                       at::IntArrayRef new_size, at::IntArrayRef pool, int64_t padding_mode,
                                       bool active_flag) {
    return ShiftPoolFunction<ND>::apply(input, weights, borders, new_size, pool, padding_mode, active_flag)[0];
}
template <int ND> Tensor shift_pool_public(const Tensor &input, const Tensor &weights, const Tensor &borders,
                                           at::IntArrayRef pool, int64_t padding_mode, bool active_flag) {
    auto bands = check_borders(input, borders, ND);
    return PoolOps<ND>::forward().call(input, weights, std::get<0>(bands), std::get<1>(bands), pool, padding_mode, active_flag);
}

// ---- quantized HIP forward (QuantizedCUDA key; new -- the reference only has QuantizedCPU) --------------
int quant_dtype(at::ScalarType t, const char *what) {
    switch (t) {
    case at::kQInt8: return SHIFTND_I8;
    case at::kQUInt8: return SHIFTND_U8;
    case at::kQInt32: return SHIFTND_I32;
    default: TORCH_CHECK(false, "\"", what, "\" not implemented for '", c10::toString(t), "'");
    }
    return -1;
}

template <int ND> Tensor qshift_forward_hip(const Tensor &input_, const Tensor &weights, const Tensor &borders,
                                            at::IntArrayRef new_size, int64_t padding_mode, bool /*active_flag*/) {
    TORCH_CHECK(input_.is_cuda() && input_.is_quantized(), "input must be a quantized CUDA tensor");
    TORCH_CHECK(weights.is_quantized(), "weights must be a quantized tensor");
    TORCH_CHECK(input_.dim() == ND + 2, "shift", ND, "d: expected a ", ND + 2, "-D input");
    if (padding_mode < 0 || padding_mode > 4) return Tensor();
    c10::DeviceGuard device_guard(input_.device());
    const int dtype = quant_dtype(input_.scalar_type(), "q_shiftnd_cuda");
    const int wdtype = quant_dtype(weights.scalar_type(), "q_shiftnd_cuda");
    int32_t b[6];
    if (static_cast<int>(new_size.size()) == ND + 2) read_borders_for(borders, input_, new_size.slice(2), ND, b);
    else read_borders(borders, b);
    Tensor wrepr = weights.int_repr().to(input_.device()).contiguous();
    TORCH_CHECK(wrepr.dim() == 2 && wrepr.size(0) == input_.size(1) && wrepr.size(1) == ND,
                "shift", ND, "d: weights must have shape [C, ", ND, "]");
    const bool cl = input_.is_contiguous(at::MemoryFormat::ChannelsLast) || input_.is_contiguous(at::MemoryFormat::ChannelsLast3d);
    // a channels-last input keeps its format (shifts_quantized.cpp:119-121).  Two tile transposes around the contiguous
    // kernel beat the channel-fastest kernel (N128 C512 56x56 quint8: 0.09 + 0.14 + 0.09 ms against 0.69 ms)
    bool via_transpose = cl && is_channels_last_dense(input_);
    Tensor out_cl;  // the channels-last result: written by the LDS-tiled kernel, or by the layout change at the end
    if (via_transpose) {  // the LDS-tiled channels-last kernel keeps the format in one pass
        out_cl = at::_empty_affine_quantized(new_size, input_.options().memory_format(input_.suggest_memory_format()),
                                                    input_.q_scale(), input_.q_zero_point(), c10::nullopt);
        shiftnd_problem pd;
        fill_problem(pd, ND, input_, b, padding_mode, false, dtype);
        int64_t xd[5], od[5];
        fill_strides(input_, ND, xd);
        fill_strides(out_cl, ND, od);
        if (shiftnd_forward_serves_channels_last(&pd, input_.data_ptr(), xd, out_cl.data_ptr(), od)) {
            check_status(shiftnd_forward_quantized(&pd, input_.data_ptr(), xd, wrepr.data_ptr(), wdtype, weights.q_zero_point(),
                                                   input_.q_zero_point(), out_cl.data_ptr(), od, current_stream(input_)),
                         "shiftnd_forward_quantized (HIP)");
            return out_cl;
        }
    }
    const Tensor input = via_transpose ? channels_last_to_contiguous(input_) : input_;
    Tensor output = (cl && !via_transpose)
                        ? at::_empty_affine_quantized(new_size, input.options().memory_format(input.suggest_memory_format()),
                                                      input.q_scale(), input.q_zero_point(), c10::nullopt)
                        : at::_empty_affine_quantized(new_size, input.options().memory_format(at::MemoryFormat::Contiguous),
                                                      input.q_scale(), input.q_zero_point(), c10::nullopt);
    shiftnd_problem p;
    fill_problem(p, ND, input, b, padding_mode, false, dtype);
    int64_t xs[5], os[5];
    fill_strides(input, ND, xs);
    fill_strides(output, ND, os);
    check_status(shiftnd_forward_quantized(&p, input.data_ptr(), xs, wrepr.data_ptr(), wdtype, weights.q_zero_point(),
                                           input.q_zero_point(), output.data_ptr(), os, current_stream(input)),
                 "shiftnd_forward_quantized (HIP)");
    if (via_transpose && output.numel() > 0 && output.size(1) > 1) {
        contiguous_to_channels_last(output, out_cl);  // (allocated above: one channels-last buffer per call either way)
        return out_cl;
    }
    return output;
}

// quantized shift + average pool (the tail of a quantized module that emulates a strided depthwise conv) as one op on
// the QuantizedCUDA key: one pass for int8 / uint8 (shiftnd_forward_quantized_pooled); other element types and
// non-contiguous inputs run the quantized shift and then ATen's QuantizedCPU pool arithmetic with float HIP ops on the
// integer representation (the same values).
//
// ATen's QuantizedCPU average pool rounds in two ways (include/shiftnd_hip.h: SHIFTND_REQUANT_*): its channels-last kernel
// -- taken for every 3-D tensor and for a 4-D tensor that is_contiguous(ChannelsLast), which a contiguous one with C == 1
// or H == W == 1 also is; avg_pool1d pools the [N, C, 1, L] view -- adds the zero point after the rounding, its contiguous
// kernel before.  `y_sizes` / `y_channels_last`: the shift output the reference's module would hand to its pool
// (ops/quantized/shifts_quantized.cpp:119-125 keeps a channels-last input's layout).
template <int ND> bool qpool_zp_outside(at::IntArrayRef y_sizes, bool y_channels_last) {
    if (ND == 3) return true;
    if (ND == 2 && y_channels_last) return true;
    const int64_t C = y_sizes[1], H = ND == 1 ? 1 : y_sizes[2], W = y_sizes[ND + 1];
    return C == 1 || (H == 1 && W == 1);
}

template <int ND> Tensor qpool_composite(const Tensor &y, at::IntArrayRef pool) {
    const int64_t zp = y.q_zero_point();
    Tensor xi = y.int_repr();
    Tensor xf = xi.to(at::kFloat) - static_cast<double>(zp);
    std::vector<int64_t> k(pool.begin(), pool.end());
    if (ND == 1) {  // (avg_pool1d has no divisor_override: pool a [N, C, 1, L] view)
        xf = xf.unsqueeze(2);
        k.insert(k.begin(), 1);
    }
    std::vector<int64_t> zeros(k.size(), 0);
    // the window counts: ones of the SPATIAL shape (an empty batch or zero channels must not be indexed -- the reference's
    // sequence returns an empty tensor for them)
    std::vector<int64_t> one_shape(xf.sizes().begin(), xf.sizes().end());
    one_shape[0] = one_shape[1] = 1;
    Tensor ones = at::ones(one_shape, xf.options());
    Tensor sums = ND == 3 ? at::avg_pool3d(xf, k, k, zeros, true, true, 1) : at::avg_pool2d(xf, k, k, zeros, true, true, 1);
    Tensor cnt = ND == 3 ? at::avg_pool3d(ones, k, k, zeros, true, true, 1) : at::avg_pool2d(ones, k, k, zeros, true, true, 1);
    const bool outside = qpool_zp_outside<ND>(y.sizes(), ND == 2 && y.is_contiguous(at::MemoryFormat::ChannelsLast));
    Tensor mult = cnt.to(at::kDouble).reciprocal().to(at::kFloat);  // float(1 / count)
    Tensor res = outside ? at::round(sums * mult) + static_cast<double>(zp)
                         : at::round(sums * mult.reciprocal().reciprocal() + static_cast<double>(zp));
    if (ND == 1) res = res.squeeze(2);
    double lo = 0, hi = 255;
    if (xi.scalar_type() == at::kChar) { lo = -128; hi = 127; }
    if (xi.scalar_type() == at::kInt) { lo = -2147483648.0; hi = 2147483647.0; }
    res = res.clamp_(lo, hi).to(xi.scalar_type());
    return at::_make_per_tensor_quantized_tensor(res, y.q_scale(), zp);
}

template <int ND> Tensor qpool_forward_hip(const Tensor &input_, const Tensor &weights, const Tensor &borders,
                                           at::IntArrayRef new_size, at::IntArrayRef pool, int64_t padding_mode, bool active_flag) {
    check_pool<ND>(pool);
    TORCH_CHECK(input_.is_cuda() && input_.is_quantized(), "input must be a quantized CUDA tensor");
    TORCH_CHECK(weights.is_quantized(), "weights must be a quantized tensor");
    TORCH_CHECK(input_.dim() == ND + 2, "shift", ND, "d_pool: expected a ", ND + 2, "-D input");
    if (padding_mode < 0 || padding_mode > 4) return Tensor();
    c10::DeviceGuard device_guard(input_.device());
    const int dtype = quant_dtype(input_.scalar_type(), "q_shiftnd_pool_cuda");
    const int wdtype = quant_dtype(weights.scalar_type(), "q_shiftnd_pool_cuda");
    if (input_.is_contiguous() && (dtype == SHIFTND_I8 || dtype == SHIFTND_U8)) {
        int32_t b[6];
        read_borders(borders, b);
        Tensor wrepr = weights.int_repr().to(input_.device()).contiguous();
        TORCH_CHECK(wrepr.dim() == 2 && wrepr.size(0) == input_.size(1) && wrepr.size(1) == ND,
                    "shift", ND, "d_pool: weights must have shape [C, ", ND, "]");
        shiftnd_problem p;
        fill_problem(p, ND, input_, b, padding_mode, false, dtype);
        const PoolArgs<ND> pa(p, pool);
        std::vector<int64_t> ysize = {input_.size(0), input_.size(1)};
        for (int r = 0; r < ND; ++r) ysize.push_back(b[2 * r + 1] - b[2 * r]);
        const int32_t requant = qpool_zp_outside<ND>(ysize, false) ? SHIFTND_REQUANT_ZP_OUTSIDE : SHIFTND_REQUANT_ZP_INSIDE;
        Tensor output = at::_empty_affine_quantized(pa.output_size(input_), input_.options().memory_format(at::MemoryFormat::Contiguous),
                                                    input_.q_scale(), input_.q_zero_point(), c10::nullopt);
        const int rc = shiftnd_forward_quantized_pooled(&p, pa.k, input_.data_ptr(), wrepr.data_ptr(), wdtype, weights.q_zero_point(),
                                                        input_.q_zero_point(), requant, output.data_ptr(), current_stream(input_));
        if (rc == SHIFTND_OK) return output;
        TORCH_CHECK(rc == SHIFTND_ERR_NOT_FUSED, "shiftnd_forward_quantized_pooled (HIP): ", shiftnd_status_string(rc));
    }
    return qpool_composite<ND>(qshift_forward_hip<ND>(input_, weights, borders, new_size, padding_mode, active_flag), pool);
}

std::tuple<Tensor, Tensor> qshift_backward(const Tensor &, const Tensor &, const Tensor &, const Tensor &, int64_t, bool) {
    TORCH_CHECK(0, "backwards on quantized tensor are not supported");
}

// ---- fixed (grouped) shifts: integer shifts that nobody learns ------------------------------------------------------
// shift{N}d_fixed(input, shifts, borders, padding_mode) is the sparse forward under a [C, N] table of integers; its autograd node
// keeps the table, the borders and the input's SIZES -- never the input -- and its backward is _shift{N}d_fixed_backward, the input
// gradient alone (on HIP tensors shiftnd_backward's x == NULL form: no read of x, no weight gradient).  The table is converted once
// to the tensor's dtype: exact for |s| <= 256 in bf16, <= 2048 in fp16, 2^24 in fp32.
Tensor fixed_table(const Tensor &shifts, const Tensor &like, int nd) {
    TORCH_CHECK(like.dim() == nd + 2, "shift", nd, "d_fixed: expected a ", nd + 2, "-D tensor");
    TORCH_CHECK(shifts.dim() == 2 && shifts.size(0) == like.size(1) && shifts.size(1) == nd,
                "shift", nd, "d_fixed: shifts must have shape [C, ", nd, "]");
    TORCH_CHECK(shifts.device() == like.device(), "shift", nd, "d_fixed: shifts must be on the input's device");
    TORCH_CHECK(is_integer_or_float(shifts), "shift", nd, "d_fixed: shifts must be integers or floats");
    return shifts.detach().to(like.scalar_type()).contiguous();
}

template <int ND> struct FixedShiftFunction : public torch::autograd::Function<FixedShiftFunction<ND>> {
    static variable_list forward(AutogradContext *ctx, const Tensor &input, const Tensor &shifts, const Tensor &borders,
                                 at::IntArrayRef new_size, int64_t padding_mode) {
        at::AutoDispatchBelowADInplaceOrView guard;
        Tensor table = fixed_table(shifts, input, ND);
        auto output = ShiftOps<ND>::forward().call(input, table, borders, new_size, padding_mode, false);
        ctx->saved_data["padding_mode"] = padding_mode;
        ctx->saved_data["input_size"] = input.sizes().vec();
        ctx->save_for_backward({table, borders});
        return {output};
    }
    static variable_list backward(AutogradContext *ctx, const variable_list &grad_output) {
        auto saved = ctx->get_saved_variables();
        const auto padding_mode = ctx->saved_data["padding_mode"].toInt();
        const auto input_size = ctx->saved_data["input_size"].toIntVector();
        return {FixedOps<ND>::backward().call(grad_output[0], saved[0], saved[1], input_size, padding_mode), Tensor(), Tensor(), Tensor(),
                Tensor()};
    }
};

// (`d_fixed:` in the quantized refusal of the pooled entry below is a known slip of the prefix, DESIGN section 3.32: kept)
template <int ND> Tensor shift_fixed_public(const Tensor &input, const Tensor &shifts, const Tensor &borders, int64_t padding_mode) {
    TORCH_CHECK(!input.is_quantized(), "shift", ND, "d_fixed: quantized inputs are not supported (the quantized modules already shift by integers)");
    TORCH_CHECK(padding_mode >= 0 && padding_mode <= 4, "shift", ND, "d_fixed: padding_mode must be 0..4");
    auto bands = check_borders(input, borders, ND);
    return FixedShiftFunction<ND>::apply(input, shifts, std::get<0>(bands), at::IntArrayRef(std::get<1>(bands)), padding_mode)[0];
}

template <int ND> Tensor shift_fixed_backward_hip(const Tensor &grad_, const Tensor &shifts, const Tensor &borders,
                                                  at::IntArrayRef input_size, int64_t padding_mode) {
    TORCH_CHECK(grad_.is_cuda(), "grad must be a CUDA tensor");
    TORCH_CHECK(grad_.dim() == ND + 2 && static_cast<int>(input_size.size()) == ND + 2, "shift", ND, "d_fixed backward: expected ",
                ND + 2, "-D tensors");
    TORCH_CHECK(padding_mode >= 0 && padding_mode <= 4, "shift", ND, "d_fixed backward: padding_mode must be 0..4");
    TORCH_CHECK(grad_.size(0) == input_size[0] && grad_.size(1) == input_size[1], "shift", ND, "d_fixed backward: grad does not match input_size");
    c10::DeviceGuard device_guard(grad_.device());
    int32_t b[6];
    read_borders(borders, b);
    bool cut = false;
    for (int r = 0; r < ND; ++r) {
        TORCH_CHECK(grad_.size(2 + r) == b[2 * r + 1] - b[2 * r], "shift", ND, "d_fixed backward: grad does not match borders");
        cut = cut || b[2 * r] != 0 || b[2 * r + 1] != input_size[2 + r];
    }
    const int dtype = to_shiftnd_dtype(grad_.scalar_type(), "shiftnd_fixed_backward_cuda");
    Tensor w = fixed_table(shifts, grad_, ND);
    Tensor grad_input = at::empty(input_size, grad_.options(), at::MemoryFormat::Contiguous);
    shiftnd_problem p;
    fill_problem(p, ND, grad_input, b, padding_mode, false, dtype);
    int64_t gs[5], gxs[5];
    fill_strides(grad_input, ND, gxs);
    // a dense channels-last gradient: the whole-input window runs the forward routes, which may read it as it lies; otherwise (and
    // for every cut window) one tile transpose, then the contiguous kernels
    bool direct = false;
    if (is_channels_last_dense(grad_) && !cut) {
        fill_strides(grad_, ND, gs);
        direct = shiftnd_forward_serves_channels_last(&p, grad_.data_ptr(), gs, grad_input.data_ptr(), gxs) != 0;
    }
    const Tensor grad = (is_channels_last_dense(grad_) && !direct) ? channels_last_to_contiguous(grad_) : grad_;
    fill_strides(grad, ND, gs);
    // the whole-input window needs room for the negated table (include/shiftnd_hip.h); a cut window needs nothing
    const size_t ws_bytes = cut ? 0 : static_cast<size_t>(w.numel()) * w.element_size();
    Tensor workspace = workspace_like(grad, ws_bytes);
    check_status(shiftnd_backward(&p, grad.data_ptr(), gs, nullptr, nullptr, w.data_ptr(), grad_input.data_ptr(), gxs, nullptr,
                                  ws_bytes ? workspace.data_ptr() : nullptr, ws_bytes, current_stream(grad)),
                 "shiftnd_backward, input gradient only (HIP)");
    return grad_input;
}

// ---- fixed shifts with a stride: shift{N}d_fixed_pool = avg_pool(shift{N}d_fixed(x)), kernel = stride = pool, ceil_mode ----------
// The forward is _shift{N}d_pool_forward under the converted table (on HIP tensors the fused sparse forward, active = 0; composed
// where that answers NOT_FUSED; on CPU tensors the two-step sequence).  The node keeps the table, the borders, the input's sizes and
// the pool -- never the input, never a full-size tensor -- and its backward is _shift{N}d_fixed_pool_backward: on HIP tensors
// shiftnd_backward_pooled's x == NULL form, a gather of the pooled gradient with one division.
template <int ND> struct FixedShiftPoolFunction : public torch::autograd::Function<FixedShiftPoolFunction<ND>> {
    static variable_list forward(AutogradContext *ctx, const Tensor &input, const Tensor &shifts, const Tensor &borders,
                                 at::IntArrayRef new_size, at::IntArrayRef pool, int64_t padding_mode) {
        at::AutoDispatchBelowADInplaceOrView guard;
        Tensor table = fixed_table(shifts, input, ND);
        auto output = PoolOps<ND>::forward().call(input, table, borders, new_size, pool, padding_mode, false);
        ctx->saved_data["padding_mode"] = padding_mode;
        ctx->saved_data["input_size"] = input.sizes().vec();
        ctx->saved_data["pool"] = pool.vec();
        ctx->save_for_backward({table, borders});
        return {output};
    }
    static variable_list backward(AutogradContext *ctx, const variable_list &grad_output) {
        auto saved = ctx->get_saved_variables();
        const auto padding_mode = ctx->saved_data["padding_mode"].toInt();
        const auto input_size = ctx->saved_data["input_size"].toIntVector();
        const auto pool = ctx->saved_data["pool"].toIntVector();
        return {FixedPoolOps<ND>::backward().call(grad_output[0], saved[0], saved[1], input_size, pool, padding_mode), Tensor(), Tensor(),
                Tensor(), Tensor(), Tensor()};
    }
};

template <int ND> Tensor shift_fixed_pool_public(const Tensor &input, const Tensor &shifts, const Tensor &borders, at::IntArrayRef pool,
                                                 int64_t padding_mode) {
    TORCH_CHECK(!input.is_quantized(), "shift", ND, "d_fixed: quantized inputs are not supported (the quantized modules already shift by integers)");
    TORCH_CHECK(padding_mode >= 0 && padding_mode <= 4, "shift", ND, "d_fixed_pool: padding_mode must be 0..4");
    check_pool<ND>(pool);
    auto bands = check_borders(input, borders, ND);
    return FixedShiftPoolFunction<ND>::apply(input, shifts, std::get<0>(bands), at::IntArrayRef(std::get<1>(bands)), pool, padding_mode)[0];
}

template <int ND> Tensor shift_fixed_pool_backward_hip(const Tensor &grad_, const Tensor &shifts, const Tensor &borders,
                                                       at::IntArrayRef input_size, at::IntArrayRef pool, int64_t padding_mode) {
    check_pool<ND>(pool);
    TORCH_CHECK(grad_.is_cuda(), "grad must be a CUDA tensor");
    TORCH_CHECK(grad_.dim() == ND + 2 && static_cast<int>(input_size.size()) == ND + 2, "shift", ND, "d_fixed_pool backward: expected ",
                ND + 2, "-D tensors");
    TORCH_CHECK(padding_mode >= 0 && padding_mode <= 4, "shift", ND, "d_fixed_pool backward: padding_mode must be 0..4");
    TORCH_CHECK(grad_.size(0) == input_size[0] && grad_.size(1) == input_size[1], "shift", ND,
                "d_fixed_pool backward: grad does not match input_size");
    c10::DeviceGuard device_guard(grad_.device());
    int32_t b[6];
    read_borders(borders, b);
    const int dtype = to_shiftnd_dtype(grad_.scalar_type(), "shiftnd_fixed_pool_backward_cuda");
    Tensor w = fixed_table(shifts, grad_, ND);
    Tensor grad_input = at::empty(input_size, grad_.options(), at::MemoryFormat::Contiguous);
    shiftnd_problem p;
    fill_problem(p, ND, grad_input, b, padding_mode, false, dtype);
    const PoolArgs<ND> pa(p, pool);
    pa.check_grad(grad_, "d_fixed_pool");
    // the pooled entry points take contiguous tensors: a dense channels-last gradient through the tile transpose, any other layout
    // through ATen's copy
    const Tensor grad = is_channels_last_dense(grad_) ? channels_last_to_contiguous(grad_) : grad_.contiguous();
    check_status(shiftnd_backward_pooled(&p, pa.k, grad.data_ptr(), nullptr, w.data_ptr(), grad_input.data_ptr(), nullptr, nullptr, 0,
                                         current_stream(grad)),
                 "shiftnd_backward_pooled, input gradient only (HIP)");
    return grad_input;
}

// ---- temporal shift (TSM, arXiv 1811.08383): fixed shifts across the frames of [N*T, C, ...] --------------------------------
// temporal_shift(input, shifts, n_segment, padding_mode): every run of n_segment consecutive rows of dim 0 is one clip, and
// channel c of frame t is channel c of frame pad(t - shifts[c]) of the same clip -- shift2d_fixed of the [N, C, T, M] view under
// the table (s_c, 0), without the two layout changes that view would cost.  The autograd node keeps the table alone; the backward
// is _temporal_shift_backward, the same gather under -s.  On HIP tensors both are ONE shiftnd_forward / shiftnd_backward
// (x == NULL form) call on the strides {T*C*M, M, C*M, 1}, which shiftnd_segment.hip serves at copy rate.
// (temporal_check and temporal_quantized_check are also called from torch_cpu_backend.cpp)
void temporal_check(const Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    TORCH_CHECK(!input.is_quantized(), "temporal_shift: quantized inputs are not supported");
    segment_check("temporal_shift", input, shifts, n_segment, padding_mode, "shifts", is_integer_or_float(shifts), "integers or floats");
}

// the node of temporal_shift (TemporalOps) and of temporal_shift_cl (TemporalClOps)
template <class Ops> struct TemporalShiftFunction : public torch::autograd::Function<TemporalShiftFunction<Ops>> {
    static variable_list forward(AutogradContext *ctx, const Tensor &input, const Tensor &shifts, int64_t n_segment,
                                 int64_t padding_mode) {
        at::AutoDispatchBelowADInplaceOrView guard;
        auto output = Ops::forward().call(input, shifts, n_segment, padding_mode);
        ctx->saved_data["n_segment"] = n_segment;
        ctx->saved_data["padding_mode"] = padding_mode;
        ctx->save_for_backward({shifts.detach()});
        return {output};
    }
    static variable_list backward(AutogradContext *ctx, const variable_list &grad_output) {
        auto saved = ctx->get_saved_variables();
        return {Ops::backward().call(grad_output[0], saved[0], ctx->saved_data["n_segment"].toInt(), ctx->saved_data["padding_mode"].toInt()),
                Tensor(), Tensor(), Tensor()};
    }
};

template <class Ops> Tensor temporal_autograd(const Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    temporal_check(input, shifts, n_segment, padding_mode);
    return TemporalShiftFunction<Ops>::apply(input, shifts, n_segment, padding_mode)[0];
}

template <class Ops> Tensor temporal_autograd_backward(const Tensor &grad, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    temporal_check(grad, shifts, n_segment, padding_mode);
    return GuardedBackward<Ops>::kernel(grad, shifts, n_segment, padding_mode);
}

// one C-ABI call on the segment-major strides; backward: the input gradient through shiftnd_backward's x == NULL form, which takes
// the table as the forward does and negates it in the workspace.  The table is this route's own and stays here: [C, 2] of the
// TENSOR's dtype (that form takes no fp32 table for a 16-bit tensor), where temporal_cl_hip below builds a [C] table, fp32 for
// 16-bit tensors, negates it itself and calls shiftnd_forward in both directions.
Tensor temporal_hip(const Tensor &t_, const Tensor &shifts, int64_t n_segment, int64_t padding_mode, bool backward) {
    TORCH_CHECK(t_.is_cuda(), "temporal_shift: expected a CUDA tensor");
    temporal_check(t_, shifts, n_segment, padding_mode);
    c10::DeviceGuard device_guard(t_.device());
    const int dtype = to_shiftnd_dtype(t_.scalar_type(), "temporal_shift_cuda");
    const Tensor t = t_.contiguous();
    Tensor out = at::empty(t.sizes(), t.options(), at::MemoryFormat::Contiguous);
    if (t.numel() == 0) return out;   // (after allocating; the _cl adapters never see an empty tensor: it is not channels-last dense)
    // [C, 2], column 1 (the planes' own dim) zero: built on the device, no host sync.  Like fixed_table: exact for |s| <= 256 in
    // bf16, <= 2048 in fp16
    Tensor w = at::zeros({t.size(1), 2}, t.options());
    w.select(1, 0).copy_(shifts.detach().reshape({t.size(1)}));
    shiftnd_problem p;
    int64_t st[5];
    segment_problem(p, st, t, n_segment, padding_mode, false, dtype, false, "temporal_shift");
    int rc;
    if (!backward) {
        rc = shiftnd_forward(&p, t.data_ptr(), st, w.data_ptr(), out.data_ptr(), st, current_stream(t));
    } else {
        const size_t ws_bytes = static_cast<size_t>(w.numel()) * w.element_size();
        Tensor workspace = workspace_like(t, ws_bytes);
        rc = shiftnd_backward(&p, t.data_ptr(), st, nullptr, nullptr, w.data_ptr(), out.data_ptr(), st, nullptr, workspace.data_ptr(),
                              ws_bytes, current_stream(t));
    }
    check_status(rc, "temporal_shift (HIP)");
    return out;
}

Tensor temporal_forward_hip(const Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    return temporal_hip(input, shifts, n_segment, padding_mode, false);
}
Tensor temporal_backward_hip(const Tensor &grad, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    return temporal_hip(grad, shifts, n_segment, padding_mode, true);
}

// ---- quantized temporal shift: temporal_shift_quantized(input, shifts, n_segment, padding_mode) -------------------------------------
// The gather of temporal_shift on the int_repr of a per-tensor quantized tensor (quint8, qint8, qint32): a plane is copied, or
// filled with the input's zero point, which dequantizes to exactly 0.  Scale and zero point pass through -- no requantization, no
// gradient.  A separate op: temporal_shift itself refuses quantized tensors.
void temporal_quantized_check(const Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    TORCH_CHECK(input.is_quantized(), "temporal_shift_quantized: expected a quantized input");
    TORCH_CHECK(input.qscheme() == at::kPerTensorAffine, "temporal_shift_quantized: expected a per-tensor quantized input");
    segment_check("temporal_shift_quantized", input, shifts, n_segment, padding_mode, "shifts",
                  !shifts.is_quantized() && is_integer_or_float(shifts), "integers or floats");
}

// the quantized routes' table: int32, rounded half to even like the sparse shift's weights -- exact for every shift, unlike the
// float op's table of the tensor dtype.  [C] here; the segment-major route pads it to [C, 2], the channels-last route has no such form
Tensor quantized_shift_table(const Tensor &shifts, int64_t C) {
    const Tensor s = shifts.detach().reshape({C});
    return at::isFloatingType(s.scalar_type()) ? at::round(s) : s;
}

// ONE shiftnd_forward_quantized call on the segment-major strides (shiftnd_segment.hip).  The table is [C, 2] int32 with column 1
// zero, built on the device without a host sync
Tensor temporal_quantized_hip(const Tensor &input_, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    TORCH_CHECK(input_.is_cuda(), "temporal_shift_quantized: expected a CUDA tensor");
    temporal_quantized_check(input_, shifts, n_segment, padding_mode);
    c10::DeviceGuard device_guard(input_.device());
    const int dtype = quant_dtype(input_.scalar_type(), "temporal_shift_quantized_cuda");
    const Tensor t = input_.contiguous();
    Tensor out = at::_empty_affine_quantized(t.sizes(), t.options().memory_format(at::MemoryFormat::Contiguous), t.q_scale(),
                                             t.q_zero_point(), c10::nullopt);
    if (t.numel() == 0) return out;
    shiftnd_problem p;
    int64_t st[5];
    segment_problem(p, st, t, n_segment, padding_mode, false, dtype, false, "temporal_shift_quantized");
    Tensor w = at::zeros({t.size(1), 2}, t.options().dtype(at::kInt));
    w.select(1, 0).copy_(quantized_shift_table(shifts, t.size(1)));
    check_status(shiftnd_forward_quantized(&p, t.data_ptr(), st, w.data_ptr(), SHIFTND_I32, 0, t.q_zero_point(), out.data_ptr(), st,
                                           current_stream(t)),
                 "temporal_shift_quantized (HIP)");
    return out;
}

// ---- channels-last temporal shift: temporal_shift_cl / _temporal_shift_cl_backward / temporal_shift_quantized_cl ----------------
// The values of temporal_shift / temporal_shift_quantized with the layout of the argument kept (memory_format=torch.preserve_format
// in the Python wrappers): a dense channels-last tensor (is_channels_last_dense: 3 to 5 dims, unit channel stride) comes back in its
// own strides, every other tensor exactly as the plain ops return it.  On HIP tensors a channels-last tensor is ONE flagged C-ABI
// call on the tensor as it lies (SHIFTND_SHIFT_DIM0 on the strides {T*M*C, 1, M*C, C}: shiftnd_frames.hip), no layout change in
// either direction; the gradient is the same call on the gradient under the negated table.  On CPU tensors the plain op computes
// and the result is laid out in the argument's strides.
// Every _cl adapter on HIP tensors goes in this order: not dense channels-last -> the plain adapter; then the device check; then
// the argument check.  Their 32-bit refusal speaks as `temporal_shift:`, for the learnable pair too (a known slip).
Tensor empty_with_strides_of(const Tensor &t) {
    if (!t.is_quantized()) return at::empty_strided(t.sizes(), t.strides(), t.options());
    // quantized: dense storage in memory order (dim 0, spatial dims, channels), seen with the channels as dim 1
    std::vector<int64_t> sizes{t.size(0)}, order{0, t.dim() - 1};
    for (int64_t d = 2; d < t.dim(); ++d) {
        sizes.push_back(t.size(d));
        order.push_back(d - 1);
    }
    sizes.push_back(t.size(1));
    Tensor out = at::_empty_affine_quantized(sizes, t.options().memory_format(at::MemoryFormat::Contiguous), t.q_scale(), t.q_zero_point(),
                                             c10::nullopt)
                     .permute(order);
    return out.strides() == t.strides() ? out : out.as_strided(t.sizes(), t.strides());   // (dims of size 1: the argument's own strides)
}

Tensor in_layout_of(const Tensor &values, const Tensor &like) {
    if (!is_channels_last_dense(like)) return values;
    Tensor out = empty_with_strides_of(like);
    out.copy_(values);
    return out;
}

// CPU tensors (reached below the Autograd key): the plain ops' values in the argument's layout
Tensor temporal_cl_forward_cpu(const Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    return in_layout_of(TemporalOps::forward().call(input, shifts, n_segment, padding_mode), input);
}
Tensor temporal_cl_backward_cpu(const Tensor &grad, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    return in_layout_of(TemporalOps::backward().call(grad, shifts, n_segment, padding_mode), grad);
}
Tensor temporal_quantized_cl_cpu(const Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    static auto plain = typed_op<temporal_sig>("temporal_shift_quantized");
    return in_layout_of(plain.call(input, shifts, n_segment, padding_mode), input);
}

// a dense channels-last tensor: ONE flagged shiftnd_forward on the tensor as it lies; backward: the same call under the negated
// table (grad_x[t] = grad_out[pad(t + s)]).  The [C] table is built on the device without a host sync: fp32 for 16-bit tensors
// (SHIFTND_WEIGHTS_F32: every shift exact), the tensor's dtype for fp32 / fp64.  Every other tensor: the plain op.
Tensor temporal_cl_hip(const Tensor &t, const Tensor &shifts, int64_t n_segment, int64_t padding_mode, bool backward) {
    if (!is_channels_last_dense(t)) return temporal_hip(t, shifts, n_segment, padding_mode, backward);
    TORCH_CHECK(t.is_cuda(), "temporal_shift_cl: expected a CUDA tensor");
    temporal_check(t, shifts, n_segment, padding_mode);
    c10::DeviceGuard device_guard(t.device());
    const bool half = t.scalar_type() == at::kHalf || t.scalar_type() == at::kBFloat16;
    const int dtype = to_shiftnd_dtype(t.scalar_type(), "temporal_shift_cl_cuda") | (half ? SHIFTND_WEIGHTS_F32 : 0);
    Tensor out = at::empty_strided(t.sizes(), t.strides(), t.options());
    Tensor w = shifts.detach().reshape({t.size(1)}).to(half ? at::kFloat : t.scalar_type());
    w = backward ? w.neg() : w.contiguous();
    shiftnd_problem p;
    int64_t st[5];
    segment_problem(p, st, t, n_segment, padding_mode, false, dtype | SHIFTND_SHIFT_DIM0, true, "temporal_shift");
    check_status(shiftnd_forward(&p, t.data_ptr(), st, w.data_ptr(), out.data_ptr(), st, current_stream(t)), "temporal_shift_cl (HIP)");
    return out;
}

Tensor temporal_cl_forward_hip(const Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    return temporal_cl_hip(input, shifts, n_segment, padding_mode, false);
}
Tensor temporal_cl_backward_hip(const Tensor &grad, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    return temporal_cl_hip(grad, shifts, n_segment, padding_mode, true);
}

// ... of a quantized tensor: ONE flagged shiftnd_forward_quantized, an int32 [C] table, the zero point as the fill
Tensor temporal_quantized_cl_hip(const Tensor &t, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    if (!is_channels_last_dense(t)) return temporal_quantized_hip(t, shifts, n_segment, padding_mode);
    TORCH_CHECK(t.is_cuda(), "temporal_shift_quantized_cl: expected a CUDA tensor");
    temporal_quantized_check(t, shifts, n_segment, padding_mode);
    c10::DeviceGuard device_guard(t.device());
    const int dtype = quant_dtype(t.scalar_type(), "temporal_shift_quantized_cl_cuda");
    Tensor out = empty_with_strides_of(t);
    const Tensor w = quantized_shift_table(shifts, t.size(1)).to(at::kInt).contiguous();
    shiftnd_problem p;
    int64_t st[5];
    segment_problem(p, st, t, n_segment, padding_mode, false, dtype | SHIFTND_SHIFT_DIM0, true, "temporal_shift");
    check_status(shiftnd_forward_quantized(&p, t.data_ptr(), st, w.data_ptr(), SHIFTND_I32, 0, t.q_zero_point(), out.data_ptr(), st,
                                           current_stream(t)),
                 "temporal_shift_quantized_cl (HIP)");
    return out;
}

// ---- learnable temporal shift: a TRAINED per-channel shift across the frames of [N*T, C, ...] ------------------------------------
// temporal_shift_learnable(input, weights, n_segment, padding_mode, active_flag) ==
//     shift1d(x.view(N, T, C, M).permute(0, 3, 2, 1).reshape(N*M, C, T), weights.view(C, 1), padding_mode, active_flag)
//         .view(N, M, C, T).permute(0, 3, 2, 1).reshape(x.shape)
// and its gradients are that expression's.  The CPU key is literally that, on the CPU 1-D ops; on HIP tensors forward and backward
// are ONE shiftnd_forward / shiftnd_backward call each under SHIFTND_SHIFT_DIM0 on the strides {T*C*M, M, C*M, 1}
// (shiftnd_tshift.hip): no layout change, no table.  The autograd node keeps the input and the weights.
void tsl_check(const Tensor &input, const Tensor &weights, int64_t n_segment, int64_t padding_mode) {
    TORCH_CHECK(!input.is_quantized(), "temporal_shift_learnable: quantized inputs are not supported");
    segment_check("temporal_shift_learnable", input, weights, n_segment, padding_mode, "weights",
                  at::isFloatingType(weights.scalar_type()), "floats");
}

// the public entry, the node and the two Autograd-key kernels of temporal_shift_learnable (LearnableOps) and of
// temporal_shift_learnable_cl (LearnableClOps, whose node keeps the input as it lies: no copy)
template <class Ops> Tensor tsl_public(const Tensor &input, const Tensor &weights, int64_t n_segment, int64_t padding_mode, bool active_flag) {
    tsl_check(input, weights, n_segment, padding_mode);
    return Ops::forward().call(input, weights, n_segment, padding_mode, active_flag);
}

template <class Ops> struct LearnableTemporalShiftFunction : public torch::autograd::Function<LearnableTemporalShiftFunction<Ops>> {
    static variable_list forward(AutogradContext *ctx, const Tensor &input, const Tensor &weights, int64_t n_segment,
                                 int64_t padding_mode, bool active_flag) {
        at::AutoDispatchBelowADInplaceOrView guard;
        auto output = Ops::forward().call(input, weights, n_segment, padding_mode, active_flag);
        ctx->saved_data["n_segment"] = n_segment;
        ctx->saved_data["padding_mode"] = padding_mode;
        ctx->saved_data["active_flag"] = active_flag;
        ctx->save_for_backward({input, weights});
        return {output};
    }
    static variable_list backward(AutogradContext *ctx, const variable_list &grad_output) {
        auto saved = ctx->get_saved_variables();
        auto result = Ops::backward().call(grad_output[0], saved[1], saved[0], ctx->saved_data["n_segment"].toInt(),
                                           ctx->saved_data["padding_mode"].toInt(), ctx->saved_data["active_flag"].toBool());
        return {std::get<0>(result), std::get<1>(result), Tensor(), Tensor(), Tensor()};
    }
};

template <class Ops> Tensor tsl_autograd(const Tensor &input, const Tensor &weights, int64_t n_segment, int64_t padding_mode, bool active_flag) {
    tsl_check(input, weights, n_segment, padding_mode);
    return LearnableTemporalShiftFunction<Ops>::apply(input, weights, n_segment, padding_mode, active_flag)[0];
}
template <class Ops>
std::tuple<Tensor, Tensor> tsl_autograd_backward(const Tensor &grad, const Tensor &weights, const Tensor &input, int64_t n_segment,
                                                 int64_t padding_mode, bool active_flag) {
    tsl_check(input, weights, n_segment, padding_mode);
    return GuardedBackward<Ops>::kernel(grad, weights, input, n_segment, padding_mode, active_flag);
}

// CPU tensors: the definition, on the CPU key's 1-D forward / backward (torch_cpu_backend.cpp) for the dtypes they take
Tensor tsl_lines(const Tensor &t, int64_t T) {   // [N*T, C, ...] -> [N*M, C, T], contiguous
    const int64_t C = t.size(1), N = t.size(0) / T, M = t.numel() / (t.size(0) * C);
    return t.contiguous().view({N, T, C, M}).permute({0, 3, 2, 1}).reshape({N * M, C, T});
}
Tensor tsl_frames(const Tensor &lines, at::IntArrayRef sizes, int64_t T) {   // ... and back
    const int64_t C = sizes[1], N = sizes[0] / T, M = lines.size(0) / N;
    return lines.view({N, M, C, T}).permute({0, 3, 2, 1}).reshape(sizes);
}
Tensor tsl_borders(int64_t T) {
    Tensor b = at::empty({6}, at::TensorOptions().dtype(at::kInt).device(at::kCPU));
    const int32_t v[6] = {0, static_cast<int32_t>(T), 0, 1, 0, 1};
    for (int i = 0; i < 6; ++i) b.data_ptr<int32_t>()[i] = v[i];
    return b;
}

Tensor tsl_forward_cpu(const Tensor &input, const Tensor &weights, int64_t n_segment, int64_t padding_mode, bool active_flag) {
    TORCH_CHECK(input.device().is_cpu() && weights.device().is_cpu(), "temporal_shift_learnable_cpu: expected CPU tensors");
    tsl_check(input, weights, n_segment, padding_mode);
    if (input.numel() == 0) return at::empty(input.sizes(), input.options(), at::MemoryFormat::Contiguous);
    const Tensor lines = tsl_lines(input, n_segment);
    const Tensor out = ShiftOps<1>::forward().call(lines, weights.reshape({input.size(1), 1}), tsl_borders(n_segment), lines.sizes(),
                                                   padding_mode, active_flag);
    return tsl_frames(out, input.sizes(), n_segment);
}

std::tuple<Tensor, Tensor> tsl_backward_cpu(const Tensor &grad, const Tensor &weights, const Tensor &input, int64_t n_segment,
                                            int64_t padding_mode, bool active_flag) {
    TORCH_CHECK(grad.device().is_cpu() && input.device().is_cpu() && weights.device().is_cpu(),
                "temporal_shift_learnable_cpu: expected CPU tensors");
    tsl_check(input, weights, n_segment, padding_mode);
    TORCH_CHECK(grad.sizes() == input.sizes(), "temporal_shift_learnable backward: grad does not match the input");
    if (input.numel() == 0)
        return std::make_tuple(at::empty(input.sizes(), input.options(), at::MemoryFormat::Contiguous), at::zeros_like(weights));
    auto result = ShiftOps<1>::backward().call(tsl_lines(grad, n_segment), weights.reshape({input.size(1), 1}), tsl_lines(input, n_segment),
                                               tsl_borders(n_segment), padding_mode, active_flag);
    return std::make_tuple(tsl_frames(std::get<0>(result), input.sizes(), n_segment), std::get<1>(result).reshape(weights.sizes()));
}

// The segment-major kernels count the tensor in 32-bit two-byte units (tshift_geometry_ok, csrc/shiftnd_tshift.hip: planes * units
// per plane + 16 < 2^31) and SHIFTND_SHIFT_DIM0 has no fallback: refuse a larger tensor here, before anything is allocated
void tsl_check_size(const Tensor &input, const char *who) {
    const int64_t units = input.numel() * static_cast<int64_t>(input.element_size()) / 2;
    TORCH_CHECK(units + 16 < (1LL << 31), who, ": a contiguous tensor of ", units, " two-byte units is beyond the segment-major kernels' ",
                "limit of 2^31 - 16 two-byte units (4 GiB); pass a channels-last tensor with memory_format=torch.preserve_format, ",
                "or split the batch");
}

// HIP tensors, the four learnable families (Ops: LearnableOps, LearnableClOps, PerClipLearnableOps, PerClipLearnableClOps): one
// flagged C-ABI call per pass.  The plain and the per-clip route make their tensors contiguous, refuse what the segment-major kernels
// cannot count, and answer an empty tensor themselves; the _cl routes (Ops::kAsItLies) hand every tensor that is not dense
// channels-last to their plain route (Ops::Plain) first and then take their tensors as they lie -- no contiguous(), no size check (the frame kernels have no such limit), no
// empty tensor (none is dense channels-last), results in the argument's strides (grad_x: the gradient's).
template <class Ops>
Tensor tsl_forward_hip(const Tensor &input_, const Tensor &weights, int64_t n_segment, int64_t padding_mode, bool active_flag) {
    if constexpr (Ops::kAsItLies)
        if (!is_channels_last_dense(input_)) return tsl_forward_hip<typename Ops::Plain>(input_, weights, n_segment, padding_mode, active_flag);
    TORCH_CHECK(input_.is_cuda(), Ops::name(), ": expected a CUDA tensor");
    Ops::check(input_, weights, n_segment, padding_mode);
    const int mixed = weights_flag(Ops::kCuda, input_, "input", weights);
    c10::DeviceGuard device_guard(input_.device());
    const int dtype = to_shiftnd_dtype(input_.scalar_type(), Ops::kCuda) | mixed;
    if (!Ops::kAsItLies) tsl_check_size(input_, "temporal_shift_learnable");
    const Tensor input = Ops::kAsItLies ? input_ : input_.contiguous();
    Tensor output = Ops::kAsItLies ? at::empty_strided(input.sizes(), input.strides(), input.options())
                                   : at::empty(input.sizes(), input.options(), at::MemoryFormat::Contiguous);
    if (input.numel() == 0) return output;
    const Tensor w = weights.contiguous();
    shiftnd_problem p;
    int64_t st[5];
    segment_problem(p, st, input, n_segment, padding_mode, active_flag, dtype | Ops::kFlags, Ops::kAsItLies, Ops::kProblemName);
    const int rc = shiftnd_forward(&p, input.data_ptr(), st, w.data_ptr(), output.data_ptr(), st, current_stream(input));
    TORCH_CHECK(rc == SHIFTND_OK, Ops::name(), " (HIP): ", shiftnd_status_string(rc));
    return output;
}

template <class Ops>
std::tuple<Tensor, Tensor> tsl_backward_hip(const Tensor &grad_, const Tensor &weights, const Tensor &input_, int64_t n_segment,
                                            int64_t padding_mode, bool active_flag) {
    if constexpr (Ops::kAsItLies)
        if (!is_channels_last_dense(input_) || !is_channels_last_dense(grad_) || grad_.sizes() != input_.sizes())
            return tsl_backward_hip<typename Ops::Plain>(grad_, weights, input_, n_segment, padding_mode, active_flag);   // (contiguous grad_x)
    TORCH_CHECK(grad_.is_cuda() && input_.is_cuda(), Ops::name(), ": expected CUDA tensors");
    Ops::check(input_, weights, n_segment, padding_mode);
    check_same(Ops::kBackwardCuda, grad_, "grad", input_, "input");
    const int mixed = weights_flag(Ops::kBackwardCuda, grad_, "grad", weights);
    TORCH_CHECK(grad_.sizes() == input_.sizes(), Ops::name(), " backward: grad does not match the input");
    c10::DeviceGuard device_guard(grad_.device());
    const int dtype = to_shiftnd_dtype(grad_.scalar_type(), Ops::kBackwardCuda) | mixed;
    if (!Ops::kAsItLies) tsl_check_size(input_, "temporal_shift_learnable backward");
    const Tensor input = Ops::kAsItLies ? input_ : input_.contiguous(), grad = Ops::kAsItLies ? grad_ : grad_.contiguous();
    const Tensor w = weights.contiguous();
    Tensor grad_input = Ops::kAsItLies ? at::empty_strided(grad.sizes(), grad.strides(), grad.options())
                                       : at::empty(input.sizes(), input.options(), at::MemoryFormat::Contiguous);
    Tensor grad_weights = at::empty_like(w, at::MemoryFormat::Contiguous);   // (the weights' dtype: fp32 for a mixed call)
    if (input.numel() == 0) return std::make_tuple(grad_input, grad_weights.zero_());   // (no kernel runs: the zero gradient is written here)
    shiftnd_problem p;
    int64_t st[5];
    segment_problem(p, st, input, n_segment, padding_mode, active_flag, dtype | Ops::kFlags, Ops::kAsItLies, Ops::kProblemName);
    const size_t ws_bytes = shiftnd_backward_workspace_bytes(&p);
    Tensor workspace = workspace_like(input, ws_bytes);
    const int rc = shiftnd_backward(&p, grad.data_ptr(), st, input.data_ptr(), st, w.data_ptr(), grad_input.data_ptr(), st,
                                    grad_weights.data_ptr(), workspace.data_ptr(), ws_bytes, current_stream(grad));
    TORCH_CHECK(rc == SHIFTND_OK, Ops::name(), " backward (HIP): ", shiftnd_status_string(rc));
    return std::make_tuple(grad_input, grad_weights);
}

// ---- channels-last learnable temporal shift: temporal_shift_learnable_cl / _temporal_shift_learnable_cl_forward / _backward ---------
// The values and gradients of temporal_shift_learnable with the layout of the argument kept (memory_format=torch.preserve_format in
// the Python wrappers).  On HIP tensors a dense channels-last input is ONE flagged C-ABI call per pass on the tensors as they lie
// (SHIFTND_SHIFT_DIM0 | SHIFTND_FRAMES on the strides {T*M*C, 1, M*C, C}: shiftnd_frames_learn.hip), no layout change in either
// direction; the backward takes that route when the saved input and the gradient are both dense channels-last and grad_x then has
// the gradient's strides.  Every other tensor goes the plain op's way.  The frame kernels stage nothing, and the sizes they take
// include every size the segment-major kernels take (those stop at 2^31 two-byte units a tensor), so the option never refuses a
// call that the plain op serves.  The entry, the node and the Autograd-key kernels are the plain family's under LearnableClOps.

// CPU tensors: the plain op's routine computes, the results are laid into the arguments' strides (grad_x: the gradient's)
Tensor tsl_cl_forward_cpu(const Tensor &input, const Tensor &weights, int64_t n_segment, int64_t padding_mode, bool active_flag) {
    return in_layout_of(tsl_forward_cpu(input, weights, n_segment, padding_mode, active_flag), input);
}
std::tuple<Tensor, Tensor> tsl_cl_backward_cpu(const Tensor &grad, const Tensor &weights, const Tensor &input, int64_t n_segment,
                                               int64_t padding_mode, bool active_flag) {
    auto result = tsl_backward_cpu(grad, weights, input, n_segment, padding_mode, active_flag);
    return std::make_tuple(in_layout_of(std::get<0>(result), grad), std::get<1>(result));
}

// ---- per-clip temporal shift: torchshifts_per_clip::temporal_shift_learnable_per_clip / temporal_shift_per_clip ---------------------
// The temporal shifts under a table of shape [N, C], N = input.size(0) / n_segment: clip n is shifted by row n (a shift that a small
// net predicts from the clip -- TIN's OffsetNet, arXiv 2001.06499 -- or per-clip temporal jitter).  By definition, for every clip n,
//     out[n*T:(n+1)*T] = temporal_shift_learnable(x[n*T:(n+1)*T], weights[n], T, padding_mode, active_flag)
// with that call's x.grad, and weights.grad[n] that call's weights.grad; the fixed op is the same loop over temporal_shift, without a
// table gradient.  The CPU key is literally that loop.  On HIP tensors every pass is ONE C-ABI call on the contiguous tensor under
// SHIFTND_SHIFT_DIM0 | SHIFTND_PER_CLIP (shiftnd_tshift.hip, the kernels of temporal_shift_learnable): the learnable op's backward
// is shiftnd_backward; the fixed op's forward is shiftnd_forward with active == 0, which copies bit patterns, and its backward the
// same call on the gradient under the negated table, so that no kernel reads the input or forms a weight gradient.  Its table is
// built like the channels-last routes': fp32 for 16-bit tensors (every shift exact), the tensor's dtype for fp32 / fp64.
// A namespace of its own for the reason torchshifts_inplace:: has one.
struct PerClipOps {   // (the learnable pair: PerClipLearnableOps, beside LearnableOps)
    static const char *name() { return "temporal_shift_per_clip"; }
    static auto &forward() { static auto op = typed_op<temporal_sig>("temporal_shift_per_clip", "torchshifts_per_clip"); return op; }
    static auto &backward() { static auto op = typed_op<temporal_sig>("_temporal_shift_per_clip_backward", "torchshifts_per_clip"); return op; }
};
struct PerClipClOps {   // (the learnable pair: PerClipLearnableClOps)
    static const char *name() { return "temporal_shift_per_clip_cl"; }
    static auto &forward() { static auto op = typed_op<temporal_sig>("temporal_shift_per_clip_cl", "torchshifts_per_clip_cl"); return op; }
    static auto &backward() { static auto op = typed_op<temporal_sig>("_temporal_shift_per_clip_cl_backward", "torchshifts_per_clip_cl"); return op; }
};

void tslpc_check(const Tensor &input, const Tensor &weights, int64_t n_segment, int64_t padding_mode) {
    TORCH_CHECK(!input.is_quantized(), "temporal_shift_learnable_per_clip: quantized inputs are not supported");
    segment_check("temporal_shift_learnable_per_clip", input, weights, n_segment, padding_mode, "weights",
                  at::isFloatingType(weights.scalar_type()), "floats", true);
}
void tpc_check(const Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    TORCH_CHECK(!input.is_quantized(), "temporal_shift_per_clip: quantized inputs are not supported");
    segment_check("temporal_shift_per_clip", input, shifts, n_segment, padding_mode, "shifts", is_integer_or_float(shifts),
                  "integers or floats", true);
}

// the public entry and the Autograd-key kernels: the nodes are temporal_shift_learnable's (input and weights kept) and
// temporal_shift's (the table alone kept).  Ops: PerClipLearnableOps / PerClipOps, and the _cl families' PerClipLearnableClOps /
// PerClipClOps
template <class Ops> Tensor tslpc_public(const Tensor &input, const Tensor &weights, int64_t n_segment, int64_t padding_mode, bool active_flag) {
    tslpc_check(input, weights, n_segment, padding_mode);
    return Ops::forward().call(input, weights, n_segment, padding_mode, active_flag);
}
template <class Ops> Tensor tslpc_autograd(const Tensor &input, const Tensor &weights, int64_t n_segment, int64_t padding_mode, bool active_flag) {
    tslpc_check(input, weights, n_segment, padding_mode);
    return LearnableTemporalShiftFunction<Ops>::apply(input, weights, n_segment, padding_mode, active_flag)[0];
}
template <class Ops>
std::tuple<Tensor, Tensor> tslpc_autograd_backward(const Tensor &grad, const Tensor &weights, const Tensor &input, int64_t n_segment,
                                                   int64_t padding_mode, bool active_flag) {
    tslpc_check(input, weights, n_segment, padding_mode);
    return GuardedBackward<Ops>::kernel(grad, weights, input, n_segment, padding_mode, active_flag);
}
template <class Ops> Tensor tpc_autograd(const Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    tpc_check(input, shifts, n_segment, padding_mode);
    return TemporalShiftFunction<Ops>::apply(input, shifts, n_segment, padding_mode)[0];
}
template <class Ops> Tensor tpc_autograd_backward(const Tensor &grad, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    tpc_check(grad, shifts, n_segment, padding_mode);
    return GuardedBackward<Ops>::kernel(grad, shifts, n_segment, padding_mode);
}

// CPU tensors: the loop of the definition over the per-channel CPU routines
Tensor tslpc_forward_cpu(const Tensor &input, const Tensor &weights, int64_t n_segment, int64_t padding_mode, bool active_flag) {
    TORCH_CHECK(input.device().is_cpu() && weights.device().is_cpu(), "temporal_shift_learnable_per_clip_cpu: expected CPU tensors");
    tslpc_check(input, weights, n_segment, padding_mode);
    if (input.numel() == 0) return at::empty(input.sizes(), input.options(), at::MemoryFormat::Contiguous);
    std::vector<Tensor> clips;
    for (int64_t n = 0; n < weights.size(0); ++n)
        clips.push_back(tsl_forward_cpu(input.narrow(0, n * n_segment, n_segment), weights.select(0, n), n_segment, padding_mode, active_flag));
    return at::cat(clips, 0);
}

std::tuple<Tensor, Tensor> tslpc_backward_cpu(const Tensor &grad, const Tensor &weights, const Tensor &input, int64_t n_segment,
                                              int64_t padding_mode, bool active_flag) {
    TORCH_CHECK(grad.device().is_cpu() && input.device().is_cpu() && weights.device().is_cpu(),
                "temporal_shift_learnable_per_clip_cpu: expected CPU tensors");
    tslpc_check(input, weights, n_segment, padding_mode);
    TORCH_CHECK(grad.sizes() == input.sizes(), "temporal_shift_learnable_per_clip backward: grad does not match the input");
    if (input.numel() == 0)
        return std::make_tuple(at::empty(input.sizes(), input.options(), at::MemoryFormat::Contiguous), at::zeros_like(weights));
    std::vector<Tensor> gx, gw;
    for (int64_t n = 0; n < weights.size(0); ++n) {
        auto clip = tsl_backward_cpu(grad.narrow(0, n * n_segment, n_segment), weights.select(0, n),
                                     input.narrow(0, n * n_segment, n_segment), n_segment, padding_mode, active_flag);
        gx.push_back(std::get<0>(clip));
        gw.push_back(std::get<1>(clip));
    }
    return std::make_tuple(at::cat(gx, 0), at::stack(gw, 0));
}

Tensor tpc_cpu(const Tensor &t, const Tensor &shifts, int64_t n_segment, int64_t padding_mode, bool backward) {
    TORCH_CHECK(t.device().is_cpu() && shifts.device().is_cpu(), "temporal_shift_per_clip_cpu: expected CPU tensors");
    tpc_check(t, shifts, n_segment, padding_mode);
    if (t.numel() == 0) return at::empty(t.sizes(), t.options(), at::MemoryFormat::Contiguous);
    auto &op = backward ? TemporalOps::backward() : TemporalOps::forward();
    std::vector<Tensor> clips;
    for (int64_t n = 0; n < shifts.size(0); ++n)
        clips.push_back(op.call(t.narrow(0, n * n_segment, n_segment), shifts.select(0, n), n_segment, padding_mode));
    return at::cat(clips, 0);
}
Tensor tpc_forward_cpu(const Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    return tpc_cpu(input, shifts.detach(), n_segment, padding_mode, false);
}
Tensor tpc_backward_cpu(const Tensor &grad, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    return tpc_cpu(grad, shifts.detach(), n_segment, padding_mode, true);
}

// HIP tensors: one call under SHIFTND_SHIFT_DIM0 | SHIFTND_PER_CLIP on the segment-major strides (the learnable pair: tsl_forward_hip /
// tsl_backward_hip under PerClipLearnableOps)
// `as_it_lies` (the _cl op): a dense channels-last tensor is the call under SHIFTND_SHIFT_DIM0 | SHIFTND_CLIP_FRAMES on the tensor as it
// lies (shiftnd_frames.hip) -- no contiguous(), no size check (the frame kernels have no such limit), the result in the argument's
// strides; every other tensor goes the plain way
Tensor tpc_hip(const Tensor &t_, const Tensor &shifts, int64_t n_segment, int64_t padding_mode, bool backward, bool as_it_lies = false) {
    TORCH_CHECK(t_.is_cuda(), "temporal_shift_per_clip: expected a CUDA tensor");
    tpc_check(t_, shifts, n_segment, padding_mode);
    c10::DeviceGuard device_guard(t_.device());
    const bool half = t_.scalar_type() == at::kHalf || t_.scalar_type() == at::kBFloat16;
    const int dtype = to_shiftnd_dtype(t_.scalar_type(), "temporal_shift_per_clip_cuda") | (half ? SHIFTND_WEIGHTS_F32 : 0);
    const bool lies = as_it_lies && is_channels_last_dense(t_);
    if (!lies) tsl_check_size(t_, "temporal_shift_per_clip");
    const Tensor t = lies ? t_ : t_.contiguous();
    Tensor out = lies ? at::empty_strided(t.sizes(), t.strides(), t.options()) : at::empty(t.sizes(), t.options(), at::MemoryFormat::Contiguous);
    if (t.numel() == 0) return out;
    Tensor w = shifts.detach();
    if (at::isFloatingType(w.scalar_type())) w = w.round();   // (half to even, before the table's type can move an entry onto a half)
    w = w.to(half ? at::kFloat : t.scalar_type());
    // (grad_x[t] = grad_out[pad(t + s)]: the forward under -s.)  The library reads a dense [N, C] array, and round / to / neg keep the
    // strides of a transposed table: contiguous after them, in both directions
    w = (backward ? w.neg() : w).contiguous();
    shiftnd_problem p;
    int64_t st[5];
    segment_problem(p, st, t, n_segment, padding_mode, false, dtype | SHIFTND_SHIFT_DIM0 | (lies ? SHIFTND_CLIP_FRAMES : SHIFTND_PER_CLIP), lies,
                    lies ? "temporal_shift_per_clip_cl" : "temporal_shift_per_clip");
    check_status(shiftnd_forward(&p, t.data_ptr(), st, w.data_ptr(), out.data_ptr(), st, current_stream(t)),
                 lies ? "temporal_shift_per_clip_cl (HIP)" : "temporal_shift_per_clip (HIP)");
    return out;
}
Tensor tpc_forward_hip(const Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    return tpc_hip(input, shifts, n_segment, padding_mode, false);
}
Tensor tpc_backward_hip(const Tensor &grad, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    return tpc_hip(grad, shifts, n_segment, padding_mode, true);
}

// ---- temporal interlacing: torchshifts_interlace::temporal_interlace / _temporal_interlace_forward / _backward ----------------------
// The TIN layer's core (arXiv 2001.06499): the per-clip interpolating shift followed by a per-clip, per-frame, per-channel weight.
// By definition, with offsets [N, C] and scales [N, T, C]:
//     y   = temporal_shift_learnable_per_clip(input, offsets, n_segment, padding_mode, active_flag)
//     out = y * scales.reshape(N*T, C, 1, ...)
// and the gradients are that composition's.  The CPU key is literally that, on the per-clip ops.  On HIP tensors every pass is ONE
// C-ABI call on the contiguous tensor under SHIFTND_SHIFT_DIM0 | SHIFTND_INTERLACE (shiftnd_interlace.hip): the two small tables
// travel as one packed array (one cat), the packed gradient is split back into views.  The autograd node keeps the input and the two
// tables, nothing of the output's size.  A namespace of its own for the reason torchshifts_inplace:: has one.
void tin_check(const Tensor &input, const Tensor &offsets, const Tensor &scales, int64_t n_segment, int64_t padding_mode) {
    TORCH_CHECK(!input.is_quantized(), "temporal_interlace: quantized inputs are not supported");
    segment_check("temporal_interlace", input, offsets, n_segment, padding_mode, "offsets", at::isFloatingType(offsets.scalar_type()),
                  "floats", true);
    TORCH_CHECK(scales.dim() == 3 && scales.size(0) == offsets.size(0) && scales.size(1) == n_segment && scales.size(2) == input.size(1),
                "temporal_interlace: scales must have shape [N, T, C] = [", offsets.size(0), ", ", n_segment, ", ", input.size(1), "]");
    TORCH_CHECK(scales.device() == input.device(), "temporal_interlace: scales must be on the input's device");
    TORCH_CHECK(scales.scalar_type() == offsets.scalar_type(), "temporal_interlace: scales must have the offsets' type (",
                c10::toString(offsets.scalar_type()), "), not ", c10::toString(scales.scalar_type()));
}

// the public entry, the node and the Autograd-key kernels.  Ops: InterlaceOps, and the _cl family's InterlaceClOps
template <class Ops>
Tensor tin_public(const Tensor &input, const Tensor &offsets, const Tensor &scales, int64_t n_segment, int64_t padding_mode,
                  bool active_flag) {
    tin_check(input, offsets, scales, n_segment, padding_mode);
    return Ops::forward().call(input, offsets, scales, n_segment, padding_mode, active_flag);
}

template <class Ops> struct InterlaceFunction : public torch::autograd::Function<InterlaceFunction<Ops>> {
    static variable_list forward(AutogradContext *ctx, const Tensor &input, const Tensor &offsets, const Tensor &scales,
                                 int64_t n_segment, int64_t padding_mode, bool active_flag) {
        at::AutoDispatchBelowADInplaceOrView guard;
        auto output = Ops::forward().call(input, offsets, scales, n_segment, padding_mode, active_flag);
        ctx->saved_data["n_segment"] = n_segment;
        ctx->saved_data["padding_mode"] = padding_mode;
        ctx->saved_data["active_flag"] = active_flag;
        ctx->save_for_backward({input, offsets, scales});
        return {output};
    }
    static variable_list backward(AutogradContext *ctx, const variable_list &grad_output) {
        auto saved = ctx->get_saved_variables();
        auto result = Ops::backward().call(grad_output[0], saved[1], saved[2], saved[0], ctx->saved_data["n_segment"].toInt(),
                                           ctx->saved_data["padding_mode"].toInt(), ctx->saved_data["active_flag"].toBool());
        return {std::get<0>(result), std::get<1>(result), std::get<2>(result), Tensor(), Tensor(), Tensor()};
    }
};

template <class Ops>
Tensor tin_autograd(const Tensor &input, const Tensor &offsets, const Tensor &scales, int64_t n_segment, int64_t padding_mode,
                    bool active_flag) {
    tin_check(input, offsets, scales, n_segment, padding_mode);
    return InterlaceFunction<Ops>::apply(input, offsets, scales, n_segment, padding_mode, active_flag)[0];
}
template <class Ops>
std::tuple<Tensor, Tensor, Tensor> tin_autograd_backward(const Tensor &grad, const Tensor &offsets, const Tensor &scales,
                                                         const Tensor &input, int64_t n_segment, int64_t padding_mode, bool active_flag) {
    tin_check(input, offsets, scales, n_segment, padding_mode);
    return GuardedBackward<Ops>::kernel(grad, offsets, scales, input, n_segment, padding_mode, active_flag);
}

// scales [N, T, C] as a factor of the [N*T, C, ...] tensor `like`: [N*T, C, 1, ...]
Tensor tin_plane_scales(const Tensor &scales, const Tensor &like) {
    std::vector<int64_t> shape(like.dim(), 1);
    shape[0] = like.size(0);
    shape[1] = like.size(1);
    return scales.reshape(shape);
}

// CPU tensors: the definition, on the per-clip ops
Tensor tin_forward_cpu(const Tensor &input, const Tensor &offsets, const Tensor &scales, int64_t n_segment, int64_t padding_mode,
                       bool active_flag) {
    TORCH_CHECK(input.device().is_cpu() && offsets.device().is_cpu() && scales.device().is_cpu(), "temporal_interlace_cpu: expected CPU tensors");
    tin_check(input, offsets, scales, n_segment, padding_mode);
    const Tensor y = PerClipLearnableOps::forward().call(input, offsets, n_segment, padding_mode, active_flag);
    return y * tin_plane_scales(scales, input);
}

std::tuple<Tensor, Tensor, Tensor> tin_backward_cpu(const Tensor &grad, const Tensor &offsets, const Tensor &scales, const Tensor &input,
                                                    int64_t n_segment, int64_t padding_mode, bool active_flag) {
    TORCH_CHECK(grad.device().is_cpu() && input.device().is_cpu() && offsets.device().is_cpu() && scales.device().is_cpu(),
                "temporal_interlace_cpu: expected CPU tensors");
    tin_check(input, offsets, scales, n_segment, padding_mode);
    TORCH_CHECK(grad.sizes() == input.sizes(), "temporal_interlace backward: grad does not match the input");
    const Tensor y = PerClipLearnableOps::forward().call(input, offsets, n_segment, padding_mode, active_flag);
    auto shifted = PerClipLearnableOps::backward().call(grad * tin_plane_scales(scales, input), offsets, input, n_segment, padding_mode,
                                                        active_flag);
    if (input.numel() == 0) return std::make_tuple(std::get<0>(shifted), std::get<1>(shifted), at::zeros_like(scales));
    const Tensor grad_scales = (grad * y).reshape({scales.size(0), scales.size(1), scales.size(2), -1}).sum(3).to(scales.scalar_type());
    return std::make_tuple(std::get<0>(shifted), std::get<1>(shifted), grad_scales);
}

// HIP tensors: one flagged C-ABI call per pass under the packed table.  Ops: InterlaceOps -- the tensors made contiguous, what the
// segment-major kernels cannot count refused -- and InterlaceClOps (Ops::kAsItLies), which hands every tensor that is not dense
// channels-last to InterlaceOps first and then takes its tensors as they lie under SHIFTND_INTERLACE_FRAMES: no contiguous(), results
// in the argument's strides (grad_x: the gradient's).  The segment-major size check (2^31 two-byte units) does not apply; the frame
// kernels' own bounds do -- N * T * C < 2^31 for the packed table, which the plain route needs as well, and the backward's groups and
// records (include/shiftnd_hip.h) -- and a tensor beyond them raises "invalid argument" here: there is no route to fall back to that
// takes what these refuse
template <class Ops>
Tensor tin_forward_hip(const Tensor &input_, const Tensor &offsets, const Tensor &scales, int64_t n_segment, int64_t padding_mode,
                       bool active_flag) {
    if constexpr (Ops::kAsItLies)
        if (!is_channels_last_dense(input_)) return tin_forward_hip<typename Ops::Plain>(input_, offsets, scales, n_segment, padding_mode, active_flag);
    TORCH_CHECK(input_.is_cuda(), Ops::name(), ": expected a CUDA tensor");
    tin_check(input_, offsets, scales, n_segment, padding_mode);
    const int mixed = weights_flag(Ops::kCuda, input_, "input", offsets);
    c10::DeviceGuard device_guard(input_.device());
    const int dtype = to_shiftnd_dtype(input_.scalar_type(), Ops::kCuda) | mixed;
    if (!Ops::kAsItLies) tsl_check_size(input_, "temporal_interlace");
    const Tensor input = Ops::kAsItLies ? input_ : input_.contiguous();   // (the default op makes a channels-last input contiguous first)
    Tensor output = Ops::kAsItLies ? at::empty_strided(input.sizes(), input.strides(), input.options())
                                   : at::empty(input.sizes(), input.options(), at::MemoryFormat::Contiguous);
    if (input.numel() == 0) return output;
    const Tensor table = at::cat({offsets.reshape({-1}), scales.reshape({-1})});
    shiftnd_problem p;
    int64_t st[5];
    segment_problem(p, st, input, n_segment, padding_mode, active_flag, dtype | Ops::kFlags, Ops::kAsItLies, Ops::name());
    const int rc = shiftnd_forward(&p, input.data_ptr(), st, table.data_ptr(), output.data_ptr(), st, current_stream(input));
    TORCH_CHECK(rc == SHIFTND_OK, Ops::name(), " (HIP): ", shiftnd_status_string(rc));
    return output;
}

template <class Ops>
std::tuple<Tensor, Tensor, Tensor> tin_backward_hip(const Tensor &grad_, const Tensor &offsets, const Tensor &scales, const Tensor &input_,
                                                    int64_t n_segment, int64_t padding_mode, bool active_flag) {
    if constexpr (Ops::kAsItLies)
        if (!is_channels_last_dense(input_) || !is_channels_last_dense(grad_) || grad_.sizes() != input_.sizes())
            return tin_backward_hip<typename Ops::Plain>(grad_, offsets, scales, input_, n_segment, padding_mode, active_flag);   // (contiguous grad_x)
    TORCH_CHECK(grad_.is_cuda() && input_.is_cuda(), Ops::name(), ": expected CUDA tensors");
    tin_check(input_, offsets, scales, n_segment, padding_mode);
    check_same(Ops::kBackwardCuda, grad_, "grad", input_, "input");
    const int mixed = weights_flag(Ops::kBackwardCuda, grad_, "grad", offsets);
    TORCH_CHECK(grad_.sizes() == input_.sizes(), Ops::name(), " backward: grad does not match the input");
    c10::DeviceGuard device_guard(grad_.device());
    const int dtype = to_shiftnd_dtype(grad_.scalar_type(), Ops::kBackwardCuda) | mixed;
    if (!Ops::kAsItLies) tsl_check_size(input_, "temporal_interlace backward");
    const Tensor input = Ops::kAsItLies ? input_ : input_.contiguous(), grad = Ops::kAsItLies ? grad_ : grad_.contiguous();
    Tensor grad_input = Ops::kAsItLies ? at::empty_strided(grad.sizes(), grad.strides(), grad.options())
                                       : at::empty(input.sizes(), input.options(), at::MemoryFormat::Contiguous);
    const Tensor table = at::cat({offsets.reshape({-1}), scales.reshape({-1})});
    Tensor grad_table = at::empty_like(table);   // (the tables' dtype: fp32 for a mixed call)
    if (input.numel() == 0) grad_table.zero_();   // (no kernel runs: the zero gradient is written here)
    else {
        shiftnd_problem p;
        int64_t st[5];
        segment_problem(p, st, input, n_segment, padding_mode, active_flag, dtype | Ops::kFlags, Ops::kAsItLies, Ops::name());
        const size_t ws_bytes = shiftnd_backward_workspace_bytes(&p);
        Tensor workspace = workspace_like(input, ws_bytes);
        const int rc = shiftnd_backward(&p, grad.data_ptr(), st, input.data_ptr(), st, table.data_ptr(), grad_input.data_ptr(), st,
                                        grad_table.data_ptr(), workspace.data_ptr(), ws_bytes, current_stream(grad));
        TORCH_CHECK(rc == SHIFTND_OK, Ops::name(), " backward (HIP): ", shiftnd_status_string(rc));
    }
    return std::make_tuple(grad_input, grad_table.narrow(0, 0, offsets.numel()).view(offsets.sizes()),
                           grad_table.narrow(0, offsets.numel(), scales.numel()).view(scales.sizes()));
}

// ---- channels-last temporal interlacing: torchshifts_interlace_cl::temporal_interlace_cl / _temporal_interlace_cl_forward / _backward --
// The values and gradients of temporal_interlace with the layout of the argument kept (memory_format=torch.preserve_format in the
// Python wrappers).  On HIP tensors a dense channels-last input is ONE C-ABI call per pass on the tensors as they lie, under
// SHIFTND_SHIFT_DIM0 | SHIFTND_INTERLACE_FRAMES (shiftnd_interlace_frames.hip), through tin_forward_hip / tin_backward_hip under
// InterlaceClOps -- the backward takes the route when the saved input and the gradient are both dense channels-last, grad_x then
// has the gradient's strides; every other HIP tensor goes the plain op's way.  CPU tensors: the definition on the channels-last
// per-clip ops, laid out in the argument's strides; a tensor that is not dense channels-last runs the plain op's routine, so its
// results are the default's bit for bit.  The node keeps input, offsets and scales (InterlaceFunction<InterlaceClOps>).  A
// namespace of its own, so that the op set of torchshifts_interlace:: stays.
Tensor tin_cl_forward_cpu(const Tensor &input, const Tensor &offsets, const Tensor &scales, int64_t n_segment, int64_t padding_mode,
                          bool active_flag) {
    if (!is_channels_last_dense(input)) return tin_forward_cpu(input, offsets, scales, n_segment, padding_mode, active_flag);
    TORCH_CHECK(input.device().is_cpu() && offsets.device().is_cpu() && scales.device().is_cpu(), "temporal_interlace_cl_cpu: expected CPU tensors");
    tin_check(input, offsets, scales, n_segment, padding_mode);
    const Tensor y = PerClipLearnableClOps::forward().call(input, offsets, n_segment, padding_mode, active_flag);
    return in_layout_of(y * tin_plane_scales(scales, input), input);
}

std::tuple<Tensor, Tensor, Tensor> tin_cl_backward_cpu(const Tensor &grad, const Tensor &offsets, const Tensor &scales, const Tensor &input,
                                                       int64_t n_segment, int64_t padding_mode, bool active_flag) {
    if (!is_channels_last_dense(input) || !is_channels_last_dense(grad) || grad.sizes() != input.sizes())
        return tin_backward_cpu(grad, offsets, scales, input, n_segment, padding_mode, active_flag);
    TORCH_CHECK(grad.device().is_cpu() && input.device().is_cpu() && offsets.device().is_cpu() && scales.device().is_cpu(),
                "temporal_interlace_cl_cpu: expected CPU tensors");
    tin_check(input, offsets, scales, n_segment, padding_mode);
    const Tensor plane = tin_plane_scales(scales, input);
    const Tensor y = PerClipLearnableClOps::forward().call(input, offsets, n_segment, padding_mode, active_flag);
    auto shifted = PerClipLearnableClOps::backward().call(grad * plane, offsets, input, n_segment, padding_mode, active_flag);
    // (the sum autograd forms for the factor of y * plane)
    const Tensor grad_scales = (grad * y).sum_to_size(plane.sizes()).reshape(scales.sizes()).to(scales.scalar_type());
    return std::make_tuple(in_layout_of(std::get<0>(shifted), grad), std::get<1>(shifted), grad_scales);
}

// ---- channels-last per-clip temporal shift: torchshifts_per_clip_cl::temporal_shift_learnable_per_clip_cl / temporal_shift_per_clip_cl --
// The values and gradients of the per-clip ops with the layout of the argument kept (memory_format=torch.preserve_format in the
// Python wrappers).  On HIP tensors a dense channels-last input is ONE C-ABI call per pass on the tensors as they lie, under
// SHIFTND_SHIFT_DIM0 | SHIFTND_CLIP_FRAMES (the frame kernels under a row stride): the learnable pair through tsl_forward_hip /
// tsl_backward_hip under PerClipLearnableClOps -- the backward takes the route when the saved input and the gradient are both dense
// channels-last, grad_x then has the gradient's strides -- the fixed op through tpc_hip, whose backward is the forward call on the
// gradient under the negated table.  Every other HIP tensor goes the plain per-clip op's way.  CPU tensors: the per-clip CPU routines
// compute and the results are laid into the arguments' strides.  The entry, the nodes and the Autograd-key kernels are the per-clip
// family's under PerClipLearnableClOps / PerClipClOps; a namespace of its own, so that the op set of torchshifts_per_clip:: stays.
Tensor tslpc_cl_forward_cpu(const Tensor &input, const Tensor &weights, int64_t n_segment, int64_t padding_mode, bool active_flag) {
    return in_layout_of(tslpc_forward_cpu(input, weights, n_segment, padding_mode, active_flag), input);
}
std::tuple<Tensor, Tensor> tslpc_cl_backward_cpu(const Tensor &grad, const Tensor &weights, const Tensor &input, int64_t n_segment,
                                                 int64_t padding_mode, bool active_flag) {
    auto result = tslpc_backward_cpu(grad, weights, input, n_segment, padding_mode, active_flag);
    return std::make_tuple(in_layout_of(std::get<0>(result), grad), std::get<1>(result));
}
Tensor tpc_cl_forward_cpu(const Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    return in_layout_of(tpc_forward_cpu(input, shifts, n_segment, padding_mode), input);
}
Tensor tpc_cl_backward_cpu(const Tensor &grad, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    return in_layout_of(tpc_backward_cpu(grad, shifts, n_segment, padding_mode), grad);
}
Tensor tpc_cl_forward_hip(const Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    return tpc_hip(input, shifts, n_segment, padding_mode, false, true);
}
Tensor tpc_cl_backward_hip(const Tensor &grad, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    return tpc_hip(grad, shifts, n_segment, padding_mode, true, true);
}

// ---- in-place temporal shift: torchshifts_inplace::temporal_shift_ / temporal_shift_quantized_ -------------------------------------
// The values of temporal_shift / temporal_shift_quantized written into the argument, which is returned.  A second library namespace,
// because the op set of torchshifts:: is the reference's surface plus the families above and stays as it is.  On HIP tensors a dense
// input (contiguous or channels-last, is_channels_last_dense) of at most kInplaceFrames frames per clip is ONE flagged C-ABI call
// with out == x on the tensor as it lies (shiftnd_inplace.hip): only the shifted channels' bytes are read or written, nothing of the
// input's size is allocated.  The [C] table is built like the channels-last routes': fp32 for 16-bit tensors (every shift exact),
// the tensor's dtype for fp32 / fp64, int32 for quantized tensors.  Every other input -- not dense, a slice, more frames -- and every
// CPU tensor is input.copy_(<the out-of-place op>(input)): the same values.  The autograd node marks the input dirty and keeps the
// table, n_segment, the padding and whether the input was dense channels-last; its backward is OUT of place (a gradient buffer may
// be shared with other consumers): _temporal_shift_cl_backward for a dense channels-last input, _temporal_shift_backward otherwise.
constexpr int64_t kInplaceFrames = 16;   // (the frame slots of frames_inplace: include/shiftnd_hip.h)

using temporal_inplace_sig = Tensor &(Tensor &, const Tensor &, int64_t, int64_t);

struct InplaceOps {
    static const char *name() { return "temporal_shift_"; }
    static auto &forward() { static auto op = typed_op<temporal_inplace_sig>("temporal_shift_", "torchshifts_inplace"); return op; }
    static auto &backward() { return TemporalOps::backward(); }
};
struct InplaceClOps : InplaceOps {
    static auto &backward() { return TemporalClOps::backward(); }
};

void temporal_inplace_check(const Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    TORCH_CHECK(!input.is_quantized(), "temporal_shift_: quantized inputs are not supported");
    segment_check("temporal_shift_", input, shifts, n_segment, padding_mode, "shifts", is_integer_or_float(shifts), "integers or floats");
}

void temporal_quantized_inplace_check(const Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    TORCH_CHECK(input.is_quantized(), "temporal_shift_quantized_: expected a quantized input");
    TORCH_CHECK(input.qscheme() == at::kPerTensorAffine, "temporal_shift_quantized_: expected a per-tensor quantized input");
    segment_check("temporal_shift_quantized_", input, shifts, n_segment, padding_mode, "shifts",
                  !shifts.is_quantized() && is_integer_or_float(shifts), "integers or floats");
}

struct TemporalShiftInplaceFunction : public torch::autograd::Function<TemporalShiftInplaceFunction> {
    static variable_list forward(AutogradContext *ctx, const Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
        ctx->mark_dirty({input});
        ctx->saved_data["n_segment"] = n_segment;
        ctx->saved_data["padding_mode"] = padding_mode;
        ctx->saved_data["channels_last"] = is_channels_last_dense(input);
        ctx->save_for_backward({shifts.detach()});
        at::AutoDispatchBelowADInplaceOrView guard;
        InplaceOps::forward().call(const_cast<Tensor &>(input), shifts, n_segment, padding_mode);
        return {input};
    }
    static variable_list backward(AutogradContext *ctx, const variable_list &grad_output) {
        auto saved = ctx->get_saved_variables();
        const int64_t n_segment = ctx->saved_data["n_segment"].toInt(), padding_mode = ctx->saved_data["padding_mode"].toInt();
        Tensor grad = ctx->saved_data["channels_last"].toBool()
                          ? GuardedBackward<InplaceClOps>::kernel(grad_output[0], saved[0], n_segment, padding_mode)
                          : GuardedBackward<InplaceOps>::kernel(grad_output[0], saved[0], n_segment, padding_mode);
        return {grad, Tensor(), Tensor(), Tensor()};
    }
};

Tensor &temporal_inplace_autograd(Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    temporal_inplace_check(input, shifts, n_segment, padding_mode);
    TemporalShiftInplaceFunction::apply(input, shifts, n_segment, padding_mode);
    return input;
}

// the fallback of every backend: the out-of-place op of the input's layout, copied into the input
Tensor &temporal_inplace_by_copy(Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    auto &op = is_channels_last_dense(input) ? TemporalClOps::forward() : TemporalOps::forward();
    input.copy_(op.call(input, shifts, n_segment, padding_mode));
    return input;
}

// a quantized tensor's storage as plain integers, the same sizes and strides (copy_ between them moves the int_repr and nothing else)
Tensor int_repr_alias(const Tensor &t) {
    const auto type = t.scalar_type() == at::kQUInt8 ? at::kByte : (t.scalar_type() == at::kQInt8 ? at::kChar : at::kInt);
    return at::empty({0}, t.options().dtype(type)).set_(t.storage(), t.storage_offset(), t.sizes(), t.strides());
}

Tensor &temporal_quantized_inplace_by_copy(Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    static auto plain = typed_op<temporal_sig>("temporal_shift_quantized"), cl = typed_op<temporal_sig>("temporal_shift_quantized_cl");
    const Tensor result = (is_channels_last_dense(input) ? cl : plain).call(input, shifts, n_segment, padding_mode);
    int_repr_alias(input).copy_(int_repr_alias(result));   // (scale and zero point are the input's own: untouched)
    return input;
}

Tensor &temporal_inplace_cpu(Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    temporal_inplace_check(input, shifts, n_segment, padding_mode);
    return temporal_inplace_by_copy(input, shifts, n_segment, padding_mode);
}

// (no autograd node above the quantized op: the version counter is bumped here)
Tensor &temporal_quantized_inplace_cpu(Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    temporal_quantized_inplace_check(input, shifts, n_segment, padding_mode);
    at::AutoDispatchBelowADInplaceOrView guard;
    input.unsafeGetTensorImpl()->bump_version();
    return temporal_quantized_inplace_by_copy(input, shifts, n_segment, padding_mode);
}

// served as it lies: dense in one of the two layouts, few enough frames
bool inplace_served(const Tensor &t, int64_t n_segment) {
    return n_segment <= kInplaceFrames && t.numel() > 0 && (t.is_contiguous() || is_channels_last_dense(t));
}

Tensor &temporal_inplace_hip(Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    TORCH_CHECK(input.is_cuda(), "temporal_shift_: expected a CUDA tensor");
    temporal_inplace_check(input, shifts, n_segment, padding_mode);
    if (input.numel() == 0) return input;
    if (!inplace_served(input, n_segment)) return temporal_inplace_by_copy(input, shifts, n_segment, padding_mode);
    c10::DeviceGuard device_guard(input.device());
    const bool half = input.scalar_type() == at::kHalf || input.scalar_type() == at::kBFloat16;
    const int dtype = to_shiftnd_dtype(input.scalar_type(), "temporal_shift__cuda") | (half ? SHIFTND_WEIGHTS_F32 : 0);
    const Tensor w = shifts.detach().reshape({input.size(1)}).to(half ? at::kFloat : input.scalar_type()).contiguous();
    shiftnd_problem p;
    int64_t st[5];
    segment_problem(p, st, input, n_segment, padding_mode, false, dtype | SHIFTND_SHIFT_DIM0, !input.is_contiguous(), "temporal_shift_");
    check_status(shiftnd_forward(&p, input.data_ptr(), st, w.data_ptr(), input.data_ptr(), st, current_stream(input)), "temporal_shift_ (HIP)");
    return input;
}

Tensor &temporal_quantized_inplace_hip(Tensor &input, const Tensor &shifts, int64_t n_segment, int64_t padding_mode) {
    TORCH_CHECK(input.is_cuda(), "temporal_shift_quantized_: expected a CUDA tensor");
    temporal_quantized_inplace_check(input, shifts, n_segment, padding_mode);
    if (input.numel() == 0) return input;
    at::AutoDispatchBelowADInplaceOrView guard;
    input.unsafeGetTensorImpl()->bump_version();
    if (!inplace_served(input, n_segment)) return temporal_quantized_inplace_by_copy(input, shifts, n_segment, padding_mode);
    c10::DeviceGuard device_guard(input.device());
    const int dtype = quant_dtype(input.scalar_type(), "temporal_shift_quantized__cuda");
    const Tensor w = quantized_shift_table(shifts, input.size(1)).to(at::kInt).contiguous();
    shiftnd_problem p;
    int64_t st[5];
    segment_problem(p, st, input, n_segment, padding_mode, false, dtype | SHIFTND_SHIFT_DIM0, !input.is_contiguous(), "temporal_shift_quantized_");
    check_status(shiftnd_forward_quantized(&p, input.data_ptr(), st, w.data_ptr(), SHIFTND_I32, 0, input.q_zero_point(), input.data_ptr(), st,
                                           current_stream(input)),
                 "temporal_shift_quantized_ (HIP)");
    return input;
}

// ---- online temporal shift: torchshifts_online::temporal_shift_online_ / temporal_shift_online_quantized_ --------------------------
// One step of the uni-directional TSM on a frame batch [B, C, ...] against a state [D, B, C, ...] whose slot k holds frame t-1-k
// (include/shiftnd_hip.h, SHIFTND_STREAM): for a channel with shift s in 1..D the frame shows slot s-1, the slots move one place on
// and slot 0 takes the incoming frame.  Both tensors are written; the frame is returned.  An inference op: there is no autograd
// formula and a tensor that requires grad raises.  On HIP tensors a dense frame (contiguous or channels-last,
// is_channels_last_dense) with a state of 1..kOnlineSlots slots in the same layout is ONE flagged C-ABI call (shiftnd_stream.hip),
// with no host synchronisation, so a step can be captured in a graph; a table that already has the kernel's kind -- fp32 for 16-bit
// tensors, the tensor's dtype for fp32 / fp64, int32 for quantized tensors -- is passed as it is, with no allocation (the modules
// keep such a table), any other table is converted first.  Every other input -- CPU tensors, more slots, views that are not dense --
// runs the composite below on index_select / index_copy_: the same values.  The composite reads the table on the host, and it alone
// can refuse a negative entry; the kernel clamps (torchshifts.functional.temporal_shift_online_state validates a table once).
constexpr int64_t kOnlineSlots = 15;   // (the slots beside the frame in frames_stream's 16 registers: include/shiftnd_hip.h)

// bytes [first, last) a strided tensor can touch, relative to its storage
std::pair<int64_t, int64_t> byte_extent(const Tensor &t) {
    int64_t last = t.storage_offset();
    for (int64_t d = 0; d < t.dim(); ++d) last += (t.size(d) - 1) * t.stride(d);
    return {t.storage_offset() * static_cast<int64_t>(t.element_size()), (last + 1) * static_cast<int64_t>(t.element_size())};
}

void online_check(const char *op_name, const Tensor &input, const Tensor &state, const Tensor &shifts) {
    TORCH_CHECK(input.dim() >= 2 && input.dim() <= 5, op_name, ": expected a [B, C, ...] frame of 2 to 5 dims");
    TORCH_CHECK(state.dim() == input.dim() + 1 && state.sizes().slice(1) == input.sizes(), op_name, ": state must have shape [D, ",
                input.sizes(), "], one slot per cached frame, but its shape is ", state.sizes());
    TORCH_CHECK(state.scalar_type() == input.scalar_type(), op_name, ": state must have the input's dtype (", c10::toString(input.scalar_type()),
                "), but it is ", c10::toString(state.scalar_type()));
    TORCH_CHECK(state.device() == input.device(), op_name, ": state must be on the input's device");
    TORCH_CHECK(shifts.dim() == 1 && shifts.size(0) == input.size(1), op_name, ": shifts must have shape [C]");
    TORCH_CHECK(shifts.device() == input.device(), op_name, ": shifts must be on the input's device");
    TORCH_CHECK(!shifts.is_quantized() && is_integer_or_float(shifts), op_name, ": shifts must be integers or floats");
    TORCH_CHECK(!input.requires_grad() && !state.requires_grad() && !shifts.requires_grad(), op_name,
                ": an inference op without an autograd formula, but an argument requires grad");
    if (input.numel() > 0 && state.numel() > 0 && input.storage().is_alias_of(state.storage())) {
        const auto a = byte_extent(input), b = byte_extent(state);
        TORCH_CHECK(a.second <= b.first || b.second <= a.first, op_name, ": input and state overlap in memory");
    }
}

void online_float_check(const Tensor &input, const Tensor &state, const Tensor &shifts) {
    TORCH_CHECK(!input.is_quantized() && !state.is_quantized(), "temporal_shift_online_: quantized tensors are not supported");
    online_check("temporal_shift_online_", input, state, shifts);
}

void online_quantized_check(const Tensor &input, const Tensor &state, const Tensor &shifts) {
    const char *op_name = "temporal_shift_online_quantized_";
    TORCH_CHECK(input.is_quantized(), op_name, ": expected a quantized input");
    TORCH_CHECK(input.qscheme() == at::kPerTensorAffine, op_name, ": expected a per-tensor quantized input");
    TORCH_CHECK(state.is_quantized() && state.qscheme() == at::kPerTensorAffine, op_name, ": expected a per-tensor quantized state");
    online_check(op_name, input, state, shifts);
    TORCH_CHECK(state.q_scale() == input.q_scale() && state.q_zero_point() == input.q_zero_point(), op_name,
                ": state must have the input's scale and zero point (", input.q_scale(), ", ", input.q_zero_point(), "), but it has (",
                state.q_scale(), ", ", state.q_zero_point(), ")");
}

// both tensors are written below every autograd key: the version counters are bumped here
void online_bump(Tensor &input, Tensor &state) {
    input.unsafeGetTensorImpl()->bump_version();
    state.unsafeGetTensorImpl()->bump_version();
}

// the step on plain tensors of any strides, one group of channels per shift value.  Reads the table on the host
void online_composite(const char *op_name, Tensor input, Tensor state, const Tensor &shifts) {
    const int64_t D = state.size(0);
    if (D == 0 || input.numel() == 0) return;
    const Tensor s = (at::isFloatingType(shifts.scalar_type()) ? at::round(shifts.detach()) : shifts.detach()).to(at::kLong);
    TORCH_CHECK(s.numel() == 0 || s.min().item<int64_t>() >= 0, op_name, ": a negative shift reads the future; an online table is causal (every entry >= 0)");
    const Tensor clamped = s.clamp_max(D);
    for (int64_t v = 1; v <= D; ++v) {
        const Tensor idx = at::nonzero(clamped == v).reshape({-1});
        if (idx.numel() == 0) continue;
        const Tensor shown = state.select(0, v - 1).index_select(1, idx);
        for (int64_t k = v - 1; k >= 1; --k) state.select(0, k).index_copy_(1, idx, state.select(0, k - 1).index_select(1, idx));
        state.select(0, 0).index_copy_(1, idx, input.index_select(1, idx));
        input.index_copy_(1, idx, shown);
    }
}

Tensor &online_cpu(Tensor &input, Tensor &state, const Tensor &shifts) {
    online_float_check(input, state, shifts);
    at::AutoDispatchBelowADInplaceOrView guard;
    online_bump(input, state);
    online_composite("temporal_shift_online_", input, state, shifts);
    return input;
}

Tensor &online_quantized_composite(Tensor &input, Tensor &state, const Tensor &shifts) {
    online_composite("temporal_shift_online_quantized_", int_repr_alias(input), int_repr_alias(state), shifts);
    return input;
}

Tensor &online_quantized_cpu(Tensor &input, Tensor &state, const Tensor &shifts) {
    online_quantized_check(input, state, shifts);
    at::AutoDispatchBelowADInplaceOrView guard;
    online_bump(input, state);
    return online_quantized_composite(input, state, shifts);
}

// served as they lie: a dense frame, 1..kOnlineSlots slots with the frame's own strides, one frame batch apart
bool online_served(const Tensor &input, const Tensor &state) {
    const int64_t D = state.size(0);
    if (D < 1 || D > kOnlineSlots || input.numel() == 0 || !(input.is_contiguous() || is_channels_last_dense(input))) return false;
    return state.strides().slice(1) == input.strides() && (D == 1 || state.stride(0) == input.numel());
}

// the writer of the online problem: {B, C, D, M} with the slot stride in the S0 place of the state's strides `ss`; `fs`: the frame's
void online_problem(shiftnd_problem &p, int64_t ss[5], int64_t fs[5], const Tensor &input, int64_t D, int dtype_bits, const char *who) {
    const int64_t B = input.size(0), C = input.size(1), M = input.numel() / (B * C);
    TORCH_CHECK(M <= INT32_MAX, who, ": the frame size must fit 32 bits");
    const bool channels_last = !input.is_contiguous();
    p.ndim = 2;
    p.dtype = dtype_bits | SHIFTND_SHIFT_DIM0 | SHIFTND_STREAM;
    p.padding_mode = 0;
    p.active = 0;
    const int64_t sizes[5] = {B, C, D, M, 1};
    const int64_t contiguous[5] = {C * M, M, B * C * M, 1, 0}, nhwc[5] = {M * C, 1, B * M * C, C, 0};
    const int32_t borders[6] = {0, static_cast<int32_t>(D), 0, static_cast<int32_t>(M), 0, 1};
    for (int i = 0; i < 5; ++i) p.sizes[i] = sizes[i], ss[i] = fs[i] = channels_last ? nhwc[i] : contiguous[i];
    fs[2] = 0;
    for (int i = 0; i < 6; ++i) p.borders[i] = borders[i];
}

// the [C] table in the kind the kernel reads; a table that has it already is passed as it is
Tensor online_table(const Tensor &shifts, at::ScalarType kind) {
    if (shifts.scalar_type() == kind && shifts.is_contiguous()) return shifts;
    const Tensor s = shifts.detach();
    return (at::isIntegralType(kind, false) && at::isFloatingType(s.scalar_type()) ? at::round(s) : s).to(kind).contiguous();
}

Tensor &online_hip(Tensor &input, Tensor &state, const Tensor &shifts) {
    TORCH_CHECK(input.is_cuda(), "temporal_shift_online_: expected a CUDA tensor");
    online_float_check(input, state, shifts);
    if (input.numel() == 0 || state.size(0) == 0) return input;
    at::AutoDispatchBelowADInplaceOrView guard;
    online_bump(input, state);
    c10::DeviceGuard device_guard(input.device());
    if (!online_served(input, state)) {
        online_composite("temporal_shift_online_", input, state, shifts);
        return input;
    }
    const bool half = input.scalar_type() == at::kHalf || input.scalar_type() == at::kBFloat16;
    const int dtype = to_shiftnd_dtype(input.scalar_type(), "temporal_shift_online__cuda") | (half ? SHIFTND_WEIGHTS_F32 : 0);
    const Tensor w = online_table(shifts, half ? at::kFloat : input.scalar_type());
    shiftnd_problem p;
    int64_t ss[5], fs[5];
    online_problem(p, ss, fs, input, state.size(0), dtype, "temporal_shift_online_");
    check_status(shiftnd_forward(&p, state.data_ptr(), ss, w.data_ptr(), input.data_ptr(), fs, current_stream(input)),
                 "temporal_shift_online_ (HIP)");
    return input;
}

Tensor &online_quantized_hip(Tensor &input, Tensor &state, const Tensor &shifts) {
    TORCH_CHECK(input.is_cuda(), "temporal_shift_online_quantized_: expected a CUDA tensor");
    online_quantized_check(input, state, shifts);
    if (input.numel() == 0 || state.size(0) == 0) return input;
    at::AutoDispatchBelowADInplaceOrView guard;
    online_bump(input, state);
    c10::DeviceGuard device_guard(input.device());
    if (!online_served(input, state)) return online_quantized_composite(input, state, shifts);
    const int dtype = quant_dtype(input.scalar_type(), "temporal_shift_online_quantized__cuda");
    const Tensor w = online_table(shifts, at::kInt);
    shiftnd_problem p;
    int64_t ss[5], fs[5];
    online_problem(p, ss, fs, input, state.size(0), dtype, "temporal_shift_online_quantized_");
    check_status(shiftnd_forward_quantized(&p, state.data_ptr(), ss, w.data_ptr(), SHIFTND_I32, 0, input.q_zero_point(), input.data_ptr(), fs,
                                           current_stream(input)),
                 "temporal_shift_online_quantized_ (HIP)");
    return input;
}

// ---- quantized interpolating temporal shift: torchshifts_quantized_learnable::temporal_shift_learnable_quantized ------------------
// temporal_shift_learnable's interpolation on the int_repr of a per-tensor quantized tensor (quint8, qint8, qint32), defined in the
// integer domain: with q = int_repr, zp the zero point and F = fp32 (8-bit) / fp64 (qint32),
//     out = clamp(zp + rint(temporal_shift_learnable((q - zp).to(F), weights.to(F), active_flag=True)), the dtype's range)
// Scale and zero point pass through, the result is contiguous, there is no gradient.  active_flag == False IS temporal_shift_quantized
// under the same table (which rounds it half to even): that route, nothing new launched.  On HIP tensors ONE flagged
// shiftnd_forward_quantized call with the fp32 table as it is (shiftnd_tshift_quant.hip): no host sync, nothing allocated but the output.
// (tslq_check is also called from torch_cpu_backend.cpp)
void tslq_check_as(const char *op_name, const Tensor &input, const Tensor &weights, int64_t n_segment, int64_t padding_mode);
void tslq_check(const Tensor &input, const Tensor &weights, int64_t n_segment, int64_t padding_mode) {
    tslq_check_as("temporal_shift_learnable_quantized", input, weights, n_segment, padding_mode);
}
// ... under the name of the op that refuses (the _cl op takes the same arguments)
void tslq_check_as(const char *op_name, const Tensor &input, const Tensor &weights, int64_t n_segment, int64_t padding_mode) {
    TORCH_CHECK(input.is_quantized(), op_name, ": expected a quantized input");
    TORCH_CHECK(input.qscheme() == at::kPerTensorAffine, op_name, ": expected a per-tensor quantized input");
    segment_check(op_name, input, weights, n_segment, padding_mode, "weights", !weights.is_quantized() && weights.scalar_type() == at::kFloat,
                  "fp32");
    TORCH_CHECK(!weights.requires_grad(), op_name, ": weights must not require grad (the quantized op has no gradient; pass weights.detach())");
}

// the kernel counts the tensor's elements in 32 bits and the flagged call has no fallback: refuse a larger tensor before anything is
// allocated
void tslq_check_size(const Tensor &input) {
    TORCH_CHECK(input.numel() + 16 < (1LL << 31), "temporal_shift_learnable_quantized: a tensor of ", input.numel(),
                " elements is beyond the kernel's limit of 2^31 - 16 units; split the batch");
}

Tensor tslq_hip(const Tensor &input_, const Tensor &weights, int64_t n_segment, int64_t padding_mode, bool active_flag) {
    tslq_check(input_, weights, n_segment, padding_mode);   // (first: a table on another device is named as such under either key)
    TORCH_CHECK(input_.is_cuda(), "temporal_shift_learnable_quantized: expected a CUDA tensor");
    if (!active_flag) return temporal_quantized_hip(input_, weights, n_segment, padding_mode);
    c10::DeviceGuard device_guard(input_.device());
    const int dtype = quant_dtype(input_.scalar_type(), "temporal_shift_learnable_quantized_cuda");
    tslq_check_size(input_);
    const Tensor t = is_channels_last_dense(input_) ? channels_last_to_contiguous(input_) : input_.contiguous();   // (a tile transpose of the int_repr)
    Tensor out = at::_empty_affine_quantized(t.sizes(), t.options().memory_format(at::MemoryFormat::Contiguous), t.q_scale(),
                                             t.q_zero_point(), c10::nullopt);
    if (t.numel() == 0) return out;
    const Tensor w = weights.contiguous();   // ([C] and [C, 1] are the same C floats)
    shiftnd_problem p;
    int64_t st[5];
    segment_problem(p, st, t, n_segment, padding_mode, true, dtype | SHIFTND_SHIFT_DIM0, false, "temporal_shift_learnable_quantized");
    check_status(shiftnd_forward_quantized(&p, t.data_ptr(), st, w.data_ptr(), SHIFTND_F32, 0, t.q_zero_point(), out.data_ptr(), st,
                                           current_stream(t)),
                 "temporal_shift_learnable_quantized (HIP)");
    return out;
}

// ---- ... keeping a channels-last layout: torchshifts_quantized_learnable_cl::temporal_shift_learnable_quantized_cl ----------------
// The values of temporal_shift_learnable_quantized with the layout of the argument kept (memory_format=torch.preserve_format in the
// Python wrappers): a dense channels-last tensor (is_channels_last_dense) comes back in its own strides with its scale
// and zero point, every other tensor exactly as the plain op returns it.  On HIP tensors a channels-last tensor is ONE
// shiftnd_forward_quantized call under SHIFTND_SHIFT_DIM0 | SHIFTND_FRAMES on the tensor as it lies (shiftnd_frames_quant.hip): no
// contiguous(), no transpose, no host sync, nothing allocated but the output.  active_flag == False IS temporal_shift_quantized_cl
// under the same table.  On CPU tensors the plain op computes and the result is laid out in the argument's strides.
Tensor tslq_cl_cpu(const Tensor &input, const Tensor &weights, int64_t n_segment, int64_t padding_mode, bool active_flag) {
    static auto plain = typed_op<tsl_forward_sig>("temporal_shift_learnable_quantized", "torchshifts_quantized_learnable");
    tslq_check_as("temporal_shift_learnable_quantized_cl", input, weights, n_segment, padding_mode);   // (the refusals under this op's name)
    return in_layout_of(plain.call(input, weights, n_segment, padding_mode, active_flag), input);
}

// the frame kernels' limits (frames_geometry_ok, include/shiftnd_hip.h) and the flagged call has no fallback: refuse a larger tensor
// before anything is allocated
void tslq_cl_check_size(const Tensor &t, int64_t T) {
    const int64_t limit = 1LL << 31, C = t.size(1), M = t.numel() / (t.size(0) * C);
    const int64_t row_groups = (M + 7) / 8;   // (frames_geometry_ok: a frame kernel's workgroup takes at least eight steps of rows)
    TORCH_CHECK(T < (1LL << 30) && M < limit && C < limit && t.size(0) < limit && t.size(0) * row_groups < limit &&
                    t.numel() * static_cast<int64_t>(t.element_size()) <= (1LL << 46),
                "temporal_shift_learnable_quantized_cl: a tensor of ", t.size(0), " frames of ", M, " pixels and ", C,
                " channels is beyond the frame kernels' limits (2^31 frames, pixels, channels or row groups, 2^46 bytes); split the batch");
}

Tensor tslq_cl_hip(const Tensor &input, const Tensor &weights, int64_t n_segment, int64_t padding_mode, bool active_flag) {
    if (!is_channels_last_dense(input)) return tslq_hip(input, weights, n_segment, padding_mode, active_flag);
    const char *op_name = "temporal_shift_learnable_quantized_cl";
    tslq_check_as(op_name, input, weights, n_segment, padding_mode);   // (first: a table on another device is named as such under either key)
    TORCH_CHECK(input.is_cuda(), op_name, ": expected a CUDA tensor");
    if (!active_flag) return temporal_quantized_cl_hip(input, weights, n_segment, padding_mode);
    c10::DeviceGuard device_guard(input.device());
    const int dtype = quant_dtype(input.scalar_type(), "temporal_shift_learnable_quantized_cl_cuda");
    tslq_cl_check_size(input, n_segment);
    Tensor out = empty_with_strides_of(input);   // (a dense channels-last tensor is not empty)
    const Tensor w = weights.contiguous();       // ([C] and [C, 1] are the same C floats)
    shiftnd_problem p;
    int64_t st[5];
    segment_problem(p, st, input, n_segment, padding_mode, true, dtype | SHIFTND_SHIFT_DIM0 | SHIFTND_FRAMES, true, op_name);
    check_status(shiftnd_forward_quantized(&p, input.data_ptr(), st, w.data_ptr(), SHIFTND_F32, 0, input.q_zero_point(), out.data_ptr(), st,
                                           current_stream(input)),
                 "temporal_shift_learnable_quantized_cl (HIP)");
    return out;
}

// ---- quantized temporal interlacing: torchshifts_quantized_interlace::temporal_interlace_quantized --------------------------------
// temporal_interlace (scales given) and temporal_shift_learnable_per_clip (scales None) on the int_repr of a per-tensor quantized
// tensor (quint8, qint8, qint32), defined in the integer domain: with q = int_repr, zp the zero point and F = fp32
// (8-bit) / fp64 (qint32),
//     out = clamp(zp + rint(temporal_interlace((q - zp).to(F), offsets.to(F), scales.to(F), active_flag)), the dtype's range)
// The tensor's scale and zero point pass through (a scale entry above 1 can saturate: the clamp is part of the definition), the
// result is contiguous, there is no gradient; both values of active_flag are this op's own.  On HIP tensors ONE flagged
// shiftnd_forward_quantized call (shiftnd_interlace_quant.hip) -- SHIFTND_PER_CLIP under the [N, C] table as it is, SHIFTND_INTERLACE
// under the packed table (one cat of the two small tables): no host sync, nothing else allocated but the output.
// (tiq_check is also called from torch_cpu_backend.cpp)
void tiq_check(const Tensor &input, const Tensor &offsets, const c10::optional<Tensor> &scales, int64_t n_segment, int64_t padding_mode) {
    const char *op_name = "temporal_interlace_quantized";
    TORCH_CHECK(input.is_quantized(), op_name, ": expected a quantized input");
    TORCH_CHECK(input.qscheme() == at::kPerTensorAffine, op_name, ": expected a per-tensor quantized input");
    // (the padding mode is looked at after both tables, below: segment_check sees a valid one)
    segment_check(op_name, input, offsets, n_segment, 0, "offsets", !offsets.is_quantized() && offsets.scalar_type() == at::kFloat, "fp32",
                  true);
    if (scales.has_value()) {
        const Tensor &sc = *scales;
        TORCH_CHECK(sc.dim() == 3 && sc.size(0) == offsets.size(0) && sc.size(1) == n_segment && sc.size(2) == input.size(1), op_name,
                    ": scales must have shape [N, T, C] = [", offsets.size(0), ", ", n_segment, ", ", input.size(1), "]");
        TORCH_CHECK(sc.device() == input.device(), op_name, ": scales must be on the input's device");
        TORCH_CHECK(!sc.is_quantized() && sc.scalar_type() == at::kFloat, op_name, ": scales must be fp32");
    }
    TORCH_CHECK(padding_mode >= 0 && padding_mode <= 4, op_name, ": padding_mode must be 0..4");
    TORCH_CHECK(!offsets.requires_grad(), op_name, ": offsets must not require grad (the quantized op has no gradient; pass offsets.detach())");
    TORCH_CHECK(!scales.has_value() || !scales->requires_grad(), op_name,
                ": scales must not require grad (the quantized op has no gradient; pass scales.detach())");
}

// the kernel counts the tensor's elements in 32 bits and the flagged call has no fallback: refuse a larger tensor before anything is
// allocated
void tiq_check_size(const Tensor &input) {
    TORCH_CHECK(input.numel() + 16 < (1LL << 31), "temporal_interlace_quantized: a tensor of ", input.numel(),
                " elements is beyond the kernel's limit of 2^31 - 16 units; split the batch");
}

Tensor tiq_hip(const Tensor &input_, const Tensor &offsets, const c10::optional<Tensor> &scales, int64_t n_segment, int64_t padding_mode,
               bool active_flag) {
    tiq_check(input_, offsets, scales, n_segment, padding_mode);   // (first: a table on another device is named as such under either key)
    TORCH_CHECK(input_.is_cuda(), "temporal_interlace_quantized: expected a CUDA tensor");
    c10::DeviceGuard device_guard(input_.device());
    const int dtype = quant_dtype(input_.scalar_type(), "temporal_interlace_quantized_cuda");
    tiq_check_size(input_);
    const Tensor t = is_channels_last_dense(input_) ? channels_last_to_contiguous(input_) : input_.contiguous();   // (a tile transpose of the int_repr)
    Tensor out = at::_empty_affine_quantized(t.sizes(), t.options().memory_format(at::MemoryFormat::Contiguous), t.q_scale(),
                                             t.q_zero_point(), c10::nullopt);
    if (t.numel() == 0) return out;
    // the [N, C] table as it is, or the packed one: N * C offsets followed by N * T * C scales
    const Tensor w = scales.has_value() ? at::cat({offsets.reshape({-1}), scales->reshape({-1})}) : offsets.contiguous();
    shiftnd_problem p;
    int64_t st[5];
    segment_problem(p, st, t, n_segment, padding_mode, active_flag,
                    dtype | SHIFTND_SHIFT_DIM0 | (scales.has_value() ? SHIFTND_INTERLACE : SHIFTND_PER_CLIP), false,
                    "temporal_interlace_quantized");
    check_status(shiftnd_forward_quantized(&p, t.data_ptr(), st, w.data_ptr(), SHIFTND_F32, 0, t.q_zero_point(), out.data_ptr(), st,
                                           current_stream(t)),
                 "temporal_interlace_quantized (HIP)");
    return out;
}

int64_t cuda_version() { return -1; }  // no CUDA toolkit: extension.py only compares when torch.version.cuda is set
int64_t hip_version() { return HIP_VERSION; }

}  // namespace torchshifts_amd

using namespace torchshifts_amd;

// Every block lists the families in the order of the header: shift, pool, fixed, fixed pool, temporal, temporal cl, learnable,
// learnable cl.
TORCH_LIBRARY(torchshifts, m) {
    m.def("_cuda_version", &cuda_version);
    m.def("_hip_version", &hip_version);
    m.def("shift1d", &shift_public<1>);
    m.def("shift2d", &shift_public<2>);
    m.def("shift3d", &shift_public<3>);
    m.def("_check_borders", &check_borders_op);
    m.def("torchshifts::_shift1d_forward(Tensor input, Tensor weights, Tensor borders, int[] new_size, int padding_mode, bool active_flag) -> Tensor");
    m.def("torchshifts::_shift1d_backward(Tensor grad, Tensor weights, Tensor input, Tensor borders, int padding_mode, bool active_flag) -> (Tensor, Tensor)");
    m.def("torchshifts::_shift2d_forward(Tensor input, Tensor weights, Tensor borders, int[] new_size, int padding_mode, bool active_flag) -> Tensor");
    m.def("torchshifts::_shift2d_backward(Tensor grad, Tensor weights, Tensor input, Tensor borders, int padding_mode, bool active_flag) -> (Tensor, Tensor)");
    m.def("torchshifts::_shift3d_forward(Tensor input, Tensor weights, Tensor borders, int[] new_size, int padding_mode, bool active_flag) -> Tensor");
    m.def("torchshifts::_shift3d_backward(Tensor grad, Tensor weights, Tensor input, Tensor borders, int padding_mode, bool active_flag) -> (Tensor, Tensor)");
    // shift + avg_pool(kernel = stride = pool, ceil_mode=True) as one op (not in the reference)
    m.def("torchshifts::shift1d_pool(Tensor input, Tensor weights, Tensor borders, int[] pool, int padding_mode, bool active_flag) -> Tensor", &shift_pool_public<1>);
    m.def("torchshifts::shift2d_pool(Tensor input, Tensor weights, Tensor borders, int[] pool, int padding_mode, bool active_flag) -> Tensor", &shift_pool_public<2>);
    m.def("torchshifts::shift3d_pool(Tensor input, Tensor weights, Tensor borders, int[] pool, int padding_mode, bool active_flag) -> Tensor", &shift_pool_public<3>);
    m.def("torchshifts::_shift1d_pool_forward(Tensor input, Tensor weights, Tensor borders, int[] new_size, int[] pool, int padding_mode, bool active_flag) -> Tensor");
    m.def("torchshifts::_shift1d_pool_backward(Tensor grad, Tensor weights, Tensor input, Tensor borders, int[] pool, int padding_mode, bool active_flag) -> (Tensor, Tensor)");
    m.def("torchshifts::_shift2d_pool_forward(Tensor input, Tensor weights, Tensor borders, int[] new_size, int[] pool, int padding_mode, bool active_flag) -> Tensor");
    m.def("torchshifts::_shift2d_pool_backward(Tensor grad, Tensor weights, Tensor input, Tensor borders, int[] pool, int padding_mode, bool active_flag) -> (Tensor, Tensor)");
    m.def("torchshifts::_shift3d_pool_forward(Tensor input, Tensor weights, Tensor borders, int[] new_size, int[] pool, int padding_mode, bool active_flag) -> Tensor");
    m.def("torchshifts::_shift3d_pool_backward(Tensor grad, Tensor weights, Tensor input, Tensor borders, int[] pool, int padding_mode, bool active_flag) -> (Tensor, Tensor)");
    // fixed (grouped) shifts: integer shifts without a weight gradient (not in the reference)
    m.def("torchshifts::shift1d_fixed(Tensor input, Tensor shifts, Tensor borders, int padding_mode) -> Tensor", &shift_fixed_public<1>);
    m.def("torchshifts::shift2d_fixed(Tensor input, Tensor shifts, Tensor borders, int padding_mode) -> Tensor", &shift_fixed_public<2>);
    m.def("torchshifts::shift3d_fixed(Tensor input, Tensor shifts, Tensor borders, int padding_mode) -> Tensor", &shift_fixed_public<3>);
    m.def("torchshifts::_shift1d_fixed_backward(Tensor grad, Tensor shifts, Tensor borders, int[] input_size, int padding_mode) -> Tensor");
    m.def("torchshifts::_shift2d_fixed_backward(Tensor grad, Tensor shifts, Tensor borders, int[] input_size, int padding_mode) -> Tensor");
    m.def("torchshifts::_shift3d_fixed_backward(Tensor grad, Tensor shifts, Tensor borders, int[] input_size, int padding_mode) -> Tensor");
    // ... followed by avg_pool(kernel = stride = pool, ceil_mode=True) as one op
    m.def("torchshifts::shift1d_fixed_pool(Tensor input, Tensor shifts, Tensor borders, int[] pool, int padding_mode) -> Tensor", &shift_fixed_pool_public<1>);
    m.def("torchshifts::shift2d_fixed_pool(Tensor input, Tensor shifts, Tensor borders, int[] pool, int padding_mode) -> Tensor", &shift_fixed_pool_public<2>);
    m.def("torchshifts::shift3d_fixed_pool(Tensor input, Tensor shifts, Tensor borders, int[] pool, int padding_mode) -> Tensor", &shift_fixed_pool_public<3>);
    m.def("torchshifts::_shift1d_fixed_pool_backward(Tensor grad, Tensor shifts, Tensor borders, int[] input_size, int[] pool, int padding_mode) -> Tensor");
    m.def("torchshifts::_shift2d_fixed_pool_backward(Tensor grad, Tensor shifts, Tensor borders, int[] input_size, int[] pool, int padding_mode) -> Tensor");
    m.def("torchshifts::_shift3d_fixed_pool_backward(Tensor grad, Tensor shifts, Tensor borders, int[] input_size, int[] pool, int padding_mode) -> Tensor");
    // temporal shift (TSM): fixed shifts across the frames of [N*T, C, ...] (not in the reference)
    m.def("torchshifts::temporal_shift(Tensor input, Tensor shifts, int n_segment, int padding_mode) -> Tensor");
    m.def("torchshifts::_temporal_shift_backward(Tensor grad, Tensor shifts, int n_segment, int padding_mode) -> Tensor");
    // ... of a per-tensor quantized tensor: the same gather on the int_repr, the zero point as the fill (QuantizedCPU / QuantizedCUDA)
    m.def("torchshifts::temporal_shift_quantized(Tensor input, Tensor shifts, int n_segment, int padding_mode) -> Tensor");
    // ... with the argument's layout kept: a dense channels-last tensor comes back channels-last (memory_format=torch.preserve_format)
    m.def("torchshifts::temporal_shift_cl(Tensor input, Tensor shifts, int n_segment, int padding_mode) -> Tensor");
    m.def("torchshifts::_temporal_shift_cl_backward(Tensor grad, Tensor shifts, int n_segment, int padding_mode) -> Tensor");
    m.def("torchshifts::temporal_shift_quantized_cl(Tensor input, Tensor shifts, int n_segment, int padding_mode) -> Tensor");
    // learnable temporal shift: a trained per-channel shift across the frames, sparse or interpolating (not in the reference)
    m.def("torchshifts::temporal_shift_learnable(Tensor input, Tensor weights, int n_segment, int padding_mode, bool active_flag) -> Tensor", &tsl_public<LearnableOps>);
    m.def("torchshifts::_temporal_shift_learnable_forward(Tensor input, Tensor weights, int n_segment, int padding_mode, bool active_flag) -> Tensor");
    m.def("torchshifts::_temporal_shift_learnable_backward(Tensor grad, Tensor weights, Tensor input, int n_segment, int padding_mode, bool active_flag) -> (Tensor, Tensor)");
    // ... with the argument's layout kept: a dense channels-last tensor is served as it lies, forward and backward
    m.def("torchshifts::temporal_shift_learnable_cl(Tensor input, Tensor weights, int n_segment, int padding_mode, bool active_flag) -> Tensor", &tsl_public<LearnableClOps>);
    m.def("torchshifts::_temporal_shift_learnable_cl_forward(Tensor input, Tensor weights, int n_segment, int padding_mode, bool active_flag) -> Tensor");
    m.def("torchshifts::_temporal_shift_learnable_cl_backward(Tensor grad, Tensor weights, Tensor input, int n_segment, int padding_mode, bool active_flag) -> (Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(torchshifts, Autograd, m) {
    m.impl("_shift1d_forward", TORCH_FN(shift_autograd<1>));
    m.impl("_shift1d_backward", TORCH_FN(GuardedBackward<ShiftOps<1>>::kernel));
    m.impl("_shift2d_forward", TORCH_FN(shift_autograd<2>));
    m.impl("_shift2d_backward", TORCH_FN(GuardedBackward<ShiftOps<2>>::kernel));
    m.impl("_shift3d_forward", TORCH_FN(shift_autograd<3>));
    m.impl("_shift3d_backward", TORCH_FN(GuardedBackward<ShiftOps<3>>::kernel));
    m.impl("_shift1d_pool_forward", TORCH_FN(pool_autograd<1>));
    m.impl("_shift1d_pool_backward", TORCH_FN(GuardedBackward<PoolOps<1>>::kernel));
    m.impl("_shift2d_pool_forward", TORCH_FN(pool_autograd<2>));
    m.impl("_shift2d_pool_backward", TORCH_FN(GuardedBackward<PoolOps<2>>::kernel));
    m.impl("_shift3d_pool_forward", TORCH_FN(pool_autograd<3>));
    m.impl("_shift3d_pool_backward", TORCH_FN(GuardedBackward<PoolOps<3>>::kernel));
    m.impl("_shift1d_fixed_backward", TORCH_FN(GuardedBackward<FixedOps<1>>::kernel));
    m.impl("_shift2d_fixed_backward", TORCH_FN(GuardedBackward<FixedOps<2>>::kernel));
    m.impl("_shift3d_fixed_backward", TORCH_FN(GuardedBackward<FixedOps<3>>::kernel));
    m.impl("_shift1d_fixed_pool_backward", TORCH_FN(GuardedBackward<FixedPoolOps<1>>::kernel));
    m.impl("_shift2d_fixed_pool_backward", TORCH_FN(GuardedBackward<FixedPoolOps<2>>::kernel));
    m.impl("_shift3d_fixed_pool_backward", TORCH_FN(GuardedBackward<FixedPoolOps<3>>::kernel));
    m.impl("temporal_shift", TORCH_FN(temporal_autograd<TemporalOps>));
    m.impl("_temporal_shift_backward", TORCH_FN(temporal_autograd_backward<TemporalOps>));
    m.impl("temporal_shift_cl", TORCH_FN(temporal_autograd<TemporalClOps>));
    m.impl("_temporal_shift_cl_backward", TORCH_FN(temporal_autograd_backward<TemporalClOps>));
    m.impl("_temporal_shift_learnable_forward", TORCH_FN(tsl_autograd<LearnableOps>));
    m.impl("_temporal_shift_learnable_backward", TORCH_FN(tsl_autograd_backward<LearnableOps>));
    m.impl("_temporal_shift_learnable_cl_forward", TORCH_FN(tsl_autograd<LearnableClOps>));
    m.impl("_temporal_shift_learnable_cl_backward", TORCH_FN(tsl_autograd_backward<LearnableClOps>));
}

// CPU tensors, the families that compose other ops: the reference's two-step sequence (shift op on the CPU key, then ATen's pool),
// the plain temporal ops' values in the argument's layout, the learnable shift on the 1-D ops
TORCH_LIBRARY_IMPL(torchshifts, CPU, m) {
    m.impl("_shift1d_pool_forward", TORCH_FN(pool_forward_composed<1>));
    m.impl("_shift1d_pool_backward", TORCH_FN(pool_backward_composed<1>));
    m.impl("_shift2d_pool_forward", TORCH_FN(pool_forward_composed<2>));
    m.impl("_shift2d_pool_backward", TORCH_FN(pool_backward_composed<2>));
    m.impl("_shift3d_pool_forward", TORCH_FN(pool_forward_composed<3>));
    m.impl("_shift3d_pool_backward", TORCH_FN(pool_backward_composed<3>));
    m.impl("temporal_shift_cl", TORCH_FN(temporal_cl_forward_cpu));
    m.impl("_temporal_shift_cl_backward", TORCH_FN(temporal_cl_backward_cpu));
    m.impl("_temporal_shift_learnable_forward", TORCH_FN(tsl_forward_cpu));
    m.impl("_temporal_shift_learnable_backward", TORCH_FN(tsl_backward_cpu));
    m.impl("_temporal_shift_learnable_cl_forward", TORCH_FN(tsl_cl_forward_cpu));
    m.impl("_temporal_shift_learnable_cl_backward", TORCH_FN(tsl_cl_backward_cpu));
}

TORCH_LIBRARY_IMPL(torchshifts, CUDA, m) {
    m.impl("_shift1d_forward", TORCH_FN(shift_forward_hip<1>));
    m.impl("_shift1d_backward", TORCH_FN(shift_backward_hip<1>));
    m.impl("_shift2d_forward", TORCH_FN(shift_forward_hip<2>));
    m.impl("_shift2d_backward", TORCH_FN(shift_backward_hip<2>));
    m.impl("_shift3d_forward", TORCH_FN(shift_forward_hip<3>));
    m.impl("_shift3d_backward", TORCH_FN(shift_backward_hip<3>));
    m.impl("_shift1d_pool_forward", TORCH_FN(pool_forward_hip<1>));
    m.impl("_shift1d_pool_backward", TORCH_FN(pool_backward_hip<1>));
    m.impl("_shift2d_pool_forward", TORCH_FN(pool_forward_hip<2>));
    m.impl("_shift2d_pool_backward", TORCH_FN(pool_backward_hip<2>));
    m.impl("_shift3d_pool_forward", TORCH_FN(pool_forward_hip<3>));
    m.impl("_shift3d_pool_backward", TORCH_FN(pool_backward_hip<3>));
    m.impl("_shift1d_fixed_backward", TORCH_FN(shift_fixed_backward_hip<1>));
    m.impl("_shift2d_fixed_backward", TORCH_FN(shift_fixed_backward_hip<2>));
    m.impl("_shift3d_fixed_backward", TORCH_FN(shift_fixed_backward_hip<3>));
    m.impl("_shift1d_fixed_pool_backward", TORCH_FN(shift_fixed_pool_backward_hip<1>));
    m.impl("_shift2d_fixed_pool_backward", TORCH_FN(shift_fixed_pool_backward_hip<2>));
    m.impl("_shift3d_fixed_pool_backward", TORCH_FN(shift_fixed_pool_backward_hip<3>));
    m.impl("temporal_shift", TORCH_FN(temporal_forward_hip));
    m.impl("_temporal_shift_backward", TORCH_FN(temporal_backward_hip));
    m.impl("temporal_shift_cl", TORCH_FN(temporal_cl_forward_hip));
    m.impl("_temporal_shift_cl_backward", TORCH_FN(temporal_cl_backward_hip));
    m.impl("_temporal_shift_learnable_forward", TORCH_FN(tsl_forward_hip<LearnableOps>));
    m.impl("_temporal_shift_learnable_backward", TORCH_FN(tsl_backward_hip<LearnableOps>));
    m.impl("_temporal_shift_learnable_cl_forward", TORCH_FN(tsl_forward_hip<LearnableClOps>));
    m.impl("_temporal_shift_learnable_cl_backward", TORCH_FN(tsl_backward_hip<LearnableClOps>));
}

TORCH_LIBRARY_IMPL(torchshifts, QuantizedCPU, m) {
    m.impl("temporal_shift_quantized_cl", TORCH_FN(temporal_quantized_cl_cpu));
}

TORCH_LIBRARY_IMPL(torchshifts, QuantizedCUDA, m) {
    m.impl("_shift1d_forward", TORCH_FN(qshift_forward_hip<1>));
    m.impl("_shift1d_backward", TORCH_FN(qshift_backward));
    m.impl("_shift2d_forward", TORCH_FN(qshift_forward_hip<2>));
    m.impl("_shift2d_backward", TORCH_FN(qshift_backward));
    m.impl("_shift3d_forward", TORCH_FN(qshift_forward_hip<3>));
    m.impl("_shift3d_backward", TORCH_FN(qshift_backward));
    m.impl("_shift1d_pool_forward", TORCH_FN(qpool_forward_hip<1>));
    m.impl("_shift2d_pool_forward", TORCH_FN(qpool_forward_hip<2>));
    m.impl("_shift3d_pool_forward", TORCH_FN(qpool_forward_hip<3>));
    m.impl("temporal_shift_quantized", TORCH_FN(temporal_quantized_hip));
    m.impl("temporal_shift_quantized_cl", TORCH_FN(temporal_quantized_cl_hip));
}

// the per-clip temporal shifts: their own namespace (the op set of torchshifts:: is pinned)
TORCH_LIBRARY(torchshifts_per_clip, m) {
    m.def("torchshifts_per_clip::temporal_shift_learnable_per_clip(Tensor input, Tensor weights, int n_segment, int padding_mode, bool active_flag) -> Tensor", &tslpc_public<PerClipLearnableOps>);
    m.def("torchshifts_per_clip::_temporal_shift_learnable_per_clip_forward(Tensor input, Tensor weights, int n_segment, int padding_mode, bool active_flag) -> Tensor");
    m.def("torchshifts_per_clip::_temporal_shift_learnable_per_clip_backward(Tensor grad, Tensor weights, Tensor input, int n_segment, int padding_mode, bool active_flag) -> (Tensor, Tensor)");
    m.def("torchshifts_per_clip::temporal_shift_per_clip(Tensor input, Tensor shifts, int n_segment, int padding_mode) -> Tensor");
    m.def("torchshifts_per_clip::_temporal_shift_per_clip_backward(Tensor grad, Tensor shifts, int n_segment, int padding_mode) -> Tensor");
}

TORCH_LIBRARY_IMPL(torchshifts_per_clip, Autograd, m) {
    m.impl("_temporal_shift_learnable_per_clip_forward", TORCH_FN(tslpc_autograd<PerClipLearnableOps>));
    m.impl("_temporal_shift_learnable_per_clip_backward", TORCH_FN(tslpc_autograd_backward<PerClipLearnableOps>));
    m.impl("temporal_shift_per_clip", TORCH_FN(tpc_autograd<PerClipOps>));
    m.impl("_temporal_shift_per_clip_backward", TORCH_FN(tpc_autograd_backward<PerClipOps>));
}
TORCH_LIBRARY_IMPL(torchshifts_per_clip, CPU, m) {
    m.impl("_temporal_shift_learnable_per_clip_forward", TORCH_FN(tslpc_forward_cpu));
    m.impl("_temporal_shift_learnable_per_clip_backward", TORCH_FN(tslpc_backward_cpu));
    m.impl("temporal_shift_per_clip", TORCH_FN(tpc_forward_cpu));
    m.impl("_temporal_shift_per_clip_backward", TORCH_FN(tpc_backward_cpu));
}
TORCH_LIBRARY_IMPL(torchshifts_per_clip, CUDA, m) {
    m.impl("_temporal_shift_learnable_per_clip_forward", TORCH_FN(tsl_forward_hip<PerClipLearnableOps>));
    m.impl("_temporal_shift_learnable_per_clip_backward", TORCH_FN(tsl_backward_hip<PerClipLearnableOps>));
    m.impl("temporal_shift_per_clip", TORCH_FN(tpc_forward_hip));
    m.impl("_temporal_shift_per_clip_backward", TORCH_FN(tpc_backward_hip));
}

// the per-clip temporal shifts with the argument's layout kept: a namespace of its own, so that torchshifts_per_clip:: keeps its op set
TORCH_LIBRARY(torchshifts_per_clip_cl, m) {
    m.def("torchshifts_per_clip_cl::temporal_shift_learnable_per_clip_cl(Tensor input, Tensor weights, int n_segment, int padding_mode, bool active_flag) -> Tensor", &tslpc_public<PerClipLearnableClOps>);
    m.def("torchshifts_per_clip_cl::_temporal_shift_learnable_per_clip_cl_forward(Tensor input, Tensor weights, int n_segment, int padding_mode, bool active_flag) -> Tensor");
    m.def("torchshifts_per_clip_cl::_temporal_shift_learnable_per_clip_cl_backward(Tensor grad, Tensor weights, Tensor input, int n_segment, int padding_mode, bool active_flag) -> (Tensor, Tensor)");
    m.def("torchshifts_per_clip_cl::temporal_shift_per_clip_cl(Tensor input, Tensor shifts, int n_segment, int padding_mode) -> Tensor");
    m.def("torchshifts_per_clip_cl::_temporal_shift_per_clip_cl_backward(Tensor grad, Tensor shifts, int n_segment, int padding_mode) -> Tensor");
}
TORCH_LIBRARY_IMPL(torchshifts_per_clip_cl, Autograd, m) {
    m.impl("_temporal_shift_learnable_per_clip_cl_forward", TORCH_FN(tslpc_autograd<PerClipLearnableClOps>));
    m.impl("_temporal_shift_learnable_per_clip_cl_backward", TORCH_FN(tslpc_autograd_backward<PerClipLearnableClOps>));
    m.impl("temporal_shift_per_clip_cl", TORCH_FN(tpc_autograd<PerClipClOps>));
    m.impl("_temporal_shift_per_clip_cl_backward", TORCH_FN(tpc_autograd_backward<PerClipClOps>));
}
TORCH_LIBRARY_IMPL(torchshifts_per_clip_cl, CPU, m) {
    m.impl("_temporal_shift_learnable_per_clip_cl_forward", TORCH_FN(tslpc_cl_forward_cpu));
    m.impl("_temporal_shift_learnable_per_clip_cl_backward", TORCH_FN(tslpc_cl_backward_cpu));
    m.impl("temporal_shift_per_clip_cl", TORCH_FN(tpc_cl_forward_cpu));
    m.impl("_temporal_shift_per_clip_cl_backward", TORCH_FN(tpc_cl_backward_cpu));
}
TORCH_LIBRARY_IMPL(torchshifts_per_clip_cl, CUDA, m) {
    m.impl("_temporal_shift_learnable_per_clip_cl_forward", TORCH_FN(tsl_forward_hip<PerClipLearnableClOps>));
    m.impl("_temporal_shift_learnable_per_clip_cl_backward", TORCH_FN(tsl_backward_hip<PerClipLearnableClOps>));
    m.impl("temporal_shift_per_clip_cl", TORCH_FN(tpc_cl_forward_hip));
    m.impl("_temporal_shift_per_clip_cl_backward", TORCH_FN(tpc_cl_backward_hip));
}

// temporal interlacing (the per-clip shift times a scale per clip, frame and channel): a namespace of its own, so that the op sets
// of the namespaces above stay
TORCH_LIBRARY(torchshifts_interlace, m) {
    m.def("torchshifts_interlace::temporal_interlace(Tensor input, Tensor offsets, Tensor scales, int n_segment, int padding_mode, bool active_flag) -> Tensor", &tin_public<InterlaceOps>);
    m.def("torchshifts_interlace::_temporal_interlace_forward(Tensor input, Tensor offsets, Tensor scales, int n_segment, int padding_mode, bool active_flag) -> Tensor");
    m.def("torchshifts_interlace::_temporal_interlace_backward(Tensor grad, Tensor offsets, Tensor scales, Tensor input, int n_segment, int padding_mode, bool active_flag) -> (Tensor, Tensor, Tensor)");
}
TORCH_LIBRARY_IMPL(torchshifts_interlace, Autograd, m) {
    m.impl("_temporal_interlace_forward", TORCH_FN(tin_autograd<InterlaceOps>));
    m.impl("_temporal_interlace_backward", TORCH_FN(tin_autograd_backward<InterlaceOps>));
}
TORCH_LIBRARY_IMPL(torchshifts_interlace, CPU, m) {
    m.impl("_temporal_interlace_forward", TORCH_FN(tin_forward_cpu));
    m.impl("_temporal_interlace_backward", TORCH_FN(tin_backward_cpu));
}
TORCH_LIBRARY_IMPL(torchshifts_interlace, CUDA, m) {
    m.impl("_temporal_interlace_forward", TORCH_FN(tin_forward_hip<InterlaceOps>));
    m.impl("_temporal_interlace_backward", TORCH_FN(tin_backward_hip<InterlaceOps>));
}

// temporal interlacing with the argument's layout kept: a namespace of its own, so that torchshifts_interlace:: keeps its op set
TORCH_LIBRARY(torchshifts_interlace_cl, m) {
    m.def("torchshifts_interlace_cl::temporal_interlace_cl(Tensor input, Tensor offsets, Tensor scales, int n_segment, int padding_mode, bool active_flag) -> Tensor", &tin_public<InterlaceClOps>);
    m.def("torchshifts_interlace_cl::_temporal_interlace_cl_forward(Tensor input, Tensor offsets, Tensor scales, int n_segment, int padding_mode, bool active_flag) -> Tensor");
    m.def("torchshifts_interlace_cl::_temporal_interlace_cl_backward(Tensor grad, Tensor offsets, Tensor scales, Tensor input, int n_segment, int padding_mode, bool active_flag) -> (Tensor, Tensor, Tensor)");
}
TORCH_LIBRARY_IMPL(torchshifts_interlace_cl, Autograd, m) {
    m.impl("_temporal_interlace_cl_forward", TORCH_FN(tin_autograd<InterlaceClOps>));
    m.impl("_temporal_interlace_cl_backward", TORCH_FN(tin_autograd_backward<InterlaceClOps>));
}
TORCH_LIBRARY_IMPL(torchshifts_interlace_cl, CPU, m) {
    m.impl("_temporal_interlace_cl_forward", TORCH_FN(tin_cl_forward_cpu));
    m.impl("_temporal_interlace_cl_backward", TORCH_FN(tin_cl_backward_cpu));
}
TORCH_LIBRARY_IMPL(torchshifts_interlace_cl, CUDA, m) {
    m.impl("_temporal_interlace_cl_forward", TORCH_FN(tin_forward_hip<InterlaceClOps>));
    m.impl("_temporal_interlace_cl_backward", TORCH_FN(tin_backward_hip<InterlaceClOps>));
}

// the in-place temporal shift: its own namespace (the op set of torchshifts:: is pinned)
TORCH_LIBRARY(torchshifts_inplace, m) {
    m.def("torchshifts_inplace::temporal_shift_(Tensor(a!) input, Tensor shifts, int n_segment, int padding_mode) -> Tensor(a!)");
    m.def("torchshifts_inplace::temporal_shift_quantized_(Tensor(a!) input, Tensor shifts, int n_segment, int padding_mode) -> Tensor(a!)");
}

TORCH_LIBRARY_IMPL(torchshifts_inplace, Autograd, m) { m.impl("temporal_shift_", TORCH_FN(temporal_inplace_autograd)); }
TORCH_LIBRARY_IMPL(torchshifts_inplace, CPU, m) { m.impl("temporal_shift_", TORCH_FN(temporal_inplace_cpu)); }
TORCH_LIBRARY_IMPL(torchshifts_inplace, CUDA, m) { m.impl("temporal_shift_", TORCH_FN(temporal_inplace_hip)); }
TORCH_LIBRARY_IMPL(torchshifts_inplace, QuantizedCPU, m) { m.impl("temporal_shift_quantized_", TORCH_FN(temporal_quantized_inplace_cpu)); }
TORCH_LIBRARY_IMPL(torchshifts_inplace, QuantizedCUDA, m) { m.impl("temporal_shift_quantized_", TORCH_FN(temporal_quantized_inplace_hip)); }

// the online temporal shift: its own namespace (the op sets of the three above are pinned).  No Autograd key: an inference op
TORCH_LIBRARY(torchshifts_online, m) {
    m.def("torchshifts_online::temporal_shift_online_(Tensor(a!) input, Tensor(b!) state, Tensor shifts) -> Tensor(a!)");
    m.def("torchshifts_online::temporal_shift_online_quantized_(Tensor(a!) input, Tensor(b!) state, Tensor shifts) -> Tensor(a!)");
}

TORCH_LIBRARY_IMPL(torchshifts_online, CPU, m) { m.impl("temporal_shift_online_", TORCH_FN(online_cpu)); }
TORCH_LIBRARY_IMPL(torchshifts_online, CUDA, m) { m.impl("temporal_shift_online_", TORCH_FN(online_hip)); }
TORCH_LIBRARY_IMPL(torchshifts_online, QuantizedCPU, m) { m.impl("temporal_shift_online_quantized_", TORCH_FN(online_quantized_cpu)); }
TORCH_LIBRARY_IMPL(torchshifts_online, QuantizedCUDA, m) { m.impl("temporal_shift_online_quantized_", TORCH_FN(online_quantized_hip)); }

// the quantized interpolating temporal shift: its own namespace (the op sets above are pinned).  No Autograd key: an inference op
// (QuantizedCPU: torch_cpu_backend.cpp)
TORCH_LIBRARY(torchshifts_quantized_learnable, m) {
    m.def("torchshifts_quantized_learnable::temporal_shift_learnable_quantized(Tensor input, Tensor weights, int n_segment, int padding_mode, bool active_flag) -> Tensor");
}

TORCH_LIBRARY_IMPL(torchshifts_quantized_learnable, QuantizedCUDA, m) { m.impl("temporal_shift_learnable_quantized", TORCH_FN(tslq_hip)); }

// ... keeping a channels-last layout: its own namespace again (the op set above is pinned too).  No Autograd key.  The QuantizedCPU
// kernel composes the plain op, so it is registered here
TORCH_LIBRARY(torchshifts_quantized_learnable_cl, m) {
    m.def("torchshifts_quantized_learnable_cl::temporal_shift_learnable_quantized_cl(Tensor input, Tensor weights, int n_segment, int padding_mode, bool active_flag) -> Tensor");
}

TORCH_LIBRARY_IMPL(torchshifts_quantized_learnable_cl, QuantizedCPU, m) { m.impl("temporal_shift_learnable_quantized_cl", TORCH_FN(tslq_cl_cpu)); }
TORCH_LIBRARY_IMPL(torchshifts_quantized_learnable_cl, QuantizedCUDA, m) { m.impl("temporal_shift_learnable_quantized_cl", TORCH_FN(tslq_cl_hip)); }

// quantized temporal interlacing / the quantized per-clip temporal shift (scales None): a namespace of its own.  No Autograd key: an
// inference op (QuantizedCPU: torch_cpu_backend.cpp)
TORCH_LIBRARY(torchshifts_quantized_interlace, m) {
    m.def("torchshifts_quantized_interlace::temporal_interlace_quantized(Tensor input, Tensor offsets, Tensor? scales, int n_segment, int padding_mode, bool active_flag) -> Tensor");
}

TORCH_LIBRARY_IMPL(torchshifts_quantized_interlace, QuantizedCUDA, m) { m.impl("temporal_interlace_quantized", TORCH_FN(tiq_hip)); }
