/*
 * shiftnd_hip.h -- C ABI of the MI355X-native shiftnd library (libshiftnd_hip.so).
 *
 * This is the drop-in boundary of the hot path: plain pointers, sizes and strides, no torch types.
 * Each entry point replaces one backend function of the reference
 * (DeadAt0m/ActiveSparseShifts-PyTorch, paths relative to torchshifts/csrc/ops/):
 *
 *   shiftnd_forward            <- shiftnd_forward<nD,pad,active>   cuda/shifts_cuda.cu:202-266
 *                                 (== cpu/shifts_cpu.cpp:216-232), i.e. the backend behind
 *                                 torchshifts::_shift{1,2,3}d_forward (shifts.cpp:168-181)
 *   shiftnd_backward           <- shiftnd_backward<nD,pad,active>  cuda/shifts_cuda.cu:270-345
 *                                 (== cpu/shifts_cpu.cpp:237-255), behind
 *                                 torchshifts::_shift{1,2,3}d_backward
 *   shiftnd_forward_quantized  <- qshiftnd<nD,pad>                 quantized/shifts_quantized.cpp:107-130
 *                                 (the reference has no GPU quantized path; this is new)
 *   shiftnd_check_borders      <- check_borders                    shifts.cpp:93-135 (host only)
 *   shiftnd_forward_pooled /   <- the module-level sequence `_reduction_fn(shift(x))` of the reference's
 *   shiftnd_backward_pooled       depthwise-conv emulation (torchshifts/modules/shifts.py:81-89, 150-153:
 *                                 shift, then avg_pool{N}d(kernel = stride, ceil_mode=True)) in one pass
 *
 * Conventions
 *   - Tensors are described the way the reference's kernels see them: sizes[5] = {N, C, H, W, D}
 *     of the INPUT (unused trailing spatial dims = 1) and element strides[5] in the same order
 *     (unused = 0).  ndim = number of spatial dims (1..3).
 *   - weights: device pointer to a contiguous [C, ndim] array of the input's dtype
 *     (column s shifts spatial dim s: H, W, D -- functional.py:76-77); fp32 for fp16 / bf16 tensors
 *     when p->dtype carries SHIFTND_WEIGHTS_F32 (mixed precision, below).
 *   - borders: 6 HOST ints {l_i, r_i, l_j, r_j, l_k, r_k}, the absolute [l, r) window that
 *     check_borders produces; the output has spatial sizes r - l.
 *   - padding_mode: 0 zeros, 1 border, 2 periodic, 3 reflect, 4 symmetric
 *     (BIPadding, kernels/shifts_kernels.h:5).
 *   - All device pointers must belong to the device that is current on the calling thread;
 *     `stream` is a hipStream_t (NULL = default stream).  Calls only enqueue work: no host
 *     synchronisation, no allocation (graph-capture safe).
 *   - Every function returns SHIFTND_OK (0) or a negative shiftnd_status; nothing is thrown.
 *   - Numerics contract: SSL forward / SSL input-grad / quantized are pure
 *     gathers and bit-exact; for fp32 / fp64 tensors interpolation is evaluated as v1*(1-x)+v2*x
 *     with separate multiplies and add (no FMA contraction), bit-identical to the reference's CPU
 *     build; 16-bit inputs are widened to fp32, interpolated there (one multiply and one fused
 *     multiply-add per lerp) and rounded once (RNE) on store; the weight gradient sums products in
 *     the compute type (fused multiply-add), accumulates them in fp64 by a deterministic two-stage
 *     reduction and rounds once to the tensor dtype.
 *   - Mixed precision (SHIFTND_WEIGHTS_F32): the fp32 weight enters the 16-bit kernels' compute type
 *     (fp32) as it is and is never rounded to 16 bits: the sparse shift is rintf(w), the backward
 *     prepares its shift and fractions from the fp32 value, the interpolation fractions are the fp32
 *     ones.  out and grad_x keep the tensor dtype under the 16-bit contract above (widened,
 *     interpolated in fp32, rounded once); grad_w is fp32, the fp64 sum narrowed once.  With weights
 *     that 16 bits hold exactly a mixed call runs the same kernel as the same-dtype call and returns
 *     the same bits in out and grad_x.
 */
#ifndef SHIFTND_HIP_H_
#define SHIFTND_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHIFTND_ABI_VERSION 5
#define SHIFTND_API __attribute__((visibility("default")))

typedef enum shiftnd_dtype {
    SHIFTND_F32 = 0,
    SHIFTND_F64 = 1,
    SHIFTND_F16 = 2,
    SHIFTND_BF16 = 3,
    SHIFTND_I8 = 4,  /* qint8  int_repr */
    SHIFTND_U8 = 5,  /* quint8 int_repr */
    SHIFTND_I32 = 6  /* qint32 int_repr */
} shiftnd_dtype;

/*
 * Mixed precision (what torch.autocast produces: 16-bit activations, fp32 parameters).  OR-ed onto SHIFTND_F16 or SHIFTND_BF16
 * in shiftnd_problem.dtype: `weights` is a const float [C, ndim] array and `grad_w` a float [C, ndim] array; x, out, grad_out
 * and grad_x keep the 16-bit type.  No other combination of tensor and weight types exists.
 *   Honoured by shiftnd_forward, shiftnd_backward, shiftnd_forward_pooled, shiftnd_backward_pooled; shiftnd_pooled_sizes, both
 *   *_workspace_bytes and both *_serves_channels_last give the answer they give without the flag.
 *   Errors, before anything is launched:
 *     - on any other dtype (F32, F64, the quantized types), and on the quantized entry points: SHIFTND_ERR_UNSUPPORTED_DTYPE
 *       (the workspace queries and *_serves_channels_last, which return no status, answer 0);
 *     - together with the x == NULL && grad_w == NULL forms of shiftnd_backward / shiftnd_backward_pooled:
 *       SHIFTND_ERR_INVALID_ARGUMENT (a fixed table is converted to the tensor dtype by its owner).
 * Without the flag nothing changes.
 */
#define SHIFTND_WEIGHTS_F32 0x100

/*
 * The learnable temporal shift (a trained per-channel shift across the frames of a video tensor [N*T, C, H, W], seen as the
 * problem [N, C, T, H*W] with strides {T*C*M, M, C*M, 1}).  OR-ed onto a float dtype in shiftnd_problem.dtype: `weights` and
 * `grad_w` are [C] arrays, ONE entry per channel; the 1-D shift (sparse or interpolating, p->active) acts on spatial dim 0 only
 * and every other spatial dim is untouched.  out, grad_x and grad_w are those of the 1-D problem [N * S1 * S2, C, S0] on the
 * permuted tensors.  Combines with SHIFTND_WEIGHTS_F32.
 *   Honoured by shiftnd_forward, shiftnd_backward and shiftnd_backward_workspace_bytes (which then sizes this plan alone).
 *   Accepted: ndim 2 or 3; F32, F64, F16, BF16; both values of p->active; every padding mode; the whole window; all tensors
 *   (x, out, grad_out, grad_x) dense in memory order N, S0, C, S1, S2 (a dim of size 1 has no stride to check) at element-aligned
 *   bases; N, C, S1 * S2 and N * S0 * C below 2^31, S0 below 2^30, fewer than 2^31 - 16 two-byte units in the tensor.  There is
 *   no fallback under the flag: C == 1, S0 == 1 and S1 * S2 == 1 are served by the same kernels (shiftnd_last_kernel():
 *   tshift_forward / tshift_backward, *_ragged for planes that are not whole 16-byte pieces or bases off the 16-byte grid;
 *   shiftnd_last_path(): SHIFTND_PATH_PLANE).
 *   Errors, before anything is launched: the quantized types SHIFTND_ERR_UNSUPPORTED_DTYPE (the workspace query answers 0);
 *   ndim 1, a cut window, any other layout, a size beyond the limits, the x == NULL && grad_w == NULL form of shiftnd_backward:
 *   SHIFTND_ERR_INVALID_ARGUMENT.  Every other entry point refuses the flag as an unknown dtype (shiftnd_forward_quantized: with
 *   a float dtype; its own use of the flag is below).
 *
 * Channels-last tensors (the FIXED temporal shift of an NHWC video tensor): under the flag shiftnd_forward also takes x and out that
 * are both dense in memory order N, S0, S1, S2, C (a dim of size 1 has no stride to check), element-aligned bases -- the video tensor
 * [N*T, C, H, W] in channels-last memory, seen as {ndim 2, sizes N, C, T, M = H*W} with strides {T*M*C, 1, M*C, C}.  Strides alone
 * cannot tell that call from a genuine 2-D shift of an NHWC tensor, which is why it is the flag that asks for it.
 *   Accepted: p->active == 0 (the sparse shift: rint of the entry); ndim 2 or 3; the whole window; F32, F64, F16, BF16, the last two
 *   also with SHIFTND_WEIGHTS_F32; every padding mode.  Bounds of the kernel's index arithmetic (64-bit byte offsets throughout;
 *   32-bit frame and workgroup indices, the 32-bit padding map): N, C and S1 * S2 below 2^31, S0 below 2^30, N * S0 below 2^31,
 *   N * S0 * ceil(S1 * S2 / 8) below 2^31 (the grid), the tensor below 2^46 bytes.  A tensor that both layouts describe (S1 * S2 == 1
 *   or C == 1) stays with the tshift kernels.  Served by csrc/shiftnd_frames.hip without a fallback (shiftnd_last_kernel():
 *   frames_forward for pixel rows -- C elements -- of whole 16-byte pieces at 16-byte-aligned bases, frames_forward_ragged
 *   otherwise; shiftnd_last_path(): SHIFTND_PATH_CL): a thread copies its 16-byte piece of the rows from the same pixel of the
 *   source frame, or fills it; a piece whose channels do not share one source frame is assembled element by element (exact, slow).
 *   The input gradient of that shift is the same call on the gradient under the negated table (grad_x[t] = grad_out[pad(t + s)]);
 *   shiftnd_backward does not take the layout.
 *   shiftnd_forward_quantized honours the flag for this layout ALONE: I8 / U8 / I32 tensors, same sizes and limits; wq is a [C]
 *   integer table of wq_dtype (shift = entry - w_zero_point), zeros padding fills with x_zero_point.  SHIFTND_WEIGHTS_F32 with a
 *   quantized dtype, or a float dtype with the flag on that entry point: SHIFTND_ERR_UNSUPPORTED_DTYPE; segment-major quantized
 *   tensors, a cut window, ndim 1, a size beyond the bounds: SHIFTND_ERR_INVALID_ARGUMENT.
 *   Errors, before anything is launched: p->active == 1 on the channels-last layout, x and out in different layouts (channels-last
 *   with segment-major or NCHW-dense), a size beyond the bounds: SHIFTND_ERR_INVALID_ARGUMENT.
 *
 * Quantized, interpolating (the trained shift of a per-tensor quantized video tensor): shiftnd_forward_quantized under the flag with
 * wq_dtype == SHIFTND_F32 -- wq is the fp32 [C] table of trained shifts, w_zero_point 0 -- interpolates I8 / U8 / I32 tensors in the
 * integer domain.  With q the int_repr, zp = x_zero_point and (iw, dw) = (floor(w), w - floor(w)) in F = fp32 (I8 / U8) or fp64 (I32):
 *     out = clamp(zp + rint((q[pad(t - iw)] - zp) * (1 - dw) + (q[pad(t - iw + 1)] - zp) * dw), the element type's range)
 * two multiplies and one add in F, rint half to even; a filled frame (zeros padding) contributes 0, which is zp in out.  The scale
 * does not enter and nothing is dequantized.
 *   Accepted: p->active == 1; ndim 2 or 3; every padding mode; the whole window; x and out distinct, both dense in memory order
 *   N, S0, C, S1, S2 at element-aligned bases; x_zero_point inside the element type's range; N, C, S1 * S2 and N * S0 * C below 2^31,
 *   S0 below 2^30, fewer than 2^31 - 16 elements in the tensor.  Served by csrc/shiftnd_tshift_quant.hip without a fallback
 *   (shiftnd_last_kernel(): tshift_forward_quantized for every element type and unit width; shiftnd_last_path(): SHIFTND_PATH_PLANE).
 *   Errors, before anything is launched: a float dtype, and p->active == 0 (the sparse shift is the integer table's call: a float
 *   table stays what it was there, an unsupported table type): SHIFTND_ERR_UNSUPPORTED_DTYPE; any other flag bit beside
 *   SHIFTND_SHIFT_DIM0, a nonzero w_zero_point, out == x, channels-last views, a cut window, ndim 1, a size beyond the limits:
 *   SHIFTND_ERR_INVALID_ARGUMENT.  A float wq_dtype other than SHIFTND_F32, and SHIFTND_F32 without the flag, stay
 *   SHIFTND_ERR_UNSUPPORTED_DTYPE.
 *   ... of channels-last tensors: SHIFTND_SHIFT_DIM0 | SHIFTND_FRAMES on p->dtype with wq_dtype == SHIFTND_F32 is the same call --
 *   the same table, the same arithmetic, the same result bit for bit -- on x and out that are BOTH dense channels-last views (memory
 *   order N, S0, S1, S2, C: strides {S0*M*C, 1, M*C, C} for sizes {N, C, S0, M}) at element-aligned bases.  The flag pair is required:
 *   such views under SHIFTND_SHIFT_DIM0 alone stay refused.  Accepted: p->active == 1; ndim 2 or 3; every padding mode; the whole
 *   window; x and out distinct; w_zero_point 0; x_zero_point inside the element type's range; the bounds of the channels-last sparse
 *   shift above (N, C, S1 * S2 and N * S0 below 2^31, S0 below 2^30, 2^46 bytes).  Served by csrc/shiftnd_frames_quant.hip without a
 *   fallback (shiftnd_last_kernel(): frames_forward_quantized, or frames_forward_quantized_ragged where a channel row or a base is
 *   not a multiple of 16 bytes; shiftnd_last_path(): SHIFTND_PATH_CL).  Errors, before anything is launched: p->active == 0 and a
 *   float dtype: SHIFTND_ERR_UNSUPPORTED_DTYPE; any further flag bit, a nonzero w_zero_point, out == x, segment-major tensors, a cut
 *   window, ndim 1, a size beyond the limits: SHIFTND_ERR_INVALID_ARGUMENT.
 *   ... under a per-clip table, and interlaced: SHIFTND_SHIFT_DIM0 plus exactly ONE of SHIFTND_PER_CLIP / SHIFTND_INTERLACE on p->dtype
 *   with wq_dtype == SHIFTND_F32 and w_zero_point 0, on segment-major tensors (csrc/shiftnd_interlace_quant.hip).
 *     SHIFTND_PER_CLIP:  wq is the fp32 [N, C] table, one row per clip: clip n is shifted by w = wq[n * C + c]; s = 1.
 *     SHIFTND_INTERLACE: wq is the packed fp32 array of the float interlace call -- the N * C offsets followed by the N * S0 * C
 *                        scales: w = wq[n * C + c], s = wq[N * C + (n * S0 + t) * C + c].
 *     out = clamp(zp + rint(((q[pad(t - iw)] - zp) * (1 - dw) + (q[pad(t - iw + 1)] - zp) * dw) * s), the element type's range)
 *   the interpolation above, then ONE multiply by the plane's scale in F, rint half to even; a filled frame contributes 0, which is zp
 *   in out under any finite scale.  The tensor's scale does not enter, so a scale entry above 1 can saturate: the clamp is part of the
 *   definition.  p->active == 0 is served too: (iw, dw) = (rint(w) half to even, 0), the scale still applied.  Offsets and scales
 *   must be finite (not validated).
 *   Accepted: p->active 0 or 1; ndim 2 or 3; every padding mode; the whole window; x and out distinct, both dense in memory order
 *   N, S0, C, S1, S2 at element-aligned bases; wq aligned to 4 bytes; x_zero_point inside the element type's range; the limits of the
 *   [C]-table call above (N * S0 * C below 2^31 bounds both table indices; fewer than 2^31 - 16 elements).  Served without a fallback
 *   (shiftnd_last_kernel(): tinterlace_forward_quantized for every element type, unit width and both bits; shiftnd_last_path():
 *   SHIFTND_PATH_PLANE); no workspace (shiftnd_backward_workspace_bytes: 0).  Errors, before anything is launched: a float dtype:
 *   SHIFTND_ERR_UNSUPPORTED_DTYPE; both bits together, any further flag bit, a nonzero w_zero_point, out == x, channels-last views, a
 *   cut window, ndim 1, a size beyond the limits, a misaligned table: SHIFTND_ERR_INVALID_ARGUMENT.  An integer wq_dtype under either
 *   bit stays what it was, SHIFTND_ERR_UNSUPPORTED_DTYPE.
 *
 * In place (the FIXED temporal shift written into its input): under the flag, out == x -- the same pointer, with identical strides --
 * and p->active == 0 is a call of its own, served by csrc/shiftnd_inplace.hip.  A thread owns one naturally aligned power-of-two
 * piece (at most 16 bytes: the widest that divides the plane's bytes, or the channel row's bytes, and the base) at the same offset in
 * every frame of one clip, gathers the pieces of the frames whose content changes into registers and stores them; it reads and
 * writes no byte outside its piece, so there is no hazard between threads, and a channel whose shift maps every frame to itself
 * (shift 0, S0 == 1, a whole period) is neither read nor written.  No workspace.
 *   shiftnd_forward: F32, F64, F16, BF16; `weights` a [C] array of the tensor dtype, or fp32 under SHIFTND_WEIGHTS_F32.
 *   shiftnd_forward_quantized: I8, U8, I32; wq a [C] integer table of wq_dtype, zeros padding fills with x_zero_point.  For the
 *   in-place form ALONE this entry point also takes the segment-major layout (with out != x it stays refused).
 *   Accepted: both dense layouts -- segment-major (memory order N, S0, C, S1, S2) and channels-last (N, S0, S1, S2, C); a tensor both
 *   describe (S1 * S2 == 1 or C == 1) is served as segment-major, with the same result -- ndim 2 or 3, the whole window, every padding
 *   mode, element-aligned bases, S0 <= 16 (the kernel keeps a clip's frames in 16 register slots).  Bounds: those of the channels-last
 *   layout above and N * ceil(C * S1 * S2 / 256) below 2^31 (the grid).  shiftnd_last_kernel(): frames_inplace for 16-byte pieces,
 *   frames_inplace_ragged for narrower ones; shiftnd_last_path(): SHIFTND_PATH_PLANE for segment-major, SHIFTND_PATH_CL for
 *   channels-last.
 *   Errors, before anything is launched (the out-of-place kernels would race on such a call): S0 > 16, p->active == 1, a cut window,
 *   SHIFTND_FRAMES, x and out strides that differ, a layout that is neither dense form, a size beyond the bounds:
 *   SHIFTND_ERR_INVALID_ARGUMENT.
 *   out == x WITHOUT the flag, and tensors that overlap in part, stay undefined: the kernels declare x and out __restrict__.
 * Without the flag nothing changes.
 */
#define SHIFTND_SHIFT_DIM0 0x200

/*
 * The learnable temporal shift on channels-last tensors.  OR-ed onto a float dtype TOGETHER WITH SHIFTND_SHIFT_DIM0 (and, for F16 /
 * BF16, optionally SHIFTND_WEIGHTS_F32): "the tensors are dense in memory order N, S0, S1, S2, C; serve the call with the
 * channels-last frame kernels or refuse it".  The problem, `weights` and `grad_w` are those of SHIFTND_SHIFT_DIM0; only the layout
 * differs: the video tensor [N*T, C, H, W] in channels-last memory, seen as {ndim 2, sizes N, C, T, M = H*W} with strides
 * {T*M*C, 1, M*C, C}.  The flag is explicit, so a tensor that both layouts describe (S1 * S2 == 1 or C == 1) goes to the frame
 * kernels under it.
 *   shiftnd_forward, p->active == 0: frames_forward, the kernel and the bits of the call without this flag.
 *   shiftnd_forward, p->active == 1: the interpolating forward (shiftnd_last_kernel(): frames_active_forward, *_ragged for pixel rows
 *   -- C elements -- that are not whole 16-byte pieces or bases off the 16-byte grid).
 *   shiftnd_backward: grad_out, x and grad_x all dense channels-last, grad_w [C] in the weights' type, deterministic
 *   (frames_backward / frames_backward_ragged).  The x == NULL form is refused.
 *   shiftnd_backward_workspace_bytes: that kernel's plan, a function of the geometry alone; sizeof(double) for an empty problem.
 *   Served calls report SHIFTND_PATH_CL; an empty problem SHIFTND_PATH_EMPTY with grad_w zeroed.
 *   Accepted: ndim 2 or 3; F32, F64, F16, BF16; every padding mode; the whole window; element-aligned bases.  Bounds: those of the
 *   channels-last layout above (N, C and S1 * S2 below 2^31, S0 below 2^30, N * S0 below 2^31, N * S0 * ceil(S1 * S2 / 8) below
 *   2^31, the tensor below 2^46 bytes) and, for the backward's partial records, N * ceil(S1 * S2 / rows) below 2^31 and those
 *   records (24 bytes per group and channel) below 2^46 bytes, where rows >= 1 is the rows of a workgroup (at most 8 steps of
 *   max(1, 256 / ceil(C * elsize / 16)) rows).  The kernels stage nothing, so S0 has no further limit.
 *   Errors, before anything is launched: a quantized dtype SHIFTND_ERR_UNSUPPORTED_DTYPE (the workspace query answers 0); ndim 1,
 *   a cut window, any tensor that is not dense channels-last (segment-major and NCHW-dense included), a size beyond the bounds,
 *   the x == NULL form: SHIFTND_ERR_INVALID_ARGUMENT; a workspace below the plan: SHIFTND_ERR_WORKSPACE_TOO_SMALL.
 * Without SHIFTND_SHIFT_DIM0 the bit is an unknown dtype bit: SHIFTND_ERR_UNSUPPORTED_DTYPE.  Without the bit nothing changes.
 */
#define SHIFTND_FRAMES 0x400

/*
 * The temporal shift under a PER-CLIP table (a shift that a small net predicts from the clip itself: TIN's OffsetNet, arXiv
 * 2001.06499; per-clip temporal jitter).  OR-ed onto a float dtype TOGETHER WITH SHIFTND_SHIFT_DIM0 (and, for F16 / BF16, optionally
 * SHIFTND_WEIGHTS_F32): `weights` and `grad_w` are contiguous [N, C] arrays, ONE entry per clip and channel, N = sizes[0].  Clip n is
 * the SHIFTND_SHIFT_DIM0 problem {1, C, S0, S1, S2} on its own frames under row n of the table: out and grad_x carry the bits of
 * that call, and grad_w[n] is its grad_w -- the fp64 sum of clip n's products in a fixed order, narrowed once to the weights' type,
 * deterministic.  (0x800 is not assigned: it stays an unknown dtype bit.)
 *   Honoured by shiftnd_forward (both values of p->active), shiftnd_backward (full form) and shiftnd_backward_workspace_bytes,
 *   which answers the bytes it answers without the bit: the partial records are re-indexed, not multiplied.
 *   Accepted: the geometry, layout and limits of SHIFTND_SHIFT_DIM0 on segment-major tensors (memory order N, S0, C, S1, S2), and
 *   N * C below 2^31.  The same kernels serve the call -- the table's row stride is a run-time field of theirs -- so
 *   shiftnd_last_kernel() reports tshift_forward[_ragged] / tshift_backward[_ragged] and shiftnd_last_path() SHIFTND_PATH_PLANE.
 *   An empty problem: SHIFTND_PATH_EMPTY, with the N * C entries of grad_w zeroed.
 *   On shiftnd_forward_quantized with wq_dtype == SHIFTND_F32 the bit selects the quantized per-clip shift ("Quantized,
 *   interpolating ... under a per-clip table" above: I8 / U8 / I32 tensors, wq the fp32 [N, C] table, p->active 0 or 1).
 *   Errors, before anything is launched: a quantized dtype on shiftnd_forward / shiftnd_backward, the bit on
 *   shiftnd_forward_quantized with an integer table or on the pooled entry points, and
 *   the bit without SHIFTND_SHIFT_DIM0 (an unknown dtype bit): SHIFTND_ERR_UNSUPPORTED_DTYPE; together with SHIFTND_FRAMES, out == x
 *   (the in-place form), channels-last tensors, the x == NULL && grad_w == NULL form of shiftnd_backward, N * C of 2^31 or more,
 *   and whatever SHIFTND_SHIFT_DIM0 refuses: SHIFTND_ERR_INVALID_ARGUMENT.  The workspace query answers 0 for a refused problem.
 * Without the bit nothing changes.
 */
#define SHIFTND_PER_CLIP 0x1000

/*
 * The ONLINE temporal shift (the uni-directional TSM of arXiv 1811.08383, section 4.2): frames arrive one at a time and the channels
 * that shift are taken from a cached state of the previous frames.  OR-ed onto a dtype TOGETHER WITH SHIFTND_SHIFT_DIM0 (and, for
 * F16 / BF16, optionally SHIFTND_WEIGHTS_F32).  One call is one step on a frame batch [B, C, spatial...] of B independent streams:
 *   p->sizes = {B, C, D, spatial...} (ndim 2 or 3), the whole window, p->active == 0, padding mode 0 or 1 (neither is looked at
 *   further: the state's initial bytes ARE the padding -- zeros / the zero point for mode 0, the first frame for mode 1);
 *   `x` is the STATE, D slots of the frame's shape and strides, with the slot stride in the S0 place of x_strides; slot k holds
 *   frame t-1-k.  It is READ AND WRITTEN although the parameter is const-qualified;
 *   `out` is the FRAME, read and written; the S0 entry of out_strides is ignored;
 *   `weights` is the [C] table, in the kinds the in-place form takes: the tensor dtype, or fp32 under SHIFTND_WEIGHTS_F32
 *   (shiftnd_forward); wq_dtype with w_zero_point (shiftnd_forward_quantized, I8 / U8 / I32 tensors; x_zero_point is not used).
 * For every channel c with s = min(max(s_c, 0), D) > 0 (out[t] = x[t - s_c]: a positive entry reads the past):
 *     frame[:, c] <- slot[s-1][:, c];   slot[k][:, c] <- slot[k-1][:, c] for k = s-1 .. 1;   slot[0][:, c] <- the incoming frame[:, c]
 * A channel with s == 0 is neither read nor written, in the frame or in the state, and slots k >= s of a channel are never touched.
 * An entry outside [0, D] is clamped: the kernel cannot raise, validating the table is the caller's job.
 *   Served by csrc/shiftnd_stream.hip: a thread owns one naturally aligned power-of-two piece (at most 16 bytes: the widest that
 *   divides the plane's bytes, or the channel row's bytes, and both bases) at the same offset in the frame and in every slot of one
 *   stream, gathers the s + 1 pieces of its line into registers and stores them one place on.  No workspace, no allocation, no
 *   synchronisation.  shiftnd_last_kernel(): frames_stream for 16-byte pieces, frames_stream_ragged for narrower ones;
 *   shiftnd_last_path(): SHIFTND_PATH_PLANE for contiguous tensors, SHIFTND_PATH_CL for channels-last ones, SHIFTND_PATH_EMPTY for an
 *   empty frame or D == 0 (nothing moves).
 *   Accepted: frame and state both dense contiguous (memory order B, C, spatial) or both dense channels-last (B, spatial, C), slots
 *   one frame batch apart; a pair both layouts describe is served as contiguous; element-aligned bases; D <= 15 (the kernel keeps a
 *   line in 16 register slots).  Bounds: those of the in-place form with D in the place of S0.
 *   Errors, before anything is launched: SHIFTND_FRAMES or SHIFTND_PER_CLIP beside the bit, D > 15, a cut window, p->active == 1,
 *   padding mode 2..4 (periodic, reflect and symmetric padding look into the future), a layout that is neither dense form, frame
 *   and state in different layouts, a frame that overlaps the state, a size beyond the bounds, and shiftnd_backward:
 *   SHIFTND_ERR_INVALID_ARGUMENT.  shiftnd_backward_workspace_bytes answers 0.
 * Without SHIFTND_SHIFT_DIM0 the bit is an unknown dtype bit on every entry point: SHIFTND_ERR_UNSUPPORTED_DTYPE.  Without the bit
 * nothing changes.  (0x800 stays unassigned.)
 */
#define SHIFTND_STREAM 0x2000

/*
 * The temporal shift under a PER-CLIP table on CHANNELS-LAST tensors: SHIFTND_PER_CLIP's table on SHIFTND_FRAMES' layout, under a
 * bit of its own (SHIFTND_FRAMES | SHIFTND_PER_CLIP stays refused).  OR-ed onto a float dtype TOGETHER WITH SHIFTND_SHIFT_DIM0 (and,
 * for F16 / BF16, optionally SHIFTND_WEIGHTS_F32): the tensors are dense channels-last exactly as under SHIFTND_FRAMES (memory order
 * N, S0, S1, S2, C; strides {T*M*C, 1, M*C, C}), and `weights` / `grad_w` are contiguous [N, C] arrays, one row per clip, exactly
 * as under SHIFTND_PER_CLIP.  Clip n is the SHIFTND_SHIFT_DIM0 | SHIFTND_FRAMES problem {1, C, S0, S1, S2} on its own frames under
 * row n: out and grad_x carry the bits of that call, and grad_w[n] is the fp64 sum of clip n's products in a fixed order, narrowed
 * once to the weights' type, deterministic.
 *   shiftnd_forward, p->active == 0: frames_forward / frames_forward_ragged;  p->active == 1: frames_active_forward / *_ragged.
 *   shiftnd_backward, full form: frames_backward / *_ragged.  The same kernels as under SHIFTND_FRAMES -- the table's row stride is
 *   a run-time field of theirs, and a workgroup lies inside one clip, so it forms its row's base once.
 *   shiftnd_backward_workspace_bytes: the bytes it answers for the same geometry under SHIFTND_FRAMES (the partial records are
 *   re-indexed, not multiplied); sizeof(double) for an empty problem.
 *   Served calls report SHIFTND_PATH_CL; an empty problem SHIFTND_PATH_EMPTY, with the N * C entries of grad_w zeroed.
 *   Accepted: what SHIFTND_FRAMES accepts (ndim 2 or 3; F32, F64, F16, BF16; every padding mode; the whole window; element-aligned
 *   bases; its bounds), and N * C below 2^31.
 *   Errors, before anything is launched (the workspace query answers 0): a quantized dtype, the bit on shiftnd_forward_quantized or
 *   on the pooled entry points, and the bit without SHIFTND_SHIFT_DIM0 (an unknown dtype bit, on every entry point):
 *   SHIFTND_ERR_UNSUPPORTED_DTYPE; the bit beside SHIFTND_FRAMES, SHIFTND_PER_CLIP or SHIFTND_STREAM, out == x, ndim 1, a cut
 *   window, any tensor that is not dense channels-last, the x == NULL form of shiftnd_backward, N * C of 2^31 or more, a size
 *   beyond the bounds: SHIFTND_ERR_INVALID_ARGUMENT; a workspace below the plan: SHIFTND_ERR_WORKSPACE_TOO_SMALL.
 * Without the bit nothing changes.  (0x800 stays unassigned.)
 */
#define SHIFTND_CLIP_FRAMES 0x4000

/*
 * Temporal INTERLACING (the TIN layer, arXiv 2001.06499): the per-clip temporal shift followed by a per-clip, per-frame, per-channel
 * weight, in one kernel per pass.  OR-ed onto a float dtype TOGETHER WITH SHIFTND_SHIFT_DIM0 (and, for F16 / BF16, optionally
 * SHIFTND_WEIGHTS_F32).  With y = the SHIFTND_SHIFT_DIM0 | SHIFTND_PER_CLIP result under offsets[N, C] (out[t] = x[t - w]):
 *     out[n, t, c, :] = scale[n, t, c] * y[n, t, c, :]
 * and the gradients are that composition's: grad_x is the per-clip backward applied to scale * grad_out, grad_offsets[n, c] that
 * backward's table gradient, grad_scale[n, t, c] = sum over the plane of grad_out * y.
 *   The call signatures have no room for a second table, so under the flag `weights` points to ONE contiguous array: the N * C
 *   offsets [N, C] immediately followed by the N * S0 * C scales [N, S0, C], both of the weights' type (the tensor dtype; fp32 under
 *   SHIFTND_WEIGHTS_F32).  `grad_w` has the same layout and is fully overwritten.
 *   Numerics: F32 / F64 -- out and grad_x carry the bits of the composition: the scale is a multiply of its own, applied AFTER the
 *   lerp in the forward and to each loaded gradient frame BEFORE the lerp in the backward, no FMA contraction across it.  F16 / BF16 --
 *   widened to fp32, interpolated, scaled and rounded ONCE (the composition rounds twice).  Both gradient tables: products accumulated
 *   in fp64 in a fixed order, narrowed once to the weights' type, deterministic; y in grad_scale's sum is the unrounded compute-type
 *   value.  p->active == 0 keeps the sparse kernels' rule: out is the source plane times the scale, and the table gradient is formed
 *   as tshift_backward forms it.
 *   Honoured by shiftnd_forward (both values of p->active), shiftnd_backward (full form) and shiftnd_backward_workspace_bytes, which
 *   sizes both sets of partial records (per workgroup for the offsets, per wave and frame for the scales) as a function of the
 *   geometry alone; sizeof(double) for an empty problem.
 *   Accepted: the geometry, layout and limits of SHIFTND_PER_CLIP -- segment-major tensors (memory order N, S0, C, S1, S2), ndim 2 or
 *   3, the whole window, every padding mode, element-aligned bases, out of place -- and N * S0 * C below 2^31 (the scales' index).
 *   Served by csrc/shiftnd_interlace.hip without a fallback: shiftnd_last_kernel() reports tinterlace_forward / tinterlace_backward
 *   (*_ragged for planes that are not whole 16-byte pieces or bases off the 16-byte grid), shiftnd_last_path() SHIFTND_PATH_PLANE.  An
 *   empty problem: SHIFTND_PATH_EMPTY, with the N * C + N * S0 * C entries of grad_w zeroed.
 *   On shiftnd_forward_quantized with wq_dtype == SHIFTND_F32 the bit selects quantized temporal interlacing ("Quantized,
 *   interpolating ... interlaced" above: I8 / U8 / I32 tensors, wq the packed fp32 table, p->active 0 or 1, no workspace).
 *   Errors, before anything is launched (the workspace query answers 0): a quantized dtype on shiftnd_forward / shiftnd_backward, the
 *   bit on shiftnd_forward_quantized with an integer table or
 *   on the pooled entry points, and the bit without SHIFTND_SHIFT_DIM0 (an unknown dtype bit, on every entry point):
 *   SHIFTND_ERR_UNSUPPORTED_DTYPE; the bit beside SHIFTND_FRAMES, SHIFTND_PER_CLIP, SHIFTND_STREAM or SHIFTND_CLIP_FRAMES, out == x,
 *   channels-last tensors, ndim 1, a cut window, the x == NULL form of shiftnd_backward, a size beyond the bounds:
 *   SHIFTND_ERR_INVALID_ARGUMENT; a workspace below the plan: SHIFTND_ERR_WORKSPACE_TOO_SMALL.
 * Without the bit nothing changes.  (0x800 stays unassigned.)
 */
#define SHIFTND_INTERLACE 0x8000

/*
 * Temporal interlacing on CHANNELS-LAST tensors: SHIFTND_INTERLACE's problem and packed table on SHIFTND_FRAMES' layout, under a bit
 * of its own (SHIFTND_INTERLACE on channels-last strides, and beside any other bit of the family, stays refused).  OR-ed onto a
 * float dtype TOGETHER WITH SHIFTND_SHIFT_DIM0 (and, for F16 / BF16, optionally SHIFTND_WEIGHTS_F32): the tensors are dense
 * channels-last exactly as under SHIFTND_FRAMES (memory order N, S0, S1, S2, C; strides {T*M*C, 1, M*C, C}), and `weights` /
 * `grad_w` are the ONE packed array of SHIFTND_INTERLACE: the N * C offsets [N, C] immediately followed by the N * S0 * C scales
 * [N, S0, C].  Values and numerics are SHIFTND_INTERLACE's: out and grad_x carry the bits of that call on contiguous copies of the
 * same data, in every dtype; both gradient tables are fp64 sums in a fixed order, narrowed once, deterministic.
 *   shiftnd_forward, both values of p->active: frames_interlace_forward / *_ragged (pieces of a pixel's channel row under 16 bytes).
 *   shiftnd_backward, full form: frames_interlace_backward / *_ragged.  S0 is not bounded: nothing in the kernels is sized by it.
 *   shiftnd_backward_workspace_bytes, a function of the geometry alone: with M = S1 * S2 pixels a frame, es the element size,
 *       pieces = ceil(C * es / 16),  rps = pieces < 256 ? 256 / pieces : 1   (integer division),
 *       steps  = 8, halved while steps > 1 and N * ceil(M / (rps * steps)) < 768,
 *       chunks = ceil(M / (rps * steps)),
 *   it answers chunks * N * C * (1 + S0) * 8 bytes: one double per workgroup and offset, and per workgroup, frame and scale;
 *   sizeof(double) for an empty problem.
 *   Served calls report SHIFTND_PATH_CL; an empty problem SHIFTND_PATH_EMPTY, with the N * C + N * S0 * C entries of grad_w zeroed.
 *   Accepted: what SHIFTND_FRAMES accepts (ndim 2 or 3; F32, F64, F16, BF16; every padding mode; the whole window; element-aligned
 *   bases; its bounds), N * S0 * C below 2^31 (the scales' index), N * chunks below 2^31 and the records below 2^46 bytes.
 *   Errors, before anything is launched (the workspace query answers 0): a quantized dtype, the bit on shiftnd_forward_quantized or
 *   on the pooled entry points, and the bit without SHIFTND_SHIFT_DIM0 (an unknown dtype bit, on every entry point):
 *   SHIFTND_ERR_UNSUPPORTED_DTYPE; the bit beside SHIFTND_FRAMES, SHIFTND_PER_CLIP, SHIFTND_STREAM, SHIFTND_CLIP_FRAMES or
 *   SHIFTND_INTERLACE, out == x, ndim 1, a cut window, any tensor that is not dense channels-last (segment-major strides), the
 *   x == NULL form of shiftnd_backward, N * S0 * C of 2^31 or more, a size beyond the bounds: SHIFTND_ERR_INVALID_ARGUMENT; a
 *   workspace below the plan: SHIFTND_ERR_WORKSPACE_TOO_SMALL.
 * Without the bit nothing changes.  (0x800 stays unassigned.)
 */
#define SHIFTND_INTERLACE_FRAMES 0x10000

typedef enum shiftnd_status {
    SHIFTND_OK = 0,
    SHIFTND_ERR_INVALID_ARGUMENT = -1,
    SHIFTND_ERR_UNSUPPORTED_DTYPE = -2,
    SHIFTND_ERR_WORKSPACE_TOO_SMALL = -3,
    SHIFTND_ERR_LAUNCH_FAILED = -4,
    SHIFTND_ERR_TOO_LARGE = -5,
    SHIFTND_ERR_NOT_FUSED = -6 /* pooled entry points: geometry not served; run shift and pool separately */
} shiftnd_status;

/* Which kernel family served the last call made on this host thread (for tests/benchmarks). */
typedef enum shiftnd_path {
    SHIFTND_PATH_NONE = 0,
    SHIFTND_PATH_EMPTY = 1,   /* zero-element problem: nothing launched */
    SHIFTND_PATH_PLANE = 2,   /* per-(N,C)-plane kernels, LDS index maps, 16-byte rows */
    SHIFTND_PATH_STRIDED = 3, /* generic strided fallback (channels-last, ragged rows, huge dims) */
    SHIFTND_PATH_SWEEP = 4,   /* one 16-byte chunk per thread, XCD-contiguous sweep (the HBM-rate path) */
    SHIFTND_PATH_CL = 5       /* channels-last input: lanes = consecutive channels of a pixel */
} shiftnd_path;

/* Problem geometry shared by the entry points. */
typedef struct shiftnd_problem {
    int32_t ndim;          /* spatial dims: 1, 2 or 3 */
    int32_t dtype;         /* shiftnd_dtype of input/output (and of float weights), optionally | SHIFTND_WEIGHTS_F32 | SHIFTND_SHIFT_DIM0 | SHIFTND_FRAMES | SHIFTND_PER_CLIP | SHIFTND_STREAM | SHIFTND_CLIP_FRAMES | SHIFTND_INTERLACE | SHIFTND_INTERLACE_FRAMES */
    int32_t padding_mode;  /* 0..4 */
    int32_t active;        /* 0: sparse shift (rounded integer shift); 1: active (interpolated) */
    int64_t sizes[5];      /* input N, C, H, W, D */
    int32_t borders[6];    /* l_i, r_i, l_j, r_j, l_k, r_k (unused dims: 0, 1) */
} shiftnd_problem;

SHIFTND_API int shiftnd_abi_version(void);
SHIFTND_API const char *shiftnd_status_string(int status);
SHIFTND_API int shiftnd_last_path(void);
/* Diagnostics: name (without template arguments) of the main kernel the last call on this thread launched. */
SHIFTND_API const char *shiftnd_last_kernel(void);
/* 0 = automatic (sweep, else plane, else channels-last, else strided), 1 = force the strided fallback,
 * 2 = plane kernels or fail, 3 = sweep kernels or fail, 4 = channels-last kernels or fail (testing).
 * THREAD-LOCAL like shiftnd_last_path: the policy and the tuning knobs below apply to calls made on the calling
 * thread only, so a diagnostic setter can never re-route a concurrent caller (dispatcher threads, autograd
 * worker threads always run with the defaults). */
SHIFTND_API void shiftnd_set_path_policy(int policy);
/* Diagnostics: launch-planning knobs, by kernel family (csrc/shiftnd_api.hip routes them).  0-7 plane kernels
 * (0: minimum workgroups wanted, 1: target bytes per workgroup, 2: gather-forward unroll, 3: backward form, 5: affine
 * LDS reads, 6: XCD-contiguous block ids), 8-11 sweep kernels (9 / 11: max threads; the row steps per workgroup 8 / 10 once
 * chose are fixed), 12-15 sliding-window kernels (12: which problems take
 * them, 13: workgroups wanted, 14: minimum rows per band), 16-19 one-byte small-plane kernel (16: on / off, 17: planes
 * per round, 18: LDS bytes, 19: rounds per workgroup), 20-22 LDS-tiled channels-last kernels (20: on / off, 21: rows
 * per band, 22: XCD-contiguous block ids; 23: the direct NDHWC backward 0 = automatic, 1 = never, 2 = whenever eligible), 24-26 small-plane / row-band kernels (24: on / off, 25: planes per round or rows per band, 26: rounds per
 * workgroup), 27 flat-stream kernels for ragged rows (0 = automatic, 1 = never, 2 = whenever eligible), 28-30 one-byte row kernel (28: element sizes served, 29: rows per band, 30: workgroups wanted), 32-35
 * one-step kernels (32: 2-D backward, 33: sparse-shift forward by direct loads, 34: forwards through LDS; each 0 =
 * automatic, 1 = never, 2 = whenever eligible; 33 also: 3 = the 16-bit pooled gather forward off, 4 = the interpolating one off;
 * 35: bit set of opt-in forms, csrc/shiftnd_step.hip; round 6: bit 6 = the band-walk kernel for the cropped / interpolating 2-D pooled
 * backward, bit 7 = one row group per thread in crop_backward's sparse forms, bit 8 = two everywhere, bit 10 = the per-channel
 * kernels for cropped 3-D volumes and 2-D windows whose planes are not whole pieces, bit 11 = crop_backward3 / crop_forward3 instead of
 * the walk kernels with the window inside), 36-37 quantized
 * pool (36: 1 = the element-per-thread kernel only, 2 = the plane kernel first, 3 = the band kernel first; 37: workgroups wanted), 38 planes per workgroup of the 3-D walk
 * kernels; for the sizing knobs 0 means automatic.
 * Results never depend on them.
 * shiftnd_backward_workspace_bytes (and the pooled form) returns the larger of the default knobs' plan and the calling
 * thread's: a backward whose own plan needs more than it was given runs the default plan instead, so sizing on one
 * thread and running on another never ends in SHIFTND_ERR_WORKSPACE_TOO_SMALL. */
SHIFTND_API void shiftnd_set_tuning(int knob, int value);
/* Diagnostics: the sweep kernels' arithmetic padding map evaluated on the host: source index of
 * coordinate p (0 <= p <= len) under `shift`, or -1 for "fill". */
SHIFTND_API int shiftnd_debug_map(int64_t p, int64_t shift, int64_t len, int padding_mode);

/*
 * Host helper: the reference's check_borders (shifts.cpp:93-135).
 * sizes/nsizes: full tensor shape; user: ndim x 2 cut amounts (left, right) or NULL for no crop.
 * Writes borders[6] and new_sizes[nsizes].
 */
SHIFTND_API int shiftnd_check_borders(const int64_t *sizes, int nsizes, const int32_t *user, int ndim,
                          int32_t borders[6], int64_t *new_sizes);

/*
 * 1 when shiftnd_forward would serve this call with a kernel made for a dense channels-last INPUT (x_strides) and the
 * given output layout (channels-last or NCHW-contiguous) -- the caller then need not change the input's layout first
 * (the torch operator library transposes channels-last inputs otherwise); 0 for every other call.
 */
SHIFTND_API int shiftnd_forward_serves_channels_last(const shiftnd_problem *p, const void *x, const int64_t x_strides[5],
                                                     const void *out, const int64_t out_strides[5]);

/*
 * The same question for shiftnd_backward: 1 when the saved input, the incoming gradient and grad_x, all dense
 * channels-last as their strides say, are served by a kernel made for that layout (no layout change needed).
 */
SHIFTND_API int shiftnd_backward_serves_channels_last(const shiftnd_problem *p, const void *grad_out,
                                                      const int64_t grad_out_strides[5], const void *x,
                                                      const int64_t x_strides[5], const void *grad_x,
                                                      const int64_t grad_x_strides[5]);

/*
 * Forward, float dtypes (F32, F64, F16, BF16; F16 / BF16 also with SHIFTND_WEIGHTS_F32).
 * out has sizes {N, C, r_i-l_i, r_j-l_j, r_k-l_k}; out_strides are its element strides.
 *
 * Segment-major tensors: x and out in memory order N, S0, C, S1, S2 -- the first spatial dim OUTSIDE the channel dim, i.e. dense
 * strides {S0*C*inner, inner, C*inner, [S2,] 1} with inner = the product of the spatial sizes after the first.  That is a video
 * tensor [N*T, C, H, W] seen as the problem {ndim 2, sizes N, C, T, H*W} with strides {T*C*M, M, C*M, 1}: a shift of column 0 moves
 * channels across the T frames of a clip (the Temporal Shift Module).  A sparse shift (active == 0) of float tensors in this layout,
 * whole window, ndim >= 2, C > 1, S0 > 1, same layout on both sides, under 2^32 bytes, is served at copy rate by the kernels of
 * csrc/shiftnd_segment.hip (shiftnd_last_kernel: segment_forward for planes of whole 16-byte pieces at 16-byte-aligned bases,
 * segment_forward_ragged otherwise; SHIFTND_PATH_PLANE), for any [C, ndim] table -- planes whose channel also shifts an inner dim are
 * gathered element by element inside the same kernel.  So is shiftnd_backward's x == NULL form on such strides (whole window).  Every
 * other call with these strides keeps the strided kernels.
 *
 * shiftnd_forward_quantized takes the same route under the same conditions: I8 / U8 / I32 tensors with an I8 / U8 / I32 table, the
 * shift of a row its entries minus w_zero_point, a filled plane the input's zero point.  One-byte elements are streamed in units of
 * one byte (planes of an odd number of bytes, bases on any byte; a one-byte tensor of 2^31 - 16 bytes or more keeps the strided
 * kernel), and the kernel names and the path are those above.  Tensors the channel-fastest kernels take first (inner == 1: memory
 * order N, S0, C is channels-last) stay with them, as for floats.
 */
SHIFTND_API int shiftnd_forward(const shiftnd_problem *p,
                    const void *x, const int64_t x_strides[5],
                    const void *weights,
                    void *out, const int64_t out_strides[5],
                    void *stream);

/*
 * Backward, float dtypes.  grad_out has the forward output's sizes; grad_x the input's sizes;
 * grad_w is a contiguous [C, ndim] array of the weights' dtype (the tensor dtype; fp32 with SHIFTND_WEIGHTS_F32) and is fully
 * overwritten.
 * workspace: device scratch of at least shiftnd_backward_workspace_bytes(p) bytes
 * (fp64 partial sums of the weight gradient); its contents need not be initialised.
 *
 * Input gradient only (fixed / frozen shifts): x == NULL and grad_w == NULL together, p->active == 0.  Nothing of the
 * input is read and no weight gradient is formed; grad_x is bit for bit what the full call writes:
 *   grad_x[n,c,i,j,k] = inside the window ? grad_out[n,c, pad(i-l_i+s_i), pad(j-l_j+s_j), pad(k-l_k+s_k)] : 0,  s = rint(w).
 * x_strides is ignored (may be NULL).  Workspace of this form:
 *   - window == whole input (no cut): C * ndim * sizeof(element) bytes, 8-byte aligned -- the negated shift table, on
 *     which the forward kernels run (grad_x = sparse forward of grad_out under -w); fewer bytes, or a NULL workspace,
 *     return SHIFTND_ERR_WORKSPACE_TOO_SMALL before anything is launched;
 *   - cut window: none, workspace may be NULL with workspace_bytes == 0.
 * shiftnd_backward_workspace_bytes(p) covers both (it stays the upper bound of every form).
 * p->active == 1 with this form, or only one of x / grad_w NULL, is SHIFTND_ERR_INVALID_ARGUMENT; nothing is launched.
 */
SHIFTND_API size_t shiftnd_backward_workspace_bytes(const shiftnd_problem *p);

SHIFTND_API int shiftnd_backward(const shiftnd_problem *p,
                     const void *grad_out, const int64_t grad_out_strides[5],
                     const void *x, const int64_t x_strides[5],
                     const void *weights,
                     void *grad_x, const int64_t grad_x_strides[5],
                     void *grad_w,
                     void *workspace, size_t workspace_bytes,
                     void *stream);

/*
 * Quantized forward (dtype I8, U8 or I32 = int_repr of the quantized input; p->active ignored).
 * wq: device pointer to the contiguous [C, ndim] int_repr of the quantized weights, of type
 * wq_dtype (I8, U8 or I32); shift = wq - w_zero_point; scale is ignored
 * (kernels/shifts_kernels.h:553-555).  x_zero_point is the fill value (:569).
 */
SHIFTND_API int shiftnd_forward_quantized(const shiftnd_problem *p,
                              const void *x, const int64_t x_strides[5],
                              const void *wq, int32_t wq_dtype, int64_t w_zero_point,
                              int64_t x_zero_point,
                              void *out, const int64_t out_strides[5],
                              void *stream);

/*
 * Fused shift + average pool.  The reference's modules follow the shift with
 * avg_pool{N}d(kernel_size = stride = pool, ceil_mode=True) when they emulate a strided depthwise conv
 * (torchshifts/modules/shifts.py:81-89, 150-153); these entry points produce the same result without
 * writing / re-reading the full-size shift output.
 *   pool:   p->ndim ints, window (= stride) per spatial dim (H, W, D), each >= 1.
 *   Tensors are contiguous N, C, spatial: x and grad_x have the input's sizes, out / grad_pooled have spatial
 *   sizes ceil((r - l) / pool).  shiftnd_pooled_sizes writes them.
 *   Numerics: the window is summed in ATen's order in fp32 (fp64 for fp64) and divided by the number of window
 *   elements inside the shift output; fp32 / fp64 results are bit-identical to the two-step sequence.
 *   workspace: at least shiftnd_backward_pooled_workspace_bytes(p, pool) bytes (the pooled launch plan can need more
 *   partial-sum groups than the plain backward of the same tensor).
 * Return SHIFTND_ERR_NOT_FUSED when the geometry is not served (the caller then runs shift and pool
 * separately); nothing has been launched in that case.
 *
 * shiftnd_backward_pooled, input gradient only (fixed / frozen shifts with a stride): x == NULL and grad_w == NULL together,
 * p->active == 0 -- the convention of shiftnd_backward.  Nothing of the input is read and no weight gradient is formed:
 *   grad_x[n,c,i,j,k] = inside the window ? grad_pooled[n,c, t_i / K_i, t_j / K_j, t_k / K_k] / cnt : 0
 *   t_d = pad(o_d + s_d) in [0, O_d),  o_d = i_d - l_d,  s = rint(w),  O_d = r_d - l_d,  K = pool
 *   cnt = prod_d min(K_d, O_d - (t_d / K_d) * K_d)        (ceil_mode: the last window of a dim may be partial)
 * the sparse shift's grad_x applied to ATen's average-pool backward: a gather of grad_pooled with one division, in fp32 for
 * fp16 / bf16 tensors and fp64 for fp64, rounded once to the tensor type -- bit for bit the grad_x of the full form for a
 * sparse shift, and of the two-step sequence.  No workspace: workspace may be NULL with workspace_bytes == 0.  This form never
 * returns SHIFTND_ERR_NOT_FUSED (the element-wide kernel serves every geometry).  p->active == 1 with this form, or only one of
 * x / grad_w NULL, is SHIFTND_ERR_INVALID_ARGUMENT; nothing is launched.
 */
SHIFTND_API int shiftnd_pooled_sizes(const shiftnd_problem *p, const int32_t *pool, int64_t pooled_spatial[3]);

SHIFTND_API size_t shiftnd_backward_pooled_workspace_bytes(const shiftnd_problem *p, const int32_t *pool);

SHIFTND_API int shiftnd_forward_pooled(const shiftnd_problem *p, const int32_t *pool,
                           const void *x, const void *weights, void *out, void *stream);

SHIFTND_API int shiftnd_backward_pooled(const shiftnd_problem *p, const int32_t *pool,
                            const void *grad_pooled, const void *x, const void *weights,
                            void *grad_x, void *grad_w,
                            void *workspace, size_t workspace_bytes, void *stream);

#define SHIFTND_REQUANT_ZP_INSIDE 0
#define SHIFTND_REQUANT_ZP_OUTSIDE 1

/*
 * ABI 5: the same tail for the quantized forward (torchshifts/quantized/modules/shifts.py:19-20: a quantized module that
 * emulates a strided depthwise conv returns _reduction_fn(shift(x))): out = avg_pool(qshift(x)) in one pass, contiguous
 * int8 / uint8 tensors (p->dtype), quantized weights as in shiftnd_forward_quantized.  Requantization is ATen's
 * QuantizedCPU average pool in fp32 on acc = sum(x_int - x_zero_point) over the window, clamped to the type's range; scale
 * and zero point of the result are the input's.  ATen itself rounds in two ways and `requant` names the one wanted:
 *   SHIFTND_REQUANT_ZP_INSIDE   nearbyint(x_zero_point + acc * (1 / count))  -- its kernel for contiguous 1-D / 2-D tensors
 *                               (quantize_val -> fbgemm::Quantize: the zero point is added before the rounding)
 *   SHIFTND_REQUANT_ZP_OUTSIDE  nearbyint(acc * (1 / count)) + x_zero_point  -- its channels-last kernel, which also serves
 *                               every 3-D tensor and any [N, C, H, W] tensor whose shift output is channels-last-contiguous
 *                               too (C == 1 or H == W == 1)
 * (they differ when the zero point is odd and the window mean is a tie).  The torch operator library picks the form ATen
 * would use for the reference's shift output (torch_binding.cpp: qpool_zp_outside).  SHIFTND_ERR_NOT_FUSED for other element types (nothing launched).
 */
SHIFTND_API int shiftnd_forward_quantized_pooled(const shiftnd_problem *p, const int32_t *pool, const void *x, const void *wq,
                                     int32_t wq_dtype, int64_t w_zero_point, int64_t x_zero_point, int32_t requant, void *out,
                                     void *stream);

/*
 * Layout change between channels-last and contiguous tensors: dst[b][c][r] = src[b][r][c] for dense
 * src[batch][rows][cols] and dst[batch][cols][rows] of element_bytes-byte (1, 2, 4, 8) elements.
 * Channels-last [N, H, W, C] -> contiguous [N, C, H, W]: rows = H*W, cols = C; the reverse: rows = C, cols = H*W.
 * The reference's float ops return an NCHW-contiguous tensor even for a channels-last input
 * (cpu/shifts_cpu.cpp:221) and its CUDA backend walks such an input through its strides; host glue that meets a
 * channels-last tensor changes the layout with this call (a tile transpose at copy bandwidth) and runs the
 * contiguous kernels, which is several times faster than any kernel that touches both layouts at once.
 */
SHIFTND_API int shiftnd_transpose(const void *src, void *dst, int64_t batch, int64_t rows, int64_t cols,
                      int32_t element_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SHIFTND_HIP_H_ */
