// Launch plans of the 1x1 convolution family that cidnet_pw_plan (pw.hip) reports from other translation units: each is
// computed by the functions the launcher of that file calls.  Both write their fields to out[] and return CIDNET_OK, or
// CIDNET_ERR_SHAPE (nothing written) where the *_supported predicate of the path refuses the shape.
#pragma once

namespace cidnet {

// pwx.hip, cidnet_pw_conv_bf16x3_pre_t: cpg, KB, MT, WM, chunks, MTW, tiles_per_sample
int pwx_plan_fields(int M, int K, long HW, int* out);
// pwb.hip, cidnet_pw_bwd_fused: MT, NT, 32-pixel chunks per sample, blocks, most chunks of one block
int pwb_plan_fields(int B, int M, int N, long HW, int* out);

}  // namespace cidnet
