// What the conv3 translation units use of one another on the host (conv3_fwd.hip, conv3_big.hip,
// conv3_b16.hip, conv3_wgrad.hip): the big-box forward of conv3_big.hip and its two switches.
#pragma once
#include <hip/hip_runtime.h>

// most input channels of the BNIN forms (the input's BatchNorm scale / shift table in LDS)
constexpr int kBgBnMax = 128;

// conv3_big.hip (hidden: the library exports its extern "C" pcms_ names only)
#pragma GCC visibility push(hidden)
bool big_fwd_ok(int dtype, int N, int D, int H, int W, int c0, int c1);
int big_slots(int N, int D, int H, int W, int Cout);
// launches conv3_fwd_big_kernel for a big_fwd_ok conv; p: a Conv3Params filled by conv3_fwd_any
// (untyped: conv_common.h gives every unit its own Conv3Params in an anonymous namespace)
int big_fwd_launch(const void* p, hipStream_t s);
int big_min_boxes();  // pcms_conv3_big_min_boxes' value
int big_max_wgs();    // pcms_conv3_big_max_wgs' value
#pragma GCC visibility pop
