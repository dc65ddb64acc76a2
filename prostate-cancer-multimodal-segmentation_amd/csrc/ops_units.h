// What the ops translation units share (ops_layout.hip, ops_bn.hip, ops_pool.hip, ops_head.hip,
// ops_update.hip, losses.hip): the block size, the capped grid of every grid-stride launch, the storage /
// cache-policy dispatch of their launch sites, the BatchNorm-backward element and the two host
// launchers of kernels that a second family uses.
#pragma once
#include "common.h"
#include <algorithm>
#include <type_traits>

constexpr int TPB = 256;

// hidden: the library exports its extern "C" pcms_ names only
#pragma GCC visibility push(hidden)
// ops_bn.hip: pcms_stream_grid_cap's value (default INT_MAX: no extra cap) and
// pcms_bn_bwd_rows_cap's (the partial-row cap of the BN-backward reduce passes, the pool one too)
extern int g_stream_grid_cap;
extern int g_bn_rows_cap;
// ops_bn.hip: the two-stage BatchNorm-backward finalize (colsum2_kernel, bn_bwd_finalize_kernel)
// of `rows` partial rows [C][2] -> dgamma / dbeta (+=) and the apply coefficients; ws:
// pcms_bn_ws_doubles(C)
int bn_bwd_finalize2_launch(const float* part, int rows, int C, double count, const float* gamma,
                            const float* invstd, float* dgamma, float* dbeta, float* coef, double* ws, hipStream_t s);
// ops_layout.hip: rows_sum_kernel, out[c] (+= when acc) the sum of part[rows][C] in row order
int rows_sum_launch(bool acc, const float* part, int rows, int C, float* out, hipStream_t s);
#pragma GCC visibility pop

// Every grid-stride launch and every row-count / workspace query of these units caps its grid
// at min(the site's cap, pcms_stream_grid_cap) -- the default leaves every site at its own cap;
// a small value makes a test-sized input take the many-trips-per-thread paths of the kernels
// (their unrolled main loops, wraps across samples).
static inline int stream_grid(long work, int per_block, int cap = 8192) {
  return grid_for(work, per_block, std::min(cap, g_stream_grid_cap));
}

// Launch-site dispatch.  Storage: f(bf16_t{}) for PCMS_BF16, f(float{}) for any other dtype.
// Policy: a kernel's bool template argument from a run-time flag -- f(std::true_type{}) for the
// non-temporal form (most sites), f(std::false_type{}) for the cached one.  for_stream: both,
// f(T{}, NT{}).  A site instantiates every form its lambda can name, launched or not.
template <typename F> static int for_storage(int dtype, F&& f) { return dtype == PCMS_BF16 ? f(bf16_t{}) : f(float{}); }
template <typename F> static int for_policy(bool nt, F&& f) { return nt ? f(std::true_type{}) : f(std::false_type{}); }
template <typename F> static int for_stream(int dtype, bool nt, F&& f) {
  return for_storage(dtype, [&](auto t) { return for_policy(nt, [&](auto p) { return f(t, p); }); });
}
// elements per 16-byte vector / bytes per element of a dtype's storage
static inline int vec_of(int dtype) { return dtype == PCMS_BF16 ? 8 : 4; }
static inline int bytes_of(int dtype) { return dtype == PCMS_BF16 ? 2 : 4; }

// BatchNorm + ReLU backward of one element, dy = k1 g + k2 xhat + k3 with g = da [y sc + sh > 0]:
// the operations written out (fma(y, sc, sh) for the mask, fma(k2, xhat, k1 g) + k3) so that
// every kernel applying it rounds the same way -- the compiler's own contraction of the plain
// expression picked fma(k1, g, k2 xhat) in one kernel and fma(k2, xhat, k1 g) in another
__device__ __forceinline__ float bn_bwd_dy(float da, float y, float sc, float sh, float mu, float is, float k1,
                                           float k2, float k3) {
#pragma clang fp contract(off)
  const float g = __builtin_fmaf(y, sc, sh) > 0.f ? da : 0.f;
  const float xhat = (y - mu) * is;
  return __builtin_fmaf(k2, xhat, k1 * g) + k3;
}
