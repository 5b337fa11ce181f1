// promote.hip -- the reference's per-key accumulation step when clients disagree on a key's dtype.
//
// The reference's FedAvg loop (python/fedml/ml/aggregator/agg_operator.py:37-44) is, per key,
//   avg = x_0 * w_0;   avg += x_i * w_i  (i = 1..K-1)
// and its plain-sum branch (:55-63) avg = x_0; avg += x_i.  When client i's tensor has another
// dtype than avg, `avg += t` is PyTorch's in-place add across dtypes: both operands are cast to the
// promoted type C = promote_types(avg, t), added in C (C's op-math: float for bf16/f16/f32,
// double for f64), and the sum is cast back to avg's dtype.  The casts are c10's: int64 -> float
// types and f64 -> bf16/f16 go THROUGH float32 (two roundings), which tests/golden/g19_* (made by
// the reference itself) pin.  The terms t_i = x_i * w_i are the engine's ordinary K = 1 weighted
// sums (same kernels, same bits as the reference's `x * w` in x's dtype); this kernel is only the
// cross-dtype `avg += t`, one element per lane, HBM-bound (read avg and t, write avg).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "elem.h"
#include "fa_internal.h"

using namespace fa_detail;

namespace {

// element e of a tensor of dtype DT, widened exactly (float for f32/bf16/f16, double for f64, int64
// as is)
template <int DT>
__device__ __forceinline__ typename El<DT>::A ld(const void* p, int64_t e) {
  return El<DT>::from_bits(((const typename El<DT>::S*)p)[e]);
}

// PyTorch's promote_types for the pairs that reach this kernel (acc a float dtype)
template <int A, int B>
constexpr int promoted() {
  if (B == FA_DTYPE_I64 || A == B) return A;
  if (A == FA_DTYPE_F64 || B == FA_DTYPE_F64) return FA_DTYPE_F64;
  return FA_DTYPE_F32;  // f32 with anything below it, and bf16 with f16
}

// x itself; before a rounding to bf16 pinned as an f32 in a register (elem.h: pin_f32, which the f16
// rounding there applies itself): without the pin hipcc compiles this kernel's bf16 forms to another,
// four times longer instruction stream
template <int C, class X>
__device__ __forceinline__ X pinned(X x) {
  if constexpr (C == FA_DTYPE_BF16) return pin_f32(x);
  else return x;
}

// c10 cast of an exactly-widened value to dtype C (returned in C's op-math type): to double float ->
// double is exact and int64 correctly rounded; to the float types THROUGH float32 (float types exact,
// int64 correctly rounded; no f64 here), then rounded once to C
template <int C, class V>
__device__ __forceinline__ typename El<C>::A to_common(V v) {
  return El<C>::rnd(pinned<C>((typename El<C>::A)v));
}

// C's add, rounded to C
template <int C, class V>
__device__ __forceinline__ V add_in(V a, V b) {
  return El<C>::rnd(pinned<C>(op_add(a, b)));
}

// c10 cast of a C value to the accumulator dtype A (double -> float rounds first), stored
template <int A, class V>
__device__ __forceinline__ void store(void* p, int64_t e, V v) {
  ((typename El<A>::S*)p)[e] = El<A>::bits(pinned<A>((typename El<A>::A)v));
}

template <int A, int B>
__global__ void __launch_bounds__(kBlock) k_promote_add(const void* __restrict__ acc, const void* __restrict__ t,
                                                        void* out, int64_t n) {
  constexpr int C = promoted<A, B>();
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += stride) {
    const auto a = to_common<C>(ld<A>(acc, e));
    const auto b = to_common<C>(ld<B>(t, e));
    store<A>(out, e, add_in<C>(a, b));
  }
}

template <int A, int B>
void launch(const void* acc, const void* t, void* out, int64_t n, hipStream_t st) {
  const int64_t blocks = std::min<int64_t>((n + kBlock - 1) / kBlock, 65536);
  hipLaunchKernelGGL((k_promote_add<A, B>), dim3((unsigned)blocks), dim3(kBlock), 0, st, acc, t, out, n);
}

template <int A>
int dispatch_t(int t_dtype, const void* acc, const void* t, void* out, int64_t n, hipStream_t st) {
  switch (t_dtype) {
    case FA_DTYPE_F32: launch<A, FA_DTYPE_F32>(acc, t, out, n, st); return FA_OK;
    case FA_DTYPE_BF16: launch<A, FA_DTYPE_BF16>(acc, t, out, n, st); return FA_OK;
    case FA_DTYPE_F16: launch<A, FA_DTYPE_F16>(acc, t, out, n, st); return FA_OK;
    case FA_DTYPE_F64: launch<A, FA_DTYPE_F64>(acc, t, out, n, st); return FA_OK;
    case FA_DTYPE_I64: launch<A, FA_DTYPE_I64>(acc, t, out, n, st); return FA_OK;
    default: return fail(FA_ERR_DTYPE, "fa_promote_add: term dtype %d not supported", t_dtype);
  }
}

}  // namespace

extern "C" int fa_promote_add(fa_ctx* ctx, int acc_dtype, int t_dtype, int64_t n, const void* d_acc,
                              const void* d_t, void* d_out, void* hip_stream) {
  if (!ctx || n < 0 || (n > 0 && (!d_acc || !d_t || !d_out)))
    return fail(FA_ERR_INVALID, "fa_promote_add: invalid arguments");
  if (n == 0) return FA_OK;
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FA_ERR_HIP, "fa_promote_add: hipSetDevice(%d) failed", ctx->device);
  hipStream_t st = (hipStream_t)hip_stream;
  int rc;
  switch (acc_dtype) {
    case FA_DTYPE_F32: rc = dispatch_t<FA_DTYPE_F32>(t_dtype, d_acc, d_t, d_out, n, st); break;
    case FA_DTYPE_BF16: rc = dispatch_t<FA_DTYPE_BF16>(t_dtype, d_acc, d_t, d_out, n, st); break;
    case FA_DTYPE_F16: rc = dispatch_t<FA_DTYPE_F16>(t_dtype, d_acc, d_t, d_out, n, st); break;
    case FA_DTYPE_F64: rc = dispatch_t<FA_DTYPE_F64>(t_dtype, d_acc, d_t, d_out, n, st); break;
    default: return fail(FA_ERR_DTYPE, "fa_promote_add: accumulator dtype %d must be a float type", acc_dtype);
  }
  if (rc != FA_OK) return rc;
  FA_HIP(hipGetLastError());
  return FA_OK;
}
