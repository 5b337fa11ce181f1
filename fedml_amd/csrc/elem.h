// elem.h -- the one device copy of the element arithmetic and the storage-type conversions, shared by
// every kernel family whose results must agree to the bit (fedagg.hip, wsum_dist.hip, signvote.hip, fedopt_adaptive.hip, promote.hip,
// median_common.h, trimmed.hip).  It works on bits and values only: each family keeps its own loads
// and stores (generic or global address space, temporal or not), which differ on purpose.  Not part
// of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include "fa_internal.h"

namespace fa_detail {

// Exact per-op arithmetic: one IEEE operation, never fused.
__device__ __forceinline__ float op_mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float op_add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float op_sub(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float op_div(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double op_mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double op_add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double op_sub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double op_div(double a, double b) { return __ddiv_rn(a, b); }

// The f32 -> f16 rounding must see a MATERIALISED f32 value: otherwise the gfx950 backend folds
// fptrunc(fmul(fpext(h), c)) into v_fma_mixlo_f16, which rounds the exact product to f16 ONCE,
// while the reference (PyTorch CPU) rounds it to f32 first and then to f16 (double rounding).
// The empty asm pins the f32 intermediate in a VGPR (no instruction is emitted).
__device__ __forceinline__ float pin_f32(float x) {
  asm("" : "+v"(x));
  return x;
}

// Per storage dtype:
//   A          op type (the exact widening of a stored element);  S  the stored element as loads see it
//   V, SZ      elements per 16 bytes, element size
//   from_bits  S -> A, exact;  bits  A -> S, rounded once to the storage type;  rnd  that value as an A
//   unpack     the V elements of 16 raw bytes;  pack  V values -> 16 bytes, each rounded once
template <int DT> struct El;

template <> struct El<FA_DTYPE_F32> {
  using A = float; using S = float;
  static constexpr int V = 4, SZ = 4;
  __device__ static float from_bits(float s) { return s; }
  __device__ static float bits(float x) { return x; }
  __device__ static float rnd(float x) { return x; }
  __device__ static void unpack(u32x4 r, float* x) {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = __uint_as_float(r[j]);
  }
  __device__ static u32x4 pack(const float* a) {
    return u32x4{__float_as_uint(a[0]), __float_as_uint(a[1]), __float_as_uint(a[2]), __float_as_uint(a[3])};
  }
};

// the two 16-bit types: two elements per 32-bit word, the even one in the low half
template <class E> struct El16 {
  using A = float; using S = unsigned short;
  static constexpr int V = 8, SZ = 2;
  __device__ static u32x4 pack(const float* a) {
    u32x4 w;
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = (unsigned)E::bits(a[2 * j]) | ((unsigned)E::bits(a[2 * j + 1]) << 16);
    return w;
  }
};
template <> struct El<FA_DTYPE_BF16> : El16<El<FA_DTYPE_BF16>> {
  __device__ static float from_bits(unsigned short s) { return __uint_as_float((unsigned)s << 16); }
  __device__ static unsigned short bits(float x) { return __builtin_bit_cast(unsigned short, (__bf16)x); }
  __device__ static float rnd(float x) { return (float)(__bf16)x; }
  __device__ static void unpack(u32x4 r, float* x) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[2 * j] = __uint_as_float(r[j] << 16);
      x[2 * j + 1] = __uint_as_float(r[j] & 0xFFFF0000u);
    }
  }
};
template <> struct El<FA_DTYPE_F16> : El16<El<FA_DTYPE_F16>> {
  __device__ static float from_bits(unsigned short s) { return (float)__builtin_bit_cast(_Float16, s); }
  __device__ static unsigned short bits(float x) { return __builtin_bit_cast(unsigned short, (_Float16)pin_f32(x)); }
  __device__ static float rnd(float x) { return (float)(_Float16)pin_f32(x); }
  __device__ static void unpack(u32x4 r, float* x) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[2 * j] = from_bits((unsigned short)(r[j] & 0xFFFFu));
      x[2 * j + 1] = from_bits((unsigned short)(r[j] >> 16));
    }
  }
};

// the 64-bit types: two elements per 16 bytes
template <class T> struct El64 {
  using A = T; using S = T;
  static constexpr int V = 2, SZ = 8;
  __device__ static T from_bits(T s) { return s; }
  __device__ static T bits(T x) { return x; }
  __device__ static T rnd(T x) { return x; }
  __device__ static void unpack(u32x4 r, T* x) {
    x[0] = __builtin_bit_cast(T, u32x2{r[0], r[1]});
    x[1] = __builtin_bit_cast(T, u32x2{r[2], r[3]});
  }
  __device__ static u32x4 pack(const T* a) {
    const u32x2 lo = __builtin_bit_cast(u32x2, a[0]), hi = __builtin_bit_cast(u32x2, a[1]);
    return u32x4{lo[0], lo[1], hi[0], hi[1]};
  }
};
template <> struct El<FA_DTYPE_F64> : El64<double> {};
template <> struct El<FA_DTYPE_I64> : El64<long long> {};  // raw elements only: the int64 arithmetic is fedagg.hip's

}  // namespace fa_detail
