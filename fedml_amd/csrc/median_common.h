// median_common.h -- device helpers shared by the per-column kernels of the robust family
// (median.hip: coordinate-wise median; trimmed.hip: coordinate-wise trimmed mean; wsum_dist.hip: the
// fused weighted sum and squared distances): raw global loads, the per-column element access, the
// order-preserving float key, the segment record, the flat / tile-interleaved column addressing, and
// the slot load of the kernels that walk one 4-KiB slot per client (signvote.hip, fedopt_adaptive.hip).
// The conversions are elem.h's; the common host path is median_host.h.  Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "elem.h"
#include "fa_internal.h"

namespace fa_detail {

// Raw element loads in the global address space (global_load_*: vmcnt only).  Generic (flat)
// loads also count in lgkmcnt, so every s_waitcnt for the next scalar pointer load drained them and
// the per-client loads of a column ran one HBM round trip at a time.
template <typename T>
__device__ __forceinline__ T gld(const void* p, int64_t e) {
  return ((const __attribute__((address_space(1))) T*)p)[e];
}

// non-temporal: each client element is read once (K = 16 / 32 medians 6% / 3% faster)
template <typename T>
__device__ __forceinline__ T gld_nt(const void* p, int64_t e) {
  return __builtin_nontemporal_load((const __attribute__((address_space(1))) T*)p + e);
}

// uniform base + 32-bit byte offset (zero-extended): selects the saddr form of global_load
template <typename T>
__device__ __forceinline__ T gld_nt_off(const void* p, unsigned off) {
  return __builtin_nontemporal_load((const __attribute__((address_space(1))) T*)((const char*)p + off));
}

// A column's element of a float dtype below float64: non-temporal loads widened exactly (elem.h),
// the store of a value that came from the dtype, and a raw copy of a client's element.
template <int DT> struct MedT {
  using E = El<DT>;
  using S = typename E::S;
  static constexpr int kBytes = E::SZ;
  __device__ static float load(const void* p, int64_t e) { return E::from_bits(gld_nt<S>(p, e)); }
  __device__ static float load_off(const void* p, unsigned off) { return E::from_bits(gld_nt_off<S>(p, off)); }
  // exact, v came from the dtype: no rounding, and no pin (elem.h's bits() would round bf16 and pin f16)
  __device__ static void store(void* p, int64_t e, float v) {
    if constexpr (DT == FA_DTYPE_BF16) ((S*)p)[e] = (S)(__float_as_uint(v) >> 16);
    else if constexpr (DT == FA_DTYPE_F16) ((S*)p)[e] = __builtin_bit_cast(S, (_Float16)v);
    else ((S*)p)[e] = v;
  }
  using W = typename std::conditional<sizeof(S) == 4, unsigned, S>::type;  // the element as an integer word
  __device__ static void store_bits_off(void* p, int64_t e, const void* src, unsigned off) {
    ((W*)p)[e] = gld_nt_off<W>(src, off);
  }
};

// order-preserving key of a float (unsigned order == numeric order for non-NaN values; -0.0 sorts
// just below +0.0, which the zero rescan below accounts for)
__device__ __forceinline__ unsigned fkey(float x) {
  const unsigned u = __float_as_uint(x);
  return u ^ ((unsigned)((int)u >> 31) | 0x80000000u);
}
constexpr unsigned kPosZeroKey = 0x80000000u, kNegZeroKey = 0x7FFFFFFFu;
__device__ __forceinline__ float fkey_inv(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

struct MSeg {
  int64_t numel;
  int64_t tile_start;
  void* out;
  int64_t tstride;  // 0: flat client segments; > 0: tile-interleaved inputs, bytes between a client's tiles
  int32_t ptr_base;
  int32_t aligned;  // every input and the output are 16-byte aligned (read by wsum_dist.hip only)
};
static_assert(sizeof(MSeg) == 40, "MSeg layout");

// Byte offset of a workgroup's first column e0 from a client's segment start: flat segments e0 * SZ;
// tiled inputs (tstride > 0, FA_TILE_BYTES tiles of E elements; fedml_amd/arena.py tiled=True)
// (e0 / E) * tstride + (e0 % E) * SZ.  A workgroup's columns never straddle a tile (its column count
// divides E), so a client's element is `uniform base (SGPRs: pointer + this offset) + the lane's
// 32-bit byte offset` in both layouts -- every load keeps global_load's saddr form, for any segment size.
template <int SZ>
__device__ __forceinline__ int64_t col_base(int64_t e0, int64_t tstride) {
  constexpr int64_t E = FA_TILE_BYTES / SZ;
  return tstride ? (e0 / E) * tstride + (e0 % E) * SZ : e0 * SZ;
}
__device__ __forceinline__ const void* at(const void* p, int64_t ub) { return (const char*)p + ub; }

// One client's V elements of this lane, for the kernels whose workgroup owns one 4-KiB slot per
// client (signvote.hip, fedopt_adaptive.hip).  VEC: one 16-byte load at byte offset off[0]; else
// element loads at the clamped element indices off[j] (coalesced across the wave: element j of lane l
// is the slot's element j * kBlock + l).
template <int DT, bool VEC>
struct SlotLoad {
  using T = El<DT>;
  using A = typename T::A;
  static constexpr int V = T::V;
  static constexpr int NR = VEC ? 1 : V;
  using Raw = typename std::conditional<VEC, u32x4, A>::type;

  int64_t off[NR];

  __device__ void load(Raw (&r)[NR], const void* p) const {
    if constexpr (VEC) {
      r[0] = __builtin_nontemporal_load((const __attribute__((address_space(1))) u32x4*)((const char*)p + off[0]));
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) r[j] = T::from_bits(gld<typename T::S>(p, off[j]));
    }
  }
  __device__ static void get(const Raw (&r)[NR], A (&x)[V]) {
    if constexpr (VEC) {
      T::unpack(r[0], x);
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) x[j] = r[j];
    }
  }
};

// float64 has no MedT (no network runs on it): its element size, and any dtype's element
// at(p, ub) + lane offset c (elements) widened exactly to double, for the in-order kernels
template <int DT> constexpr int elem_bytes() { if constexpr (DT == FA_DTYPE_F64) return 8; else return MedT<DT>::kBytes; }
template <int DT>
__device__ __forceinline__ double load_d(const void* p, int64_t c) {
  if constexpr (DT == FA_DTYPE_F64) return gld<double>(p, c);
  else return (double)MedT<DT>::load(p, c);
}

}  // namespace fa_detail
