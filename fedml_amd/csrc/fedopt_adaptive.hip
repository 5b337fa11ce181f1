// fedopt_adaptive.hip -- MI355X (gfx950) kernel + C ABI of the adaptive FedOpt server steps
// (include/fedagg.h: fa_fedavg_adaptive, fa_fedavg_adaptive_tiled): FedAdam, FedYogi and FedAdagrad of
// Reddi et al., "Adaptive Federated Optimization" (ICLR 2021), and torch.optim.Adam / Adagrad, fused
// into the FedAvg pass.
//
// Per element: avg = the ordered MUL_W sum of the clients (fedagg.hip's arithmetic), the
// pseudo-gradient g = p - avg, the second moment v by the rule, the first moment m (with momentum),
// and p -= step_size * num / (sqrt(v) / c2 + eps) -- float32, every op rounded once, nothing fused
// (the contract and its op order: include/fedagg.h).  p, m and v are flat and updated in place.
//
// k_fedavg_adaptive: k_sign_vote's shape (signvote.hip) -- a workgroup owns ONE 4-KiB slot per client
// (a slot = one arena tile, so the tiled and the flat layout differ only in the slot's address),
// 16 bytes per lane and client, non-temporal, kU clients' loads issued before any is consumed.  The
// loads of p, v and m are issued BEFORE the client stream, so their latency hides under it, and all
// three are stored with non-temporal 16-byte stores.  Unaligned segments and a segment's ragged last
// slot take the same code with coalesced element loads.  No reduction across lanes: no LDS, no
// atomics.  The rule and "has momentum" are template parameters; bias correction is not (without it
// c2 == 1.0f, and a division by 1 is exact).  Numbers: DESIGN.md.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "elem.h"
#include "fa_internal.h"
#include "median_common.h"
#include "median_host.h"

using namespace fa_detail;

namespace {

constexpr int kU = 8;   // clients whose loads are in flight together (whole aligned slots)
constexpr int kUE = 4;  // the same on the element path

using T = El<FA_DTYPE_F32>;
constexpr int V = T::V;
constexpr int64_t E = FA_TILE_BYTES / T::SZ;  // a slot's elements

// The host scalars, each cast double -> float once.
struct AdArgs {
  float b1, one_m_b1, b2, one_m_b2, eps, wd, c2, step_size;
  int has_wd;  // weight_decay != 0 as a double
};

// One element of the contract; p, m and v are the stored values and are replaced.
template <int RULE, bool MOM>
__device__ __forceinline__ void ad_update(float& p, float& m, float& v, float avg, const AdArgs& a) {
  float g = op_sub(p, avg);
  if (a.has_wd) g = op_add(g, op_mul(p, a.wd));  // uniform
  const float g2 = op_mul(g, g);
  if constexpr (RULE == FA_ADAPT_ADAM) {
    v = op_add(op_mul(v, a.b2), op_mul(g2, a.one_m_b2));
  } else if constexpr (RULE == FA_ADAPT_YOGI) {
    const float d = op_sub(v, g2);
    const float s = (float)((int)(d > 0.f) - (int)(d < 0.f));  // NaN: neither comparison holds
    v = op_sub(v, op_mul(op_mul(a.one_m_b2, g2), s));
  } else {
    v = op_add(v, g2);
  }
  float num = g;
  if constexpr (MOM) {
    m = op_add(op_mul(m, a.b1), op_mul(g, a.one_m_b1));
    num = m;
  }
  // correctly rounded float sqrt, as rmsprop_update (fedagg.hip): the float64 sqrt is correctly
  // rounded and its rounding to float32 is innocuous; v_sqrt_f32 is ~1 ulp
  const float root = __double2float_rn(__dsqrt_rn((double)v));
  const float den = op_add(op_div(root, a.c2), a.eps);
  p = op_sub(p, op_mul(a.step_size, op_div(num, den)));
}

// The slot tl of segment sg.  param, mom (MOM) and var: the segment's flat parameter and state.
template <int RULE, bool MOM, bool VEC>
__device__ __forceinline__ void ad_slot(const MSeg& sg, int64_t tl, const void* const* __restrict__ in,
                                        float* __restrict__ mom, float* __restrict__ var,
                                        const double* __restrict__ coef, int k, const AdArgs& a) {
  using L = SlotLoad<FA_DTYPE_F32, VEC>;
  constexpr int NR = L::NR;
  constexpr int U = VEC ? kU : kUE;
  const int tid = (int)threadIdx.x;
  const int64_t e0 = tl * E;  // a multiple of E: the slot is one whole tile
  const int64_t ts = sg.tstride;
  float* param = (float*)sg.out;

  // ld: the clients' slot (flat or tiled); st: the same elements of the flat parameter and state
  L ld, st;
  unsigned live = 0;  // bit j: the lane's element j lies inside the segment
  if constexpr (VEC) {
    st.off[0] = e0 * T::SZ + (int64_t)tid * 16;
    ld.off[0] = (ts ? tl * ts : e0 * T::SZ) + (int64_t)tid * 16;
    live = ~0u;
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int64_t e = e0 + (int64_t)j * kBlock + tid;
      if (e < sg.numel) live |= 1u << j;
      const int64_t ec = e < sg.numel ? e : sg.numel - 1;  // clamped: every load unconditional
      st.off[j] = ec;
      ld.off[j] = ts ? (ec / E) * (ts / T::SZ) + ec % E : ec;
    }
  }

  // the parameter and the state first: their latency hides under the client stream.  The lane that
  // owns an element reads it here and only then stores it (a clamped lane's copy is dropped).
  typename L::Raw rp[NR], rv[NR], rm[NR];
  st.load(rp, param);
  st.load(rv, var);
  if constexpr (MOM) st.load(rm, mom);

  float acc[V];
#pragma unroll
  for (int v = 0; v < V; ++v) acc[v] = -0.0f;  // -0 + t == t bitwise for every t
  // whole groups unguarded, so every load of a group is issued before the first client's arithmetic
  int i0 = 0;
  for (; i0 + U <= k; i0 += U) {
    typename L::Raw r[U][NR];
#pragma unroll
    for (int u = 0; u < U; ++u) ld.load(r[u], in[i0 + u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float x[V];
      L::get(r[u], x);
      const float c = (float)coef[i0 + u];
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = op_add(acc[v], op_mul(x[v], c));
    }
  }
  if (i0 < k) {
    typename L::Raw r[U][NR];
#pragma unroll
    for (int u = 0; u < U; ++u) ld.load(r[u], in[min(i0 + u, k - 1)]);  // clamped: every load unconditional
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (i0 + u < k) {  // wave-uniform
        float x[V];
        L::get(r[u], x);
        const float c = (float)coef[i0 + u];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = op_add(acc[v], op_mul(x[v], c));
      }
    }
  }

  float p[V], sv[V], sm[V] = {};
  L::get(rp, p);
  L::get(rv, sv);
  if constexpr (MOM) L::get(rm, sm);
#pragma unroll
  for (int v = 0; v < V; ++v) ad_update<RULE, MOM>(p[v], sm[v], sv[v], acc[v], a);

  if constexpr (VEC) {
    using G4 = __attribute__((address_space(1))) u32x4;
    __builtin_nontemporal_store(T::pack(p), (G4*)((char*)param + st.off[0]));
    __builtin_nontemporal_store(T::pack(sv), (G4*)((char*)var + st.off[0]));
    if constexpr (MOM) __builtin_nontemporal_store(T::pack(sm), (G4*)((char*)mom + st.off[0]));
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (live >> j & 1u) {
        const int64_t e = e0 + (int64_t)j * kBlock + tid;
        param[e] = p[j];
        var[e] = sv[j];
        if constexpr (MOM) mom[e] = sm[j];
      }
  }
}

// vars[j], moms[j] (MOM; not read otherwise): the state of the table's segment j; st_al[j]: both are
// 16-byte aligned (MSeg.aligned covers the parameter and the clients).
template <int RULE, bool MOM>
__global__ void __launch_bounds__(kBlock)
k_fedavg_adaptive(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ ptrs,
                  void* const* __restrict__ vars, void* const* __restrict__ moms, const int* __restrict__ st_al,
                  const double* __restrict__ coef, int k, AdArgs a) {
  const int64_t tile = blockIdx.x;
  const int si = nseg > 1 ? find_seg(segs, nseg, tile) : 0;
  const MSeg sg = segs[si];
  const int64_t tl = tile - sg.tile_start;
  const void* const* in = ptrs + sg.ptr_base;
  float* var = (float*)vars[si];
  float* mom = MOM ? (float*)moms[si] : nullptr;
  if (sg.aligned && st_al[si] && (tl + 1) * E <= sg.numel) ad_slot<RULE, MOM, true>(sg, tl, in, mom, var, coef, k, a);
  else ad_slot<RULE, MOM, false>(sg, tl, in, mom, var, coef, k, a);
}

template <int RULE>
void ad_launch(bool mom, dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp, void* const* dv,
               void* const* dm, const int* dal, const double* dc, int k, const AdArgs& a) {
  const dim3 block(kBlock);
  if (mom) hipLaunchKernelGGL((k_fedavg_adaptive<RULE, true>), grid, block, 0, st, ds, n, dp, dv, dm, dal, dc, k, a);
  else hipLaunchKernelGGL((k_fedavg_adaptive<RULE, false>), grid, block, 0, st, ds, n, dp, dv, dm, dal, dc, k, a);
}

// a: d_out = the parameters.  Checks in the order of include/fedagg.h.
int ad_impl(const ColArgs& a, const double* coef, void* const* d_m, void* const* d_v, int rule, double lr,
            double beta1, double beta2, double eps, double weight_decay, int bias_correction, int64_t step) {
  if (const int rc = col_check_args(a)) return rc;
  const int k = a.k;
  if (!coef) return fail(FA_ERR_INVALID, "%s: coef is NULL", a.fn);
  if (!d_v) return fail(FA_ERR_INVALID, "%s: d_v is NULL", a.fn);
  if ((d_m == nullptr) != (beta1 == 0.0))
    return fail(FA_ERR_INVALID, "%s: d_m must be NULL exactly when beta1 == 0 (beta1 %g)", a.fn, beta1);
  if (rule != FA_ADAPT_ADAM && rule != FA_ADAPT_YOGI && rule != FA_ADAPT_ADAGRAD)
    return fail(FA_ERR_INVALID, "%s: rule %d is none of FA_ADAPT_ADAM, FA_ADAPT_YOGI, FA_ADAPT_ADAGRAD", a.fn, rule);
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || step < 1)
    return fail(FA_ERR_INVALID, "%s: need 0 <= beta1 < 1, 0 <= beta2 < 1, eps >= 0 and step >= 1 (got %g, %g, %g, %lld)",
                a.fn, beta1, beta2, eps, (long long)step);
  int nseg;
  int64_t tiles;
  if (const int rc = col_count(a, E, &nseg, &tiles)) return rc;
  const bool mom = d_m != nullptr;
  for (int s = 0; s < a.num_segments; ++s) {
    if (a.seg_numel[s] == 0) continue;
    if (!d_v[s]) return fail(FA_ERR_INVALID, "%s: segment %d: second moment NULL", a.fn, s);
    if (mom && !d_m[s]) return fail(FA_ERR_INVALID, "%s: segment %d: first moment NULL", a.fn, s);
  }
  if (nseg == 0) return FA_OK;

  AdArgs ad;
  ad.b1 = (float)beta1;
  ad.one_m_b1 = (float)(1.0 - beta1);
  ad.b2 = (float)beta2;
  ad.one_m_b2 = (float)(1.0 - beta2);
  ad.eps = (float)eps;
  ad.wd = (float)weight_decay;
  ad.has_wd = weight_decay != 0.0;
  ad.c2 = bias_correction ? (float)std::sqrt(1.0 - std::pow(beta2, (double)step)) : 1.0f;
  ad.step_size = (float)(bias_correction ? lr / (1.0 - std::pow(beta1, (double)step)) : lr);

  // the payload: the k coefficients, the non-empty segments' second-moment pointers, (with momentum)
  // their first-moment pointers, and one int per segment: both are 16-byte aligned
  const size_t coef_bytes = sizeof(double) * (size_t)k;
  const size_t ptr_bytes = sizeof(void*) * (size_t)nseg;
  const size_t al_off = coef_bytes + (mom ? 2 : 1) * ptr_bytes;
  const size_t extra = al_off + ((sizeof(int) * (size_t)nseg + 7) & ~size_t(7));
  return col_stage_launch(
      a, E, nseg, tiles, extra,
      [&](void* h) {
        for (int i = 0; i < k; ++i) ((double*)h)[i] = coef[i];
        void** hv = (void**)((char*)h + coef_bytes);
        void** hm = hv + nseg;
        int* hal = (int*)((char*)h + al_off);
        for (int s = 0, j = 0; s < a.num_segments; ++s) {
          if (!a.seg_numel[s]) continue;
          hv[j] = d_v[s];
          if (mom) hm[j] = d_m[s];
          hal[j] = al16(d_v[s]) && (!mom || al16(d_m[s])) ? 1 : 0;
          ++j;
        }
        if (nseg & 1) hal[nseg] = 0;  // the padding is staged too
      },
      [&](dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp, const void* payload) {
        const char* pl = (const char*)payload;
        const double* dc = (const double*)pl;
        void* const* dv = (void* const*)(pl + coef_bytes);
        void* const* dm = mom ? dv + nseg : nullptr;
        const int* dal = (const int*)(pl + al_off);
        switch (rule) {
          case FA_ADAPT_ADAM: ad_launch<FA_ADAPT_ADAM>(mom, grid, st, ds, n, dp, dv, dm, dal, dc, k, ad); break;
          case FA_ADAPT_YOGI: ad_launch<FA_ADAPT_YOGI>(mom, grid, st, ds, n, dp, dv, dm, dal, dc, k, ad); break;
          default: ad_launch<FA_ADAPT_ADAGRAD>(mom, grid, st, ds, n, dp, dv, dm, dal, dc, k, ad); break;
        }
      });
}

}  // namespace

extern "C" {

int fa_fedavg_adaptive(fa_ctx* ctx, int32_t num_segments, const int64_t* seg_numel, int32_t k, const void* const* d_in,
                       const double* coef, void* const* d_param, void* const* d_m, void* const* d_v, int rule,
                       double lr, double beta1, double beta2, double eps, double weight_decay, int bias_correction,
                       int64_t step, void* hip_stream) {
  return ad_impl({"fa_fedavg_adaptive", ctx, FA_DTYPE_F32, num_segments, seg_numel, k, d_in, 0, d_param, hip_stream},
                 coef, d_m, d_v, rule, lr, beta1, beta2, eps, weight_decay, bias_correction, step);
}

int fa_fedavg_adaptive_tiled(fa_ctx* ctx, int32_t num_segments, const int64_t* seg_numel, int32_t k,
                             const void* const* d_in, int64_t tile_stride, const double* coef, void* const* d_param,
                             void* const* d_m, void* const* d_v, int rule, double lr, double beta1, double beta2,
                             double eps, double weight_decay, int bias_correction, int64_t step, void* hip_stream) {
  if (ctx && tile_stride <= 0) return fail(FA_ERR_INVALID, "fa_fedavg_adaptive_tiled: tile_stride must be > 0");
  return ad_impl({"fa_fedavg_adaptive_tiled", ctx, FA_DTYPE_F32, num_segments, seg_numel, k, d_in, tile_stride, d_param,
                  hip_stream},
                 coef, d_m, d_v, rule, lr, beta1, beta2, eps, weight_decay, bias_correction, step);
}

}  // extern "C"
