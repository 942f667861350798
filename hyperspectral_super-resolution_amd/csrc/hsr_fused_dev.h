// Device code of the two jobs a fused launch carries besides its own K1+K2 - the tail fit of the previous tile (lazy_fit) and K3 of
// an older tile as a pre-phase (apply_prephase) - shared by the K1 kernels (hsr_srf.hip, Args = SrfArgs) and the drain kernel of the
// fused pipeline (hsr_exec.hip, its own small argument record).  Args supplies the apply_* / lazy_* members these functions name;
// a record that fixes one of them at compile time (static constexpr) drops the branch behind it.
#pragma once
#include "hsr_common.h"
#include "hsr_solve.h"
#include "hsr_sync_dev.h"
#include "hsr_tree_dev.h"

namespace hsr {

__device__ __forceinline__ double ld_agent(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void stores_done_barrier() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// The fit of the PREVIOUS tile as tail work of a K1 launch (APPLY variants, no exchange).  Its partial slots were written
// by the previous launch, so - unlike fused_fit (hsr_srf.hip), which reduces the launch's OWN slots and pays memory-side coherence
// round trips for it - nothing has to cross between running workgroups: a workgroup that has finished its groups draws a
// ticket, and tickets 0 .. nb-1 reduce + solve one band each while the slower workgroups are still streaming.  Idle tail
// time instead of a launch of its own, a side stream, two events and CUs kept free for it.  Same tree as
// hsr_moments_reduce_solve (lane_slot_sum for "lane" l, butterfly_tree64 over the 64 lane sums: hsr_tree_dev.h; the same
// solve), hence the same bits.
template <int DEG, int T, class Args>
__device__ __forceinline__ void lazy_fit(const Args& a, unsigned char* smem, int t) {
  constexpr int M = moment_count(DEG);
  static_assert(T == 512, "two passes of 32 lane rows");
  int* ticket = reinterpret_cast<int*>(smem);
  __syncthreads();                                        // everybody is done with the tile buffers
  if (t == 0) *ticket = (int)(__hip_atomic_fetch_add(a.lazy_counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - a.lazy_base);
  __syncthreads();
  const int b = *ticket;
  if (b < 0 || b >= a.nb) return;                         // workgroup-uniform
  double (*lsum)[16] = reinterpret_cast<double (*)[16]>(smem + 64);
  double* mom = reinterpret_cast<double*>(smem + 64 + 64 * 16 * 8);
  double* work = mom + 16;
  const int stride = a.nb * M, m = t & 15;
  const double* row = a.lazy_partials + (size_t)b * M + (m < M ? m : 0);
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int l = pass * 32 + (t >> 4);
    double s = 0.0;                                       // lane_slot_sum (hsr_tree_dev.h), spelled out: K1's device code stays as it is
    for (int i0 = l; i0 < a.lazy_slots; i0 += 64 * 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = i0 + 64 * u;
        v[u] = (i < a.lazy_slots && m < M) ? row[(size_t)i * stride] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    lsum[l][m] = s;
  }
  __syncthreads();
  if (t < M) {
    const double s = butterfly_tree64(&lsum[0][t], 16);
    mom[t] = s;
    if (a.lazy_ready) st_agent(a.lazy_moments + (size_t)b * M + t, s);     // read by another queue while this launch still runs
    else a.lazy_moments[(size_t)b * M + t] = s;
  }
  if (a.lazy_ready) {                                     // exchange pipelines: the all-reduce and the solve follow on the side stream
    stores_done_barrier();
    if (t == 0) __hip_atomic_fetch_add(a.lazy_ready, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  __syncthreads();
  if (a.lazy_group_T > 1) {                               // one fit over a group of tiles
    const int T2 = a.lazy_group_T;
    if (a.lazy_group_index != T2 - 1) return;             // not the group's last tile: its moments are in place, nothing to solve yet
    // hsr_moments_reduce over T "slots" (the tiles' moments): lane l's sum is 0.0 + entry l (one entry per lane for T <= 64, the
    // other lanes hold 0.0), then the butterfly over the 64 lane sums - the same adds, hence the bits of the other mosaic forms.
    // The last tile's own entry comes from LDS (this workgroup has just written it), the others from earlier launches.
    double* gm = mom + 16 + kSolveWork;
    if (t < M) {
      double acc[32];                                     // butterfly_tree<64> (hsr_tree_dev.h), spelled out: K1's device code stays as it is
#pragma unroll
      for (int l = 0; l < 32; ++l) {
        const double lo = l < T2 ? 0.0 + (l == T2 - 1 ? mom[t] : a.lazy_group_moments[((size_t)l * a.nb + b) * M + t]) : 0.0;
        const int h = l + 32;
        const double hi = h < T2 ? 0.0 + (h == T2 - 1 ? mom[t] : a.lazy_group_moments[((size_t)h * a.nb + b) * M + t]) : 0.0;
        acc[l] = lo + hi;
      }
#pragma unroll
      for (int off = 16; off >= 1; off >>= 1)
#pragma unroll
        for (int l = 0; l < off; ++l) acc[l] = acc[l] + acc[l + off];
      gm[t] = acc[0];
      a.lazy_group_total[(size_t)b * M + t] = acc[0];
    }
    __syncthreads();
    if (t == 0) solve_band_t<DEG, true>(gm, a.lazy_min_count, a.lazy_coeffs + (size_t)b * (DEG + 1), work);
    return;
  }
  if (t == 0) solve_band_t<DEG, true>(mom, a.lazy_min_count, a.lazy_coeffs + (size_t)b * (DEG + 1), work);
}

// K3 as a pre-phase of a K1 launch (APPLY variants; round 3).  In the pipelined order K3 of tile i-2 only needs coefficients
// that were ready a whole K1 ago, so it does not need a launch of its own: every workgroup applies its slice of the older
// tile before it starts its groups.  What that buys (profiles/r03_strong_scaling.md): a separate K3 is 20.6 us + a launch
// boundary on a 1024 x 1024 tile and a fixed ~8 us of latency on a 128-row block; as a pre-phase it costs its bytes
// (101 MB at the chip's rate = ~15 us; 2-3 us for the block).  Same arithmetic as apply_rows_kernel (float64 Horner
// without FMA contraction, mask select, clip, channels >= nb pass through), hence the same bits.  504 of the 512 threads
// take part: 504 is a multiple of every row length in float4 (1 .. 4), so a thread keeps its channel group and its
// coefficients stay in registers.
// Exchange pipelines: the coefficients were written by a kernel of ANOTHER queue (all-reduce -> solve on the side stream) with no
// event in between, so the workgroup first polls the tile's "coefficients ready" word - set a whole K1 ago in any sane
// schedule - and reads them through to LDS (agent-scope loads: this XCD's L2 may hold the slot's previous set).
template <int N, int T, class Args>
__device__ __forceinline__ void apply_prephase(const Args& a, unsigned char* smem, int t) {
  constexpr int kUse = T / 12 * 12;
  constexpr int U = 4;
  if (a.apply_x == nullptr) return;                            // workgroup-uniform
  const bool gated = a.apply_ready != nullptr;
  double* cl = reinterpret_cast<double*>(smem);                // [nb][N]: the tile buffers are not in use yet
  if (gated) {
    if (t == 0) wait_word_at_least(a.apply_ready, a.apply_ready_value, a.sync_error, 2u);
    __syncthreads();
    if (t < a.nb * N) cl[t] = ld_agent(a.apply_coeffs + t);
    __syncthreads();
  }
  const int q = (int)(a.out_ps >> 2);
  const uint32_t nv = (uint32_t)(a.apply_npix * q);            // host: apply_npix * q < 2^31
  const uint32_t stride = gridDim.x * (uint32_t)kUse;
  const uint32_t i0 = blockIdx.x * (uint32_t)kUse + (uint32_t)(t < kUse ? t : 0);
  const int c0 = (int)(i0 % (uint32_t)q) * 4;
  double c[4][N];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ch = c0 + j < a.nb ? c0 + j : 0;
#pragma unroll
    for (int k = 0; k < N; ++k) c[j][k] = gated ? cl[ch * N + k] : a.apply_coeffs[ch * N + k];
  }
  if (gated) __syncthreads();                                  // everybody holds its coefficients: the first group's DMA may land on cl
  if (t >= kUse) return;
  const float4* x4 = reinterpret_cast<const float4*>(a.apply_x);
  float4* o4 = reinterpret_cast<float4*>(a.apply_out);
  for (uint32_t ib = i0; ib < nv; ib += stride * U) {
    float4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = ib + u * stride;
      if (i < nv) v[u] = ld_stream(x4 + i);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = ib + u * stride;
      if (i >= nv) break;
      const bool m = !a.apply_mask || a.apply_mask[i / (uint32_t)q];
      float r[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (c0 + j < a.nb) {
          float xv = r[j];
          if (m) {                      // np.polyval: y = 0; y = y*x + c, separately rounded
            const double xd = (double)xv;
            double y = 0.0;
#pragma unroll
            for (int k = 0; k < N; ++k) y = __dadd_rn(__dmul_rn(y, xd), c[j][k]);
            xv = (float)y;
          }
          r[j] = a.apply_clip ? (xv < 0.0f ? 0.0f : (xv > 1.0f ? 1.0f : xv)) : xv;
        }
      }
      st_stream(o4 + i, make_float4(r[0], r[1], r[2], r[3]));
    }
  }
}

}  // namespace hsr
