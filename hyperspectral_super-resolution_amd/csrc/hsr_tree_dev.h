// The fixed-order float64 sums of libhsr_mi355x: ONE definition of every level of the summation tree, so that every kernel that
// reduces moments performs the same adds in the same order and produces the same bits ("Where the tree is defined").
//   thread sums --wave_sum--> 4 wave sums --block_join4--> one slot per workgroup                       (moments kernels)
//   slots --lane_slot_sum--> 64 lane sums --wave_sum / butterfly_tree<64>--> one moment                 (slot reductions)
// Device code only; every function is inlined into its caller.
#pragma once
#include <hip/hip_runtime.h>

namespace hsr {

// Wave-level butterfly sum of a double (fixed tree -> deterministic).
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// The N - 1 adds of the xor butterfly (N/2, .., 1) over N entries, done by one thread: t[l] = v[l] + v[l ^ off] for l < off is
// the value every lane of the pair holds after a level, so a[0] after the last level is, for N = 64, wave_sum's result bit for
// bit.  ``entry(l)`` yields entry l (each is asked for once).  N = 16: the four levels left over the wave index when the first two
// levels of a 64-entry butterfly were in-wave shuffles (reduce_solve_batched_kernel).
template <int N, class Entry>
__device__ __forceinline__ double butterfly_tree(Entry entry) {
  static_assert(N == 64 || N == 16, "the trees in use");
  double a[N / 2];
#pragma unroll
  for (int l = 0; l < N / 2; ++l) a[l] = entry(l) + entry(l + N / 2);
#pragma unroll
  for (int off = N / 4; off >= 1; off >>= 1)
#pragma unroll
    for (int l = 0; l < off; ++l) a[l] = a[l] + a[l + off];
  return a[0];
}

// The pointer form over 64 lane sums: ``col`` = address of lane 0's sum, ``ld`` doubles between lanes.
__device__ __forceinline__ double butterfly_tree64(const double* col, int ld) {
  return butterfly_tree<64>([&](int l) { return col[(size_t)l * ld]; });
}

// One lane's sum of a slot row in a fixed order: slots first, first + 64, ... added in that order to 0.0; ``load(i)`` yields slot
// i.  The loads go out in independent batches of eight, so that a row costs one memory round trip instead of slots / 64.  An
// absent entry (a slot past the end, or ``on`` false: a thread without a row) contributes +0.0.  That cannot change a bit: a sum
// that starts at +0.0 never becomes -0.0 (x + (+0.0) == x for every x but -0.0, and -0.0 arises only from (-0.0) + (-0.0)), so the
// batched form gives the bits of the plain loop ``for (i = first; i < slots; i += 64) s += load(i)``.
template <class Load>
__device__ __forceinline__ double lane_slot_sum(int first, int slots, bool on, Load load) {
  double s = 0.0;
  for (int i0 = first; i0 < slots; i0 += 64 * 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + 64 * u;
      v[u] = (i < slots && on) ? load(i) : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  return s;
}

// The join of a 256-thread workgroup's per-thread accumulators: wave_sum of each, lane 0 of wave w to red[w][m], barrier, thread m
// hands ((w0 + w1) + w2) + w3 to ``store(m, sum)``.  Accumulators m >= m_count (<= M) are dead: not summed, not stored.  G: the
// accumulators come in groups of G (m_count a multiple of G), one test and G butterflies in flight per live group (measured on
// ridge_stats_partial_kernel, 16 pairs of which 10 live: 11.2 us, against 12.6 us with a test per accumulator;
// profiles/r19_reduction_helpers.md).  Every thread of the workgroup must call it (it holds a barrier).
template <int M, int G = 1, class Store>
__device__ __forceinline__ void block_join4(const double (&acc)[M], double (&red)[4][M], int m_count, Store store) {
  static_assert(M % G == 0, "whole groups");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int m0 = 0; m0 < M; m0 += G) {
    if (m0 < m_count) {
      double s[G];
#pragma unroll
      for (int g = 0; g < G; ++g) s[g] = wave_sum(acc[m0 + g]);
      if (lane == 0) {
#pragma unroll
        for (int g = 0; g < G; ++g) red[wave][m0 + g] = s[g];
      }
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < m_count) {
    const int m = threadIdx.x;
    store(m, ((red[0][m] + red[1][m]) + red[2][m]) + red[3][m]);
  }
}

}  // namespace hsr
