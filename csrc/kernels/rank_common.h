// Shared by rank.hip (K7s) and topk.hip (K7t): the rank key, the 64-bit rank
// word and the workgroup compare-exchange network over such words, so the two
// files order scores by one definition.
//
// Each element is one 64-bit word key << 32 | index, so one unsigned compare
// gives the whole order. A thread holds E consecutive elements in registers
// (element i of the padded segment lives in thread i / E, register i % E):
//   stride <  E        compare-exchange inside the thread's registers
//   stride <  64 E     the partner is in the same wave: __shfl_xor
//   stride >= 64 E     the partner is in another wave: through LDS, one
//                      barrier pair per stride
//
// LDS image: register e of thread t at word e * (T + 1) + t. A wave's access
// with e fixed is 64 consecutive words, and the global-order access (element
// i, lanes on consecutive i) walks e first with a step of T + 1 words = 2
// banks, so both are conflict-free; it is used to turn the coalesced global
// reads and writes into the per-thread layout and for the cross-wave strides.
#pragma once

#include "common.h"

namespace dtfs {
namespace kern {

constexpr int kRankMax = 16384;
// sort.hip's key (kept in step with it by tests/test_rank_segments_gpu.py)
constexpr uint32_t kRankKeyNaN = 0xfffffffeu, kRankKeyPad = 0xffffffffu;
constexpr uint64_t kRankPadWord = (uint64_t(kRankKeyPad) << 32) | 0x7fffffffu;

__device__ __forceinline__ uint32_t rank_key(float v, bool descending) {
  if (v != v) return kRankKeyNaN;
  uint32_t u = v == 0.f ? 0u : __float_as_uint(v);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return descending ? ~u : u;
}

// The score bits behind a key. false: the key folds several values (a zero of
// either sign, any NaN) and the caller reads the score itself.
__device__ __forceinline__ bool rank_unkey(uint32_t key, bool descending, uint32_t* bits) {
  if (key == kRankKeyNaN) return false;
  const uint32_t u = descending ? ~key : key;
  if (u == 0x80000000u) return false;
  *bits = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  return true;
}

__device__ __forceinline__ void rank_cx(uint64_t& a, uint64_t& b, bool up) {
  const bool sw = (a > b) == up;
  const uint64_t lo = sw ? b : a, hi = sw ? a : b;
  a = lo;
  b = hi;
}

// The bitonic network over the p2 (a power of two, E <= p2 <= T * E) words the
// workgroup holds in registers, ascending; the words at and above p2 are
// padding and stay where they are. wave_active: this wave holds words below
// p2. Every thread of the workgroup calls this with the same p2: the waves
// that hold only padding do nothing but meet the barriers.
template <int T, int E>
__device__ __forceinline__ void rank_network(uint64_t (&w)[E], int p2, bool wave_active, uint64_t* __restrict__ lds) {
  constexpr int LD = T + 1;
  const int tid = threadIdx.x, lane = tid & 63;
  const int base = tid * E;
  for (int size = 2; size <= p2; size <<= 1) {
    // cross-wave strides: exchange through LDS (size and p2 are the same in
    // every thread, so every wave meets every barrier)
    for (int st = size >> 1; st >= 64 * E; st >>= 1) {
      __syncthreads();  // the previous image has been read
      if (wave_active) {
#pragma unroll
        for (int e = 0; e < E; ++e) lds[e * LD + tid] = w[e];
      }
      __syncthreads();
      if (wave_active) {
        const int pt = st / E;
        const bool keep_min = ((tid & pt) == 0) == ((base & size) == 0);
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const uint64_t o = lds[e * LD + (tid ^ pt)];
          w[e] = keep_min ? (o < w[e] ? o : w[e]) : (o > w[e] ? o : w[e]);
        }
      }
    }
    if (!wave_active) continue;
    // strides inside the wave: the partner's registers through a cross-lane move
    for (int st = min(size >> 1, 32 * E); st >= E; st >>= 1) {
      const int pl = st / E;
      const bool keep_min = ((lane & pl) == 0) == ((base & size) == 0);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const uint64_t o = __shfl_xor(w[e], pl, 64);
        w[e] = keep_min ? (o < w[e] ? o : w[e]) : (o > w[e] ? o : w[e]);
      }
    }
    // strides inside the thread
#pragma unroll
    for (int st = E / 2; st >= 1; st >>= 1) {
      if (st < size) {
#pragma unroll
        for (int e = 0; e < E; ++e)
          if ((e & st) == 0) rank_cx(w[e], w[e | st], ((base + e) & size) == 0);
      }
    }
  }
}

// Rank in[0, n) (1 <= n <= T * E) with the whole workgroup; the first k ranks
// go to out_vals / out_idx. FILL: ranks [k, n) get 0 / -1; without it they are
// not written. Every thread of the workgroup calls this with the same
// arguments.
template <int T, int E, bool FILL = true>
__device__ __forceinline__ void rank_one(const float* __restrict__ in, int n, bool descending, int k,
                                         float* __restrict__ out_vals, int64_t* __restrict__ out_idx,
                                         uint64_t* __restrict__ lds) {
  constexpr int LD = T + 1;
  const int tid = threadIdx.x;
  int p2 = E;
  while (p2 < n) p2 <<= 1;
  // coalesced read -> LDS in the per-thread layout
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const int i = j * T + tid;
    if (i < p2) {
      const uint64_t w = i < n ? (uint64_t(rank_key(in[i], descending)) << 32) | uint32_t(i) : kRankPadWord;
      lds[(i % E) * LD + i / E] = w;
    }
  }
  __syncthreads();
  const bool wave_active = (tid & ~63) * E < p2;
  const int base = tid * E;
  uint64_t w[E];
  if (wave_active) {
#pragma unroll
    for (int e = 0; e < E; ++e) w[e] = base < p2 ? lds[e * LD + tid] : kRankPadWord;
  }
  rank_network<T, E>(w, p2, wave_active, lds);
  // back through LDS so that the global writes are coalesced
  __syncthreads();
  if (wave_active) {
#pragma unroll
    for (int e = 0; e < E; ++e) lds[e * LD + tid] = w[e];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const int i = j * T + tid;
    if (i < n) {
      const uint64_t v = lds[(i % E) * LD + i / E];
      const int src = int(uint32_t(v));
      if (i < k) {
        // the scores themselves, bit for bit (the key folds -0.0 and every NaN)
        uint32_t bits;
        out_vals[i] = rank_unkey(uint32_t(v >> 32), descending, &bits) ? __uint_as_float(bits) : in[src];
        out_idx[i] = src;
      } else if (FILL) {
        out_vals[i] = 0.f;
        out_idx[i] = -1;
      }
    }
  }
  __syncthreads();  // the image is free for the workgroup's next segment
}

}  // namespace kern
}  // namespace dtfs
