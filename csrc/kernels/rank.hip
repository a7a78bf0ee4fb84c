// K7s: segmented score ranking. One launch ranks S independent segments of one
// fp32 score buffer - every request of a served step at once - where sort.hip
// ranks one list per launch with one workgroup (the reference's
// Collections.sort, DCNClient.java:195, per request). One workgroup takes one
// segment; the order is exactly sort.hip's (same key, ties by candidate
// index, NaN last in both directions, the scores come back bit for bit).
//
// Each element is one 64-bit word key << 32 | index, so one unsigned compare
// gives the whole order. A thread holds E consecutive elements in registers
// (element i of the padded segment lives in thread i / E, register i % E):
//   stride <  E        compare-exchange inside the thread's registers
//   stride <  64 E     the partner is in the same wave: __shfl_xor
//   stride >= 64 E     the partner is in another wave: through LDS, one
//                      barrier pair per stride
// A launch is specialised on the largest segment it may meet (three classes:
// 1024, 4096 and 16384 slots; threads and LDS follow the class). Inside a
// class a workgroup runs the network only up to its own segment's power of
// two: the padding above it is constant and already in place, so the merge
// stages beyond it would move nothing, and the waves that hold only padding
// do nothing but meet the barriers.
//
// LDS image: register e of thread t at word e * (T + 1) + t. A wave's access
// with e fixed is 64 consecutive words, and the global-order access (element
// i, lanes on consecutive i) walks e first with a step of T + 1 words = 2
// banks, so both are conflict-free; it is used to turn the coalesced global
// reads and writes into the per-thread layout and for the cross-wave strides.
#include "common.h"
#include "launchers.h"

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

// Rank in[0, n) (1 <= n <= T * E) with the whole workgroup; the first k ranks
// go to out_vals / out_idx, ranks [k, n) get 0 / -1. Every thread of the
// workgroup calls this with the same arguments.
template <int T, int E>
__device__ __forceinline__ void rank_one(const float* __restrict__ in, int n, bool descending, int k,
                                         float* __restrict__ out_vals, int64_t* __restrict__ out_idx,
                                         uint64_t* __restrict__ lds) {
  constexpr int LD = T + 1;
  const int tid = threadIdx.x, lane = tid & 63;
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
      } else {
        out_vals[i] = 0.f;
        out_idx[i] = -1;
      }
    }
  }
  __syncthreads();  // the image is free for the workgroup's next segment
}

template <int T, int E>
__global__ void __launch_bounds__(T) rank_segments_kernel(const float* __restrict__ scores, int64_t n_scores,
                                                          const int32_t* __restrict__ offsets, int S, int descending,
                                                          int k, float* __restrict__ out_vals,
                                                          int64_t* __restrict__ out_idx) {
  __shared__ uint64_t lds[E * (T + 1)];
  for (int s = blockIdx.x; s < S; s += gridDim.x) {
    const int64_t a = offsets[s], b = offsets[s + 1];
    const int64_t n = b - a;
    if (a < 0 || n <= 0 || n > T * E || b > n_scores) continue;  // same in every thread
    rank_one<T, E>(scores + a, int(n), descending != 0, (k < 0 || k > n) ? int(n) : k, out_vals + a, out_idx + a, lds);
  }
}

// Segments from a request arena (csrc/runtime/arena.h): n_req at 0, n_ranked
// at 44, descriptors {ids_off, wts_off, rows, dst_row} int64 at 64. Ascending,
// every rank kept. Nothing is written when no request of the batch asked for a
// ranked output, nor for a descriptor that does not fit.
template <int T, int E>
__global__ void __launch_bounds__(T) rank_arena_kernel(const uint8_t* __restrict__ arena,
                                                       const float* __restrict__ scores, int64_t scores_len,
                                                       float* __restrict__ out_vals, int64_t* __restrict__ out_idx) {
  __shared__ uint64_t lds[E * (T + 1)];
  if (*reinterpret_cast<const int32_t*>(arena + 44) <= 0) return;
  const int n_req = min(*reinterpret_cast<const int32_t*>(arena), kArenaMaxRequests);
  const int64_t* desc = reinterpret_cast<const int64_t*>(arena + 64);
  for (int d = blockIdx.x; d < n_req; d += gridDim.x) {
    const int64_t rows = desc[4 * d + 2], r0 = desc[4 * d + 3];
    if (rows <= 0 || rows > T * E || r0 < 0 || r0 + rows > scores_len) continue;
    rank_one<T, E>(scores + r0, int(rows), false, int(rows), out_vals + r0, out_idx + r0, lds);
  }
}

}  // namespace kern

using namespace kern;

int rank_max_elems() { return kRankMax; }

namespace {
// One workgroup per CU at the largest class (its LDS image is 128 KiB), so a
// grid of the CU count loops over more segments than that.
constexpr int kRankGrid = 256;
}  // namespace

hipError_t launch_rank_segments(const float* scores, int64_t n_scores, const int32_t* offsets, int S, int max_len,
                                bool descending, int k, float* out_vals, int64_t* out_idx, hipStream_t st) {
  if (S <= 0) return hipSuccess;
  if (max_len > kRankMax) return hipErrorInvalidValue;
  const dim3 grid(S < kRankGrid ? S : kRankGrid);
  const int desc = descending ? 1 : 0;
  if (max_len > 0 && max_len <= 1024)
    hipLaunchKernelGGL((rank_segments_kernel<256, 4>), grid, dim3(256), 0, st, scores, n_scores, offsets, S, desc, k,
                       out_vals, out_idx);
  else if (max_len > 0 && max_len <= 4096)
    hipLaunchKernelGGL((rank_segments_kernel<512, 8>), grid, dim3(512), 0, st, scores, n_scores, offsets, S, desc, k,
                       out_vals, out_idx);
  else
    hipLaunchKernelGGL((rank_segments_kernel<1024, 16>), grid, dim3(1024), 0, st, scores, n_scores, offsets, S, desc,
                       k, out_vals, out_idx);
  return hipGetLastError();
}

hipError_t launch_rank_arena(const void* arena_dev, const float* scores, int64_t scores_len, float* out_vals,
                             int64_t* out_idx, hipStream_t st) {
  if (scores_len <= 0) return hipSuccess;
  const uint8_t* a = static_cast<const uint8_t*>(arena_dev);
  // a request has at least one row and at most scores_len of them
  const int64_t most = scores_len < kArenaMaxRequests ? scores_len : kArenaMaxRequests;
  const dim3 grid(unsigned(most < kRankGrid ? most : kRankGrid));
  if (scores_len <= 1024)
    hipLaunchKernelGGL((rank_arena_kernel<256, 4>), grid, dim3(256), 0, st, a, scores, scores_len, out_vals, out_idx);
  else if (scores_len <= 4096)
    hipLaunchKernelGGL((rank_arena_kernel<512, 8>), grid, dim3(512), 0, st, a, scores, scores_len, out_vals, out_idx);
  else
    hipLaunchKernelGGL((rank_arena_kernel<1024, 16>), grid, dim3(1024), 0, st, a, scores, scores_len, out_vals,
                       out_idx);
  return hipGetLastError();
}

}  // namespace dtfs
