// K7s: segmented score ranking. One launch ranks S independent segments of one
// fp32 score buffer - every request of a served step at once - where sort.hip
// ranks one list per launch with one workgroup (the reference's
// Collections.sort, DCNClient.java:195, per request). One workgroup takes one
// segment; the order is exactly sort.hip's (same key, ties by candidate
// index, NaN last in both directions, the scores come back bit for bit).
//
// The key, the 64-bit rank word (key << 32 | index), the register / cross-lane
// / LDS compare-exchange network and rank_one are in rank_common.h, shared
// with topk.hip.
//
// A launch is specialised on the largest segment it may meet (three classes:
// 1024, 4096 and 16384 slots; threads and LDS follow the class). Inside a
// class a workgroup runs the network only up to its own segment's power of
// two: the padding above it is constant and already in place, so the merge
// stages beyond it would move nothing, and the waves that hold only padding
// do nothing but meet the barriers.
#include "common.h"
#include "launchers.h"
#include "rank_common.h"

namespace dtfs {
namespace kern {

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
