// K7t: segmented top-k. One launch writes, for each of S independent segments
// of one fp32 score buffer, the m = min(k, n) best scores and their
// segment-local candidate indices in rank.hip's descending order (ties by
// candidate index, NaN last, the scores bit for bit) - the head of what
// rank_segments(descending) gives - and nothing else: entries [m, n) of a
// segment's span of the outputs are not written. One workgroup takes one
// segment of up to 16384 scores; k is per segment.
//
// A segment longer than kTopkSelMin whose m is at most kTopkSel is selected
// first and only the selected are ranked:
//   1. A thread reads its E scores (element j * T + tid: coalesced, straight
//      into registers) as descending keys. The word key << 32 | index of an
//      element is unique, so the m smallest words are the result and there is
//      no tie to break.
//   2. MSB-first radix select on the word, 4 bits a pass: the 32 key bits,
//      then (only while keys tie across the cut) the 16 index bits. A thread
//      counts its still-undecided elements per digit in registers (16 packed
//      counters), a wave adds them up with cross-lane moves and leaves 16
//      counts in LDS, and after ONE barrier every wave adds the waves' counts
//      and finds the digit the cut falls into by itself. No LDS atomics: the
//      cost does not depend on how the scores are distributed (served scores
//      are sigmoid outputs whose leading digits are all but constant). The
//      passes end as soon as the cut digit's elements are all wanted.
//   3. The selected words are compacted into LDS (block-wide exclusive scan of
//      the per-thread counts), loaded kTopkSel / T per thread, ranked by
//      rank_common.h's network - only the waves that hold them work - and
//      written from registers.
// Every other segment (n <= kTopkSelMin, or m > kTopkSel) runs the full
// descending network, rank_one without the 0 / -1 fill, in a second kernel of
// the same launch; each kernel leaves the other's segments alone. Launches
// whose longest segment fits 4096 scores are that kernel alone: measured
// (profiles/topk_kernel.md), selection wins 2.6x on 16384 scores and loses on
// 1500, where the network is short and only the waves that hold scores run it.
//
// No scratch (the keys and bit masks stay in registers: every loop over them
// is unrolled), and every barrier is met by every wave: n, m and the pass
// results are the same in every thread of the workgroup.
#include "common.h"
#include "launchers.h"
#include "rank_common.h"

namespace dtfs {
namespace kern {

// Most scores the select path hands to the network (its LDS buffer), and the
// segment length above which it is taken.
constexpr int kTopkSel = 1024;
constexpr int kTopkSelMin = 4096;

// LDS words (uint64) a workgroup of the class needs: rank_one's image, which
// the select path re-uses as [network image of the selected | selected words |
// per-wave digit counts, two copies | per-wave selected counts].
template <int T, int E>
struct TopkLds {
  static constexpr int ES = kTopkSel / T > 0 ? kTopkSel / T : 1;  // selected words a thread ranks
  static constexpr int kImage = ES * (T + 1);
  static constexpr int kSel = kImage;                      // uint64 [kTopkSel]
  static constexpr int kHist = kSel + kTopkSel;            // uint32 [2][T / 64][16]
  static constexpr int kWaveTot = kHist + (T / 64) * 16;   // uint32 [T / 64]
  static constexpr int kEnd = kWaveTot + (T / 64 + 1) / 2;
  static constexpr int kWords = E * (T + 1);  // rank_one's image
};

// The m (1 <= m <= kTopkSel < n <= T * E) best of in[0, n), by selection.
// (Right for every such n; topk_one sends it the segments above kTopkSelMin.)
template <int T, int E>
__device__ __forceinline__ void topk_select(const float* __restrict__ in, int n, int m, float* __restrict__ out_vals,
                                            int64_t* __restrict__ out_idx, uint64_t* __restrict__ lds) {
  using L = TopkLds<T, E>;
  constexpr int ES = L::ES, NW = T / 64;
  static_assert(ES * T == kTopkSel && E <= 16 && NW <= 16, "class shape");
  static_assert(L::kEnd <= L::kWords, "the select path lives in rank_one's LDS image");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t* hist = reinterpret_cast<uint32_t*>(lds + L::kHist);
  uint32_t* wave_tot = reinterpret_cast<uint32_t*>(lds + L::kWaveTot);
  uint64_t* selw = lds + L::kSel;

  uint32_t key[E];
  uint32_t act = 0;  // bit j: element j is inside the segment and not decided yet
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const int i = j * T + tid;
    key[j] = kRankKeyPad;
    if (i < n) {
      key[j] = rank_key(in[i], true);
      act |= 1u << j;
    }
  }
  uint32_t sel = 0;  // bit j: element j is among the m best
  int need = m;      // how many of the undecided are
  // digits of the word, most significant first: bits 63..32 (the key), then
  // 15..0 (the index; bits 31..16 of it are zero)
  for (int pass = 0; pass < 12; ++pass) {
    const int shift = pass < 8 ? 28 - 4 * pass : 12 - 4 * (pass - 8);
    // per-thread counts: 16 digits x 8 bits (a thread holds at most 16 elements)
    uint64_t lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const uint32_t src = pass < 8 ? key[j] : uint32_t(j * T + tid);
      const uint32_t d = (src >> shift) & 15u;
      const uint64_t inc = ((act >> j) & 1u) ? uint64_t(1) << ((d & 7u) * 8u) : uint64_t(0);
      lo += (d & 8u) ? uint64_t(0) : inc;
      hi += (d & 8u) ? inc : uint64_t(0);
    }
    // wave sum. 8 lanes of at most 16 fit the 8-bit counters; then 16-bit ones
#pragma unroll
    for (int s = 1; s <= 4; s <<= 1) {
      lo += __shfl_xor(lo, s, 64);
      hi += __shfl_xor(hi, s, 64);
    }
    constexpr uint64_t kEven = 0x00ff00ff00ff00ffull;
    uint64_t c0 = lo & kEven, c1 = (lo >> 8) & kEven;  // digits 0 2 4 6 / 1 3 5 7
    uint64_t c2 = hi & kEven, c3 = (hi >> 8) & kEven;  // digits 8 10 12 14 / 9 11 13 15
#pragma unroll
    for (int s = 8; s <= 32; s <<= 1) {
      c0 += __shfl_xor(c0, s, 64);
      c1 += __shfl_xor(c1, s, 64);
      c2 += __shfl_xor(c2, s, 64);
      c3 += __shfl_xor(c3, s, 64);
    }
    uint32_t* h = hist + (pass & 1) * NW * 16;
    if (lane < 16) {
      const uint64_t c = (lane & 8) ? ((lane & 1) ? c3 : c2) : ((lane & 1) ? c1 : c0);
      h[wave * 16 + lane] = uint32_t(c >> (16 * ((lane & 7) >> 1))) & 0xffffu;
    }
    // the one barrier of the pass. The copy of the counts alternates: a wave
    // writes this copy again only behind the next pass's barrier, which no wave
    // passes before it has read this one
    __syncthreads();
    int cnt = 0;
    if (lane < 16) {
#pragma unroll
      for (int w = 0; w < NW; ++w) cnt += int(h[w * 16 + lane]);
    }
    int incl = cnt;  // inclusive sum over the digits (lanes 0..15)
#pragma unroll
    for (int s = 1; s <= 8; s <<= 1) {
      const int o = __shfl_up(incl, s, 64);
      if (lane >= s) incl += o;
    }
    const uint64_t reach = __ballot(lane < 16 && incl >= need);
    // need <= the undecided, so a digit reaches it; the guard keeps a broken
    // invariant from indexing outside the 16 lanes
    const int b = reach ? __ffsll((long long)reach) - 1 : 15;
    const int below = __builtin_amdgcn_readfirstlane(__shfl(incl - cnt, b, 64));
    const int at = __builtin_amdgcn_readfirstlane(__shfl(cnt, b, 64));
    need -= below;
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const uint32_t src = pass < 8 ? key[j] : uint32_t(j * T + tid);
      const uint32_t d = (src >> shift) & 15u;
      const uint32_t bit = act & (1u << j);
      if (d < uint32_t(b)) sel |= bit;
      if (d != uint32_t(b)) act &= ~bit;
    }
    if (at <= need) {  // the whole digit is wanted (the words differ: at the latest in the last pass)
      sel |= act;
      break;
    }
  }
  // compact the selected words: exclusive scan of the per-thread counts
  const int mine = __popc(sel);
  int pos = mine;
#pragma unroll
  for (int s = 1; s <= 32; s <<= 1) {
    const int o = __shfl_up(pos, s, 64);
    if (lane >= s) pos += o;
  }
  if (lane == 63) wave_tot[wave] = uint32_t(pos);
  __syncthreads();
  pos -= mine;
#pragma unroll
  for (int w = 0; w < NW; ++w)
    if (w < wave) pos += int(wave_tot[w]);
#pragma unroll
  for (int j = 0; j < E; ++j) {
    if (((sel >> j) & 1u) && pos < kTopkSel) {
      selw[pos] = (uint64_t(key[j]) << 32) | uint32_t(j * T + tid);
      ++pos;
    }
  }
  __syncthreads();
  int p2 = ES;
  while (p2 < m) p2 <<= 1;
  const bool wave_active = (tid & ~63) * ES < p2;
  uint64_t w[ES];
#pragma unroll
  for (int e = 0; e < ES; ++e) w[e] = tid * ES + e < m ? selw[tid * ES + e] : kRankPadWord;
  rank_network<T, ES>(w, p2, wave_active, lds);
#pragma unroll
  for (int e = 0; e < ES; ++e) {
    const int r = tid * ES + e;
    if (r < m && w[e] != kRankPadWord) {
      const int src = int(uint32_t(w[e]));
      uint32_t bits;
      out_vals[r] = rank_unkey(uint32_t(w[e] >> 32), true, &bits) ? __uint_as_float(bits) : in[src];
      out_idx[r] = src;
    }
  }
  __syncthreads();  // the LDS is free for the workgroup's next segment
}

// One segment: in[0, n), 1 <= n <= T * E, k >= 1; the same in every thread.
// A launch is two kernels over the same segments, each taking those of its
// path and leaving the others alone: SELECT, and the full network. (One kernel
// with both inlined needs more than the 128 registers a 1024-thread workgroup
// has and would spill to scratch.)
template <int T, int E, bool SELECT>
__device__ __forceinline__ void topk_one(const float* __restrict__ in, int n, int k, float* __restrict__ out_vals,
                                         int64_t* __restrict__ out_idx, uint64_t* __restrict__ lds) {
  const int m = k < n ? k : n;
  const bool selects = T * E > kTopkSelMin && n > kTopkSelMin && m <= kTopkSel;
  if constexpr (SELECT) {
    if (selects) topk_select<T, E>(in, n, m, out_vals, out_idx, lds);
  } else {
    if (!selects) rank_one<T, E, false>(in, n, true, m, out_vals, out_idx, lds);
  }
}

template <int T, int E, bool SELECT>
__global__ void __launch_bounds__(T) topk_segments_kernel(const float* __restrict__ scores, int64_t n_scores,
                                                          const int32_t* __restrict__ offsets,
                                                          const int32_t* __restrict__ k, int S,
                                                          float* __restrict__ out_vals, int64_t* __restrict__ out_idx) {
  __shared__ uint64_t lds[SELECT ? TopkLds<T, E>::kEnd : TopkLds<T, E>::kWords];
  for (int s = blockIdx.x; s < S; s += gridDim.x) {
    const int64_t a = offsets[s], b = offsets[s + 1];
    const int64_t n = b - a;
    const int ks = k[s];
    if (ks <= 0 || a < 0 || n <= 0 || n > T * E || b > n_scores) continue;  // same in every thread
    topk_one<T, E, SELECT>(scores + a, int(n), ks, out_vals + a, out_idx + a, lds);
  }
}

// Segments and k from a request arena (csrc/runtime/arena.h): n_req at 0,
// n_topk at 48, the payload offset of the per-descriptor int32 k table at 56,
// descriptors {ids_off, wts_off, rows, dst_row} int64 at 64. Nothing is
// written when no request of the batch asked for a top-k output, nor for a
// descriptor whose k is 0 or that does not fit.
template <int T, int E, bool SELECT>
__global__ void __launch_bounds__(T) topk_arena_kernel(const uint8_t* __restrict__ arena,
                                                       const float* __restrict__ scores, int64_t scores_len,
                                                       float* __restrict__ out_vals, int64_t* __restrict__ out_idx) {
  __shared__ uint64_t lds[SELECT ? TopkLds<T, E>::kEnd : TopkLds<T, E>::kWords];
  if (*reinterpret_cast<const int32_t*>(arena + 48) <= 0) return;
  const int64_t tab_off = *reinterpret_cast<const int64_t*>(arena + 56);
  if (tab_off < 0 || (tab_off & 3) != 0 || tab_off > int64_t(INT32_MAX)) return;
  const int n_req = min(*reinterpret_cast<const int32_t*>(arena), kArenaMaxRequests);
  const int64_t* desc = reinterpret_cast<const int64_t*>(arena + 64);
  const int32_t* ktab = reinterpret_cast<const int32_t*>(arena + kArenaPayloadOff + tab_off);
  for (int d = blockIdx.x; d < n_req; d += gridDim.x) {
    const int64_t rows = desc[4 * d + 2], r0 = desc[4 * d + 3];
    const int kd = ktab[d];
    if (kd <= 0 || rows <= 0 || rows > T * E || r0 < 0 || r0 + rows > scores_len) continue;
    topk_one<T, E, SELECT>(scores + r0, int(rows), kd, out_vals + r0, out_idx + r0, lds);
  }
}

}  // namespace kern

using namespace kern;

int topk_select_max() { return kTopkSel; }
int topk_select_min() { return kTopkSelMin; }

namespace {
constexpr int kTopkGrid = 256;  // as rank.hip: one workgroup per CU at the largest class
}  // namespace

hipError_t launch_topk_segments(const float* scores, int64_t n_scores, const int32_t* offsets, const int32_t* k, int S,
                                int max_len, float* out_vals, int64_t* out_idx, hipStream_t st) {
  if (S <= 0) return hipSuccess;
  if (max_len > kRankMax) return hipErrorInvalidValue;
  const dim3 grid(S < kTopkGrid ? S : kTopkGrid);
  if (max_len > 0 && max_len <= 1024) {
    hipLaunchKernelGGL((topk_segments_kernel<256, 4, false>), grid, dim3(256), 0, st, scores, n_scores, offsets, k, S,
                       out_vals, out_idx);
  } else if (max_len > 0 && max_len <= 4096) {
    hipLaunchKernelGGL((topk_segments_kernel<512, 8, false>), grid, dim3(512), 0, st, scores, n_scores, offsets, k, S,
                       out_vals, out_idx);
  } else {
    hipLaunchKernelGGL((topk_segments_kernel<1024, 16, true>), grid, dim3(1024), 0, st, scores, n_scores, offsets, k,
                       S, out_vals, out_idx);
    hipLaunchKernelGGL((topk_segments_kernel<1024, 16, false>), grid, dim3(1024), 0, st, scores, n_scores, offsets, k,
                       S, out_vals, out_idx);
  }
  return hipGetLastError();
}

hipError_t launch_topk_arena(const void* arena_dev, const float* scores, int64_t scores_len, float* out_vals,
                             int64_t* out_idx, hipStream_t st) {
  if (scores_len <= 0) return hipSuccess;
  const uint8_t* a = static_cast<const uint8_t*>(arena_dev);
  // a request has at least one row and at most scores_len of them
  const int64_t most = scores_len < kArenaMaxRequests ? scores_len : kArenaMaxRequests;
  const dim3 grid(unsigned(most < kTopkGrid ? most : kTopkGrid));
  if (scores_len <= 1024) {
    hipLaunchKernelGGL((topk_arena_kernel<256, 4, false>), grid, dim3(256), 0, st, a, scores, scores_len, out_vals,
                       out_idx);
  } else if (scores_len <= 4096) {
    hipLaunchKernelGGL((topk_arena_kernel<512, 8, false>), grid, dim3(512), 0, st, a, scores, scores_len, out_vals,
                       out_idx);
  } else {
    hipLaunchKernelGGL((topk_arena_kernel<1024, 16, true>), grid, dim3(1024), 0, st, a, scores, scores_len, out_vals,
                       out_idx);
    hipLaunchKernelGGL((topk_arena_kernel<1024, 16, false>), grid, dim3(1024), 0, st, a, scores, scores_len, out_vals,
                       out_idx);
  }
  return hipGetLastError();
}

}  // namespace dtfs
